"""UpdateOperator's output stage (lgu_slam_amd.update): the trunk fan-out and the head pair on the fused
route, and the `coords1=` keyword that hands out the factor graph's float32 tensors.

What is held:
- on the CPU (the module's own route) the installed module with coords1= returns coords1 + delta.float() and
  weight.float() of its own forward, `module_calls` counts and `fused_calls`, `fanout_calls`, `pair_calls` stay 0;
- on the GPU with both thresholds at 0 the fused route takes conv3x3_fanout and head_pair (the counters advance by one
  per fused forward) and its results are bit for bit those with both thresholds above the shape, which is the separate
  launches; with coords1 the second and third results equal coords1 + delta.float() and weight.float() of that call;
  ii=None (two groups) and flow=None once each.
The GPU tests build their modules themselves and never read the reference tree.
"""
import os

import pytest

torch = pytest.importorskip("torch")

from tests import update_restatement as RU  # noqa: E402
from tests.test_update import HT, II, NUM, WD  # noqa: E402


def same_bits(a, b):
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    iv = torch.int16 if a.element_size() == 2 else torch.int32
    return bool(torch.equal(a.view(iv), b.view(iv)))


def make_coords(seed, num, ht, wd):
    g = torch.Generator().manual_seed(seed)
    ys, xs = torch.meshgrid(torch.arange(ht).float(), torch.arange(wd).float(), indexing="ij")
    return (torch.stack([xs, ys], -1)[None, None] + 2 * torch.randn((1, num, ht, wd, 2), generator=g)).contiguous()


# ---- CPU ------------------------------------------------------------------------------------------------------------
def test_on_cpu_coords1_means_the_factor_graphs_two_expressions(lgu):
    U = lgu.update
    u = RU.make_update(5)
    ins = RU.make_inputs(9, 3, 4, 5)
    ii = torch.tensor([6, 1, 6])
    coords1 = make_coords(1, 3, 4, 5)
    with torch.no_grad():
        want5, want3 = u(*ins, ii, ii), u(*ins)
        wr = U.install(u, gru_convs=True)
        got5 = u(*ins, ii, ii, coords1=coords1)
        got3 = u(*ins, coords1=coords1)
        plain = u(*ins, ii, ii)
    U.uninstall(u)
    assert (wr.module_calls, wr.fused_calls, wr.fanout_calls, wr.pair_calls) == (3, 0, 0, 0)
    assert len(got5) == 5 and len(got3) == 3 and all(same_bits(a, b) for a, b in zip(plain, want5))
    for got, want in ((got5, want5), (got3, want3)):
        assert got[1].dtype == got[2].dtype == torch.float32 and tuple(got[1].shape) == tuple(got[2].shape) == (1, 3, 4, 5, 2)
        assert torch.equal(got[1], coords1 + want[1].to(dtype=torch.float)) and torch.equal(got[2], want[2].to(dtype=torch.float))
        assert same_bits(got[0], want[0]) and all(same_bits(a, b) for a, b in zip(got[3:], want[3:]))


# ---- GPU ------------------------------------------------------------------------------------------------------------
def _need_gpu(lgu):
    assert torch.cuda.is_available(), "these tests need the MI355X"
    assert os.path.exists(lgu._lib.so_path()), "liblgu_corr.so missing — run __graft_entry__.build()"


@pytest.fixture
def no_threshold(lgu, monkeypatch):
    """The routing by size follows measurements (MIN_FUSED_*); these tests are about the fused route."""
    monkeypatch.setattr(lgu.conv1, "MIN_FUSED_PIXELS", 0)
    monkeypatch.setattr(lgu.gru, "MIN_FUSED_CONV_PIXELS", 0)


@pytest.mark.gpu
@pytest.mark.parametrize("num,ht,wd,ii", [(NUM, HT, WD, II), (1, 1, 1, [3])])
def test_fused_route_takes_the_fanout_and_the_pair_with_the_parents_bits(lgu, no_threshold, monkeypatch, num, ht, wd, ii):
    _need_gpu(lgu)
    U = lgu.update
    uc = RU.make_update(21).cuda()
    net, inp, corr, flow = RU.make_inputs(22, num, ht, wd)
    ins = (net.cuda().half(), inp.cuda().half(), corr.cuda(), flow.cuda())
    ii = torch.tensor(ii).cuda()
    coords1 = make_coords(2, num, ht, wd).cuda()
    wr = U.install(uc, gru_convs=True)

    def run(fan, pair, *args, **kw):
        monkeypatch.setattr(lgu.conv3, "MIN_FANOUT_PIXELS", 0 if fan else 1 << 40)
        monkeypatch.setattr(lgu.heads, "MIN_PAIR_PIXELS", 0 if pair else 1 << 40)
        before = (wr.fused_calls, wr.fanout_calls, wr.pair_calls, wr.module_calls)
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
            out = uc(*args, **kw)
        torch.cuda.synchronize()
        assert tuple(b - a for a, b in zip(before, (wr.fused_calls, wr.fanout_calls, wr.pair_calls, wr.module_calls))) \
            == (1, int(fan), int(pair), 0)
        return out
    # (arguments, results): with ii and flow, ii=None (two groups), flow=None
    for args, count in (((*ins, ii), 5), (ins, 3), ((*ins[:3], None, ii), 5)):
        parent = run(False, False, *args)
        assert len(parent) == count
        for fan, pair in ((True, True), (True, False), (False, True)):
            got = run(fan, pair, *args)
            assert len(got) == count and all(same_bits(a, b) for a, b in zip(got, parent)), (count, fan, pair)
        for fan, pair in ((True, True), (False, False)):      # the keyword means the same thing on both routes
            edges = run(fan, pair, *args, coords1=coords1)
            assert len(edges) == count
            assert edges[1].dtype == edges[2].dtype == torch.float32 and tuple(edges[1].shape) == tuple(edges[2].shape) == (1, num, ht, wd, 2)
            assert torch.equal(edges[1], coords1 + parent[1].to(dtype=torch.float)) and torch.equal(edges[2], parent[2].to(dtype=torch.float))
            assert same_bits(edges[0], parent[0]) and all(same_bits(a, b) for a, b in zip(edges[3:], parent[3:]))
    U.uninstall(uc)
