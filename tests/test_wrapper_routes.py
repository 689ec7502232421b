"""What the single-layer wrappers behind the update operator have in common, held to each of them through public names
only: Conv1, Conv3 (Cout 64 and 128), Conv3Stack, Head (a convolution and a tail), Upmask and FlowEncoder.

- the packed weights are cached under the layer's parameters: the same object while they are untouched, a new one, bit-equal
  to the module's own pack function, after an in-place update, a load_state_dict and a re-assigned `.data` (Conv3Stack has no
  `packed()`: its cache is held to the same rule through its results on the GPU);
- `install` twice gives one wrapper; a forward that carries another module's wrapper is refused under the installing
  module's name and nothing is bound (flow.install does not refuse, so it is not asked to); `uninstall` leaves a foreign
  wrapper where it is;
- a CPU input returns the module's own bits and counts nothing;
- on the GPU, under float16 autocast, a float32 and a half input take the fused route, counted once each, with the bits of
  the operator function on the pack function's result; a batch of 0 does too, except for Upmask, which sends it to the
  module; an empty frame and a call below the threshold reach the module's own forward.
The GPU test builds its modules itself and never reads the reference tree.
"""
import os
import re
from collections import namedtuple

import pytest

torch = pytest.importorskip("torch")
nn = torch.nn

# make: the module; cls(module, **kw): the wrapper; conv(module): the fused layer; pack: its pack function; op(x, pack):
# the fused layer's operator; reached: the class whose own forward a call that is not served ends in; thresholds(v): what to
# patch so that every call (v = 0) or none (v = 1 << 40) clears MIN_FUSED_PIXELS; out: (channels, dtype) of the result
Row = namedtuple("Row", "name home make cls kw conv pack cin op reached thresholds out")


def _conv3(cout):
    return lambda: nn.Conv2d(128, cout, 3, padding=1)


def _flow():
    return nn.Sequential(nn.Conv2d(4, 128, 7, padding=3), nn.ReLU(), nn.Conv2d(128, 64, 3, padding=1), nn.ReLU())


def rows(lgu):
    c1, c3, hd, um, fl = lgu.conv1, lgu.conv3, lgu.heads, lgu.upmask, lgu.flow
    half, f32 = torch.float16, torch.float32

    def itself(m):
        return m

    def first(m):
        return m[0]

    def dict3(v):
        return [(c3, {64: v, 128: v})]
    return [
        Row("conv1-relu", c1, lambda: nn.Conv2d(196, 128, 1), c1.Conv1, {"relu": True}, itself, c1.pack_conv1, 196,
            lambda x, p: c1.conv1x1(x, *p, cin=196, relu=True), nn.Conv2d, lambda v: [(c1, v)], (128, half)),
        Row("conv3-64", c3, _conv3(64), c3.Conv3, {}, itself, c3.pack_conv3, 128,
            lambda x, p: c3.conv3x3(x, *p), nn.Conv2d, dict3, (64, half)),
        Row("conv3-128-relu", c3, _conv3(128), c3.Conv3, {"relu": True}, itself, c3.pack_conv3, 128,
            lambda x, p: c3.conv3x3(x, *p, relu=True), nn.Conv2d, dict3, (128, half)),
        Row("stack", c3, lambda: nn.Sequential(_conv3(128)(), nn.ReLU()), c3.Conv3Stack, {}, first, c3.pack_conv3, 128,
            lambda x, p: c3.conv3x3(x, *p, relu=True), nn.Conv2d, dict3, (128, half)),
        Row("head-conv", hd, lambda: nn.Conv2d(128, 2, 3, padding=1), hd.Head, {}, itself, hd.pack_head, 128,
            lambda x, p: hd.head_conv3x3(x, *p, act="none"), nn.Conv2d, lambda v: [(hd, {1: v, 2: v})], (2, half)),
        Row("head-tail", hd, lambda: nn.Sequential(nn.Conv2d(128, 1, 3, padding=1), nn.Identity(), nn.Softplus()), hd.Head, {},
            first, hd.pack_head, 128, lambda x, p: hd.head_conv3x3(x, *p, act="softplus"), nn.Sequential,
            lambda v: [(hd, {1: v, 2: v})], (1, f32)),
        Row("upmask", um, lambda: nn.Sequential(nn.Conv2d(128, 576, 1)), um.Upmask, {}, first, um.pack_upmask, 128,
            lambda x, p: um.upmask_conv1x1(x, *p), nn.Sequential, lambda v: [(um, v)], (576, half)),
        Row("flow", fl, _flow, fl.FlowEncoder, {}, first, fl.pack_conv7, 4,
            lambda x, p: fl.flow_conv7_relu(x, *p), nn.Sequential, lambda v: [(fl, v)], (64, half)),
    ]


NAMES = ["conv1-relu", "conv3-64", "conv3-128-relu", "stack", "head-conv", "head-tail", "upmask", "flow"]


def row(lgu, name):
    return {r.name: r for r in rows(lgu)}[name]


def module(r, seed=0):
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(100 + seed)
        return r.make()


def same_bits(a, b):
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    iv = torch.int16 if a.element_size() == 2 else torch.int32
    return bool(torch.equal(a.view(iv), b.view(iv)))


def same_pack(got, want):
    return len(got) == len(want) == 2 and all(same_bits(g, w) for g, w in zip(got, want))


def test_the_table_names_every_wrapper(lgu):
    assert [r.name for r in rows(lgu)] == NAMES
    assert {r.cls for r in rows(lgu)} == {lgu.Conv1, lgu.Conv3, lgu.Conv3Stack, lgu.Head, lgu.Upmask, lgu.FlowEncoder}
    assert lgu.conv3._WRAPPERS == (lgu.Conv3, lgu.Conv3Stack)


# ---- CPU ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [n for n in NAMES if n != "stack"])
def test_the_pack_cache_follows_the_parameters(lgu, name):
    r = row(lgu, name)
    m = module(r)
    wr, conv = r.cls(m, **r.kw), r.conv(m)
    held = [wr.packed()]                # kept alive, so that `is not` cannot be fooled by a reused address
    assert wr.packed() is held[0] and same_pack(held[0], r.pack(conv.weight, conv.bias))

    def renewed():
        p = wr.packed()
        assert all(p is not q for q in held) and wr.packed() is p
        assert same_pack(p, r.pack(conv.weight, conv.bias)) and not same_pack(p, held[-1])
        held.append(p)
    with torch.no_grad():
        conv.weight.mul_(2.0)
    renewed()
    m.load_state_dict({k: v.clone() * 0.5 for k, v in m.state_dict().items()})
    renewed()
    conv.weight.data = conv.weight.data.clone() * 3.0
    renewed()
    assert wr.fused_calls == 0


def _foreign(lgu, r):
    if r.home is lgu.heads:
        return lgu.upmask.Upmask(nn.Conv2d(128, 576, 1))
    return lgu.heads.Head(nn.Conv2d(128, 2, 3, padding=1))


@pytest.mark.parametrize("name", NAMES)
def test_install_is_idempotent_and_leaves_foreign_wrappers_alone(lgu, name):
    r = row(lgu, name)
    m = module(r)
    keys = list(m.state_dict().keys())
    wr = r.home.install(m, **r.kw)
    assert type(wr) is r.cls and m.forward is wr and wr.module is m
    assert r.home.install(m, **r.kw) is wr and m.forward is wr
    assert list(m.state_dict().keys()) == keys
    r.home.uninstall(m)
    assert "forward" not in m.__dict__

    m = module(r)
    other = _foreign(lgu, r)
    m.forward = other
    r.home.uninstall(m)                 # a foreign wrapper is left alone
    assert m.forward is other
    if r.home is lgu.flow:              # flow.install does not refuse
        return
    who = r.home.__name__.rsplit(".", 1)[-1] + ".install"
    with pytest.raises(RuntimeError, match="^" + re.escape("%s: forward already carries a %s" % (who, type(other).__name__))):
        r.home.install(m, **r.kw)
    assert m.forward is other


@pytest.mark.parametrize("name", NAMES)
def test_a_cpu_input_returns_the_modules_own_bits(lgu, name):
    r = row(lgu, name)
    m = module(r)
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(7)
        x = torch.randn(2, r.cin, 3, 5)
    with torch.no_grad():
        want = m(x.clone())
        if r.kw.get("relu"):
            want = torch.relu(want)
        wr = r.cls(m, **r.kw)
        got = wr(x.clone())
    assert same_bits(got, want) and wr.fused_calls == 0


# ---- GPU ------------------------------------------------------------------------------------------------------------
class _Reached:
    """While active, `cls.forward` of `target` records the call and returns `result` instead of computing anything: an
    empty frame is something torch's own convolution refuses, and which route was taken is all that is asked."""

    def __init__(self, monkeypatch, cls, target, result):
        self.calls = 0
        orig, spy = cls.forward, self

        def forward(module, *args, **kwargs):
            if module is not target:
                return orig(module, *args, **kwargs)
            spy.calls += 1
            return result
        self._patch = lambda: monkeypatch.setattr(cls, "forward", forward)
        self._undo = lambda: monkeypatch.setattr(cls, "forward", orig)

    def __enter__(self):
        self._patch()
        return self

    def __exit__(self, *exc):
        self._undo()
        return False


def _set_thresholds(monkeypatch, r, v):
    for mod, value in r.thresholds(v):
        monkeypatch.setattr(mod, "MIN_FUSED_PIXELS", value)


@pytest.mark.gpu
def test_every_wrapper_routes_alike_on_the_gpu(lgu, monkeypatch):
    assert torch.cuda.is_available(), "these tests need the MI355X"
    assert os.path.exists(lgu._lib.so_path()), "liblgu_corr.so missing — run __graft_entry__.build()"
    for r in rows(lgu):
        _set_thresholds(monkeypatch, r, 0)
        m = module(r).cuda()
        wr, conv = r.cls(m, **r.kw), r.conv(m)
        target = conv if r.reached is nn.Conv2d else m          # whose own forward an unserved call ends in
        cout, odt = r.out
        fed = []                        # FlowEncoder: what the fused first layer hands the module's second convolution
        if r.home is lgu.flow:          # (torch's own convolution behind it need not repeat its bits from call to call)
            m[2].register_forward_pre_hook(lambda _, args: fed.append(args[0].clone()))
        with torch.random.fork_rng(devices=[]):
            torch.manual_seed(11)
            x32 = torch.randn(1, r.cin, 3, 5).cuda()
        with torch.no_grad(), torch.autocast("cuda", torch.float16):
            for x in (x32, x32.half()):
                before = wr.fused_calls
                y = wr(x)
                assert wr.fused_calls == before + 1, r.name
                want = r.op(x, r.pack(conv.weight, conv.bias))
                assert same_bits(fed[-1] if fed else y, want), (r.name, x.dtype)
                assert tuple(y.shape) == (1, cout, 3, 5) and y.dtype == odt, r.name
            # the cache follows an in-place update (the only hold on Conv3Stack's, which has no packed())
            conv.weight.mul_(2.0)
            before = wr.fused_calls
            y = wr(x32)
            want = r.op(x32, r.pack(conv.weight, conv.bias))
            assert wr.fused_calls == before + 1 and same_bits(fed[-1] if fed else y, want), r.name

            # a batch of 0: Upmask sends it to the module, the others to the operator
            before = wr.fused_calls
            y = wr(torch.zeros((0, r.cin, 3, 5), device="cuda"))
            assert tuple(y.shape) == (0, cout, 3, 5) and y.dtype == odt, r.name
            assert wr.fused_calls == before + (0 if r.home is lgu.upmask else 1), r.name

            # an empty frame, and a call below the threshold, reach the module
            sentinel = torch.zeros((1, cout, 3, 5), device="cuda", dtype=odt)
            before = wr.fused_calls
            with _Reached(monkeypatch, r.reached, target, sentinel) as spy:
                wr(torch.zeros((1, r.cin, 0, 5), device="cuda"))
                assert spy.calls == 1 and wr.fused_calls == before, r.name
                _set_thresholds(monkeypatch, r, 1 << 40)
                wr(x32)
                wr(x32.half())
                assert spy.calls == 3 and wr.fused_calls == before, r.name
        torch.cuda.synchronize()
