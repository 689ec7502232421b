"""The whole-module update operator (lgu_slam_amd.update) on the stand-in tests/update_restatement.py.

What is held:
- construction refuses a module that is not shaped like the reference's, before anything is bound; install binds the
  module's forward only, keeps the state_dict keys and every per-site install on a submodule, and refuses a foreign wrapper;
- everything the fused route does not serve (CPU tensors, fp32 mode, a bfloat16 autocast, grad, batch 2) is the module's
  own forward, bit for bit on the CPU, and `module_calls` counts it;
- on the fused route every output is bit for bit the composition written out here from the public operator functions.
  The GRU's library convolutions (gru_convs=False) are not bit-reproducible from call to call, so the composition takes the
  GRU's result from the operator's own call (a recorder around its KanBiasGRU) and checks that call's inputs; with
  gru_convs=True, where every launch is this package's, the GRU is called anew and must give the same bits;
- corr_encoder's part is within conv3_restatement.stack's bound from corr; delta and weight are within the same
  restatement's bound computed from the returned net's own bits;
- shapes and dtypes are those of the stand-in's own autocast forward.
The GPU tests build their modules themselves and never read the reference tree.
"""
import os

import pytest

torch = pytest.importorskip("torch")

from tests import conv3_restatement as R  # noqa: E402
from tests import update_restatement as RU  # noqa: E402
from tests.test_upmask import same_bits  # noqa: E402

NUM, HT, WD = 5, 6, 9
II = [4, 4, 7, 2, 7]          # unequal segments, unsorted first appearance: unique = [2, 4, 7], inverse = [1, 1, 2, 0, 2]


def _bound_nowhere(u):
    return "forward" not in u.__dict__ and all("forward" not in m.__dict__ for m in u.modules())


def _same_all(a, b):
    return len(a) == len(b) and all(same_bits(x, y) for x, y in zip(a, b))


# ---- CPU ------------------------------------------------------------------------------------------------------------
def test_exports(lgu):
    assert lgu.UpdateOperator is lgu.update.UpdateOperator
    for name in ("install", "uninstall", "UpdateOperator"):
        assert callable(getattr(lgu.update, name))


def test_a_wrongly_shaped_module_is_refused_with_nothing_bound(lgu):
    nn, U = torch.nn, lgu.update

    def spoil(fn):
        u = RU.make_update(3)
        fn(u)
        return u
    cases = {
        "corr_encoder": lambda u: u.corr_encoder.__setitem__(0, nn.Conv2d(225, 128, 1)),
        "corr_encoder ": lambda u: u.corr_encoder.__setitem__(1, nn.Identity()),
        "corr_encoder  ": lambda u: setattr(u, "corr_encoder", nn.Sequential(*list(u.corr_encoder)[:2])),
        "FlowEncoder": lambda u: u.flow_encoder.__setitem__(0, nn.Conv2d(4, 128, 5, padding=2)),
        "delta": lambda u: u.delta.__setitem__(1, nn.Identity()),
        "delta ": lambda u: u.delta.append(nn.Sigmoid()),
        "weight": lambda u: setattr(u, "weight", nn.Sequential(*list(u.weight)[:-1])),
        "weight ": lambda u: u.weight.__setitem__(2, nn.Conv2d(128, 2, 3, padding=1, bias=False)),
        "agg.conv1": lambda u: setattr(u.agg, "conv1", nn.Conv2d(128, 64, 3, padding=1)),
        "agg.conv2": lambda u: setattr(u.agg, "conv2", nn.Conv2d(128, 128, 3)),
        "agg.eta": lambda u: setattr(u.agg, "eta", u.agg.eta[0]),
        "agg.eta ": lambda u: setattr(u.agg, "eta", nn.Sequential(u.agg.eta[0], nn.Sigmoid())),
        "agg.upmask": lambda u: setattr(u.agg, "upmask", nn.Sequential(nn.Conv2d(128, 576, 1), nn.ReLU())),
        "KanBiasGRU": lambda u: setattr(u.gru, "convq", nn.Conv2d(448, 128, 1)),
        "KanBiasGRU ": lambda u: delattr(u, "gru"),
        "agg": lambda u: delattr(u, "agg"),
    }
    for what, fn in cases.items():
        u = spoil(fn)
        for make in (U.UpdateOperator, U.install):
            with pytest.raises(RuntimeError, match=what.strip()):
                make(u)
            assert _bound_nowhere(u), what
    with pytest.raises(RuntimeError):
        U.install(nn.Linear(3, 3))
    U.UpdateOperator(RU.make_update(3))      # the stand-in itself is taken


def test_on_cpu_the_installed_module_returns_its_own_forwards_bits(lgu):
    U = lgu.update
    u = RU.make_update(5)
    keys = list(u.state_dict().keys())
    ins = RU.make_inputs(9, 3, 4, 5)
    ii = torch.tensor([6, 1, 6])
    with torch.no_grad():
        want5, want3, want0 = u(*ins, ii, ii), u(*ins), u(*ins[:3])
        wr = U.install(u, gru_convs=True)
        assert isinstance(wr, U.UpdateOperator) and u.forward is wr and list(u.state_dict().keys()) == keys
        assert all("forward" not in m.__dict__ for m in u.modules() if m is not u)      # nothing bound on a submodule
        got5, got3, got0 = u(*ins, ii, ii), u(*ins), u(*ins[:3])
        got_kw = u(ins[0], ins[1], corr=ins[2], ii=ii)
    assert len(got5) == 5 and len(got3) == 3 and _same_all(got5, want5) and _same_all(got3, want3) and _same_all(got0, want0)
    assert _same_all(got_kw, u.__class__.forward(u, *ins[:3], None, ii)) and wr.module_calls == 4 and wr.fused_calls == 0
    assert tuple(got5[3].shape) == (1, 2, 4, 5) and tuple(got5[4].shape) == (1, 2, 576, 4, 5) and tuple(got5[1].shape) == (1, 3, 4, 5, 2)
    # grad flows through the module's own forward
    out = u(ins[0].clone().requires_grad_(), *ins[1:])
    assert out[1].requires_grad and wr.module_calls == 5
    # a second install returns the first wrapper with the flags set as given
    assert wr.gru.convs is True and wr.defer_upmask is False
    assert U.install(u, defer_upmask=True) is wr and wr.gru.convs is False and wr.defer_upmask is True
    assert U.install(u) is wr and wr.defer_upmask is False
    wpack, bias_h = wr.upmask_packed()
    assert wr.upmask_packed()[0] is wpack and same_bits(wpack, lgu.upmask.pack_upmask(u.agg.upmask[0].weight, u.agg.upmask[0].bias)[0])
    U.uninstall(u)
    assert _bound_nowhere(u) and list(u.state_dict().keys()) == keys and u.forward.__func__ is type(u).forward
    with torch.no_grad():
        assert _same_all(u(*ins, ii), want5)


def test_a_foreign_wrapper_is_refused_and_per_site_installs_survive(lgu):
    U = lgu.update
    u = RU.make_update(6)
    other = lgu.heads.Head(torch.nn.Conv2d(128, 2, 3, padding=1))
    u.forward = other
    with pytest.raises(RuntimeError, match="update.install: forward already carries a Head"):
        U.install(u)
    assert u.forward is other
    U.uninstall(u)                       # a foreign wrapper is left alone
    assert u.forward is other
    del u.forward
    # every per-site install of the parent, then the operator on top, then off again
    sites = {"flow": lgu.flow.install(u.flow_encoder), "gru": lgu.gru.install(u.gru, convs=True), "upmask": lgu.upmask.install(u.agg.upmask),
             "conv1": lgu.conv1.install(u.corr_encoder[0])}
    c3, hd = lgu.conv3.install_update(u), lgu.heads.install_update(u)
    bound = {m: m.__dict__["forward"] for m in u.modules() if "forward" in m.__dict__}
    assert len(bound) == 4 + len(c3) + len(hd) and set(sites.values()) | set(c3.values()) | set(hd.values()) == set(bound.values())
    ins = RU.make_inputs(10, 2, 3, 4)
    ii = torch.tensor([0, 1])
    with torch.no_grad():
        want = u(*ins, ii)
        wr = U.install(u)
        assert {m: m.__dict__["forward"] for m in u.modules() if "forward" in m.__dict__ and m is not u} == bound
        assert wr.gru is not sites["gru"] and sites["gru"].convs is True
        assert _same_all(u(*ins, ii), want) and wr.module_calls == 1
        U.uninstall(u)
        assert {m: m.__dict__["forward"] for m in u.modules() if "forward" in m.__dict__} == bound
        assert _same_all(u(*ins, ii), want)


# ---- GPU ------------------------------------------------------------------------------------------------------------
@pytest.fixture
def no_threshold(lgu, monkeypatch):
    """The routing by size follows measurements (MIN_FUSED_*); these tests are about the fused route."""
    monkeypatch.setattr(lgu.conv1, "MIN_FUSED_PIXELS", 0)
    monkeypatch.setattr(lgu.gru, "MIN_FUSED_CONV_PIXELS", 0)


def _need_gpu(lgu):
    assert torch.cuda.is_available(), "these tests need the MI355X"
    assert os.path.exists(lgu._lib.so_path()), "liblgu_corr.so missing — run __graft_entry__.build()"


class Recorder:
    """Stands where UpdateOperator keeps its KanBiasGRU: passes the call on and keeps (arguments, result)."""

    def __init__(self, inner):
        self.inner, self.calls = inner, []

    def __call__(self, *args):
        out = self.inner(*args)
        self.calls.append((args, out))
        return out


def compose(lgu, u, gru, net, inp, corr, flow, ii):
    """The fused route written out from the public operator functions, with fresh packs.  `gru`: a callable (net, inp, corr,
    flow) -> net.  Returns (outputs, corr features, flow features, aggregated features or None)."""
    C1, C3, FL, HD, AG, UM = lgu.conv1, lgu.conv3, lgu.flow, lgu.heads, lgu.aggregate, lgu.upmask
    _, num, _, ht, wd = net.shape

    def c3(x, conv):
        return C3.conv3x3(x, *C3.pack_conv3(conv.weight, conv.bias), relu=True)

    def head(x, conv, act):
        return HD.head_conv3x3(x, *HD.pack_head(conv.weight, conv.bias), act=act)

    def edges(t):
        return t.view(1, num, -1, ht, wd).permute(0, 1, 3, 4, 2)[..., :2].contiguous()
    if flow is None:
        flow = torch.zeros((1, num, 4, ht, wd), device=net.device)
    net, inp, corr, flow = (t.view(num, -1, ht, wd) for t in (net, inp, corr, flow))
    ce, fe = u.corr_encoder, u.flow_encoder
    c = c3(C1.conv1x1(corr, *C1.pack_conv1(ce[0].weight, ce[0].bias), relu=True), ce[2])
    f = c3(FL.flow_conv7_relu(flow, *FL.pack_conv7(fe[0].weight, fe[0].bias)), fe[2])
    n = gru(net, inp, c, f)
    delta = edges(head(c3(n, u.delta[0]), u.delta[2], "none"))
    weight = edges(head(c3(n, u.weight[0]), u.weight[2], "sigmoid"))
    if ii is None:
        return (n.view(1, num, -1, ht, wd), delta, weight), c, f, None
    uniq, ix = torch.unique(ii.to(net.device), return_inverse=True)
    U = uniq.shape[0]
    a = AG.scatter_mean(c3(n, u.agg.conv1).view(1, num, 128, ht, wd), ix, dim=1, dim_size=U)
    a = c3(a.view(U, 128, ht, wd), u.agg.conv2)
    eta = .01 * head(a, u.agg.eta[0], "softplus").view(1, U, ht, wd)
    up = u.agg.upmask[0]
    mask = UM.upmask_conv1x1(a, *UM.pack_upmask(up.weight, up.bias)).view(1, U, 576, ht, wd)
    return (n.view(1, num, -1, ht, wd), delta, weight, eta, mask), c, f, a


def _gpu_case(seed, num, ht, wd, ii):
    u = RU.make_update(seed)
    net, inp, corr, flow = RU.make_inputs(seed + 1, num, ht, wd)
    return u, (net, inp, corr, flow), (net.cuda().half(), inp.cuda().half(), corr.cuda(), flow.cuda()), torch.tensor(ii)


@pytest.mark.gpu
@pytest.mark.parametrize("num,ht,wd,ii", [(NUM, HT, WD, II), (1, 1, 1, [3])])
def test_fused_route_is_the_composition_of_the_operator_functions(lgu, no_threshold, num, ht, wd, ii):
    _need_gpu(lgu)
    U = lgu.update
    u, cpu_ins, ins, ii = _gpu_case(21, num, ht, wd, ii)
    uc = RU.make_update(21).cuda()
    own_u = RU.make_update(21).cuda()
    ii_dev = ii.cuda() if num > 1 else ii          # the reference moves ii to the device itself
    n_unique = len(set(ii.tolist()))
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        own = own_u(*ins, ii_dev)
        for convs in (False, True):
            wr = U.install(uc, gru_convs=convs)
            rec = Recorder(wr.gru)
            wr.gru = rec
            before = (wr.fused_calls, rec.inner.fused_calls, rec.inner.fused_conv_calls)
            for with_ii in (True, False):
                for with_flow in (True, False):
                    args = ins if with_flow else ins[:3]
                    got = uc(*args, None, ii_dev) if with_ii and not with_flow else uc(*args, ii_dev if with_ii else None)
                    (gargs, gout), = rec.calls
                    rec.calls.clear()
                    want, c, f, _ = compose(lgu, uc, lambda *a: gout, ins[0], ins[1], ins[2], ins[3] if with_flow else None,
                                            ii_dev if with_ii else None)
                    assert len(got) == (5 if with_ii else 3) and _same_all(got, want), (convs, with_ii, with_flow)
                    assert same_bits(gargs[2], c) and same_bits(gargs[3], f)
                    assert same_bits(gargs[0], ins[0].view(num, 128, ht, wd)) and same_bits(gargs[1], ins[1].view(num, 128, ht, wd))
                    if convs:      # every launch is this package's: the whole forward again, the GRU called anew
                        fresh = lgu.gru.KanBiasGRU(uc.gru, convs=True)
                        again, _, _, _ = compose(lgu, uc, fresh, ins[0], ins[1], ins[2], ins[3] if with_flow else None,
                                                 ii_dev if with_ii else None)
                        assert _same_all(got, again) and fresh.fused_conv_calls == 1
                    if with_ii and with_flow:
                        full, corr_feat = got, c
            after = (wr.fused_calls, rec.inner.fused_calls, rec.inner.fused_conv_calls)
            assert [b - a for a, b in zip(before, after)] == [4, 4, 4 if convs else 0] and wr.module_calls == 0
            wr.gru = rec.inner
            # shapes and dtypes of the stand-in's own autocast forward
            assert [(t.shape, t.dtype) for t in full] == [(t.shape, t.dtype) for t in own]
            assert tuple(full[3].shape) == (1, n_unique, ht, wd) and full[3].dtype == torch.float32
            assert tuple(full[4].shape) == (1, n_unique, 576, ht, wd) and full[0].dtype == full[4].dtype == torch.float16
            # corr_encoder's part, from corr
            ref, bound = R.stack(cpu_ins[2].view(num, -1, ht, wd), u.corr_encoder)
            err = (corr_feat.cpu().double() - ref).abs()
            print("corr_encoder (gru_convs=%s): worst error %.3g of the bound" % (convs, float((err / bound).max())))
            assert bool((err <= bound).all()), float((err / bound).max())
            # delta and weight, from the returned net's own bits
            net_out = full[0].view(num, 128, ht, wd).cpu()
            for name, t in (("delta", full[1]), ("weight", full[2])):
                ref, bound = R.stack(net_out, getattr(u, name))
                err = (t.cpu().double().permute(0, 1, 4, 2, 3).reshape(num, 2, ht, wd) - ref).abs()
                print("%s (gru_convs=%s): worst error %.3g of the bound" % (name, convs, float((err / bound).max())))
                assert bool((err <= bound).all()), (name, float((err / bound).max()))
            # where the stand-in's own forward sits (information): the two differ by the roundings of every layer
            print("max |fused - own|: net %.3g delta %.3g weight %.3g eta %.3g upmask %.3g"
                  % tuple(float((a.double() - b.double()).abs().max()) for a, b in zip(full, own)))
    U.uninstall(uc)
    assert _bound_nowhere(uc)


@pytest.mark.gpu
def test_deferred_upmask_hands_out_the_features_the_mask_is_made_of(lgu, no_threshold):
    """defer_upmask=True: the first four results keep their bits, the fifth is the input that gives the default call's mask
    under upmask_conv1x1, and upsample_from_net_ on it equals upsample_disps_ on that mask, bit for bit."""
    _need_gpu(lgu)
    U = lgu.update
    _, _, ins, ii = _gpu_case(23, NUM, HT, WD, II)
    uc = RU.make_update(23).cuda()
    ii = ii.cuda()
    g = torch.Generator().manual_seed(3)
    disps = (0.05 + 1.5 * torch.rand((9, HT, WD), generator=g)).cuda()
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        wr = U.install(uc, gru_convs=True)
        full = uc(*ins, ii)
        assert U.install(uc, gru_convs=True, defer_upmask=True) is wr
        lean = uc(*ins, ii)
        assert wr.fused_calls == 2 and wr.module_calls == 0
        feats = lean[4]
        assert tuple(feats.shape) == (1, 3, 128, HT, WD) and feats.dtype == torch.float16 and _same_all(lean[:4], full[:4])
        wpack, bias_h = wr.upmask_packed()
        mask = lgu.upmask.upmask_conv1x1(feats.view(3, 128, HT, WD), wpack, bias_h)
        assert same_bits(mask.view(1, 3, 576, HT, WD), full[4])
        ix = torch.unique(ii)
        for half_weights in (False, True):
            a = torch.full((9, 8 * HT, 8 * WD), -3.0, device="cuda")
            b = a.clone()
            lgu.upmask.upsample_from_net_(a, disps, ix, feats.view(3, 128, HT, WD), wpack, bias_h, half_weights=half_weights)
            with torch.autocast("cuda", enabled=not half_weights):
                lgu.aggregate.upsample_disps_(b, disps, ix, full[4].view(3, 576, HT, WD))
            assert same_bits(a, b) and bool((a[ix] != -3.0).all()) and bool((a[[0, 1, 3, 5, 6, 8]] == -3.0).all())
    U.uninstall(uc)


@pytest.mark.gpu
def test_everything_else_reaches_the_modules_own_forward(lgu, no_threshold, monkeypatch):
    """fp32 mode, a bfloat16 autocast, an input that requires grad and batch 2 are the module's own forward (the very
    tensors it returns) with fused_calls unchanged; float32 net / inp stay on the fused route and reach the module's GRU."""
    _need_gpu(lgu)
    U = lgu.update
    _, _, ins, ii = _gpu_case(25, NUM, HT, WD, II)
    uc = RU.make_update(25).cuda()
    wr = U.install(uc, gru_convs=True)
    seen = []
    orig = RU.Update.forward

    def forward(self, *args, **kwargs):
        out = orig(self, *args, **kwargs)
        seen.append(out)
        return out
    monkeypatch.setattr(RU.Update, "forward", forward)
    f32 = tuple(t.float() for t in ins)
    with torch.no_grad():
        assert uc(*f32, ii) is seen[-1] and len(seen) == 1                      # autocast off
        with torch.autocast("cuda", dtype=torch.bfloat16):
            assert uc(*ins, ii) is seen[-1] and len(seen) == 2
        with torch.autocast("cuda", dtype=torch.float16):
            two = tuple(t.expand(2, *t.shape[1:]).contiguous() for t in ins)
            assert uc(*two, ii) is seen[-1] and len(seen) == 3                  # batch 2
    with torch.autocast("cuda", dtype=torch.float16):
        out = uc(ins[0], ins[1], ins[2].clone().requires_grad_(), ins[3], ii)
        assert out is seen[-1] and len(seen) == 4 and out[1].requires_grad      # grad
    assert wr.fused_calls == 0 and wr.module_calls == 4
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        own = orig(uc, f32[0], f32[1], ins[2], ins[3], ii)
        got = uc(f32[0], f32[1], ins[2], ins[3], ii)                            # float32 net / inp: fused, the module's GRU
    assert len(seen) == 4 and wr.fused_calls == 1 and wr.gru.fused_calls == 0
    assert [(t.shape, t.dtype) for t in got] == [(t.shape, t.dtype) for t in own]
    U.uninstall(uc)
