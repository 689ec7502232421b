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
- shapes and dtypes are those of the stand-in's own autocast forward;
- the stand-in itself, in float64, is the reference's own UpdateModule in float64 (tests/golden/update_*.npz, made by
  tools/gen_update_golden.py) at every recorded stage and every result, with the reference's state_dict keys;
- end to end, each of the fused route's five results is as close to that float64 forward as the stand-in's own autocast
  forward on the device (rms within 1.25 of the module's, the convention of tests/test_features.py);
- every link of the fused route (flow features, the GRU, agg.conv1, the mean, agg.conv2, eta, the mask), from the bits of
  its own input, is within the derived bound of its float64 restatement.
The GPU tests build their modules themselves and never read the reference tree; they read tests/golden/ only.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import aggregate_restatement as RA  # noqa: E402
from tests import conv3_restatement as R  # noqa: E402
from tests import flowenc_restatement as RF  # noqa: E402
from tests import gruconv_restatement as RG  # noqa: E402
from tests import heads_restatement as RH  # noqa: E402
from tests import kangru_restatement as RK  # noqa: E402
from tests import update_restatement as RU  # noqa: E402
from tests import upmask_restatement as RM  # noqa: E402
from tests.test_kangru import HALF_ABS_CAP, forward_bound, half_ulp  # noqa: E402
from tests.test_upmask import same_bits  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
REFERENCE = os.environ.get("LGU_REFERENCE", "/root/reference")
U24 = 2.0 ** -24
NUM, HT, WD = 5, 6, 9
II = [4, 4, 7, 2, 7]          # unequal segments, unsorted first appearance: unique = [2, 4, 7], inverse = [1, 1, 2, 0, 2]
SEGMENTS = {"update_segments": [1, 2, 2], "update_one_frame": [3], "update_distinct": [1, 1]}      # edges per distinct ii
_FIXTURES = {}


def fixture(name):
    """{key: array} of tests/golden/<name>.npz and <name>_stages.npz, read once and never changed."""
    if name not in _FIXTURES:
        z = {}
        for suffix in ("", "_stages"):
            with np.load(os.path.join(GOLD, name + suffix + ".npz")) as f:
                z.update({k: f[k] for k in f.files})
        _FIXTURES[name] = z
    return _FIXTURES[name]


def ref64(name, key):
    return torch.from_numpy(fixture(name)[key]).double()


def rms(a, b):
    return float((a.detach().cpu().double() - b).pow(2).mean().sqrt())


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


# ---- CPU: the stand-in against the reference's own float64 forward -------------------------------------------------------
def _double(ins):
    return [None if t is None else t.double() for t in ins]


@pytest.mark.parametrize("name", sorted(RU.CASES))
def test_stand_in_in_float64_equals_the_reference_fixture(name):
    """Every recorded stage and every result.  The fixture stores the float32 rounding of the reference's float64 value,
    so a stored value v is within 2^-24 |v| of it (2^-149 where float32 is subnormal): that is the tolerance.  For the
    mean over the edges and what lies behind it (agg.conv2, eta, the mask) 1e-8 of the array's largest magnitude is
    added, the room stated for the order of the stand-in's sum (index_add_ over all edges, then one division).  This test
    found the stand-in summing a float64 mean in float32: agg.conv2 of update_distinct was 1.2 of this tolerance away."""
    z = fixture(name)
    u, ins, ii = RU.make_case(name)
    assert RU.case_sha256(u, ins, ii) == str(z["sha256"]), "inputs or weights drifted from the fixture"
    assert list(u.state_dict().keys()) == [str(k) for k in z["keys"]]
    assert ii.tolist() == z["ii"].tolist() == RU.CASES[name]["ii"]
    got = RU.run_recorded(u.double(), _double(ins), ii)
    for k in RU.STAGES + RU.RESULTS:
        want = ref64(name, k)
        assert got[k].dtype == torch.float64 and got[k].shape == want.shape, k
        tol = U24 * want.abs() + 2.0 ** -149
        if k in RU.AFTER_MEAN:
            tol = tol + 1e-8 * float(want.abs().max())
        err = (got[k] - want).abs()
        print("%s %s: worst error %.3g of the tolerance" % (name, k, float((err / tol).max())))
        assert bool((err <= tol).all()), (k, float((err / tol).max()))
    assert torch.equal(got["gru"].view_as(got["net"]), got["net"]) and np.array_equal(z["gru"].reshape(z["net"].shape), z["net"])


def test_the_fixture_cases_hold_what_they_claim():
    """On the fixture's own arrays: the segment sizes of the three cases; in update_segments a frame's aggregated input is
    the mean of its edges and differs from each edge where a frame has two; in update_one_frame the reference's flow
    features are those of a zero flow."""
    for name, sizes in SEGMENTS.items():
        z = fixture(name)
        uniq, ix = np.unique(z["ii"], return_inverse=True)
        assert np.bincount(ix).tolist() == sizes and z["mean"].shape[0] == z["agg2"].shape[0] == len(sizes), name
        assert z["eta"].shape[1] == z["upmask"].shape[1] == len(sizes) and z["agg1"].shape[0] == len(z["ii"]), name
        agg1, mean = z["agg1"].astype(np.float64), z["mean"].astype(np.float64)
        scale = np.abs(mean).max()
        for f in range(len(sizes)):
            edges = np.nonzero(ix == f)[0]
            # float32 roundings of the stored operands and of the stored mean
            assert np.abs(agg1[edges].mean(0) - mean[f]).max() <= 2 * U24 * scale, (name, f)
            for e in edges if len(edges) > 1 else []:
                # a mean that took one edge is off by a tenth of the scale somewhere: seven orders above the tolerance
                assert np.abs(agg1[e] - mean[f]).max() > 0.1 * scale, (name, f, e)
    z = fixture("update_segments")
    assert sorted(set(z["ii"].tolist())) != [int(v) for v in dict.fromkeys(z["ii"].tolist())]      # unsorted first appearances
    z = fixture("update_one_frame")
    u, ins, _ = RU.make_case("update_one_frame")
    assert ins[3] is None
    with torch.no_grad():
        zero = u.flow_encoder.double()(torch.zeros((1, 4) + z["flow_feat"].shape[2:], dtype=torch.float64))
    want = zero.expand(z["flow_feat"].shape[0], -1, -1, -1)
    got = torch.from_numpy(z["flow_feat"]).double()
    assert float(want.abs().max()) > 0 and bool(((got - want).abs() <= U24 * want.abs() + 2.0 ** -149).all())
    assert float(torch.from_numpy(fixture("update_segments")["flow_feat"]).std(dim=0).max()) > 0      # and a given flow is not


@pytest.mark.skipif(not os.path.isdir(os.path.join(REFERENCE, "droid_slam")), reason="reference tree not present")
def test_fixture_regenerates_from_the_live_reference():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_update_golden.py"), "--reference", REFERENCE,
                        "--check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr


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
    flow) -> net.  Returns (outputs, intermediates): corr_feat and flow_feat, and with ii also agg1 (agg.conv1 behind its
    ReLU), mean (the per-frame mean) and agg2 (the aggregated features, what defer_upmask hands out)."""
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
        return (n.view(1, num, -1, ht, wd), delta, weight), dict(corr_feat=c, flow_feat=f)
    uniq, ix = torch.unique(ii.to(net.device), return_inverse=True)
    U = uniq.shape[0]
    a1 = c3(n, u.agg.conv1)
    mean = AG.scatter_mean(a1.view(1, num, 128, ht, wd), ix, dim=1, dim_size=U).view(U, 128, ht, wd)
    a = c3(mean, u.agg.conv2)
    eta = .01 * head(a, u.agg.eta[0], "softplus").view(1, U, ht, wd)
    up = u.agg.upmask[0]
    mask = UM.upmask_conv1x1(a, *UM.pack_upmask(up.weight, up.bias)).view(1, U, 576, ht, wd)
    return (n.view(1, num, -1, ht, wd), delta, weight, eta, mask), dict(corr_feat=c, flow_feat=f, agg1=a1, mean=mean, agg2=a)


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
                    want, parts = compose(lgu, uc, lambda *a: gout, ins[0], ins[1], ins[2], ins[3] if with_flow else None,
                                          ii_dev if with_ii else None)
                    c = parts["corr_feat"]
                    assert len(got) == (5 if with_ii else 3) and _same_all(got, want), (convs, with_ii, with_flow)
                    assert same_bits(gargs[2], c) and same_bits(gargs[3], parts["flow_feat"])
                    assert same_bits(gargs[0], ins[0].view(num, 128, ht, wd)) and same_bits(gargs[1], ins[1].view(num, 128, ht, wd))
                    if convs:      # every launch is this package's: the whole forward again, the GRU called anew
                        fresh = lgu.gru.KanBiasGRU(uc.gru, convs=True)
                        again, _ = compose(lgu, uc, fresh, ins[0], ins[1], ins[2], ins[3] if with_flow else None,
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
            # how far the whole route is from float64, next to the stand-in's own forward, is asserted by
            # test_fused_operator_is_as_close_to_float64_as_the_module; each link's bound by test_every_link_...
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


# ---- GPU: against the reference's own float64 forward (tests/golden/update_*.npz) -----------------------------------------
def _fixture_case(name):
    """(module on the CPU, CPU inputs, device inputs as _gpu_case makes them, ii) of a fixture case, the hash checked."""
    u, ins, ii = RU.make_case(name)
    assert RU.case_sha256(u, ins, ii) == str(fixture(name)["sha256"]), "inputs or weights drifted from the fixture"
    dev = (ins[0].cuda().half(), ins[1].cuda().half(), ins[2].cuda(), None if ins[3] is None else ins[3].cuda())
    return u, ins, dev, ii


@pytest.mark.gpu
@pytest.mark.parametrize("gru_convs", [False, True])
@pytest.mark.parametrize("name", sorted(RU.CASES))
def test_fused_operator_is_as_close_to_float64_as_the_module(lgu, no_threshold, name, gru_convs):
    """Under float16 autocast (net / inp half, corr / flow float32), for each of the five results:
    rms(fused - ref) <= 1.25 rms(own - ref), ref the reference's float64 forward and own the stand-in's forward on the
    device (library kernels).  1.25 is the project's convention for "as close to float64 as the module"
    (tests/test_features.py), not fitted to this route.  update_distinct has 2 to 1152 elements per result, too few for a
    ratio of rms values: there max|fused - ref| <= max|own - ref| + one half-precision ulp at the result's largest
    magnitude."""
    _need_gpu(lgu)
    U = lgu.update
    u, _, ins, ii = _fixture_case(name)
    uc = u.cuda()
    ii_dev = ii.cuda()
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        own = uc(*ins, ii_dev)
        wr = U.install(uc, gru_convs=gru_convs)
        try:
            before = wr.fused_calls
            got = uc(*ins, ii_dev)
            assert wr.fused_calls == before + 1 and wr.module_calls == 0 and wr.gru.fused_conv_calls == int(gru_convs)
        finally:
            U.uninstall(uc)
    assert len(got) == len(own) == 5 and [(t.shape, t.dtype) for t in got] == [(t.shape, t.dtype) for t in own]
    for k, g, o in zip(RU.RESULTS, got, own):
        ref = ref64(name, k)
        assert ref.shape == g.shape, k
        if name == "update_distinct":
            e_got, e_own = (float((t.cpu().double() - ref).abs().max()) for t in (g, o))
            ulp = float(half_ulp(ref.abs().max()))
            print("%s gru_convs=%s %s: max error fused %.4g, module %.4g, one half ulp %.4g" % (name, gru_convs, k, e_got, e_own, ulp))
            assert e_got <= e_own + ulp, (k, e_got, e_own, ulp)
        else:
            r_got, r_own = rms(g, ref), rms(o, ref)
            print("%s gru_convs=%s %s: rms fused %.4g, module %.4g, ratio %.3f" % (name, gru_convs, k, r_got, r_own, r_got / r_own))
            assert r_got <= 1.25 * r_own, (k, r_got, r_own)


def _share(name, err, bound):
    worst = float((err / bound).max())
    print("%s: worst error %.3g of the bound" % (name, worst))
    assert bool((err <= bound).all()), (name, worst)


@pytest.mark.gpu
@pytest.mark.parametrize("gru_convs", [False, True])
@pytest.mark.parametrize("name", ["update_segments", "update_one_frame"])
def test_every_link_of_the_fused_route_is_within_its_derived_bound(lgu, no_threshold, name, gru_convs):
    """The operator runs with defer_upmask=True; its results are bit for bit compose()'s, whose intermediates are then the
    operator's.  Each link is held, from the bits of its own input, to the float64 restatement and allowance its own test
    file uses: nothing is propagated from link to link and no tolerance is new."""
    _need_gpu(lgu)
    U, G = lgu.update, lgu.gru
    u, cpu_ins, ins, ii = _fixture_case(name)
    num, ht, wd = (RU.CASES[name][k] for k in ("num", "ht", "wd"))
    uc = RU.make_case(name)[0].cuda()
    tag = "%s gru_convs=%s " % (name, gru_convs)
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        wr = U.install(uc, gru_convs=gru_convs, defer_upmask=True)
        rec = Recorder(wr.gru)
        wr.gru = rec
        try:
            got = uc(*ins, ii.cuda())
        finally:
            wr.gru = rec.inner
            U.uninstall(uc)
        (gargs, gout), = rec.calls
        want, parts = compose(lgu, uc, lambda *a: gout, *ins, ii.cuda())
        w, b, grid, wpack = rec.inner.packed(torch.float16)
        k = G.kan_heads(G.kangru_context(gargs[0].contiguous(), w, b), grid, wpack)
        lib_out, lib = RK.forward(uc.gru, *gargs, parts=True)        # the library's autocast forward, for gru_convs=False
    assert wr.fused_calls == 1 and wr.module_calls == 0 and rec.inner.fused_conv_calls == int(gru_convs)
    assert _same_all(got[:4], want[:4]) and same_bits(got[4], parts["agg2"].view(1, -1, 128, ht, wd))
    assert same_bits(gargs[2], parts["corr_feat"]) and same_bits(gargs[3], parts["flow_feat"])
    assert same_bits(gargs[0], ins[0].view(num, 128, ht, wd)) and same_bits(gargs[1], ins[1].view(num, 128, ht, wd))
    cpu = {key: t.cpu() for key, t in parts.items()}
    net_out, mask = got[0].view(num, 128, ht, wd).cpu(), want[4].view(-1, 576, ht, wd).cpu()
    Uq = mask.shape[0]
    assert Uq == len(SEGMENTS[name])

    # flow -> flow features (update_one_frame: the zero flow the operator makes for flow=None)
    flow = torch.zeros((num, 4, ht, wd)) if cpu_ins[3] is None else cpu_ins[3].view(num, 4, ht, wd)
    with torch.no_grad():
        s2, bound = RF.encoder(flow, u.flow_encoder)
    _share(tag + "flow features", (cpu["flow_feat"].double() - torch.relu(s2)).abs(), bound)

    # (net, inp, corr features, flow features) -> net
    if gru_convs:      # tests/test_gruconv.py's whole-forward check: the float64 chain that takes the device's own k as given
        with torch.no_grad():
            ref, bound = RG.forward(u.gru, *(t.cpu() for t in gargs), *(t.cpu() for t in k))
        _share(tag + "gru", (gout.cpu().double() - ref).abs(), bound)
    else:              # tests/test_kangru.py's check_forward: the library's autocast forward, the heads' differences propagated
        dk = [float((k[h].double() - lib[key].double()).abs().max()) for h, key in enumerate(("kz", "kr", "kq"))]
        bound = min(forward_bound(uc.gru, lib, dk, True), HALF_ABS_CAP)
        worst = float((gout.double() - lib_out.double()).abs().max())
        print("%sgru: worst difference from the library's forward %.3g of the bound %.3g" % (tag, worst / bound, bound))
        assert worst <= bound, (worst, bound, dk)

    # net -> agg.conv1 behind its ReLU, and the mean -> agg.conv2 behind its ReLU
    for key, x, conv in (("agg1", net_out, u.agg.conv1), ("agg2", cpu["mean"], u.agg.conv2)):
        with torch.no_grad():
            s, S, _ = R.conv3(x, conv.weight, conv.bias, True)
        _share(tag + key, (cpu[key].double() - torch.relu(s)).abs(), R.allowance(s, S, R.TERMS))

    # agg.conv1's output -> the mean: tests/test_aggregate.py's checks for half inputs
    ix = torch.unique(ii, return_inverse=True)[1].numpy()
    src = cpu["agg1"].numpy().reshape(1, num, -1)
    assert same_bits(cpu["mean"], torch.from_numpy(RA.scatter_mean32(src, ix, Uq).reshape(Uq, 128, ht, wd)))
    tol = (int(np.bincount(ix).max()) + 1) * 2.0 ** -11 * float(np.abs(src).max())
    worst = float(np.abs(cpu["mean"].double().numpy().reshape(1, Uq, -1) - RA.scatter_mean64(src, ix, Uq)).max())
    print("%smean: worst error %.3g of the bound" % (tag, worst / tol))
    assert worst <= tol

    # aggregated features (what defer_upmask hands out) -> eta: the tail's bound times 0.01, and the two float32 roundings
    # of the product with 0.01 (the constant's and the product's)
    feats = got[4].view(Uq, 128, ht, wd).cpu()
    with torch.no_grad():
        ref, bound = RH.tail(feats, u.agg.eta)
    assert got[3].dtype == torch.float32
    _share(tag + "eta", (got[3].view(Uq, 1, ht, wd).cpu().double() - .01 * ref).abs(), .01 * bound + 2 * U24 * .01 * ref)

    # the same features -> the mask, and through the fused upsampling with both weight roundings (the flip cap of
    # tests/upmask_restatement.within on the mask's own bits, as tests/test_upmask.py holds upsample_from_net_)
    up = u.agg.upmask[0]
    with torch.no_grad():
        s, S = RM.layer(feats, up.weight, up.bias)
    _share(tag + "mask", (mask.double() - s).abs(), R.allowance(s, S, RM.TERMS))
    disps = RM.disparities(7 + wd, Uq + 2, ht, wd)
    rows_ix = torch.arange(Uq + 1, 1, -1)
    wp, bias_h = wr.upmask_packed()
    for hw in (False, True):
        out = torch.full((Uq + 2, 8 * ht, 8 * wd), -3.0, device="cuda")
        lgu.upmask.upsample_from_net_(out, disps.cuda(), rows_ix.cuda(), got[4].view(Uq, 128, ht, wd), wp, bias_h, half_weights=hw)
        rows, want_up, bound = RM.upsample(disps.numpy(), rows_ix.numpy(), mask.numpy(), hw)
        r = RM.upsample_ratio(out.cpu().numpy()[rows], want_up, bound)
        print("%supsample half_weights=%s: worst %.3g of max|d|, %.3g of the outputs above %g (cap %g)"
              % (tag, hw, r.max(), (r > RM.UPS_TOL).mean(), RM.UPS_TOL, RM.HALF_FLIP_FRACTION))
        assert RM.within(r, hw), (hw, r.max(), (r > RM.UPS_TOL).mean())
        assert bool((out[[0, 1]] == -3.0).all())
