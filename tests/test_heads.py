"""The fused narrow 3x3 heads with 128 input channels (lgu_slam_amd.heads, csrc/heads.hip) against the float64 restatement
of their rounding model, tests/heads_restatement.py.

Numerics contract (include/lgu_corr.h):
- a single product is exact: impulses and the zero input are bit for bit (act none);
- every element of h = half(s): |h - s64| <= 1154·2^-24·S + 2^-11·(|s64| + 1154·2^-24·S) + 2^-25 with S = Σ|x_h·w_h| + |b_h|:
  fp32 accumulation in any order, one half rounding, the half subnormal floor (tests/conv3_restatement.allowance);
- sigmoid: that allowance times its largest slope 1/4, one half rounding and 4 fp32 units of its own;
- softplus (float32 out): that allowance (slope <= 1) plus k·2^-24·y with k = heads_restatement.K_SOFTPLUS = 4 = max(4, 2 x the
  1.72 units measured for torch's own HIP softplus against float64 on this test's h, MI355X);
- NaN reaches exactly its 3x3 neighbourhood through all three activations; an image's bits do not depend on the batch.
The module's own autocast forward is not held to the single-layer bound; the test prints where it sits.
The alignment audit of lgu_head3x3_c128_h16 (its operands travel in a parameter block, so the registry of
tests/alignment_cases.py does not see it) is test_guard_bands_and_alignment here.
The GPU tests build their modules themselves and never read the reference tree.
"""
import ctypes
import os

import pytest

torch = pytest.importorskip("torch")

from tests import conv3_restatement as R  # noqa: E402
from tests import flowenc_restatement as RF  # noqa: E402
from tests import heads_restatement as RH  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = "lgu_head3x3_c128_h16"
COUTS = (1, 2)
ACTS = RH.ACTS
# the issue's shapes.  The kernel's tile is 32 x 4 pixels: 5 x 65 and 17 x 130 straddle it in both directions
SHAPES = [(1, 1, 1), (1, 2, 3), (2, 9, 33), (1, 5, 65), (3, 16, 40), (1, 17, 130)]
BOUND_SHAPES = SHAPES + [(1, 60, 80)]
_CASES = {}
_NO_CPU = " must be a HIP device tensor: lgu_slam_amd has no CPU fallback"


def same_bits(a, b):
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    iv = torch.int16 if a.element_size() == 2 else torch.int32
    return bool(torch.equal(a.view(iv), b.view(iv)))


def case(cout, shape):
    """(conv, x, s64, S) on the CPU for one Cout and shape, computed once and never changed."""
    if (cout, shape) not in _CASES:
        m = RH.make_head(50 + cout, cout)
        x = R.make_input(2000 + shape[1] * shape[2], *shape)
        with torch.no_grad():
            _CASES[(cout, shape)] = (m, x) + RH.head(x, m.weight, m.bias)
    return _CASES[(cout, shape)]


# ---- CPU ------------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_entry(lgu):
    from tests.test_abi import declared_symbols
    lib = ctypes.CDLL(lgu._lib._build.SO_PATH)
    assert ENTRY in declared_symbols() and hasattr(lib, ENTRY)
    sig = lgu._lib.SIGNATURES[ENTRY]
    assert sig[0] is lgu._lib.HeadArgs and issubclass(sig[0], ctypes.Structure) and sig[1] is ctypes.c_void_p
    assert [f[0] for f in sig[0]._fields_] == ["x", "wpack", "bias", "out", "N", "H", "W", "Cout", "flags"]
    assert ctypes.sizeof(sig[0]) == 4 * 8 + 5 * 4 + 4
    assert "heads.hip" in lgu._build.SOURCES
    assert lgu.Head is lgu.heads.Head
    H = lgu.heads
    text = open(os.path.join(ROOT, "include", "lgu_corr.h")).read()
    for cout in COUTS:
        assert H.WPACK_HALVES[cout] == 4 * ((9 * cout + 15) // 16) * 64 * 8
        assert "#define LGU_HEAD_WPACK_HALVES_%d %d\n" % (cout, H.WPACK_HALVES[cout]) in text
    for name, value in (("X_HALF", H.X_HALF), ("SIGMOID", H.SIGMOID), ("SOFTPLUS", H.SOFTPLUS)):
        assert "#define LGU_HEAD_%s %d " % (name, value) in text
    assert H.ACTS == {"none": 0, "sigmoid": H.SIGMOID, "softplus": H.SOFTPLUS}
    assert set(H.MIN_FUSED_PIXELS) == set(COUTS) and H.PASSTHROUGH == ("GradientClip", "Identity")


@pytest.mark.parametrize("cout", COUTS)
def test_pack_puts_every_weight_in_its_documented_slot_and_nothing_else(lgu, cout):
    g = torch.Generator().manual_seed(5)
    w = torch.randn((cout, 128, 3, 3), generator=g)
    b = torch.randn((cout,), generator=g)
    wpack, bias_h = lgu.heads.pack_head(w, b)
    nt = (9 * cout + 15) // 16
    assert wpack.dtype == torch.float16 and wpack.is_contiguous() and wpack.numel() == lgu.heads.WPACK_HALVES[cout]
    assert tuple(wpack.shape) == (4, nt, 64, 8) and same_bits(bias_h, b.half())
    # a weight tensor that names its own index: the value at (co, c, ky, kx) is its flat index, exact in int32
    idx = torch.arange(cout * 128 * 9, dtype=torch.int32).view(cout, 128, 3, 3)
    kc, t_, lane, j = torch.meshgrid(torch.arange(4), torch.arange(nt), torch.arange(64), torch.arange(8), indexing="ij")
    q = 16 * t_ + (lane & 15)
    used = q < 9 * cout
    co, c, tap = q % cout, 32 * kc + 8 * (lane >> 4) + j, torch.clamp(q // cout, max=8)
    slot_src = idx[co, c, tap // 3, tap % 3]                        # which weight the documented formula puts in each slot
    assert sorted(slot_src[used].tolist()) == list(range(cout * 128 * 9))    # every weight once
    assert int((~used).sum()) == (16 * nt - 9 * cout) * 128                 # the stated zero columns, nothing else
    want = torch.where(used, w.half()[co, c, tap // 3, tap % 3], torch.zeros((), dtype=torch.float16))
    assert same_bits(wpack, want)
    assert bool((wpack[~used].view(torch.int16) == 0).all())
    with pytest.raises(RuntimeError, match="weight must be"):
        lgu.heads.pack_head(w[:, :64], b)
    with pytest.raises(RuntimeError, match="weight must be"):
        lgu.heads.pack_head(torch.zeros(3, 128, 3, 3), torch.zeros(3))
    with pytest.raises(RuntimeError, match="weight must be"):
        lgu.heads.pack_head(torch.zeros(cout, 128, 1, 1), b)
    with pytest.raises(RuntimeError, match="bias must be"):
        lgu.heads.pack_head(w, torch.zeros(cout + 1))


@pytest.mark.parametrize("cout,shape", [(1, (1, 1, 1)), (2, (1, 2, 3)), (1, (2, 9, 33)), (2, (2, 9, 33))])
def test_restatement_equals_float64_conv2d_on_the_rounded_operands(cout, shape):
    m, x, s64, S = case(cout, shape)
    F = torch.nn.functional
    xh, wh, bh = R.h64(x), R.h64(m.weight), R.h64(m.bias)
    s = F.conv2d(xh, wh, bh, padding=1)
    Sc = F.conv2d(xh.abs(), wh.abs(), bh.abs(), padding=1)
    # the operands are half values, so every product is exact in float64; the two sums differ in order only
    assert bool(((s - s64).abs() <= 2.0 ** -44 * S).all()) and bool(((Sc - S).abs() <= 2.0 ** -44 * S).all())
    assert bool((S >= s64.abs()).all()) and bool((R.allowance(s64, S, RH.TERMS) > 0).all())
    assert RH.TERMS == 128 * 9 + 2 == 1154
    # the tails are the same construction: the bare layer, and the activations of the float64 sums with their allowances
    for act in ACTS:
        ref, bound = RH.tail(x, RH.make_tail(50 + cout, cout, act))
        want = RH.act64(s64, act)
        assert bool(((ref - want).abs() <= 2.0 ** -44 * (S + 1)).all())
        allow = RH.act_allowance(want, R.allowance(s64, S, RH.TERMS), act)
        assert bool(((bound - allow).abs() <= 1e-9 * bound).all()) and bool((bound > 0).all())
    sp = torch.tensor([-30.0, -1.0, 0.0, 1.0, 30.0], dtype=torch.float64)
    assert bool(((RH.softplus64(sp) - F.softplus(sp, threshold=1000.0)).abs() <= 2.0 ** -50 * (1 + sp.abs())).all())


def _cpu_module_cases():
    yield "conv1", RH.make_head(3, 1), R.make_input(1, 2, 5, 7)
    yield "conv2", RH.make_head(4, 2), R.make_input(2, 1, 4, 9)
    yield "eta", RH.make_tail(5, 1, "softplus"), R.make_input(3, 2, 3, 6)
    yield "tail_sigmoid", RH.make_tail(6, 2, "sigmoid"), R.make_input(4, 1, 5, 4)
    yield "tail_none", RH.make_tail(7, 2, "none"), R.make_input(5, 1, 2, 3)


@pytest.mark.parametrize("name,m,x", [pytest.param(*c, id=c[0]) for c in _cpu_module_cases()])
def test_cpu_inputs_reach_the_module_and_install_keeps_the_state_dict(lgu, name, m, x):
    H = lgu.heads
    keys = list(m.state_dict().keys())
    with torch.no_grad():
        want = m(x.clone())
        direct = H.Head(m)
        assert same_bits(direct(x.clone()), want) and direct.fused_calls == 0
        wr = H.install(m)
        assert isinstance(wr, H.Head) and m.forward is wr and H.install(m) is wr
        assert list(m.state_dict().keys()) == keys and len(list(m.parameters())) == 2
        got = m(x.clone())
    want_grad = m(x.clone().requires_grad_())
    assert want_grad.requires_grad and same_bits(want_grad, want)
    H.uninstall(m)
    assert "forward" not in m.__dict__ and list(m.state_dict().keys()) == keys
    assert m.forward.__func__ is type(m).forward
    assert wr.fused_calls == 0 and same_bits(got, want)
    assert wr.act == {"conv1": "none", "conv2": "none", "eta": "softplus", "tail_sigmoid": "sigmoid", "tail_none": "none"}[name]


def test_construction_and_install_refuse_other_architectures(lgu):
    nn, H = torch.nn, lgu.heads

    def conv(cin=128, cout=2, **kw):
        kw.setdefault("padding", 1)
        return nn.Conv2d(cin, cout, 3, **kw)
    H.Head(conv())
    H.Head(nn.Sequential(conv(cout=1), nn.Identity(), R.Identity(), nn.Softplus()))
    H.Head(nn.Sequential(conv()))
    bad = [conv(cout=3), conv(cin=64), conv(padding=0), conv(stride=2), conv(bias=False), conv(dilation=2),
           nn.Sequential(conv(cout=1), nn.Softplus(beta=2)), nn.Sequential(conv(cout=1), nn.Softplus(threshold=10)),
           nn.Sequential(conv(), nn.ReLU(), nn.Sigmoid()),                   # an unknown middle member
           nn.Sequential(conv(), nn.Sigmoid(), nn.Sigmoid()),                # two activations
           nn.Sequential(conv(), nn.Softplus(), nn.Sigmoid()),
           nn.Sequential(conv(), nn.Sigmoid(), R.Identity()),                # the activation is not the last member
           nn.Sequential(conv(), nn.Tanh()),
           nn.Sequential(R.Identity(), conv()), nn.Sequential(conv(cout=3), nn.Sigmoid()), nn.Sequential(),
           nn.Linear(128, 2)]
    for m in bad:
        with pytest.raises(RuntimeError, match="Head: the module must be"):
            H.Head(m)
        with pytest.raises(RuntimeError, match="Head: the module must be"):
            H.install(m)
        assert "forward" not in m.__dict__
    # a forward that carries another wrapper is refused
    m = R.make_conv(1, 128)
    c3 = lgu.conv3.install(m)
    with pytest.raises(RuntimeError, match="heads.install: forward already carries a Conv3"):
        H.install(m)
    assert m.forward is c3
    lgu.conv3.uninstall(m)


def _cpu_runs(u, net, corr, motn):
    with torch.no_grad():
        return [u.corr_encoder(corr.clone()), u.flow_encoder(motn.clone()), u.delta(net.clone()), u.weight(net.clone()),
                u.agg(net.clone()), u.agg.eta(net.clone())]


def test_install_update_composes_with_conv3_in_both_orders_on_cpu(lgu):
    H, C = lgu.heads, lgu.conv3
    u = RH.make_update(11)
    keys, nparams = list(u.state_dict().keys()), len(list(u.parameters()))
    assert "agg.eta.0.weight" in keys
    net, corr, motn = R.make_input(1, 2, 4, 5), R.make_input(2, 2, 4, 5, C=R.COR_PLANES), RF.make_input(3, 2, 4, 5)
    want = _cpu_runs(u, net, corr, motn)
    for heads_first in (False, True):
        order = (H, C) if heads_first else (C, H)
        first, second = order[0].install_update(u), order[1].install_update(u)
        hw, cw = (first, second) if heads_first else (second, first)
        assert list(hw) == ["delta[2]", "weight[2]", "agg.eta"] and all(type(w) is H.Head for w in hw.values())
        assert [w.act for w in hw.values()] == ["none", "none", "softplus"]
        assert u.delta[2].forward is hw["delta[2]"] and u.weight[2].forward is hw["weight[2]"] and u.agg.eta.forward is hw["agg.eta"]
        assert type(u.delta.forward) is C.Conv3Stack and type(u.weight.forward) is C.Conv3Stack
        again = H.install_update(u)
        assert all(again[k] is hw[k] for k in hw)
        assert list(u.state_dict().keys()) == keys and len(list(u.parameters())) == nparams
        assert all(same_bits(a, b) for a, b in zip(_cpu_runs(u, net, corr, motn), want))
        assert u.agg.eta(net.clone().requires_grad_()).requires_grad
        assert all(w.fused_calls == 0 for w in list(hw.values()) + list(cw.values()))
        order[0].uninstall_update(u)
        order[1].uninstall_update(u)
        for m in (u.delta, u.delta[2], u.weight, u.weight[2], u.agg.eta, u.agg.conv1, u.corr_encoder):
            assert "forward" not in m.__dict__
    assert list(u.state_dict().keys()) == keys and all(same_bits(a, b) for a, b in zip(_cpu_runs(u, net, corr, motn), want))
    # alone, too
    hw = H.install_update(u)
    assert all(same_bits(a, b) for a, b in zip(_cpu_runs(u, net, corr, motn), want)) and "forward" not in u.delta.__dict__
    H.uninstall_update(u)
    # a site that does not match is refused before anything is bound
    for attr, repl, name in (("eta", torch.nn.Sequential(torch.nn.Conv2d(128, 1, 3, padding=1), torch.nn.Sigmoid()), "agg.eta"),
                             ("eta", torch.nn.Conv2d(128, 1, 3, padding=1), "agg.eta")):
        v = RH.make_update(12)
        setattr(v.agg, attr, repl)
        with pytest.raises(RuntimeError, match="heads.install_update: " + name.replace(".", r"\.")):
            H.install_update(v)
        assert "forward" not in v.delta[2].__dict__ and "forward" not in v.weight[2].__dict__
    v = RH.make_update(12)
    v.weight[2] = torch.nn.Conv2d(128, 3, 3, padding=1)
    with pytest.raises(RuntimeError, match=r"heads.install_update: weight\[2\]"):
        H.install_update(v)
    assert "forward" not in v.delta[2].__dict__ and "forward" not in v.agg.eta.__dict__
    v = RH.make_update(12)
    other = lgu.flow.install(v.flow_encoder)      # a foreign wrapper on one of the sites: refused before anything is bound
    v.agg.eta.forward = other
    with pytest.raises(RuntimeError, match="the forward of agg.eta already carries a FlowEncoder"):
        H.install_update(v)
    assert "forward" not in v.delta[2].__dict__ and "forward" not in v.weight[2].__dict__


def test_operator_refusals_in_their_order(lgu):
    """The act name, shape of x, pack size, bias shape, contiguity, dtypes, no-grad, device: each refusal's text, and
    which of two defects is reported.  None of them touches a device."""
    f = lgu.heads.head_conv3x3
    H = torch.float16

    def z(*shape, dtype=torch.float32):
        return torch.zeros(shape, dtype=dtype)

    def nc(t):
        return torch.zeros(tuple(t.shape) + (2,), dtype=t.dtype)[..., 0]

    bad_act = "act must be one of 'none', 'sigmoid', 'softplus', got 'relu'"
    for cout in COUTS:
        nt = (9 * cout + 15) // 16
        x, wp, bh = z(1, 128, 2, 2), z(4, nt, 64, 8, dtype=H), z(cout, dtype=H)
        other = 3 - cout
        no_grad = ("head_conv3x3 has no autograd: its outputs would carry no gradient. Call it under torch.no_grad() or pass "
                   "detached inputs")
        cases = [
            ((x, wp, bh), "x" + _NO_CPU),
            ((x.half(), wp, bh), "x" + _NO_CPU),
            ((z(1, 127, 2, 2), wp, bh), "x must be (N,128,H,W), got (1, 127, 2, 2)"),
            ((z(128, 2, 2), wp, bh), "x must be (N,128,H,W), got (128, 2, 2)"),
            ((x, z(4, nt, 64, 7, dtype=H), bh), "wpack must hold 2048 or 4096 halves (pack_head), got (4, %d, 64, 7)" % nt),
            ((x, wp, z(other, dtype=H)), "bias_h must be (%d,), got (%d,)" % (cout, other)),
            ((nc(x), wp, bh), "x must be contiguous"),
            ((x, nc(wp), bh), "wpack must be contiguous"),
            ((x, wp, nc(bh)), "bias_h must be contiguous"),
            ((x.double(), wp, bh), "expected scalar type Float or Half but found Double (x)"),
            ((x.bfloat16(), wp, bh), "expected scalar type Float or Half but found BFloat16 (x)"),
            ((x, wp.float(), bh), "expected scalar type Half but found Float (wpack)"),
            ((x, wp, bh.bfloat16()), "expected scalar type Half but found BFloat16 (bias_h)"),
            ((x.clone().requires_grad_(), wp, bh), no_grad),
            # two defects: the earlier check reports
            ((z(1, 127, 2, 2), z(5, dtype=H), bh), "x must be (N,128,H,W), got (1, 127, 2, 2)"),
            ((nc(x), z(5, dtype=H), bh), "wpack must hold 2048 or 4096 halves (pack_head), got (5,)"),
            ((nc(x), wp, z(other, dtype=H)), "bias_h must be (%d,), got (%d,)" % (cout, other)),
            ((x.double(), wp, nc(bh)), "bias_h must be contiguous"),
            ((x.clone().requires_grad_(), wp, bh.float()), "expected scalar type Half but found Float (bias_h)"),
            ((x.double().requires_grad_(), wp, bh), "expected scalar type Float or Half but found Double (x)"),
        ]
        if cout == 1:      # a tensor of one element is contiguous whatever its strides
            cases = [c for c in cases if c[1] != "bias_h must be contiguous"]
        for args, message in cases:
            for act in ACTS:
                with pytest.raises(RuntimeError) as info:
                    f(*args, act=act)
                assert type(info.value) is RuntimeError and str(info.value) == message
            with pytest.raises(RuntimeError) as info:       # the act name comes first of all
                f(*args, act="relu")
            assert type(info.value) is RuntimeError and str(info.value) == bad_act
        with torch.no_grad():      # grad mode off: the no-grad refusal does not apply, the device refusal is next
            with pytest.raises(RuntimeError) as info:
                f(x.clone().requires_grad_(), wp, bh)
            assert str(info.value) == "x" + _NO_CPU


# ---- GPU ------------------------------------------------------------------------------------------------------------
@pytest.fixture
def no_threshold(lgu, monkeypatch):
    """The wrappers' routing by size follows a measurement (MIN_FUSED_PIXELS); these tests are about the fused path."""
    monkeypatch.setattr(lgu.heads, "MIN_FUSED_PIXELS", {1: 0, 2: 0})
    monkeypatch.setattr(lgu.conv3, "MIN_FUSED_PIXELS", {64: 0, 128: 0})


def _need_gpu(lgu):
    assert torch.cuda.is_available(), "these tests need the MI355X"
    assert os.path.exists(lgu._lib.so_path()), "liblgu_corr.so missing — run __graft_entry__.build()"


def _packed(lgu, m):
    return lgu.heads.pack_head(m.weight.detach().cuda(), m.bias.detach().cuda())


def _torch_act(h, act):
    """torch's own activation of a half tensor on the GPU, as autocast evaluates it (softplus in float32)."""
    if act == "sigmoid":
        return torch.sigmoid(h)
    if act == "softplus":
        return torch.nn.functional.softplus(h.float())
    return h


IMPULSE_AT = [(2, 2), (0, 0), (0, 4), (4, 0), (4, 4)]
IMPULSE_CH = [0, 31, 32, 127]


@pytest.mark.gpu
@pytest.mark.parametrize("cout", COUTS)
def test_impulses_give_the_weights_bit_for_bit(lgu, cout):
    """One input element = 1 (centre and the four corners of a 5x5 image, channels 0, 31, 32 and 127), bias 0: a single
    product is exact, so every output is w_h[co, c, cy-y+1, cx-x+1] and 0 outside the window."""
    _need_gpu(lgu)
    m = RH.make_head(53, cout)
    with torch.no_grad():
        m.bias.zero_()
    wh = m.weight.detach().half()
    x = torch.zeros((len(IMPULSE_AT) * len(IMPULSE_CH), 128, 5, 5))
    want = torch.zeros((x.shape[0], cout, 5, 5), dtype=torch.float16)
    for i, (cy, cx) in enumerate(IMPULSE_AT):
        for k, c in enumerate(IMPULSE_CH):
            n = len(IMPULSE_CH) * i + k
            x[n, c, cy, cx] = 1.0
            for ky in range(3):
                for kx in range(3):
                    y, xx = cy - ky + 1, cx - kx + 1
                    if 0 <= y < 5 and 0 <= xx < 5:
                        want[n, :, y, xx] = wh[:, c, ky, kx]
    wpack, bias_h = _packed(lgu, m)
    got = lgu.heads.head_conv3x3(x.cuda(), wpack, bias_h)
    got_h = lgu.heads.head_conv3x3(x.half().cuda(), wpack, bias_h)
    torch.cuda.synchronize()
    assert int((want != 0).sum()) == 4 * (9 + 4 * 4) * cout
    assert same_bits(got, want), "max |diff| %g" % float((got.cpu().float() - want.float()).abs().max())
    assert same_bits(got_h, want)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("cout", COUTS)
def test_zero_input_gives_act_of_the_bias_everywhere(lgu, cout, shape):
    _need_gpu(lgu)
    m = RH.make_head(50 + cout, cout)
    wpack, bias_h = _packed(lgu, m)
    x = torch.zeros((shape[0], 128) + shape[1:], device="cuda")
    bh = m.bias.detach().half().view(1, cout, 1, 1).expand(shape[0], cout, *shape[1:]).contiguous()
    for act in ACTS:
        got = lgu.heads.head_conv3x3(x, wpack, bias_h, act=act)
        theirs = _torch_act(bh.cuda(), act)
        torch.cuda.synchronize()
        assert got.dtype == theirs.dtype and got.shape == theirs.shape
        if act == "none":
            assert same_bits(got, bh)
            continue
        y = RH.act64(bh.double(), act)
        allow = RH.act_allowance(y, torch.zeros_like(y), act)
        diff = (got.cpu().double() - theirs.cpu().double()).abs()
        assert bool((diff <= allow).all()), (act, float((diff / allow).max()))
        assert bool(((got.cpu().double() - y).abs() <= allow).all())


@pytest.mark.gpu
@pytest.mark.parametrize("shape", BOUND_SHAPES)
@pytest.mark.parametrize("cout", COUTS)
def test_every_element_is_within_the_derived_bound(lgu, cout, shape):
    """|h - s64| <= allowance(s64, S, 1154), and the activations within their allowances on top of it (module docstring).
    Prints the error of torch's own HIP softplus on this test's h in units of 2^-24 y, the measurement K_SOFTPLUS follows
    (MI355X: at most 1.72 over all cases)."""
    _need_gpu(lgu)
    m, x, s64, S = case(cout, shape)
    wpack, bias_h = _packed(lgu, m)
    base = R.allowance(s64, S, RH.TERMS)
    xc = x.cuda()
    mc = RH.make_head(50 + cout, cout).cuda()
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        own = mc(xc)
    h = None
    for act in ACTS:
        ref = RH.act64(s64, act)
        bound = RH.act_allowance(ref, base, act)
        got = lgu.heads.head_conv3x3(xc, wpack, bias_h, act=act)
        from_half = lgu.heads.head_conv3x3(xc.half(), wpack, bias_h, act=act)
        rounded = lgu.heads.head_conv3x3(xc.half().float(), wpack, bias_h, act=act)
        own_a = _torch_act(own, act)
        torch.cuda.synchronize()
        if act == "none":
            h = got
        err = (got.cpu().double() - ref).abs()
        err_own = (own_a.cpu().double() - ref).abs()
        print("head_conv3x3 Cout %d %s act=%s: worst error %.3g of its bound; the module's own forward: worst %.3g of the "
              "bound, %.4f bit-identical to the kernel"
              % (cout, shape, act, float((err / bound).max()), float((err_own / bound).max()), float((own_a == got).double().mean())))
        assert got.dtype == (torch.float32 if act == "softplus" else torch.float16) == own_a.dtype
        assert tuple(got.shape) == (shape[0], cout) + shape[1:]
        assert bool((err <= bound).all()), (act, float((err / bound).max()))
        assert same_bits(from_half, rounded) and same_bits(from_half, got)   # fp32 x is rounded to half exactly once
        # the activation is a function of h alone
        if act != "none":
            y = RH.act64(h.cpu().double(), act)
            e = (got.cpu().double() - y).abs()
            assert bool((e <= RH.act_allowance(y, torch.zeros_like(y), act)).all()), act
    y = RH.softplus64(h.cpu().double())
    theirs = torch.nn.functional.softplus(h.float()).cpu().double()
    print("torch's own HIP softplus on h, Cout %d %s: worst error %.3g units of 2^-24 y"
          % (cout, shape, float(((theirs - y).abs() / (RH.U24 * y)).max())))


# a border pixel, a pixel on a tile edge (x = 31 | 32 and 63 | 64, y = 3 | 4) and an interior one
NAN_AT = [((2, 9, 33), [(1, 5, 0, 32), (0, 64, 3, 31), (1, 127, 5, 16)]),
          ((1, 17, 130), [(0, 0, 16, 129), (0, 33, 4, 64), (0, 90, 9, 50)]),
          ((1, 5, 65), [(0, 7, 0, 0), (0, 31, 3, 63), (0, 32, 4, 64)])]


@pytest.mark.gpu
@pytest.mark.parametrize("shape,ats", NAN_AT)
@pytest.mark.parametrize("cout", COUTS)
def test_nan_reaches_exactly_its_3x3_neighbourhood(lgu, cout, shape, ats):
    _need_gpu(lgu)
    m, x, _, _ = case(cout, shape)
    wpack, bias_h = _packed(lgu, m)
    for act in ACTS:
        clean = lgu.heads.head_conv3x3(x.cuda(), wpack, bias_h, act=act).cpu()
        iv = torch.int32 if act == "softplus" else torch.int16
        assert not bool(torch.isnan(clean).any())
        for at in ats:
            xn = x.clone()
            xn[at] = float("nan")
            got = lgu.heads.head_conv3x3(xn.cuda(), wpack, bias_h, act=act).cpu()
            n, _, cy, cx = at
            want = torch.zeros((shape[0], 1) + shape[1:], dtype=torch.bool)
            want[n, 0, max(cy - 1, 0):cy + 2, max(cx - 1, 0):cx + 2] = True
            assert bool((torch.isnan(got) == want.expand_as(got)).all()), (act, at)
            assert bool((got.view(iv) == clean.view(iv))[~want.expand_as(got)].all()), (act, at)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(3, 16, 40), (3, 9, 33), (2, 5, 65)])
@pytest.mark.parametrize("cout", COUTS)
def test_an_image_does_not_depend_on_its_batch(lgu, cout, shape):
    _need_gpu(lgu)
    m = RH.make_head(50 + cout, cout)
    x = R.make_input(77, *shape).cuda()
    wpack, bias_h = _packed(lgu, m)
    for act in ACTS:
        got = lgu.heads.head_conv3x3(x, wpack, bias_h, act=act)
        for k in range(shape[0]):
            assert same_bits(got[k:k + 1], lgu.heads.head_conv3x3(x[k:k + 1].contiguous(), wpack, bias_h, act=act)), (act, k)
        back = torch.flip(x, dims=(0,)).contiguous()
        assert same_bits(torch.flip(lgu.heads.head_conv3x3(back, wpack, bias_h, act=act), dims=(0,)), got), act


def _c_call(lgu, x, wpack, bias_h, out, flags, cout=None, n=None):
    N, _, H, W = x.shape
    flags |= lgu.heads.X_HALF if x.dtype == torch.float16 else 0
    args = lgu._lib.HeadArgs(x.data_ptr(), wpack.data_ptr(), bias_h.data_ptr(), out.data_ptr(), N if n is None else n, H, W,
                             out.shape[1] if cout is None else cout, flags)
    rc = lgu._lib.load().lgu_head3x3_c128_h16(args, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc


@pytest.mark.gpu
@pytest.mark.parametrize("half_x", (False, True))
@pytest.mark.parametrize("act", ("sigmoid", "softplus"))
@pytest.mark.parametrize("shape", [(2, 9, 33), (1, 6, 40)])
@pytest.mark.parametrize("cout", COUTS)
def test_guard_bands_and_alignment(lgu, no_threshold, cout, shape, act, half_x):
    """The alignment audit of DESIGN.md §4.1 for lgu_head3x3_c128_h16: x, bias and out are served at element alignment
    with the aligned call's bits, a wpack that is not 16-byte aligned, a Cout outside {1, 2} and both activation flags
    are refused with nothing written, N == 0 launches nothing, and read-only operands are unchanged.  One odd and one even
    width."""
    from tests.alignment_cases import guards_intact, shifted
    _need_gpu(lgu)
    H = lgu.heads
    m, x, _, _ = case(cout, shape)
    wpack, bias_h = _packed(lgu, m)
    xc = x.cuda().half() if half_x else x.cuda()
    odt = torch.float32 if act == "softplus" else torch.float16
    base = {"x": xc, "wpack": wpack, "bias": bias_h, "out": torch.empty((shape[0], cout) + shape[1:], dtype=odt, device="cuda")}
    assert all(t.data_ptr() % 16 == 0 for t in base.values())
    assert _c_call(lgu, base["x"], base["wpack"], base["bias"], base["out"], H.ACTS[act]) == 0
    want = base["out"].clone()
    assert same_bits(want, H.head_conv3x3(xc, wpack, bias_h, act=act))
    xs = (2, 4, 8) if half_x else (4, 8)
    os_ = (4, 8) if act == "softplus" else (2, 4, 8)
    variants = [(k, s) for k, ss in (("x", xs), ("bias", (2, 4, 8)), ("out", os_), ("wpack", (2, 4, 8))) for s in ss]
    for key, shift in variants + [("all", 0), ("all but wpack", 0)]:
        keys = [key] if key in base else [k for k in base if key == "all" or k != "wpack"]
        args = dict(base)
        for k in keys:
            args[k] = shifted(base[k], shift if key in base else base[k].element_size())
        before = {k: args[k].clone() for k in args}
        rc = _c_call(lgu, args["x"], args["wpack"], args["bias"], args["out"], H.ACTS[act])
        if "wpack" in keys:
            assert rc == lgu._lib.LGU_E_UNSUPPORTED, (key, shift, rc)
            assert same_bits(args["out"], before["out"]), "refused, but out changed"
        else:
            assert rc == 0, (key, shift, rc)
            assert same_bits(args["out"], want), "%s shifted by %d: differs from the aligned call" % (key, shift)
        for k in ("x", "wpack", "bias"):
            assert same_bits(args[k], before[k]), "read-only operand %s changed" % k
        for k in keys:
            assert guards_intact(args[k]), "%s, %d: a guard band of %s was written" % (key, shift, k)
    # a Cout the kernel does not serve and both activation flags: refused, out untouched; N == 0: nothing launched
    out = shifted(base["out"], 0)
    before = out.clone()
    assert _c_call(lgu, xc, wpack, bias_h, out, H.ACTS[act], cout=3) == lgu._lib.LGU_E_UNSUPPORTED
    assert _c_call(lgu, xc, wpack, bias_h, out, H.SIGMOID | H.SOFTPLUS) == lgu._lib.LGU_E_UNSUPPORTED
    assert _c_call(lgu, xc, wpack, bias_h, out, H.ACTS[act], n=0) == 0
    assert _c_call(lgu, xc, wpack, bias_h, out, 8) == lgu._lib.LGU_E_BADARG          # an unknown flag
    assert _c_call(lgu, xc, wpack, bias_h, out, H.ACTS[act], n=-1) == lgu._lib.LGU_E_BADARG
    assert same_bits(out, before) and guards_intact(out)
    assert tuple(H.head_conv3x3(xc[:0], wpack, bias_h, act=act).shape) == (0, cout) + shape[1:]
    assert tuple(H.head_conv3x3(xc[:, :, :0], wpack, bias_h, act=act).shape) == (shape[0], cout, 0, shape[2])


TAIL_SHAPE = (2, 9, 33)


def _modes(wr, mc, xc, calls):
    """Autocast off, a bfloat16 autocast and a grad input go to the module: the counter is unchanged and the result has
    the dtype and shape of the module's own.  (`mc` is a twin with the same weights; the library's convolution is not
    bit-reproducible between two modules, so the values are compared to the precision of the coarsest mode, bfloat16.)"""
    def like(a, b):
        return a.dtype == b.dtype and a.shape == b.shape and bool(((a.double() - b.double()).abs() <= 2.0 ** -6 * (1 + b.double().abs())).all())
    with torch.no_grad():
        assert like(wr(xc), mc(xc))
        with torch.autocast("cuda", dtype=torch.bfloat16):
            assert like(wr(xc), mc(xc))
    with torch.autocast("cuda", dtype=torch.float16):
        grad = wr(xc.clone().requires_grad_())
        assert grad.requires_grad and like(grad, mc(xc))
    assert wr.fused_calls == calls


@pytest.mark.gpu
@pytest.mark.parametrize("cout,act", [(1, "softplus"), (2, "sigmoid")])
def test_head_on_a_tail_is_within_the_propagated_bound(lgu, no_threshold, monkeypatch, cout, act):
    """Head on the reference's agg.eta (conv, GradientClip, Softplus) and on a (conv, Identity, Sigmoid) tail."""
    _need_gpu(lgu)
    H = lgu.heads
    m = RH.make_tail(71, cout, act)
    x = R.make_input(22, *TAIL_SHAPE)
    with torch.no_grad():
        ref, bound = RH.tail(x, m)
    mc = RH.make_tail(71, cout, act).cuda()      # never wrapped: the module's own forward
    wrapped = RH.make_tail(71, cout, act).cuda()
    xc = x.cuda()
    wr = H.Head(wrapped)
    assert wr.act == act
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        own = mc(xc.clone())
        got = wr(xc)
        assert wr.fused_calls == 1
        assert same_bits(wr(xc.half()), got) and wr.fused_calls == 2      # a half input is used as it is
    _modes(wr, mc, xc, 2)
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        assert H.install(wrapped) is wrapped.forward and wrapped.forward is not wr
        installed = wrapped(xc)
        assert wrapped.forward.fused_calls == 1
        H.uninstall(wrapped)
        monkeypatch.setattr(H, "MIN_FUSED_PIXELS", {1: 1 << 40, 2: 1 << 40})     # below the threshold: the module
        assert same_bits(wr(xc), own) and wr.fused_calls == 2
    torch.cuda.synchronize()
    assert got.dtype == own.dtype == (torch.float32 if act == "softplus" else torch.float16)
    assert got.shape == own.shape == (TAIL_SHAPE[0], cout) + TAIL_SHAPE[1:]
    assert same_bits(installed, got)
    err, err_own = (got.cpu().double() - ref).abs(), (own.cpu().double() - ref).abs()
    print("Head %s tail: worst error %.3g of the bound; the module's own forward %.3g; %.4f of the elements bit-identical"
          % (act, float((err / bound).max()), float((err_own / bound).max()), float((got == own).double().mean())))
    assert bool((err <= bound).all()), float((err / bound).max())


@pytest.mark.gpu
def test_install_update_under_autocast_with_conv3(lgu, no_threshold):
    _need_gpu(lgu)
    H, C = lgu.heads, lgu.conv3
    u = RH.make_update(61)
    uc = RH.make_update(61).cuda()
    net, corr, motn = R.make_input(1, *TAIL_SHAPE), R.make_input(2, *TAIL_SHAPE, C=R.COR_PLANES), RF.make_input(3, *TAIL_SHAPE)
    netc, corrc, motnc = net.cuda(), corr.cuda(), motn.cuda()

    def run():
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
            return {"corr_encoder": uc.corr_encoder(corrc), "flow_encoder": uc.flow_encoder(motnc), "delta": uc.delta(netc),
                    "weight": uc.weight(netc), "agg": uc.agg(netc), "agg.eta": uc.agg.eta(netc)}
    own = run()
    with torch.no_grad():
        bounds = {"delta": R.stack(net, u.delta), "weight": R.stack(net, u.weight), "agg.eta": RH.tail(net, u.agg.eta)}
    first = None
    for heads_first in (False, True):
        order = (H, C) if heads_first else (C, H)
        a, b = order[0].install_update(uc), order[1].install_update(uc)
        hw, cw = (a, b) if heads_first else (b, a)
        got = run()
        # conv3: one eligible convolution per stack, agg.conv1 and agg.conv2; heads: delta[2], weight[2] and agg.eta
        assert [w.fused_calls for w in cw.values()] == [1, 1, 1, 1, 1, 1]
        assert [w.fused_calls for w in hw.values()] == [1, 1, 1]
        for k, (ref, bound) in bounds.items():
            err, err_own = (got[k].cpu().double() - ref).abs(), (own[k].cpu().double() - ref).abs()
            print("install_update %s (heads first: %s): worst error %.3g of the bound; the module's own forward %.3g; %.4f "
                  "bit-identical" % (k, heads_first, float((err / bound).max()), float((err_own / bound).max()),
                                     float((got[k] == own[k]).double().mean())))
            assert got[k].dtype == own[k].dtype and got[k].shape == own[k].shape
            assert bool((err <= bound).all()), (k, float((err / bound).max()))
        assert got["agg.eta"].dtype == torch.float32 and got["delta"].dtype == got["weight"].dtype == torch.float16
        if first is None:
            first = got
            _modes(hw["agg.eta"], RH.make_update(61).cuda().agg.eta, netc, 1)
        else:
            assert all(same_bits(got[k], first[k]) for k in got)          # the order of the installs does not matter
        order[0].uninstall_update(uc)
        order[1].uninstall_update(uc)
        assert all(same_bits(p, q) for p, q in zip(run().values(), own.values()))
