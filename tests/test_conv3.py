"""The fused 3x3 convolution with 128 input channels (lgu_slam_amd.conv3, csrc/conv3.hip) against the float64 restatement
of its rounding model, tests/conv3_restatement.py.

Numerics contract (include/lgu_corr.h):
- a single product is exact: impulses and the zero input are bit for bit;
- every element: |y - act(s64)| <= 1154·2^-24·S + 2^-11·(|s64| + 1154·2^-24·S) + 2^-25 with S = Σ|x_h·w_h| + |b_h|: fp32
  accumulation in any order, one half rounding, the half subnormal floor;
- NaN reaches exactly its 3x3 neighbourhood; an image's bits do not depend on the batch;
- a Sequential: the fused layers' allowance pushed through the |w_h| of the layers after it plus those layers' own.
The module's own autocast forward is not held to the single-layer bound; the test prints where it sits (measured on an
MI355X: see DESIGN.md §3.15).
The alignment audit of lgu_conv3x3_c128_h16 (its operands travel in a parameter block, so the registry of
tests/alignment_cases.py does not see it) is test_guard_bands_and_alignment here, and the operator's refusals (which
tests/test_host.py's census does not list) are test_operator_refusals_in_their_order.
The GPU tests build their modules themselves and never read the reference tree.
"""
import ctypes
import os

import pytest

torch = pytest.importorskip("torch")

from tests import conv3_restatement as R  # noqa: E402
from tests import flowenc_restatement as RF  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = "lgu_conv3x3_c128_h16"
COUTS = (64, 128)
# the issue's shapes.  The kernel's tile is 64 x 2 pixels where that pads the image no more than 32 x 4, else 32 x 4:
# 5 x 65 straddles the first in both directions, 17 x 130 the second
SHAPES = [(1, 1, 1), (1, 2, 3), (2, 9, 33), (1, 5, 65), (3, 16, 40), (1, 17, 130), (1, 60, 80)]
STACKS = ("corr_encoder", "delta", "weight")
_CASES = {}
_NO_CPU = " must be a HIP device tensor: lgu_slam_amd has no CPU fallback"


def same_bits(a, b):
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    iv = torch.int16 if a.dtype == torch.float16 else torch.int32
    return bool(torch.equal(a.view(iv), b.view(iv)))


def case(cout, shape):
    """(conv, x, s64, S) on the CPU for one Cout and shape, computed once and never changed."""
    if (cout, shape) not in _CASES:
        m = R.make_conv(40 + cout, cout)
        x = R.make_input(1000 + shape[1] * shape[2], *shape)
        with torch.no_grad():
            _CASES[(cout, shape)] = (m, x) + R.conv3(x, m.weight, m.bias, False)[:2]
    return _CASES[(cout, shape)]


# ---- CPU ------------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_entry(lgu):
    from tests.test_abi import declared_symbols
    lib = ctypes.CDLL(lgu._lib._build.SO_PATH)
    assert ENTRY in declared_symbols() and hasattr(lib, ENTRY)
    sig = lgu._lib.SIGNATURES[ENTRY]
    assert sig[0] is lgu._lib.Conv3Args and issubclass(sig[0], ctypes.Structure) and sig[1] is ctypes.c_void_p
    assert [f[0] for f in sig[0]._fields_] == ["x", "wpack", "bias", "out", "N", "H", "W", "Cout", "flags"]
    assert ctypes.sizeof(sig[0]) == 4 * 8 + 5 * 4 + 4
    assert "conv3.hip" in lgu._build.SOURCES
    assert lgu.Conv3 is lgu.conv3.Conv3 and lgu.Conv3Stack is lgu.conv3.Conv3Stack
    text = open(os.path.join(ROOT, "include", "lgu_corr.h")).read()
    for cout in COUTS:
        assert lgu.conv3.WPACK_HALVES[cout] == 9 * 4 * (cout // 16) * 64 * 8
        assert "#define LGU_CONV3_WPACK_HALVES_%d %d\n" % (cout, lgu.conv3.WPACK_HALVES[cout]) in text
    assert "#define LGU_CONV3_X_HALF %d " % lgu.conv3.X_HALF in text and "#define LGU_CONV3_RELU %d " % lgu.conv3.RELU in text
    assert set(lgu.conv3.MIN_FUSED_PIXELS) == set(COUTS)


@pytest.mark.parametrize("cout", COUTS)
def test_pack_puts_every_weight_in_its_documented_slot_and_nothing_else(lgu, cout):
    g = torch.Generator().manual_seed(5)
    w = torch.randn((cout, 128, 3, 3), generator=g)
    b = torch.randn((cout,), generator=g)
    wpack, bias_h = lgu.conv3.pack_conv3(w, b)
    assert wpack.dtype == torch.float16 and wpack.is_contiguous() and wpack.numel() == lgu.conv3.WPACK_HALVES[cout]
    assert tuple(wpack.shape) == (9, 4, cout // 16, 64, 8) and same_bits(bias_h, b.half())
    # a weight tensor that names its own index: the value at (co, c, ky, kx) is its flat index, exact in int32
    idx = torch.arange(cout * 128 * 9, dtype=torch.int32).view(cout, 128, 3, 3)
    t, kc, ct, lane, j = torch.meshgrid(torch.arange(9), torch.arange(4), torch.arange(cout // 16), torch.arange(64),
                                        torch.arange(8), indexing="ij")
    co, c, ky, kx = 16 * ct + (lane & 15), 32 * kc + 8 * (lane >> 4) + j, t // 3, t % 3
    slot_src = idx[co, c, ky, kx]                                  # which weight the documented formula puts in each slot
    assert sorted(slot_src.flatten().tolist()) == list(range(cout * 128 * 9))   # every weight once, nothing else
    assert same_bits(wpack, w.half()[co, c, ky, kx])
    with pytest.raises(RuntimeError, match="weight must be"):
        lgu.conv3.pack_conv3(w[:, :64], b)
    with pytest.raises(RuntimeError, match="weight must be"):
        lgu.conv3.pack_conv3(torch.zeros(32, 128, 3, 3), torch.zeros(32))
    with pytest.raises(RuntimeError, match="weight must be"):
        lgu.conv3.pack_conv3(torch.zeros(cout, 128, 1, 1), b)
    with pytest.raises(RuntimeError, match="bias must be"):
        lgu.conv3.pack_conv3(w, b[:-1])


@pytest.mark.parametrize("cout,shape", [(64, (1, 1, 1)), (128, (1, 2, 3)), (64, (2, 9, 33))])
def test_restatement_equals_float64_conv2d_on_the_rounded_operands(cout, shape):
    m, x, s64, S = case(cout, shape)
    F = torch.nn.functional
    xh, wh, bh = R.h64(x), R.h64(m.weight), R.h64(m.bias)
    s = F.conv2d(xh, wh, bh, padding=1)
    Sc = F.conv2d(xh.abs(), wh.abs(), bh.abs(), padding=1)
    # the operands are half values, so every product is exact in float64; the two sums differ in order only
    assert bool(((s - s64).abs() <= 2.0 ** -44 * S).all()) and bool(((Sc - S).abs() <= 2.0 ** -44 * S).all())
    assert bool((S >= s64.abs()).all()) and bool((R.allowance(s64, S, R.TERMS) > 0).all())
    assert R.TERMS == RF.TERMS2 == 1154
    assert bool((x == 0).any()) and float(x.abs().max()) > 2.0
    # the stack's chain is the same construction: one eligible layer alone gives the layer's own sums and allowance
    ref, bound = R.stack(x, torch.nn.Sequential(m))
    assert bool(((ref - s64).abs() <= 2.0 ** -44 * S).all())
    assert bool(((bound - R.allowance(s64, S, R.TERMS)).abs() <= 1e-12 * bound).all())


def _cpu_module_cases():
    yield "conv64", R.make_conv(3, 64), R.make_input(1, 2, 5, 7), 2
    yield "conv128", R.make_conv(4, 128), R.make_input(2, 1, 4, 9), 2
    for kind in STACKS:
        yield kind, R.make_stack(7, kind), R.make_input(3, 1, 5, 6, C=R.COR_PLANES if kind == "corr_encoder" else 128), 4


@pytest.mark.parametrize("name,m,x,nparams", [pytest.param(*c, id=c[0]) for c in _cpu_module_cases()])
def test_cpu_inputs_reach_the_module_and_install_keeps_the_state_dict(lgu, name, m, x, nparams):
    C = lgu.conv3
    keys = list(m.state_dict().keys())
    cls = C.Conv3 if isinstance(m, torch.nn.Conv2d) else C.Conv3Stack
    with torch.no_grad():
        want = m(x.clone())
        direct = cls(m)
        assert same_bits(direct(x.clone()), want) and direct.fused_calls == 0
        wr = C.install(m)
        assert isinstance(wr, cls) and m.forward is wr and C.install(m) is wr
        assert list(m.state_dict().keys()) == keys and len(list(m.parameters())) == nparams
        got = m(x.clone())
    want_grad = m(x.clone().requires_grad_())
    assert want_grad.requires_grad and same_bits(want_grad, want)
    C.uninstall(m)
    assert "forward" not in m.__dict__ and list(m.state_dict().keys()) == keys
    assert wr.fused_calls == 0 and same_bits(got, want)
    if cls is C.Conv3:
        with torch.no_grad():
            assert same_bits(C.Conv3(m, relu=True)(x.clone()), torch.relu(want))


def test_install_update_on_cpu_keeps_the_module(lgu):
    C = lgu.conv3
    u = R.make_update(11)
    keys, nparams = list(u.state_dict().keys()), len(list(u.parameters()))
    net, corr, motn = R.make_input(1, 2, 4, 5), R.make_input(2, 2, 4, 5, C=R.COR_PLANES), RF.make_input(3, 2, 4, 5)

    def run():
        with torch.no_grad():
            return [u.corr_encoder(corr.clone()), u.flow_encoder(motn.clone()), u.delta(net.clone()), u.weight(net.clone()),
                    u.agg(net.clone())]
    want = run()
    for with_flow in (False, True):
        if with_flow:
            lgu.flow.install(u.flow_encoder)
        wrs = C.install_update(u)
        assert list(wrs) == ["corr_encoder", "flow_encoder[2]", "delta", "weight", "agg.conv1", "agg.conv2"]
        assert [type(w) for w in wrs.values()] == [C.Conv3Stack, C.Conv3, C.Conv3Stack, C.Conv3Stack, C.Conv3, C.Conv3]
        assert not any(w.relu for w in wrs.values() if isinstance(w, C.Conv3))
        assert u.corr_encoder.forward is wrs["corr_encoder"] and u.flow_encoder[2].forward is wrs["flow_encoder[2]"]
        assert u.agg.conv2.forward is wrs["agg.conv2"]
        again = C.install_update(u)
        assert all(again[k] is wrs[k] for k in wrs)
        assert list(u.state_dict().keys()) == keys and len(list(u.parameters())) == nparams
        assert all(same_bits(a, b) for a, b in zip(run(), want))
        assert u.delta(net.clone().requires_grad_()).requires_grad
        assert all(w.fused_calls == 0 for w in wrs.values())
        C.uninstall_update(u)
        for m in (u.corr_encoder, u.flow_encoder[2], u.delta, u.weight, u.agg.conv1, u.agg.conv2):
            assert "forward" not in m.__dict__
        if with_flow:
            assert isinstance(u.flow_encoder.forward, lgu.flow.FlowEncoder)     # flow's own wrapper is left alone
            lgu.flow.uninstall(u.flow_encoder)
    assert list(u.state_dict().keys()) == keys and all(same_bits(a, b) for a, b in zip(run(), want))
    # an object without the six sites is refused before anything is bound
    u.agg.conv2 = torch.nn.Conv2d(128, 128, 1)
    with pytest.raises(RuntimeError, match="install_update: agg.conv2"):
        C.install_update(u)
    assert "forward" not in u.corr_encoder.__dict__ and "forward" not in u.agg.conv1.__dict__


def test_construction_and_install_refuse_other_architectures(lgu):
    nn, C = torch.nn, lgu.conv3
    C.Conv3(nn.Conv2d(128, 64, 3, padding=1))
    C.Conv3Stack(nn.Sequential(nn.Conv2d(128, 128, 3, padding=1)))
    bad_convs = [nn.Conv2d(64, 128, 3, padding=1), nn.Conv2d(128, 32, 3, padding=1), nn.Conv2d(128, 128, 3, padding=0),
                 nn.Conv2d(128, 128, 3, padding=1, stride=2), nn.Conv2d(128, 128, 3, padding=1, bias=False),
                 nn.Conv2d(128, 128, 3, padding=1, dilation=2)]
    for m in bad_convs:
        with pytest.raises(RuntimeError, match="Conv3: the module must be"):
            C.Conv3(m)
        with pytest.raises(RuntimeError, match="Conv3: the module must be"):
            C.install(m)
        seq = nn.Sequential(m, nn.ReLU())
        with pytest.raises(RuntimeError, match="Conv3Stack: the module must be"):
            C.Conv3Stack(seq)
        with pytest.raises(RuntimeError, match="Conv3Stack: the module must be"):
            C.install(seq)
        assert "forward" not in m.__dict__ and "forward" not in seq.__dict__
    no_conv = nn.Sequential(nn.Conv2d(R.COR_PLANES, 128, 1), nn.ReLU(), nn.Conv2d(128, 2, 3, padding=1))
    with pytest.raises(RuntimeError, match="Conv3Stack: the module must be"):
        C.install(no_conv)
    with pytest.raises(RuntimeError, match="Conv3Stack: the module must be"):
        C.Conv3Stack(nn.Conv2d(128, 128, 3, padding=1))
    assert "forward" not in no_conv.__dict__
    other = nn.Linear(128, 128)
    with pytest.raises(RuntimeError, match="must be a Conv2d or an nn.Sequential"):
        C.install(other)
    assert "forward" not in other.__dict__
    fe = RF.make_module(1)
    fwr = lgu.flow.install(fe)
    with pytest.raises(RuntimeError, match="already carries a FlowEncoder"):
        C.install(fe)
    assert fe.forward is fwr and isinstance(C.install(fe[2]), C.Conv3)
    C.uninstall(fe[2])
    lgu.flow.uninstall(fe)
    assert "forward" not in fe.__dict__ and "forward" not in fe[2].__dict__


def test_operator_refusals_in_their_order(lgu):
    """Shape of x, pack size, bias shape, contiguity, dtypes, no-grad, device: each refusal's text, and which of two
    defects is reported.  None of them touches a device."""
    f = lgu.conv3.conv3x3
    H = torch.float16

    def z(*shape, dtype=torch.float32):
        return torch.zeros(shape, dtype=dtype)

    def nc(t):
        return torch.zeros(tuple(t.shape) + (2,), dtype=t.dtype)[..., 0]

    for cout in COUTS:
        x, wp, bh = z(1, 128, 2, 2), z(9, 4, cout // 16, 64, 8, dtype=H), z(cout, dtype=H)
        other = 192 - cout
        no_grad = "conv3x3 has no autograd: its outputs would carry no gradient. Call it under torch.no_grad() or pass detached inputs"
        cases = [
            ((x, wp, bh), "x" + _NO_CPU),
            ((x.half(), wp, bh), "x" + _NO_CPU),
            ((z(1, 127, 2, 2), wp, bh), "x must be (N,128,H,W), got (1, 127, 2, 2)"),
            ((z(128, 2, 2), wp, bh), "x must be (N,128,H,W), got (128, 2, 2)"),
            ((x, z(9, 4, cout // 16, 64, 7, dtype=H), bh), "wpack must hold 73728 or 147456 halves (pack_conv3), got (9, 4, %d, 64, 7)"
             % (cout // 16)),
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
            ((nc(x), z(5, dtype=H), bh), "wpack must hold 73728 or 147456 halves (pack_conv3), got (5,)"),
            ((nc(x), wp, z(other, dtype=H)), "bias_h must be (%d,), got (%d,)" % (cout, other)),
            ((x.double(), wp, nc(bh)), "bias_h must be contiguous"),
            ((x.clone().requires_grad_(), wp, bh.float()), "expected scalar type Half but found Float (bias_h)"),
            ((x.double().requires_grad_(), wp, bh), "expected scalar type Float or Half but found Double (x)"),
        ]
        for args, message in cases:
            for relu in (False, True):
                with pytest.raises(RuntimeError) as info:
                    f(*args, relu=relu)
                assert type(info.value) is RuntimeError and str(info.value) == message
        with torch.no_grad():      # grad mode off: the no-grad refusal does not apply, the device refusal is next
            with pytest.raises(RuntimeError) as info:
                f(x.clone().requires_grad_(), wp, bh)
            assert str(info.value) == "x" + _NO_CPU


# ---- GPU ------------------------------------------------------------------------------------------------------------
@pytest.fixture
def no_threshold(lgu, monkeypatch):
    """The wrappers' routing by size follows a measurement (MIN_FUSED_PIXELS); these tests are about the fused path."""
    monkeypatch.setattr(lgu.conv3, "MIN_FUSED_PIXELS", {64: 0, 128: 0})


def _need_gpu(lgu):
    assert torch.cuda.is_available(), "these tests need the MI355X"
    assert os.path.exists(lgu._lib.so_path()), "liblgu_corr.so missing — run __graft_entry__.build()"


def _packed(lgu, m):
    return lgu.conv3.pack_conv3(m.weight.detach().cuda(), m.bias.detach().cuda())


IMPULSE_AT = [(2, 2), (0, 0), (0, 4), (4, 0), (4, 4)]
IMPULSE_CH = [0, 31, 32, 127]


@pytest.mark.gpu
@pytest.mark.parametrize("cout", COUTS)
def test_impulses_give_the_weights_bit_for_bit(lgu, cout):
    """One input element = 1 (centre and the four corners of a 5x5 image, channels 0, 31, 32 and 127), bias 0: a single
    product is exact, so every output is act(w_h[co, c, cy-y+1, cx-x+1]) and 0 outside the window."""
    _need_gpu(lgu)
    m = R.make_conv(43, cout)
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
    for relu in (False, True):
        got = lgu.conv3.conv3x3(x.cuda(), wpack, bias_h, relu=relu)
        got_h = lgu.conv3.conv3x3(x.half().cuda(), wpack, bias_h, relu=relu)
        torch.cuda.synchronize()
        ref = torch.relu(want) if relu else want
        assert int((ref != 0).sum()) > 0.4 * 4 * (9 + 4 * 4) * cout     # about half the weights are positive
        assert same_bits(got, ref), "relu=%s: max |diff| %g" % (relu, float((got.cpu().float() - ref.float()).abs().max()))
        assert same_bits(got_h, ref)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("cout", COUTS)
def test_zero_input_gives_act_of_the_bias_everywhere(lgu, cout, shape):
    _need_gpu(lgu)
    m = R.make_conv(40 + cout, cout)
    wpack, bias_h = _packed(lgu, m)
    x = torch.zeros((shape[0], 128) + shape[1:], device="cuda")
    bh = m.bias.detach().half().view(1, cout, 1, 1).expand(shape[0], cout, *shape[1:])
    assert bool((bh < 0).any()) and bool((bh > 0).any())
    for relu in (False, True):
        got = lgu.conv3.conv3x3(x, wpack, bias_h, relu=relu)
        torch.cuda.synchronize()
        assert same_bits(got, torch.relu(bh) if relu else bh), relu


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("cout", COUTS)
def test_every_element_is_within_the_derived_bound(lgu, cout, shape):
    _need_gpu(lgu)
    m, x, s64, S = case(cout, shape)
    wpack, bias_h = _packed(lgu, m)
    bound = R.allowance(s64, S, R.TERMS)
    xc = x.cuda()
    mc = R.make_conv(40 + cout, cout).cuda()
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        own = mc(xc)
    for relu in (False, True):
        ref = R.act(s64, relu)
        want = R.act(s64.to(torch.float16), relu)
        got = lgu.conv3.conv3x3(xc, wpack, bias_h, relu=relu)
        from_half = lgu.conv3.conv3x3(xc.half(), wpack, bias_h, relu=relu)
        rounded = lgu.conv3.conv3x3(xc.half().float(), wpack, bias_h, relu=relu)
        torch.cuda.synchronize()
        own_r = torch.relu(own) if relu else own
        err = (got.cpu().double() - ref).abs()
        err_own = (own_r.cpu().double() - ref).abs()
        print("conv3x3 Cout %d %s relu=%s: worst error %.3g of its bound, %.4f of the elements are the restatement's bits; the "
              "module's own forward: worst %.3g of the bound, %.4f bit-identical to the kernel"
              % (cout, shape, relu, float((err / bound).max()), float((got.cpu() == want).double().mean()),
                 float((err_own / bound).max()), float((own_r == got).double().mean())))
        assert got.dtype == torch.float16 and tuple(got.shape) == (shape[0], cout) + shape[1:]
        assert bool((err <= bound).all()), float((err / bound).max())
        assert same_bits(from_half, rounded) and same_bits(from_half, got)   # fp32 x is rounded to half exactly once
        errh = (from_half.cpu().double() - ref).abs()
        assert bool((errh <= bound).all()), float((errh / bound).max())


# a border pixel, a pixel on a tile edge (x = 31 | 32 and 63 | 64, y = 3 | 4 and 1 | 2) and an interior one
NAN_AT = [((2, 9, 33), [(1, 5, 0, 32), (0, 64, 3, 31), (1, 127, 4, 16)]),
          ((1, 17, 130), [(0, 0, 16, 129), (0, 33, 4, 64), (0, 90, 9, 50)]),
          ((1, 5, 65), [(0, 7, 0, 0), (0, 31, 1, 63), (0, 32, 2, 64)])]


@pytest.mark.gpu
@pytest.mark.parametrize("shape,ats", NAN_AT)
@pytest.mark.parametrize("cout", COUTS)
def test_nan_reaches_exactly_its_3x3_neighbourhood(lgu, cout, shape, ats):
    _need_gpu(lgu)
    m, x, _, _ = case(cout, shape)
    wpack, bias_h = _packed(lgu, m)
    clean = lgu.conv3.conv3x3(x.cuda(), wpack, bias_h, relu=True).cpu()
    for at in ats:
        xn = x.clone()
        xn[at] = float("nan")
        got = lgu.conv3.conv3x3(xn.cuda(), wpack, bias_h, relu=True).cpu()
        n, _, cy, cx = at
        want = torch.zeros((shape[0], 1) + shape[1:], dtype=torch.bool)
        want[n, 0, max(cy - 1, 0):cy + 2, max(cx - 1, 0):cx + 2] = True
        assert bool((torch.isnan(got) == want.expand_as(got)).all()), at
        assert bool((got.view(torch.int16) == clean.view(torch.int16))[~want.expand_as(got)].all()), at


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(3, 16, 40), (3, 9, 33), (2, 5, 65)])
@pytest.mark.parametrize("cout", COUTS)
def test_an_image_does_not_depend_on_its_batch(lgu, cout, shape):
    _need_gpu(lgu)
    m = R.make_conv(40 + cout, cout)
    x = R.make_input(77, *shape).cuda()
    wpack, bias_h = _packed(lgu, m)
    got = lgu.conv3.conv3x3(x, wpack, bias_h)
    for k in range(shape[0]):
        assert same_bits(got[k:k + 1], lgu.conv3.conv3x3(x[k:k + 1].contiguous(), wpack, bias_h)), k


def _c_call(lgu, x, wpack, bias_h, out, relu=True):
    N, _, H, W = x.shape
    flags = (lgu.conv3.X_HALF if x.dtype == torch.float16 else 0) | (lgu.conv3.RELU if relu else 0)
    args = lgu._lib.Conv3Args(x.data_ptr(), wpack.data_ptr(), bias_h.data_ptr(), out.data_ptr(), N, H, W, out.shape[1], flags)
    rc = lgu._lib.load().lgu_conv3x3_c128_h16(args, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc


@pytest.mark.gpu
@pytest.mark.parametrize("half_x", (False, True))
@pytest.mark.parametrize("shape", [(2, 9, 33), (3, 16, 40)])
@pytest.mark.parametrize("cout", COUTS)
def test_guard_bands_and_alignment(lgu, no_threshold, cout, shape, half_x):
    """The alignment audit of DESIGN.md §4.1 for lgu_conv3x3_c128_h16: x, bias and out are served at element alignment
    with the aligned call's bits (out by element stores when it is not 16-byte aligned or W % 8 != 0), a wpack that is
    not 16-byte aligned is refused with nothing launched, and so is a Cout outside {64, 128}."""
    from tests.alignment_cases import guards_intact, shifted
    _need_gpu(lgu)
    m, x, _, _ = case(cout, shape)
    wpack, bias_h = _packed(lgu, m)
    xc = x.cuda().half() if half_x else x.cuda()
    base = {"x": xc, "wpack": wpack, "bias": bias_h,
            "out": torch.empty((shape[0], cout) + shape[1:], dtype=torch.float16, device="cuda")}
    assert all(t.data_ptr() % 16 == 0 for t in base.values())
    assert _c_call(lgu, base["x"], base["wpack"], base["bias"], base["out"]) == 0
    want = base["out"].clone()
    assert same_bits(want, lgu.conv3.conv3x3(xc, wpack, bias_h, relu=True))
    xs = (2, 8) if half_x else (4, 8)
    variants = [(k, s) for k, ss in (("x", xs), ("bias", (2, 4, 8)), ("out", (2, 4, 8)), ("wpack", (2, 4, 8))) for s in ss]
    for key, shift in variants + [("all", 0), ("all but wpack", 0)]:
        keys = [key] if key in base else [k for k in base if key == "all" or k != "wpack"]
        args = dict(base)
        for k in keys:
            args[k] = shifted(base[k], shift if key in base else base[k].element_size())
        before = {k: args[k].clone() for k in args}
        rc = _c_call(lgu, args["x"], args["wpack"], args["bias"], args["out"])
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
    # a Cout the kernel does not serve: refused, out untouched; N == 0: nothing launched
    out = shifted(base["out"], 0)
    before = out.clone()
    a = lgu._lib.Conv3Args(xc.data_ptr(), wpack.data_ptr(), bias_h.data_ptr(), out.data_ptr(), shape[0], shape[1], shape[2], 96,
                           lgu.conv3.X_HALF if half_x else 0)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert lgu._lib.load().lgu_conv3x3_c128_h16(a, stream) == lgu._lib.LGU_E_UNSUPPORTED
    a.Cout, a.N = cout, 0
    assert lgu._lib.load().lgu_conv3x3_c128_h16(a, stream) == 0
    torch.cuda.synchronize()
    assert same_bits(out, before) and guards_intact(out)
    assert tuple(lgu.conv3.conv3x3(xc[:0], wpack, bias_h).shape) == (0, cout) + shape[1:]
    with pytest.raises(RuntimeError, match=r"conv3x3: empty frame \(H\*W = 0\)"):
        lgu.conv3.conv3x3(xc[:, :, :0], wpack, bias_h)
    # the class serves every contiguous input
    mc = R.make_conv(40 + cout, cout).cuda()
    wr = lgu.conv3.Conv3(mc, relu=True)
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        first = wr(base["x"])
        for shift in xs:
            xsh = shifted(base["x"], shift)
            assert same_bits(wr(xsh), first) and same_bits(xsh, base["x"]) and guards_intact(xsh)
    assert wr.fused_calls == 3 and same_bits(first, want)


STACK_SHAPE = (2, 9, 33)


def _stack_input(kind):
    return R.make_input(21, *STACK_SHAPE, C=R.COR_PLANES if kind == "corr_encoder" else 128)


def _modes(wr, xc, calls):
    """What autocast off, a bfloat16 autocast and a grad input return through `wr`; `calls`: the counter before."""
    with torch.no_grad():
        plain = wr(xc)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            bf = wr(xc)
    with torch.autocast("cuda", dtype=torch.float16):
        grad = wr(xc.clone().requires_grad_())
    assert wr.fused_calls == calls and plain.dtype == torch.float32 and bf.dtype == torch.bfloat16 and grad.requires_grad
    assert grad.dtype == torch.float16


@pytest.mark.gpu
@pytest.mark.parametrize("kind", STACKS)
def test_stack_is_within_the_propagated_bound(lgu, no_threshold, monkeypatch, kind):
    _need_gpu(lgu)
    C = lgu.conv3
    m = R.make_stack(51, kind)
    x = _stack_input(kind)
    with torch.no_grad():
        ref, bound = R.stack(x, m)
    mc = R.make_stack(51, kind).cuda()
    xc = x.cuda()
    wr = C.Conv3Stack(mc)
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        own = mc(xc.clone())
        got = wr(xc)
        assert wr.fused_calls == 1                       # each of the three holds one eligible convolution
        if kind != "corr_encoder":                       # the first member is the fused layer: a half input is used as it is
            assert same_bits(wr(xc.half()), got)
            assert wr.fused_calls == 2
    calls = wr.fused_calls
    _modes(wr, xc, calls)
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        assert C.install(mc) is mc.forward
        installed = mc(xc)
        assert mc.forward.fused_calls == 1
        C.uninstall(mc)
        # below the measured threshold of its Cout a convolution is called as itself
        monkeypatch.setattr(C, "MIN_FUSED_PIXELS", {64: 1 << 40, 128: 1 << 40})
        routed = wr(xc)
        assert wr.fused_calls == calls and same_bits(routed, own)
    torch.cuda.synchronize()
    cout = 128 if kind == "corr_encoder" else 2
    assert got.dtype == own.dtype == torch.float16 and got.shape == own.shape == (STACK_SHAPE[0], cout) + STACK_SHAPE[1:]
    assert same_bits(installed, got)
    err, err_own = (got.cpu().double() - ref).abs(), (own.cpu().double() - ref).abs()
    print("Conv3Stack %s: worst error %.3g of the bound; the module's own forward %.3g; %.4f of the elements bit-identical"
          % (kind, float((err / bound).max()), float((err_own / bound).max()), float((got == own).double().mean())))
    assert bool((err <= bound).all()), float((err / bound).max())
    assert bool((err_own <= bound).all()), float((err_own / bound).max())


@pytest.mark.gpu
def test_install_update_under_autocast(lgu, no_threshold):
    _need_gpu(lgu)
    C = lgu.conv3
    u = R.make_update(61)
    uc = R.make_update(61).cuda()
    net, corr, motn = R.make_input(1, *STACK_SHAPE), R.make_input(2, *STACK_SHAPE, C=R.COR_PLANES), RF.make_input(3, *STACK_SHAPE)
    netc, corrc, motnc = net.cuda(), corr.cuda(), motn.cuda()

    def run():
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
            return {"corr_encoder": uc.corr_encoder(corrc), "flow_encoder": uc.flow_encoder(motnc), "delta": uc.delta(netc),
                    "weight": uc.weight(netc), "agg": uc.agg(netc)}
    own = run()
    wrs = C.install_update(uc)
    got = run()
    # corr_encoder, flow_encoder[2], delta, weight: one eligible convolution each; agg: conv1 and conv2
    assert [w.fused_calls for w in wrs.values()] == [1, 1, 1, 1, 1, 1]
    with torch.no_grad():
        bounds = {k: R.stack(x, getattr(u, k)) for k, x in (("corr_encoder", corr), ("flow_encoder", motn), ("delta", net),
                                                           ("weight", net))}
        # agg: relu(conv1), the mean over the edges (an fp32 sum of 2 halves, rounded once: half a unit of the mean on top
        # of the mean of the allowances), relu(conv2)
        r1, b1 = R.stack(net, torch.nn.Sequential(u.agg.conv1, u.agg.relu))
        mean = r1.mean(dim=0, keepdim=True)
        bmean = b1.mean(dim=0, keepdim=True)
        bmean = bmean + 2.0 ** -11 * (mean.abs() + bmean) + 2.0 ** -25
        wh, bh = R.h64(u.agg.conv2.weight), R.h64(u.agg.conv2.bias)
        s2, S2 = R.window_sums(mean, wh, bh, 1)
        moved = R.through(bmean, wh, 1)
        bounds["agg"] = (torch.relu(s2), moved + R.allowance(s2, S2 + moved, R.TERMS) + 2.0 ** -11 * moved)
    for k, (ref, bound) in bounds.items():
        err, err_own = (got[k].cpu().double() - ref).abs(), (own[k].cpu().double() - ref).abs()
        print("install_update %s: worst error %.3g of the bound; the module's own forward %.3g; %.4f bit-identical"
              % (k, float((err / bound).max()), float((err_own / bound).max()), float((got[k] == own[k]).double().mean())))
        assert got[k].dtype == own[k].dtype == torch.float16 and got[k].shape == own[k].shape
        assert bool((err <= bound).all()), (k, float((err / bound).max()))
        assert bool((err_own <= bound).all()), (k, float((err_own / bound).max()))
    # the installed call is the wrapper's call
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        assert same_bits(wrs["delta"](netc), got["delta"]) and same_bits(wrs["weight"](netc), got["weight"])
        assert same_bits(wrs["corr_encoder"](corrc), got["corr_encoder"])
        assert same_bits(torch.relu(wrs["agg.conv1"](netc)), torch.relu(uc.agg.conv1(netc)))
    calls = {k: w.fused_calls for k, w in wrs.items()}
    assert calls == {"corr_encoder": 2, "flow_encoder[2]": 1, "delta": 2, "weight": 2, "agg.conv1": 3, "agg.conv2": 1}
    for k in ("delta", "agg.conv1"):
        _modes(wrs[k], netc, calls[k])
    # with flow.install also on: FlowEncoder over a Conv3 on [2]
    fwr = lgu.flow.install(uc.flow_encoder)
    assert C.install_update(uc)["flow_encoder[2]"] is wrs["flow_encoder[2]"]
    twin = R.make_update(61).cuda().flow_encoder
    direct = lgu.flow.FlowEncoder(twin)
    c3 = C.install(twin[2])
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        both = uc.flow_encoder(motnc)
        want = direct(motnc)
    torch.cuda.synchronize()
    assert fwr.fused_calls == 1 and direct.fused_calls == 1 and c3.fused_calls == 1 and wrs["flow_encoder[2]"].fused_calls == 2
    assert same_bits(both, want)
    ref, bound = bounds["flow_encoder"]
    assert bool(((both.cpu().double() - ref).abs() <= bound).all())
    C.uninstall_update(uc)
    lgu.flow.uninstall(uc.flow_encoder)
    assert all(same_bits(a, b) for a, b in zip(run().values(), own.values()))
