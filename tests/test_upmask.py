"""GraphAgg's upmask layer, alone and fused with the convex upsampling (lgu_slam_amd.upmask, csrc/upmask.hip), against the
float64 restatement tests/upmask_restatement.py.

Numerics contract (include/lgu_corr.h):
- a single product is exact: impulses and the zero input are bit for bit half(b_h + x_h·w_h);
- every element of h = half(s): |h - s64| <= conv3_restatement.allowance(s64, S, terms=130), S = Σ|x_h·w_h| + |b_h|: fp32
  accumulation in any order, one half rounding, the half subnormal floor;
- the fused form is the float64 upsample restatement evaluated on the eager kernel's OWN h bits within the tolerances
  upsample_disps_ is held to: 4e-6·max_k|d_k| with float weights; with half weights, additionally at most
  2e-3 of the outputs off by one half ulp of a weight.  A half ulp of a mask value moves a weight by ~5e-4 relative, so
  this fails if the two kernels' GEMMs differ in a bit; it also fails with the weight-rounding flag swapped;
- a NaN reaches exactly its pixel (576 outputs, or the 8x8 block); a frame's bits do not depend on the batch.
The module's own autocast forward is not held to the single-layer bound; the test prints where it sits.
The GPU tests build their modules themselves and never read the reference tree.
"""
import ctypes
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import aggregate_restatement as RA  # noqa: E402
from tests import conv3_restatement as R  # noqa: E402
from tests import upmask_restatement as RU  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("lgu_upmask1x1_c128_h16", "lgu_upmask_upsample_f32")
# the issue's shapes: the smallest at which a group of 16 pixels can go wrong (H * W = 51 and 165: groups span frames and
# rows).  A workgroup takes a contiguous range of groups, one while there are at most 2 x 256 CUs of them; (4,67,71) has
# 1190 groups, three per workgroup on an MI355X, so that both staging buffers are reused
SHAPES = [(1, 1, 1), (1, 2, 3), (1, 1, 16), (2, 3, 17), (1, 5, 33), (3, 4, 16), (1, 6, 80)]
BIG = (4, 67, 71)
ALL_SHAPES = SHAPES + [BIG]
GAIN = 3.0          # mask values of spread ~3, the range tests/test_aggregate.py draws
_CASES = {}
_NO_CPU = " must be a HIP device tensor: lgu_slam_amd has no CPU fallback"


def same_bits(a, b):
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    iv = torch.int16 if a.element_size() == 2 else torch.int32
    return bool(torch.equal(a.view(iv), b.view(iv)))


def case(shape):
    """(module, x, s64, S, disps) on the CPU for one shape, computed once and never changed."""
    if shape not in _CASES:
        m = RU.make_upmask(41, GAIN)
        x = R.make_input(3000 + shape[1] * shape[2], *shape)
        with torch.no_grad():
            c = RU.conv_of(m)
            _CASES[shape] = (m, x) + RU.layer(x, c.weight, c.bias) + (RU.disparities(7 + shape[2], shape[0] + 2, *shape[1:]),)
    return _CASES[shape]


def indices(U):
    """U distinct rows of the U + 2 disparity frames, in descending order: U + 1, U, ..., 2 (rows 0 and 1 stay unnamed)."""
    return torch.tensor([U + 1 - u for u in range(U)], dtype=torch.int64)


# ---- CPU ------------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_entries(lgu):
    from tests.test_abi import declared_symbols
    lib = ctypes.CDLL(lgu._lib._build.SO_PATH)
    L, M = lgu._lib, lgu.upmask
    for e in ENTRIES:
        assert e in declared_symbols() and hasattr(lib, e) and e in L.SIGNATURES
    sig = L.SIGNATURES[ENTRIES[0]]
    assert sig[0] is L.UpmaskArgs and issubclass(sig[0], ctypes.Structure) and sig[1] is ctypes.c_void_p
    assert [f[0] for f in sig[0]._fields_] == ["x", "wpack", "bias", "out", "N", "H", "W", "flags"]
    assert ctypes.sizeof(sig[0]) == 4 * 8 + 4 * 4
    sig = L.SIGNATURES[ENTRIES[1]]
    assert sig[0] is L.UpmaskUpsArgs and issubclass(sig[0], ctypes.Structure) and sig[1] is ctypes.c_void_p
    assert [f[0] for f in sig[0]._fields_] == ["x", "wpack", "bias", "disps", "ix", "disps_up", "U", "N", "ht", "wd", "flags"]
    assert ctypes.sizeof(sig[0]) == 6 * 8 + 5 * 4 + 4
    assert "upmask.hip" in lgu._build.SOURCES
    assert lgu.Upmask is M.Upmask
    text = open(os.path.join(ROOT, "include", "lgu_corr.h")).read()
    assert M.WPACK_HALVES == 576 * 128 == 36 * 4 * 64 * 8 and M.COUT == 576 and M.CIN == 128
    assert "#define LGU_UPMASK_WPACK_HALVES %d\n" % M.WPACK_HALVES in text
    assert "#define LGU_UPMASK_COUT %d\n" % M.COUT in text
    assert "#define LGU_UPMASK_X_HALF %d " % M.X_HALF in text
    assert "#define LGU_UPS_HALF_WEIGHTS %d\n" % M.UPS_HALF_WEIGHTS in text and M.UPS_HALF_WEIGHTS == lgu.aggregate.UPS_HALF_WEIGHTS
    assert M.X_HALF & M.UPS_HALF_WEIGHTS == 0
    assert isinstance(M.MIN_FUSED_PIXELS, int) and M.MIN_FUSED_PIXELS >= 0


def test_pack_puts_every_weight_in_its_documented_slot_and_nothing_else(lgu):
    g = torch.Generator().manual_seed(5)
    w = torch.randn((576, 128, 1, 1), generator=g)
    b = torch.randn((576,), generator=g)
    wpack, bias_h = lgu.upmask.pack_upmask(w, b)
    assert wpack.dtype == torch.float16 and wpack.is_contiguous() and wpack.numel() == lgu.upmask.WPACK_HALVES
    assert tuple(wpack.shape) == (36, 4, 64, 8) and same_bits(bias_h, b.half())
    # a weight tensor that names its own index: the value at (co, c) is its flat index, exact in int32
    idx = torch.arange(576 * 128, dtype=torch.int32).view(576, 128)
    mt, kc, lane, j = torch.meshgrid(torch.arange(36), torch.arange(4), torch.arange(64), torch.arange(8), indexing="ij")
    co, c = 16 * mt + (lane & 15), 32 * kc + 8 * (lane >> 4) + j
    assert sorted(idx[co, c].flatten().tolist()) == list(range(576 * 128))      # every weight once, so nothing else
    assert same_bits(wpack, w.half()[co, c, 0, 0])
    for bad_w, bad_b, what in ((w[:, :64], b, "weight"), (w[:575], b[:575], "weight"), (torch.zeros(576, 128, 3, 3), b, "weight"),
                               (w[:, :, 0, 0], b, "weight"), (w, torch.zeros(577), "bias")):
        with pytest.raises(RuntimeError, match=what + " must be"):
            lgu.upmask.pack_upmask(bad_w, bad_b)


@pytest.mark.parametrize("shape", [(1, 1, 1), (2, 3, 17), (1, 6, 80)])
def test_restatement_equals_float64_conv2d_on_the_rounded_operands(shape):
    m, x, s64, S, disps = case(shape)
    F = torch.nn.functional
    c = RU.conv_of(m)
    xh, wh, bh = R.h64(x), R.h64(c.weight), R.h64(c.bias)
    s = F.conv2d(xh, wh, bh)
    Sc = F.conv2d(xh.abs(), wh.abs(), bh.abs())
    # the operands are half values, so every product is exact in float64; the two sums differ in order only
    assert bool(((s - s64).abs() <= 2.0 ** -44 * S).all()) and bool(((Sc - S).abs() <= 2.0 ** -44 * S).all())
    assert bool((S >= s64.abs()).all()) and bool((R.allowance(s64, S, RU.TERMS) > 0).all())
    assert RU.TERMS == 128 * 1 * 1 + 2 == 130
    # the mask values have the spread of tests/test_aggregate.py's recipe
    if s64.numel() > 10000:
        assert 2.0 < float(s64.std()) < 4.5
    # the upsample part is tests/aggregate_restatement.py applied to the given mask, rows selected by ix
    h = s64.to(torch.float16)
    U = shape[0]
    ix = indices(U)
    ix_bad = torch.cat([ix, torch.tensor([-1, U + 2])])
    hh = torch.cat([h, h[:1], h[:1]])
    for hw in (False, True):
        rows, want, bound = RU.upsample(disps.numpy(), ix_bad.numpy(), hh.numpy(), hw)
        assert rows.tolist() == ix.tolist() and want.shape == bound.shape == (U, 8 * shape[1], 8 * shape[2])
        direct = RA.cvx_upsample64(disps.numpy()[ix.numpy()], h.float().numpy(), hw)
        assert np.array_equal(want, direct)


@pytest.mark.parametrize("shape", ALL_SHAPES)
def test_the_two_restatement_roundings_alone_stay_under_the_flip_cap(shape):
    """The 2e-3 cap of the half-weight comparison is a condition on the inputs: for this file's seeds, the float32 and the
    float64 restatement of the upsampling, on the restatement's own mask half(s64), stay inside the tolerance."""
    m, x, s64, S, disps = case(shape)
    h = s64.to(torch.float16).float().numpy()
    d = disps.numpy()[indices(shape[0]).numpy()]
    bound = RA.upsample_bound(d)
    for hw in (False, True):
        r = RU.upsample_ratio(RA.cvx_upsample32(d, h, hw), RA.cvx_upsample64(d, h, hw), bound)
        print("restatements %s half_weights=%s: worst %.3g of max|d|, %.3g of the outputs above %g (cap %g)"
              % (shape, hw, r.max(), (r > RU.UPS_TOL).mean(), RU.UPS_TOL, RU.HALF_FLIP_FRACTION))
        assert RU.within(r, hw), (hw, r.max(), (r > RU.UPS_TOL).mean())
    # and the other weight rounding is far outside it
    r = RU.upsample_ratio(RA.cvx_upsample32(d, h, True), RA.cvx_upsample64(d, h, False), bound)
    if r.size >= 1000:
        assert (r > RU.UPS_TOL).mean() > 0.05 and not RU.within(r, False) and not RU.within(r, True)


def _cpu_module_cases():
    yield "sequential", RU.make_upmask(3), R.make_input(1, 2, 5, 7)
    yield "conv", RU.make_upmask(4, sequential=False), R.make_input(2, 1, 4, 9)


@pytest.mark.parametrize("name,m,x", [pytest.param(*c, id=c[0]) for c in _cpu_module_cases()])
def test_cpu_inputs_reach_the_module_and_install_keeps_the_state_dict(lgu, name, m, x):
    M = lgu.upmask
    keys = list(m.state_dict().keys())
    with torch.no_grad():
        want = m(x.clone())
        direct = M.Upmask(m)
        assert same_bits(direct(x.clone()), want) and direct.fused_calls == 0
        wr = M.install(m)
        assert isinstance(wr, M.Upmask) and m.forward is wr and M.install(m) is wr
        assert list(m.state_dict().keys()) == keys and len(list(m.parameters())) == 2
        got = m(x.clone())
    want_grad = m(x.clone().requires_grad_())
    assert want_grad.requires_grad and same_bits(want_grad, want)
    M.uninstall(m)
    assert "forward" not in m.__dict__ and list(m.state_dict().keys()) == keys
    assert m.forward.__func__ is type(m).forward
    assert wr.fused_calls == 0 and same_bits(got, want) and tuple(got.shape) == (x.shape[0], 576) + tuple(x.shape[2:])
    # the cache follows the parameters
    p1 = wr.packed()
    assert wr.packed() is p1
    with torch.no_grad():
        wr.conv.weight.mul_(2.0)
    assert wr.packed() is not p1 and same_bits(wr.packed()[0], M.pack_upmask(wr.conv.weight, wr.conv.bias)[0])


def test_construction_and_install_refuse_other_architectures(lgu):
    nn, M = torch.nn, lgu.upmask

    def conv(cin=128, cout=576, k=1, **kw):
        return nn.Conv2d(cin, cout, k, **kw)
    M.Upmask(conv())
    M.Upmask(nn.Sequential(conv()))
    bad = [conv(cout=575), conv(cin=64), conv(k=3, padding=1), conv(padding=1), conv(stride=2), conv(bias=False), conv(groups=2),
           nn.Sequential(conv(), nn.ReLU()), nn.Sequential(nn.Identity(), conv()), nn.Sequential(), nn.Sequential(conv(bias=False)),
           nn.Linear(128, 576)]
    for m in bad:
        with pytest.raises(RuntimeError, match="Upmask: the module must be"):
            M.Upmask(m)
        with pytest.raises(RuntimeError, match="Upmask: the module must be"):
            M.install(m)
        assert "forward" not in m.__dict__
    # a forward that carries another wrapper is refused, and nothing is bound
    m = nn.Sequential(conv())
    other = lgu.heads.Head(nn.Conv2d(128, 2, 3, padding=1))
    m.forward = other
    with pytest.raises(RuntimeError, match="upmask.install: forward already carries a Head"):
        M.install(m)
    assert m.forward is other
    M.uninstall(m)                      # a foreign wrapper is left alone
    assert m.forward is other


def test_operator_refusals_come_before_any_launch(lgu, monkeypatch):
    """Shapes, pack size, bias shape, contiguity, dtypes, no-grad, device: each refusal's text, and which of two defects is
    reported.  None of them reaches the launch."""
    M = lgu.upmask
    H = torch.float16
    launched = []
    monkeypatch.setattr(M, "launch", lambda *a, **k: launched.append(a))

    def z(*shape, dtype=torch.float32):
        return torch.zeros(shape, dtype=dtype)

    def nc(t):
        return torch.zeros(tuple(t.shape) + (2,), dtype=t.dtype)[..., 0]

    x, wp, bh = z(2, 128, 2, 3), z(36, 4, 64, 8, dtype=H), z(576, dtype=H)
    no_grad = " has no autograd: its outputs would carry no gradient. Call it under torch.no_grad() or pass detached inputs"
    eager = [
        ((x, wp, bh), "x" + _NO_CPU),
        ((x.half(), wp, bh), "x" + _NO_CPU),
        ((z(1, 127, 2, 2), wp, bh), "x must be (N,128,H,W), got (1, 127, 2, 2)"),
        ((z(128, 2, 2), wp, bh), "x must be (N,128,H,W), got (128, 2, 2)"),
        ((x, z(36, 4, 64, 7, dtype=H), bh), "wpack must hold 73728 halves (pack_upmask), got (36, 4, 64, 7)"),
        ((x, wp, z(575, dtype=H)), "bias_h must be (576,), got (575,)"),
        ((nc(x), wp, bh), "x must be contiguous"),
        ((x, nc(wp), bh), "wpack must be contiguous"),
        ((x, wp, nc(bh)), "bias_h must be contiguous"),
        ((x.double(), wp, bh), "expected scalar type Float or Half but found Double (x)"),
        ((x.bfloat16(), wp, bh), "expected scalar type Float or Half but found BFloat16 (x)"),
        ((x, wp.float(), bh), "expected scalar type Half but found Float (wpack)"),
        ((x, wp, bh.bfloat16()), "expected scalar type Half but found BFloat16 (bias_h)"),
        ((x.clone().requires_grad_(), wp, bh), "upmask_conv1x1" + no_grad),
        # two defects: the earlier check reports
        ((nc(x), z(5, dtype=H), bh), "wpack must hold 73728 halves (pack_upmask), got (5,)"),
        ((x.double(), wp, nc(bh)), "bias_h must be contiguous"),
        ((x.clone().requires_grad_(), wp, bh.float()), "expected scalar type Half but found Float (bias_h)"),
    ]
    for args, message in eager:
        with pytest.raises(RuntimeError) as info:
            M.upmask_conv1x1(*args)
        assert type(info.value) is RuntimeError and str(info.value) == message
    up, d, ix = z(5, 16, 24), z(5, 2, 3), torch.zeros(2, dtype=torch.int64)
    fused = [
        ((up, d, ix, x, wp, bh), "disps_up" + _NO_CPU),
        ((up, z(5, 2, 3, 1), ix, x, wp, bh), "disps must be (N,ht,wd), got (5, 2, 3, 1)"),
        ((z(5, 16, 23), d, ix, x, wp, bh), "disps_up must be (N,8ht,8wd) = (5, 16, 24), got (5, 16, 23)"),
        ((up, d, ix[None], x, wp, bh), "ix must be 1-D, got (1, 2)"),
        ((up, d, ix, z(2, 127, 2, 3), wp, bh), "x must be (N,128,H,W), got (2, 127, 2, 3)"),
        ((up, d, ix, x, wp[:35], bh), "wpack must hold 73728 halves (pack_upmask), got (35, 4, 64, 8)"),
        ((up, d, ix, x, wp, bh[:5]), "bias_h must be (576,), got (5,)"),
        ((up, d, ix, z(3, 128, 2, 3), wp, bh), "x must be (2,128,2,3), got (3, 128, 2, 3)"),
        ((up, d, ix, z(2, 128, 3, 2), wp, bh), "x must be (2,128,2,3), got (2, 128, 3, 2)"),
        ((nc(up), d, ix, x, wp, bh), "disps_up must be contiguous"),
        ((up, nc(d), ix, x, wp, bh), "disps must be contiguous"),
        ((up, d, nc(ix), x, wp, bh), "ix must be contiguous"),
        ((up, d, ix, nc(x), wp, bh), "x must be contiguous"),
        ((up.double(), d, ix, x, wp, bh), "expected scalar type Float but found Double (disps_up)"),
        ((up, d.half(), ix, x, wp, bh), "expected scalar type Float but found Half (disps)"),
        ((up, d, ix.int(), x, wp, bh), "expected scalar type Long but found Int (ix)"),
        ((up, d, ix, x.double(), wp, bh), "expected scalar type Float or Half but found Double (x)"),
        ((up, d, ix, x, wp.float(), bh), "expected scalar type Half but found Float (wpack)"),
        ((up, d, ix, x.clone().requires_grad_(), wp, bh), "upsample_from_net_" + no_grad),
        ((up, d.clone().requires_grad_(), ix, x, wp, bh), "upsample_from_net_" + no_grad),
        ((nc(up), d, ix.int(), x, wp, bh), "disps_up must be contiguous"),
    ]
    for args, message in fused:
        for hw in (None, False, True):
            with pytest.raises(RuntimeError) as info:
                M.upsample_from_net_(*args, half_weights=hw)
            assert type(info.value) is RuntimeError and str(info.value) == message
    with torch.no_grad():      # grad mode off: the no-grad refusal does not apply, the device refusal is next
        with pytest.raises(RuntimeError) as info:
            M.upmask_conv1x1(x.clone().requires_grad_(), wp, bh)
        assert str(info.value) == "x" + _NO_CPU
    assert launched == []


# ---- GPU ------------------------------------------------------------------------------------------------------------
@pytest.fixture
def no_threshold(lgu, monkeypatch):
    """The wrapper's routing by size follows a measurement (MIN_FUSED_PIXELS); these tests are about the fused path."""
    monkeypatch.setattr(lgu.upmask, "MIN_FUSED_PIXELS", 0)


def _need_gpu(lgu):
    assert torch.cuda.is_available(), "these tests need the MI355X"
    assert os.path.exists(lgu._lib.so_path()), "liblgu_corr.so missing — run __graft_entry__.build()"


def _packed(lgu, m):
    c = RU.conv_of(m)
    return lgu.upmask.pack_upmask(c.weight.detach().cuda(), c.bias.detach().cuda())


def _fused(lgu, disps, ix, x, wpack, bias_h, hw, fill=-3.0):
    up = torch.full((disps.shape[0], 8 * disps.shape[1], 8 * disps.shape[2]), fill, device="cuda")
    assert lgu.upmask.upsample_from_net_(up, disps, ix, x, wpack, bias_h, half_weights=hw) is up
    return up


IMPULSE_CH = [0, 7, 8, 31, 32, 127]


@pytest.mark.gpu
def test_zero_input_and_impulses_are_bit_for_bit(lgu):
    """Zero input: half(b_h) everywhere.  One input element = v (each of six channels at each of three pixels of a 2x17
    image, v = 1 and v = -1.5): a single product is exact, so the pixel's outputs are half(b_h + v·w_h[:, c]) and every
    other pixel keeps half(b_h)."""
    _need_gpu(lgu)
    M = lgu.upmask
    m = RU.make_upmask(43, GAIN)
    c = RU.conv_of(m)
    wpack, bias_h = _packed(lgu, m)
    bh = c.bias.detach().half()
    for shape in SHAPES:
        x = torch.zeros((shape[0], 128) + shape[1:], device="cuda")
        want = bh.view(1, 576, 1, 1).expand(shape[0], 576, *shape[1:]).contiguous()
        assert same_bits(M.upmask_conv1x1(x, wpack, bias_h), want), shape
        assert same_bits(M.upmask_conv1x1(x.half(), wpack, bias_h), want), shape
    wh = c.weight.detach().half().view(576, 128)
    at = [(0, 0), (0, 16), (1, 15)]
    x = torch.zeros((len(at) * len(IMPULSE_CH) * 2, 128, 2, 17))
    want = bh.view(1, 576, 1, 1).expand(x.shape[0], 576, 2, 17).clone()
    n = 0
    for (y, xx) in at:
        for ch in IMPULSE_CH:
            for v in (1.0, -1.5):
                x[n, ch, y, xx] = v
                want[n, :, y, xx] = RU.single(bh, wh[:, ch].float() * v)
                n += 1
    got = M.upmask_conv1x1(x.cuda(), wpack, bias_h)
    got_h = M.upmask_conv1x1(x.half().cuda(), wpack, bias_h)
    torch.cuda.synchronize()
    assert same_bits(got, want), "max |diff| %g" % float((got.cpu().float() - want.float()).abs().max())
    assert same_bits(got_h, want)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ALL_SHAPES)
def test_every_element_is_within_the_derived_bound(lgu, shape):
    """|h - s64| <= allowance(s64, S, 130), for float32 and half input; prints where the library's own forward sits."""
    _need_gpu(lgu)
    m, x, s64, S, _ = case(shape)
    wpack, bias_h = _packed(lgu, m)
    bound = R.allowance(s64, S, RU.TERMS)
    xc = x.cuda()
    mc = RU.make_upmask(41, GAIN).cuda()
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        own = mc(xc)
    got = lgu.upmask.upmask_conv1x1(xc, wpack, bias_h)
    from_half = lgu.upmask.upmask_conv1x1(xc.half(), wpack, bias_h)
    rounded = lgu.upmask.upmask_conv1x1(xc.half().float(), wpack, bias_h)
    torch.cuda.synchronize()
    err = (got.cpu().double() - s64).abs()
    err_own = (own.cpu().double() - s64).abs()
    print("upmask_conv1x1 %s: worst error %.3g of its bound; the module's own forward: worst %.3g of the bound, %.4f "
          "bit-identical to the kernel" % (shape, float((err / bound).max()), float((err_own / bound).max()),
                                           float((own == got).double().mean())))
    assert got.dtype == torch.float16 == own.dtype and tuple(got.shape) == (shape[0], 576) + shape[1:] == tuple(own.shape)
    assert bool((err <= bound).all()), float((err / bound).max())
    assert same_bits(from_half, rounded) and same_bits(from_half, got)      # fp32 x is rounded to half exactly once


@pytest.mark.gpu
@pytest.mark.parametrize("shape,ats", [((2, 3, 17), [(0, 5, 0, 15), (0, 64, 0, 16), (1, 127, 2, 16), (1, 0, 0, 0)]),
                                       ((1, 6, 80), [(0, 9, 3, 47), (0, 33, 5, 79)])])
def test_nan_reaches_exactly_its_pixel(lgu, shape, ats):
    """Eager: the pixel's 576 outputs.  Fused: the pixel's 8x8 block; every other output keeps its bits (the neighbours read
    the pixel's disparity, not its mask)."""
    _need_gpu(lgu)
    m, x, _, _, disps = case(shape)
    wpack, bias_h = _packed(lgu, m)
    ix, d = indices(shape[0]).cuda(), disps.cuda()
    clean = lgu.upmask.upmask_conv1x1(x.cuda(), wpack, bias_h).cpu()
    clean_up = {hw: _fused(lgu, d, ix, x.cuda(), wpack, bias_h, hw).cpu() for hw in (False, True)}
    assert not bool(torch.isnan(clean).any()) and not any(bool(torch.isnan(v).any()) for v in clean_up.values())
    for at in ats:
        xn = x.clone()
        xn[at] = float("nan")
        n, _, cy, cx = at
        got = lgu.upmask.upmask_conv1x1(xn.cuda(), wpack, bias_h).cpu()
        want = torch.zeros((shape[0], 1) + shape[1:], dtype=torch.bool)
        want[n, 0, cy, cx] = True
        want = want.expand_as(got)
        assert bool((torch.isnan(got) == want).all()), at
        assert bool((got.view(torch.int16) == clean.view(torch.int16))[~want].all()), at
        for hw in (False, True):
            up = _fused(lgu, d, ix, xn.cuda(), wpack, bias_h, hw).cpu()
            wu = torch.zeros_like(up, dtype=torch.bool)
            wu[int(ix[n]), 8 * cy:8 * cy + 8, 8 * cx:8 * cx + 8] = True
            assert bool((torch.isnan(up) == wu).all()), (at, hw)
            assert bool((up.view(torch.int32) == clean_up[hw].view(torch.int32))[~wu].all()), (at, hw)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(2, 3, 17), (3, 4, 16), BIG])
def test_a_frame_does_not_depend_on_its_batch(lgu, shape):
    """Both entries: a frame alone, and the batch reversed, give the frame's bits."""
    _need_gpu(lgu)
    M = lgu.upmask
    m, x, _, _, disps = case(shape)
    wpack, bias_h = _packed(lgu, m)
    xc, d, U = x.cuda(), disps.cuda(), shape[0]
    ix = indices(U).cuda()
    got = M.upmask_conv1x1(xc, wpack, bias_h)
    back = torch.flip(xc, dims=(0,)).contiguous()
    assert same_bits(torch.flip(M.upmask_conv1x1(back, wpack, bias_h), dims=(0,)), got)
    for hw in (False, True):
        up = _fused(lgu, d, ix, xc, wpack, bias_h, hw)
        assert same_bits(_fused(lgu, d, torch.flip(ix, dims=(0,)), back, wpack, bias_h, hw), up)
        for k in range(U):
            one = _fused(lgu, d, ix[k:k + 1], xc[k:k + 1].contiguous(), wpack, bias_h, hw)
            assert same_bits(one[ix[k]], up[ix[k]]), (hw, k)
            assert bool((one[[r for r in range(U + 2) if r != int(ix[k])]] == -3.0).all())
    for k in range(U):
        assert same_bits(got[k:k + 1], M.upmask_conv1x1(xc[k:k + 1].contiguous(), wpack, bias_h)), k


def _c_eager(lgu, x, wpack, bias_h, out, flags=0, n=None):
    N, _, H, W = x.shape
    flags |= lgu.upmask.X_HALF if x.dtype == torch.float16 else 0
    args = lgu._lib.UpmaskArgs(x.data_ptr(), wpack.data_ptr(), bias_h.data_ptr(), out.data_ptr(), N if n is None else n, H, W, flags)
    rc = lgu._lib.load().lgu_upmask1x1_c128_h16(args, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc


def _c_fused(lgu, x, wpack, bias_h, disps, ix, up, flags=0, u=None, n=None):
    U, _, ht, wd = x.shape
    flags |= lgu.upmask.X_HALF if x.dtype == torch.float16 else 0
    args = lgu._lib.UpmaskUpsArgs(x.data_ptr(), wpack.data_ptr(), bias_h.data_ptr(), disps.data_ptr(), ix.data_ptr(), up.data_ptr(),
                                  U if u is None else u, disps.shape[0] if n is None else n, ht, wd, flags)
    rc = lgu._lib.load().lgu_upmask_upsample_f32(args, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc


@pytest.mark.gpu
@pytest.mark.parametrize("half_x", (False, True))
@pytest.mark.parametrize("shape", [(2, 3, 17), (1, 6, 80)])
def test_guard_bands_and_alignment(lgu, shape, half_x):
    """x, bias (and the eager out, disps, ix) are served at element alignment with the aligned call's bits and no write
    outside the outputs; a wpack or a disps_up that is not 16-byte aligned is refused with nothing written; rows of disps_up
    not named by ix keep their bits; ix entries < 0 or >= N write nothing; N > U; empty U or an empty frame launches
    nothing."""
    from tests.alignment_cases import guards_intact, shifted
    _need_gpu(lgu)
    M, L = lgu.upmask, lgu._lib
    m, x, _, _, disps = case(shape)
    wpack, bias_h = _packed(lgu, m)
    U, ht, wd = shape
    N = U + 2
    xc = x.cuda().half() if half_x else x.cuda()
    d, ix = disps.cuda(), indices(U).cuda()
    want = M.upmask_conv1x1(xc, wpack, bias_h)
    HW = M.UPS_HALF_WEIGHTS
    want_up = _fused(lgu, d, ix, xc, wpack, bias_h, True)
    rest = [r for r in range(N) if r not in ix.tolist()]
    assert N > U and bool((want_up[rest] == -3.0).all()) and not bool((want_up[ix] == -3.0).any())
    # the fused result is the project's own upsampler on the eager mask, bit for bit
    for hw in (False, True):
        ref = torch.full_like(want_up, -3.0)
        with torch.autocast("cuda", enabled=not hw):
            lgu.aggregate.upsample_disps_(ref, d, ix, want)
        assert same_bits(_fused(lgu, d, ix, xc, wpack, bias_h, hw), ref), hw
    # eager: every operand at every shift
    base = {"x": xc, "wpack": wpack, "bias": bias_h, "out": torch.empty_like(want)}
    xs = (2, 4, 8) if half_x else (4, 8)
    variants = [(k, s) for k, ss in (("x", xs), ("bias", (2, 4, 8)), ("out", (2, 4, 8)), ("wpack", (2, 4, 8))) for s in ss]
    for key, shift in variants + [("all but wpack", 0)]:
        keys = [key] if key in base else [k for k in base if k != "wpack"]
        args = dict(base)
        for k in keys:
            args[k] = shifted(base[k], shift if key in base else base[k].element_size())
        if "out" not in keys:
            args["out"] = shifted(base["out"], 0)      # always carved from a poisoned buffer
        before = {k: args[k].clone() for k in args}
        rc = _c_eager(lgu, args["x"], args["wpack"], args["bias"], args["out"])
        if "wpack" in keys:
            assert rc == L.LGU_E_UNSUPPORTED, (key, shift, rc)
            assert same_bits(args["out"], before["out"]), "refused, but out changed"
        else:
            assert rc == 0, (key, shift, rc)
            assert same_bits(args["out"], want), "%s shifted by %d: differs from the aligned call" % (key, shift)
        for k in ("x", "wpack", "bias"):
            assert same_bits(args[k], before[k]), "read-only operand %s changed" % k
        for k in set(keys) | {"out"}:
            assert guards_intact(args[k]), "%s, %d: a guard band of %s was written" % (key, shift, k)
    # fused: every operand at every shift
    fbase = {"x": xc, "wpack": wpack, "bias": bias_h, "disps": d, "ix": ix, "up": torch.full_like(want_up, -3.0)}
    variants = [(k, s) for k, ss in (("x", xs), ("bias", (2, 4, 8)), ("disps", (4, 8)), ("ix", (8,)), ("wpack", (2, 4, 8)),
                                     ("up", (4, 8))) for s in ss]
    for key, shift in variants + [("all but wpack and up", 0)]:
        keys = [key] if key in fbase else [k for k in fbase if k not in ("wpack", "up")]
        args = dict(fbase)
        for k in keys:
            args[k] = shifted(fbase[k], shift if key in fbase else fbase[k].element_size())
        if "up" not in keys:
            args["up"] = shifted(fbase["up"], 0)
        before = {k: args[k].clone() for k in args}
        rc = _c_fused(lgu, args["x"], args["wpack"], args["bias"], args["disps"], args["ix"], args["up"], HW)
        if "wpack" in keys or "up" in keys:
            assert rc == L.LGU_E_UNSUPPORTED, (key, shift, rc)
            assert same_bits(args["up"], before["up"]), "refused, but disps_up changed"
        else:
            assert rc == 0, (key, shift, rc)
            assert same_bits(args["up"], want_up), "%s shifted by %d: differs from the aligned call" % (key, shift)
        for k in ("x", "wpack", "bias", "disps", "ix"):
            assert same_bits(args[k], before[k]), "read-only operand %s changed" % k
        for k in set(keys) | {"up"}:
            assert guards_intact(args[k]), "%s, %d: a guard band of %s was written" % (key, shift, k)
    # through Python: a misaligned wpack or disps_up raises UnsupportedShape and writes nothing
    with pytest.raises(L.UnsupportedShape):
        M.upmask_conv1x1(xc, shifted(wpack, 8), bias_h)
    up = shifted(fbase["up"], 4)
    with pytest.raises(L.UnsupportedShape):
        M.upsample_from_net_(up, d, ix, xc, wpack, bias_h)
    with pytest.raises(L.UnsupportedShape):
        M.upsample_from_net_(shifted(fbase["up"], 0), d, ix, xc, shifted(wpack, 2), bias_h)
    torch.cuda.synchronize()
    assert bool((up == -3.0).all()) and guards_intact(up)
    # ix entries < 0 or >= N write nothing, the valid ones are written as before
    if U > 1:
        ix2 = ix.clone()
        ix2[0] = -1
        up2 = _fused(lgu, d, ix2, xc, wpack, bias_h, True)
        ix2[0] = N
        up3 = _fused(lgu, d, ix2, xc, wpack, bias_h, True)
        keep = ix[1:]
        gone = [r for r in range(N) if r not in keep.tolist()]
        assert same_bits(up2[keep], want_up[keep]) and same_bits(up3, up2) and bool((up2[gone] == -3.0).all())
    # refusals and empty cases of the C entries: nothing written
    out = shifted(base["out"], 0)
    out.fill_(0.25)
    assert _c_eager(lgu, xc, wpack, bias_h, out, flags=2) == L.LGU_E_BADARG
    assert _c_eager(lgu, xc, wpack, bias_h, out, n=-1) == L.LGU_E_BADARG
    assert _c_eager(lgu, xc, wpack, bias_h, out, n=0) == 0
    assert bool((out == 0.25).all()) and guards_intact(out)
    up = shifted(fbase["up"], 0)
    assert _c_fused(lgu, xc, wpack, bias_h, d, ix, up, flags=4) == L.LGU_E_BADARG
    assert _c_fused(lgu, xc, wpack, bias_h, d, ix, up, u=-1) == L.LGU_E_BADARG
    assert _c_fused(lgu, xc, wpack, bias_h, d, ix, up, u=0) == 0
    assert _c_fused(lgu, xc, wpack, bias_h, d, ix, up, n=0) == 0
    assert bool((up == -3.0).all()) and guards_intact(up)
    # empty U or an empty frame launches nothing (Python)
    up = torch.full_like(want_up, -3.0)
    M.upsample_from_net_(up, d, ix[:0], xc[:0], wpack, bias_h)
    e = torch.zeros((N, 0, 8 * wd), device="cuda")
    assert M.upsample_from_net_(e, d[:, :0], ix, xc[:, :, :0], wpack, bias_h) is e
    assert bool((up == -3.0).all())
    assert tuple(M.upmask_conv1x1(xc[:0], wpack, bias_h).shape) == (0, 576, ht, wd)
    assert tuple(M.upmask_conv1x1(xc[:, :, :0], wpack, bias_h).shape) == (U, 576, 0, wd)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ALL_SHAPES)
def test_fused_upsample_equals_the_restatement_on_the_eager_kernels_own_bits(lgu, shape):
    """The fused result against the float64 upsample restatement evaluated on upmask_conv1x1's own h, with the tolerances
    upsample_disps_ is held to (module docstring), for float32 and half x and both weight roundings; with the weight-rounding
    flag swapped the same check fails.  A mask whose bits differ from the eager kernel's fails it too: shown by handing
    the restatement a mask with one value in a hundred one ulp off."""
    _need_gpu(lgu)
    m, x, s64, _, disps = case(shape)
    wpack, bias_h = _packed(lgu, m)
    U = shape[0]
    ix = indices(U)
    ix_all = torch.cat([ix, torch.tensor([-1, U + 2])]) if shape == (2, 3, 17) else ix
    for xc in (x.cuda(), x.cuda().half()):
        h = lgu.upmask.upmask_conv1x1(xc, wpack, bias_h)
        xin = torch.cat([xc, xc[:ix_all.shape[0] - U]]) if ix_all is not ix else xc
        hin = torch.cat([h, h[:ix_all.shape[0] - U]]).cpu().numpy() if ix_all is not ix else h.cpu().numpy()
        ups = {hw: _fused(lgu, disps.cuda(), ix_all.cuda(), xin, wpack, bias_h, hw).cpu().numpy() for hw in (False, True)}
        for hw in (False, True):
            rows, want, bound = RU.upsample(disps.numpy(), ix_all.numpy(), hin, hw)
            assert rows.tolist() == ix.tolist()
            r = RU.upsample_ratio(ups[hw][rows], want, bound)
            print("upsample_from_net_ %s %s half_weights=%s: worst %.3g of max|d|, %.3g of the outputs above %g"
                  % (shape, xc.dtype, hw, r.max(), (r > RU.UPS_TOL).mean(), RU.UPS_TOL))
            assert RU.within(r, hw), (hw, r.max(), (r > RU.UPS_TOL).mean())
            rest = [k for k in range(U + 2) if k not in rows.tolist()]
            assert bool((ups[hw][rest] == -3.0).all())
            if want.size >= 1000:
                swapped = RU.upsample_ratio(ups[not hw][rows], want, bound)
                assert not RU.within(swapped, hw), "the check passes with the weight-rounding flag swapped"
                # one ulp on one mask value in a hundred: the check sees it
                hb = np.ascontiguousarray(hin[[u for u in range(len(ix_all)) if 0 <= ix_all[u] < U + 2]]).copy()
                bits = hb.view(np.int16).reshape(-1)
                bits[::100] += 1
                _, moved, _ = RU.upsample(disps.numpy(), ix.numpy(), hb, hw)
                assert not RU.within(RU.upsample_ratio(ups[hw][rows], moved, bound), hw), "an ulp of the mask goes unseen"


def _like(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and bool(((a.double() - b.double()).abs() <= 2.0 ** -6 * (1 + b.double().abs())).all())


def _spy(monkeypatch, module):
    """The list of what the class's own forward returns for `module`, call by call."""
    cls, seen = type(module), []
    orig = cls.forward

    def forward(self, *args, **kwargs):
        out = orig(self, *args, **kwargs)
        if self is module:
            seen.append(out)
        return out
    monkeypatch.setattr(cls, "forward", forward)
    return seen


@pytest.mark.gpu
@pytest.mark.parametrize("sequential", (True, False))
def test_upmask_wrapper_under_autocast(lgu, no_threshold, monkeypatch, sequential):
    """Under float16 autocast Upmask(module)(x) is half, within the allowance, and fused_calls increments; a bfloat16
    autocast, autocast off and grad return what the module's own forward returns (the very tensor: the library's convolution
    is not bit-reproducible from call to call, so the values are compared with a twin `mc` of the same weights to the
    precision of the coarsest mode, bfloat16) and the counter stays."""
    _need_gpu(lgu)
    M = lgu.upmask
    shape = (2, 3, 17)
    _, x, s64, S, _ = case(shape)
    bound = R.allowance(s64, S, RU.TERMS)
    mc = RU.make_upmask(41, GAIN, sequential).cuda()
    wrapped = RU.make_upmask(41, GAIN, sequential).cuda()
    xc = x.cuda()
    wr = M.Upmask(wrapped)
    seen = _spy(monkeypatch, wrapped)
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        own = mc(xc.clone())
        got = wr(xc)
        assert wr.fused_calls == 1
        assert same_bits(wr(xc.half()), got) and wr.fused_calls == 2      # a half input is used as it is
        assert same_bits(got, M.upmask_conv1x1(xc, *wr.packed()))
    assert seen == []
    with torch.no_grad():
        y = wr(xc)
        assert y is seen[-1] and _like(y, mc(xc))
        with torch.autocast("cuda", dtype=torch.bfloat16):
            y = wr(xc)
            assert y is seen[-1] and _like(y, mc(xc))
    with torch.autocast("cuda", dtype=torch.float16):
        grad = wr(xc.clone().requires_grad_())
        assert grad is seen[-1] and grad.requires_grad and _like(grad, mc(xc))
    assert wr.fused_calls == 2 and len(seen) == 3
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        assert M.install(wrapped) is wrapped.forward and wrapped.forward is not wr
        installed = wrapped(xc)
        assert wrapped.forward.fused_calls == 1
        M.uninstall(wrapped)
        monkeypatch.setattr(M, "MIN_FUSED_PIXELS", 1 << 40)      # below the threshold: the module
        y = wr(xc)
        assert y is seen[-1] and len(seen) == 4 and _like(y, own) and wr.fused_calls == 2
    torch.cuda.synchronize()
    assert got.dtype == own.dtype == torch.float16 and got.shape == own.shape == (2, 576, 3, 17)
    assert same_bits(installed, got)
    err, err_own = (got.cpu().double() - s64).abs(), (own.cpu().double() - s64).abs()
    print("Upmask: worst error %.3g of the bound; the module's own forward %.3g; %.4f of the elements bit-identical"
          % (float((err / bound).max()), float((err_own / bound).max()), float((got == own).double().mean())))
    assert bool((err <= bound).all()), float((err / bound).max())
