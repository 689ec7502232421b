"""The fused stem and output layer of the encoders (lgu_slam_amd.encconv.enc_stem7x7 / enc_out1x1, csrc/encends.hip)
against the float64 restatement of their rounding models, tests/encends_restatement.py.

Numerics contract (include/lgu_corr.h):
- a single product is exact: an impulse gives half(b_h + x_h w_h) where the window holds it and half(b_h) elsewhere, bit for
  bit, at even and odd rows and columns; the zero input gives act(b_h);
- every element: |y - s64| <= allowance(s64, S, terms) of tests/conv3_restatement.py, terms 149 (stem) and 130 (output);
- the ReLU form is bit for bit torch.relu of the identity output; a half input gives the bits of the float32 input it is
  the rounding of;
- SPLIT: inp is bit for bit torch.relu(h[:, 128:]), net within one half rounding of a float tanh that is within 5 ulp,
  tanh(+-inf) = +-1, NaN kept;
- NaN reaches exactly the outputs whose window holds it; an image does not depend on its batch.
The alignment audit of the two entries (their operands travel in parameter blocks) is test_*_guard_bands_and_alignment.
The GPU tests build their layers themselves and never read the reference tree.
"""
import ctypes
import os

import pytest

torch = pytest.importorskip("torch")

from tests import encends_restatement as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEM, OUT = "lgu_encstem7x7_h16", "lgu_encout1x1_c128_h16"
_NO_CPU = " must be a HIP device tensor: lgu_slam_amd has no CPU fallback"
_CASES = {}


def same_bits(a, b):
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    iv = torch.int16 if a.dtype == torch.float16 else torch.int32
    return bool(torch.equal(a.view(iv), b.view(iv)))


def stem_case(size):
    """(conv, x float32, s64, S) on the CPU for one input size, computed once and never changed."""
    if ("stem", size) not in _CASES:
        conv = R.make_stem(81)
        x = R.make_image(4000 + size[1] * size[2], *size)
        with torch.no_grad():
            _CASES[("stem", size)] = (conv, x) + R.stem(x, conv)
    return _CASES[("stem", size)]


def out_case(cout, size):
    """(conv, x half, s64, S) on the CPU for one Cout and input size, computed once and never changed."""
    if (cout, size) not in _CASES:
        conv = R.make_out(82 + cout, cout)
        x = R.make_features(5000 + size[1] * size[2], *size).half()
        with torch.no_grad():
            _CASES[(cout, size)] = (conv, x) + R.out(x, conv)
    return _CASES[(cout, size)]


# ---- CPU ------------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_entries(lgu):
    from tests.test_abi import declared_symbols
    lib = ctypes.CDLL(lgu._lib._build.SO_PATH)
    E = lgu.encconv
    for entry, struct, fields, size in (
            (STEM, lgu._lib.EncStemArgs, ["x", "wpack", "bias", "out", "N", "H", "W", "Cin", "Cout", "flags"], 4 * 8 + 6 * 4),
            (OUT, lgu._lib.EncOutArgs, ["x", "wpack", "bias", "out", "inp", "N", "H", "W", "Cin", "Cout", "flags"], 5 * 8 + 6 * 4)):
        assert entry in declared_symbols() and hasattr(lib, entry)
        sig = lgu._lib.SIGNATURES[entry]
        assert sig[0] is struct and issubclass(sig[0], ctypes.Structure) and sig[1] is ctypes.c_void_p
        assert [f[0] for f in sig[0]._fields_] == fields and ctypes.sizeof(sig[0]) == size
    assert "encends.hip" in lgu._build.SOURCES
    assert lgu.enc_stem7x7 is E.enc_stem7x7 and lgu.enc_out1x1 is E.enc_out1x1
    assert lgu.pack_stem is E.pack_stem and lgu.pack_out1 is E.pack_out1
    text = open(os.path.join(ROOT, "include", "lgu_corr.h")).read()
    assert "#define LGU_ENCSTEM_X_HALF %d " % E.X_HALF in text and "#define LGU_ENCSTEM_RELU %d " % E.STEM_RELU in text
    assert "#define LGU_ENCOUT_SPLIT %d " % E.SPLIT in text and "#define LGU_ENCSTEM_WPACK_HALVES %d\n" % (7 * 2 * 64 * 8) in text
    assert set(E.MIN_OUT_PIXELS) == set(R.COUTS) and isinstance(E.MIN_STEM_PIXELS, int)
    assert set(E.MIN_FUSED_PIXELS) == set(E.SHAPES)                 # the residual stages' table keeps its keys


def test_stem_pack_puts_every_weight_in_its_documented_slot_and_zero_elsewhere(lgu):
    g = torch.Generator().manual_seed(5)
    w = torch.randn((32, 3, 7, 7), generator=g)
    b = torch.randn((32,), generator=g)
    wpack, bias_h = lgu.encconv.pack_stem(w, b)
    assert wpack.dtype == torch.float16 and wpack.is_contiguous() and tuple(wpack.shape) == (7, 2, 64, 8)
    assert same_bits(bias_h, b.half())
    co, c, ky, kx, holds = R.stem_slots()
    idx = torch.arange(32 * 3 * 49, dtype=torch.int32).view(32, 3, 7, 7)
    assert sorted(idx[co, c, ky, kx][holds].tolist()) == list(range(32 * 3 * 49))     # every weight once
    want = torch.where(holds, w.half()[co, c, ky, kx], torch.zeros((), dtype=torch.float16))
    assert same_bits(wpack, want) and int((~holds).sum()) == 7 * 2 * 64 * 8 - 32 * 3 * 49
    assert bool((wpack[~holds] == 0).all()) and not bool(torch.signbit(wpack[~holds]).any())
    for bad in (w[:, :2], torch.zeros(32, 4, 7, 7), torch.zeros(64, 3, 7, 7), torch.zeros(32, 3, 3, 3), torch.zeros(32, 3, 7)):
        with pytest.raises(RuntimeError, match="pack_stem: weight must be"):
            lgu.encconv.pack_stem(bad, b)
    with pytest.raises(RuntimeError, match="bias must be"):
        lgu.encconv.pack_stem(w, b[:-1])


@pytest.mark.parametrize("cout", R.COUTS)
def test_out_pack_puts_every_weight_in_its_documented_slot_and_nothing_else(lgu, cout):
    g = torch.Generator().manual_seed(6)
    w = torch.randn((cout, 128, 1, 1), generator=g)
    b = torch.randn((cout,), generator=g)
    wpack, bias_h = lgu.encconv.pack_out1(w, b)
    assert wpack.dtype == torch.float16 and wpack.is_contiguous() and tuple(wpack.shape) == (4, cout // 16, 64, 8)
    assert same_bits(bias_h, b.half())
    co, c = R.out_slots(cout)
    idx = torch.arange(cout * 128, dtype=torch.int32).view(cout, 128)
    assert sorted(idx[co, c].flatten().tolist()) == list(range(cout * 128))
    assert same_bits(wpack, w.half()[co, c, 0, 0])
    for bad in (w[:, :64], torch.zeros(64, 128, 1, 1), torch.zeros(cout, 128, 3, 3), torch.zeros(cout, 128)):
        with pytest.raises(RuntimeError, match="pack_out1: weight must be"):
            lgu.encconv.pack_out1(bad, b)
    with pytest.raises(RuntimeError, match="bias must be"):
        lgu.encconv.pack_out1(w, b[:-1])


@pytest.mark.parametrize("size", [(1, 1, 1), (1, 2, 3), (2, 9, 33)])
def test_restatement_equals_float64_conv2d_on_the_rounded_operands(size):
    F = torch.nn.functional
    conv, x, s64, S = stem_case(size)
    xh, wh, bh = R.h64(x), R.h64(conv.weight), R.h64(conv.bias)
    s = F.conv2d(xh, wh, bh, stride=2, padding=3)
    Sc = F.conv2d(xh.abs(), wh.abs(), bh.abs(), stride=2, padding=3)
    # the operands are half values, so every product is exact in float64; the two sums differ in order only
    assert s.shape == s64.shape == (size[0], 32) + R.out_size(size[1], size[2])
    assert bool(((s - s64).abs() <= 2.0 ** -44 * S).all()) and bool(((Sc - S).abs() <= 2.0 ** -44 * S).all())
    assert bool((S >= s64.abs()).all()) and bool((R.allowance(s64, S, R.STEM_TERMS) > 0).all())
    for cout in R.COUTS:
        conv, x, s64, S = out_case(cout, size)
        xh, wh, bh = R.h64(x), R.h64(conv.weight), R.h64(conv.bias)
        s, Sc = F.conv2d(xh, wh, bh), F.conv2d(xh.abs(), wh.abs(), bh.abs())
        assert s.shape == s64.shape == (size[0], cout) + size[1:]
        assert bool(((s - s64).abs() <= 2.0 ** -44 * S).all()) and bool(((Sc - S).abs() <= 2.0 ** -44 * S).all())
        assert bool((S >= s64.abs()).all())
    assert R.STEM_TERMS == 7 * 7 * 3 + 2 == 149 and R.OUT_TERMS == 128 + 2 == 130
    t, bound = R.tanh_bound(torch.tensor([0.0, 0.5, -3.0, float("inf")], dtype=torch.float64))
    assert t.tolist() == [0.0, float(torch.tanh(torch.tensor(0.5, dtype=torch.float64))), float(torch.tanh(torch.tensor(-3.0, dtype=torch.float64))), 1.0]
    e = 5 * 2.0 ** -23 * t.abs()
    assert torch.equal(bound, 2.0 ** -11 * (t.abs() + e) + e + 2.0 ** -25)


def _z(*shape, dtype=torch.float16):
    return torch.zeros(shape, dtype=dtype)


def _nc(t):
    return torch.zeros(tuple(t.shape) + (2,), dtype=t.dtype)[..., 0]


def test_stem_refusals_in_their_order(lgu):
    """x's rank, the pack, the bias's rank, the served channels, the pack size, then contiguity, dtypes, no-grad and device:
    each refusal's text, and which of two defects is reported.  None of them touches a device."""
    f = lgu.encconv.enc_stem7x7
    x, wp, bh = _z(1, 3, 4, 6, dtype=torch.float32), _z(7, 2, 64, 8), _z(32)
    no_grad = "enc_stem7x7 has no autograd: its outputs would carry no gradient. Call it under torch.no_grad() or pass detached inputs"
    served = "enc_stem7x7 serves (Cin, Cout) = (3, 32), got "
    cases = [
        ((x, (wp, bh)), "x" + _NO_CPU),
        ((x.half(), (wp, bh)), "x" + _NO_CPU),
        ((_z(3, 4, 6), (wp, bh)), "x must be (N,3,H,W), got (3, 4, 6)"),
        ((x, wp), "pack must be (wpack, bias_h) of pack_stem"),
        ((x, (wp, _z(32, 1))), "bias_h must be (Cout,), got (32, 1)"),
        ((_z(1, 4, 4, 6), (wp, bh)), served + "(4, 32)"),
        ((x, (wp, _z(64))), served + "(3, 64)"),
        ((x, (_z(7, 2, 64, 7), bh)), "wpack must hold 7168 halves (pack_stem), got (7, 2, 64, 7)"),
        ((_nc(x), (wp, bh)), "x must be contiguous"),
        ((x, (_nc(wp), bh)), "wpack must be contiguous"),
        ((x, (wp, _nc(bh))), "bias_h must be contiguous"),
        ((x.double(), (wp, bh)), "expected scalar type Float or Half but found Double (x)"),
        ((x, (wp.float(), bh)), "expected scalar type Half but found Float (wpack)"),
        ((x, (wp, bh.bfloat16())), "expected scalar type Half but found BFloat16 (bias_h)"),
        ((x.clone().requires_grad_(), (wp, bh)), no_grad),
        # two defects: the earlier check reports
        ((_z(3, 4, 6), wp), "x must be (N,3,H,W), got (3, 4, 6)"),
        ((x.double(), (_z(5), bh)), "wpack must hold 7168 halves (pack_stem), got (5,)"),
        ((_nc(x.double()), (wp, bh)), "x must be contiguous"),
        ((x.clone().requires_grad_(), (wp, bh.float())), "expected scalar type Half but found Float (bias_h)"),
    ]
    for args, message in cases:
        for relu in (False, True):
            with pytest.raises(RuntimeError) as info:
                f(*args, relu=relu)
            assert str(info.value) == message
            assert type(info.value) is (lgu._lib.UnsupportedShape if message.startswith(served) else RuntimeError)
    with torch.no_grad():      # grad mode off: the no-grad refusal does not apply, the device refusal is next
        with pytest.raises(RuntimeError) as info:
            f(x.clone().requires_grad_(), (wp, bh))
        assert str(info.value) == "x" + _NO_CPU


def test_out_refusals_in_their_order(lgu):
    """x's rank, the pack, the bias's rank, the served channels, split with Cout 128, the pack size, x's dtype, then
    contiguity, dtypes, no-grad and device."""
    f = lgu.encconv.enc_out1x1
    x, wp, bh = _z(1, 128, 4, 6), _z(4, 16, 64, 8), _z(256)
    wp1, bh1 = _z(4, 8, 64, 8), _z(128)
    no_grad = "enc_out1x1 has no autograd: its outputs would carry no gradient. Call it under torch.no_grad() or pass detached inputs"
    served = "enc_out1x1 serves Cin = 128 and Cout in [128, 256], got "
    split = "split=True (net, inp of 128 planes each) needs Cout = 256, got 128"
    cases = [
        ((x, (wp, bh)), {}, "x" + _NO_CPU),
        ((x, (wp1, bh1)), {}, "x" + _NO_CPU),
        ((x, (wp, bh)), dict(split=True), "x" + _NO_CPU),
        ((_z(128, 4, 6), (wp, bh)), {}, "x must be (N,128,H,W), got (128, 4, 6)"),
        ((x, wp), {}, "pack must be (wpack, bias_h) of pack_out1"),
        ((x, (wp, _z(256, 1))), {}, "bias_h must be (Cout,), got (256, 1)"),
        ((_z(1, 64, 4, 6), (wp, bh)), {}, served + "(64, 256)"),
        ((x, (wp, _z(192))), {}, served + "(128, 192)"),
        ((x, (wp1, bh1)), dict(split=True), split),
        ((x, (_z(4, 16, 64, 7), bh)), {}, "wpack must hold 32768 halves (pack_out1, 128 -> 256), got (4, 16, 64, 7)"),
        ((x, (wp, bh1)), {}, "wpack must hold 16384 halves (pack_out1, 128 -> 128), got (4, 16, 64, 8)"),
        ((x.float(), (wp, bh)), {}, "expected scalar type Half but found Float (x)"),
        ((_nc(x), (wp, bh)), {}, "x must be contiguous"),
        ((x, (_nc(wp), bh)), {}, "wpack must be contiguous"),
        ((x, (wp, _nc(bh))), {}, "bias_h must be contiguous"),
        ((x, (wp.float(), bh)), {}, "expected scalar type Half but found Float (wpack)"),
        ((x, (wp, bh.bfloat16())), {}, "expected scalar type Half but found BFloat16 (bias_h)"),
        ((x.clone().requires_grad_(), (wp, bh)), {}, no_grad),
        # two defects: the earlier check reports
        ((_z(1, 64, 4, 6), (wp1, bh1)), dict(split=True), served + "(64, 128)"),
        ((x.float(), (_z(5), bh1)), dict(split=True), split),
        ((x.float(), (_z(5), bh)), {}, "wpack must hold 32768 halves (pack_out1, 128 -> 256), got (5,)"),
        ((_nc(x.float()), (wp, bh)), {}, "expected scalar type Half but found Float (x)"),
        ((x.clone().requires_grad_(), (wp, bh.float())), {}, "expected scalar type Half but found Float (bias_h)"),
    ]
    for args, kw, message in cases:
        with pytest.raises(RuntimeError) as info:
            f(*args, **kw)
        assert str(info.value) == message
        assert type(info.value) is (lgu._lib.UnsupportedShape if message.startswith(served) else RuntimeError)


# ---- GPU ------------------------------------------------------------------------------------------------------------
def _need_gpu(lgu):
    assert torch.cuda.is_available(), "these tests need the MI355X"
    assert os.path.exists(lgu._lib.so_path()), "liblgu_corr.so missing — run __graft_entry__.build()"


def _stem_pack(lgu, conv):
    return lgu.encconv.pack_stem(conv.weight.detach().cuda(), conv.bias.detach().cuda())


def _out_pack(lgu, conv):
    return lgu.encconv.pack_out1(conv.weight.detach().cuda(), conv.bias.detach().cuda())


# in a 13x13 image: the corners, the centre, even and odd rows and columns in every combination, the last row and column
IMPULSE_AT = [(0, 0), (0, 12), (12, 0), (12, 12), (6, 6), (5, 5), (6, 5), (5, 6), (4, 7), (7, 4), (11, 12), (12, 11), (1, 0)]


@pytest.mark.gpu
def test_stem_impulses_give_bias_plus_weight_bit_for_bit(lgu):
    """One input element v (1, or -2 at every other position; each of the 3 channels) in a 13x13 image: b_h + v w_h is exact
    in fp32 (both are half values below 1/4 with no bit under 2^-24), so output (y, x) is half(b_h + v w_h[co, c, cy - 2 y + 3,
    cx - 2 x + 3]) where that tap exists and half(b_h) elsewhere, torch's rule, bit for bit."""
    _need_gpu(lgu)
    conv = R.make_stem(43)
    wh, bh = conv.weight.detach().half(), conv.bias.detach().half()
    assert float(wh.abs().max()) < 0.125 and float(bh.abs().max()) < 0.125
    x = torch.zeros((len(IMPULSE_AT) * 3, 3, 13, 13), dtype=torch.float32)
    want = bh.view(1, 32, 1, 1).expand(x.shape[0], 32, 7, 7).clone()
    hit = torch.zeros((x.shape[0], 1, 7, 7), dtype=torch.bool)
    for i, (cy, cx) in enumerate(IMPULSE_AT):
        v = 1.0 if i % 2 == 0 else -2.0
        for c in range(3):
            n = 3 * i + c
            x[n, c, cy, cx] = v
            for ky in range(7):
                for kx in range(7):
                    ny, nx = cy - ky + 3, cx - kx + 3         # = 2 y, 2 x of the output that sees it through (ky, kx)
                    if ny % 2 == 0 and nx % 2 == 0 and 0 <= ny // 2 < 7 and 0 <= nx // 2 < 7:
                        want[n, :, ny // 2, nx // 2] = (bh.double() + v * wh[:, c, ky, kx].double()).half()
                        hit[n, 0, ny // 2, nx // 2] = True
    ref = torch.nn.functional.conv2d(x.double(), wh.double(), bh.double(), stride=2, padding=3)
    assert same_bits(ref.half(), want) and bool((ref.float().double() == ref).all())   # torch's rule; the sums are exact in fp32
    reach = torch.nn.functional.conv2d((x != 0).double().sum(1, keepdim=True), torch.ones((1, 1, 7, 7), dtype=torch.float64), stride=2, padding=3) > 0
    assert torch.equal(reach, hit) and int(hit[12].sum()) == 9 and int(hit[15].sum()) == 16 and int(hit[0].sum()) == 4
    pack = _stem_pack(lgu, conv)
    for xin in (x, x.half()):
        got = lgu.encconv.enc_stem7x7(xin.cuda(), pack)
        torch.cuda.synchronize()
        assert same_bits(got, want), "max |diff| %g" % float((got.cpu().float() - want.float()).abs().max())
        assert same_bits(lgu.encconv.enc_stem7x7(xin.cuda(), pack, relu=True), torch.relu(want))
    assert int((torch.relu(want) != want).sum()) > 0


@pytest.mark.gpu
@pytest.mark.parametrize("size", [(1, 1, 1), (2, 9, 33), (1, 17, 130)])
def test_zero_input_gives_act_of_the_bias_everywhere(lgu, size):
    _need_gpu(lgu)
    conv = R.make_stem(44)
    pack = _stem_pack(lgu, conv)
    osz = (size[0], 32) + R.out_size(size[1], size[2])
    bh = conv.bias.detach().half().view(1, -1, 1, 1).expand(osz)
    assert bool((bh < 0).any()) and bool((bh > 0).any())
    for dt in (torch.float32, torch.float16):
        x = torch.zeros((size[0], 3, size[1], size[2]), dtype=dt, device="cuda")
        assert same_bits(lgu.encconv.enc_stem7x7(x, pack), bh)
        assert same_bits(lgu.encconv.enc_stem7x7(x, pack, relu=True), torch.relu(bh))
    for cout in R.COUTS:
        conv = R.make_out(45, cout)
        pack = _out_pack(lgu, conv)
        x = torch.zeros((size[0], 128, size[1], size[2]), dtype=torch.float16, device="cuda")
        bh = conv.bias.detach().half().view(1, -1, 1, 1).expand((size[0], cout) + size[1:])
        assert same_bits(lgu.encconv.enc_out1x1(x, pack), bh)
        if cout == 256:
            net, inp = lgu.encconv.enc_out1x1(x, pack, split=True)
            assert same_bits(inp, torch.relu(bh[:, 128:]))
            t, bound = R.tanh_bound(bh[:, :128].double())
            assert bool(((net.cpu().double() - t).abs() <= bound).all())


@pytest.mark.gpu
@pytest.mark.parametrize("size", R.STEM_SIZES, ids=lambda s: "%dx%dx%d" % s)
def test_stem_every_element_is_within_the_derived_bound(lgu, size):
    """Every element of the identity output within allowance(s64, S, 149); the ReLU form bit for bit torch.relu of it; a half
    input gives the bits of the float32 input it is the rounding of."""
    _need_gpu(lgu)
    conv, x, s64, S = stem_case(size)
    pack = _stem_pack(lgu, conv)
    f = lgu.encconv.enc_stem7x7
    y0, y1 = f(x.cuda(), pack), f(x.cuda(), pack, relu=True)
    torch.cuda.synchronize()
    assert y0.dtype == torch.float16 and y0.is_contiguous() and tuple(y0.shape) == tuple(s64.shape)
    allow = R.allowance(s64, S, R.STEM_TERMS)
    err = (y0.cpu().double() - s64).abs()
    worst = float((err / allow).max())
    print("stem %s: max |err| %.3e, max err / allowance %.3f" % (size, float(err.max()), worst))
    assert bool((err <= allow).all()), worst
    assert same_bits(y1, torch.relu(y0))
    assert size == (1, 1, 1) or int((y1 != y0).sum()) > 0
    xh = x.half()
    assert not torch.equal(xh.float(), x)
    assert same_bits(f(xh.cuda(), pack), y0) and same_bits(f(xh.cuda(), pack, relu=True), y1)
    assert same_bits(f(xh.float().cuda(), pack), y0)


@pytest.mark.gpu
@pytest.mark.parametrize("size", R.OUT_SIZES, ids=lambda s: "%dx%dx%d" % s)
@pytest.mark.parametrize("cout", R.COUTS)
def test_out_every_element_is_within_the_derived_bound(lgu, cout, size):
    """Every element of h within allowance(s64, S, 130); SPLIT: inp bit for bit torch.relu(h[:, 128:]), net within the tanh
    bound of h[:, :128] (the number of elements whose bits differ from torch.tanh's is printed)."""
    _need_gpu(lgu)
    conv, x, s64, S = out_case(cout, size)
    pack = _out_pack(lgu, conv)
    h = lgu.encconv.enc_out1x1(x.cuda(), pack)
    torch.cuda.synchronize()
    assert h.dtype == torch.float16 and h.is_contiguous() and tuple(h.shape) == tuple(s64.shape)
    allow = R.allowance(s64, S, R.OUT_TERMS)
    err = (h.cpu().double() - s64).abs()
    worst = float((err / allow).max())
    print("out %d %s: max |err| %.3e, max err / allowance %.3f" % (cout, size, float(err.max()), worst))
    assert bool((err <= allow).all()), worst
    if cout == 256:
        net, inp = lgu.encconv.enc_out1x1(x.cuda(), pack, split=True)
        assert net.is_contiguous() and inp.is_contiguous() and tuple(net.shape) == tuple(inp.shape) == (size[0], 128) + size[1:]
        assert same_bits(inp, torch.relu(h[:, 128:]))
        t, bound = R.tanh_bound(h[:, :128].cpu().double())
        terr = (net.cpu().double() - t).abs()
        differ = int((net != torch.tanh(h[:, :128])).sum())
        print("out 256 %s split: tanh max err / bound %.3f, %d of %d elements differ from torch.tanh's bits"
              % (size, float((terr / bound).max()), differ, net.numel()))
        assert bool((terr <= bound).all())
    else:
        with pytest.raises(RuntimeError, match="needs Cout = 256"):
            lgu.encconv.enc_out1x1(x.cuda(), pack, split=True)


@pytest.mark.gpu
def test_split_keeps_infinities_and_nan(lgu):
    """One infinite input gives h = +-inf by the sign of its weight: net = +-1 and inp = inf or 0 there; a NaN input gives NaN
    in net and inp at its pixel; every other pixel has the clean call's bits."""
    _need_gpu(lgu)
    conv, x, _, _ = out_case(256, (2, 9, 33))
    pack = _out_pack(lgu, conv)
    x = x.clone()
    x[1, 5, 2, 7] = float("inf")
    x[0, 77, 8, 32] = float("nan")
    xc = x.cuda()
    h = lgu.encconv.enc_out1x1(xc, pack).cpu()
    net, inp = (t.cpu() for t in lgu.encconv.enc_out1x1(xc, pack, split=True))
    clean_net, clean_inp = (t.cpu() for t in lgu.encconv.enc_out1x1(out_case(256, (2, 9, 33))[1].cuda(), pack, split=True))
    hi = h[1, :, 2, 7]
    wsign = torch.sign(conv.weight.detach().half()[:, 5, 0, 0].float())
    assert bool(torch.isinf(hi).all()) and torch.equal(torch.sign(hi.float()), wsign)
    assert bool((wsign[:128] > 0).any()) and bool((wsign[:128] < 0).any()) and bool((wsign[128:] > 0).any()) and bool((wsign[128:] < 0).any())
    assert same_bits(net[1, :, 2, 7], wsign[:128].half())                        # tanh(+-inf) = +-1
    assert same_bits(inp[1, :, 2, 7], torch.relu(hi[128:]))                      # inf or 0
    assert bool(torch.isnan(h[0, :, 8, 32]).all()) and bool(torch.isnan(net[0, :, 8, 32]).all()) and bool(torch.isnan(inp[0, :, 8, 32]).all())
    touched = torch.zeros((2, 1, 9, 33), dtype=torch.bool)
    touched[1, 0, 2, 7] = touched[0, 0, 8, 32] = True
    keep = ~touched.expand(-1, 128, -1, -1)
    assert same_bits(net[keep], clean_net[keep]) and same_bits(inp[keep], clean_inp[keep])
    assert int(torch.isnan(net).sum()) == int(torch.isnan(inp).sum()) == 128


NAN_SIZES = [(1, 1, 1), (1, 2, 3), (2, 9, 33), (2, 10, 34), (1, 5, 65)]


@pytest.mark.gpu
@pytest.mark.parametrize("size", NAN_SIZES, ids=lambda s: "%dx%dx%d" % s)
def test_stem_nan_reaches_exactly_its_window(lgu, size):
    """NaNs (and an infinity) at the corners, the last row and column and interior even and odd positions of x: y is not
    finite exactly where a float64 convolution of the mask with ones is positive (torch's rule for stride and padding),
    NaN for a NaN, and every other output keeps the clean call's bits."""
    _need_gpu(lgu)
    conv, x, _, _ = stem_case(size)
    pack = _stem_pack(lgu, conv)
    N, H, W = size
    ats = sorted({(0, 0), (H - 1, W - 1), (0, W - 1), (H - 1, 0), (H // 2, W // 2), (H // 2 | 1 if H > 1 else 0, W // 2 | 1 if W > 1 else 0),
                  (min(H - 1, 4), min(W - 1, 63)), (min(H - 1, 5), min(W - 1, 64))})
    F = torch.nn.functional
    clean = lgu.encconv.enc_stem7x7(x.cuda(), pack).cpu()
    for k, (cy, cx) in enumerate(ats):
        for bad in (float("nan"),) + ((float("inf"),) if k == 0 else ()):
            xn = x.clone()
            xn[N - 1, k % 3, cy, cx] = bad
            mask = torch.zeros((N, 1, H, W), dtype=torch.float64)
            mask[N - 1, 0, cy, cx] = 1.0
            hit = (F.conv2d(mask, torch.ones((1, 1, 7, 7), dtype=torch.float64), stride=2, padding=3) > 0).expand(-1, 32, -1, -1)
            for relu in (False, True):
                for xin in (xn, xn.half()):
                    got = lgu.encconv.enc_stem7x7(xin.cuda(), pack, relu=relu).cpu()
                    bad_out = torch.isnan(got) if bad != bad else ~torch.isfinite(got)
                    if bad == bad and relu:        # relu(-inf) = 0: only the positive side stays infinite
                        assert bool((bad_out <= hit).all())
                    else:
                        assert torch.equal(bad_out, hit), (cy, cx, relu)
                    want = torch.relu(clean) if relu else clean
                    assert same_bits(got[~hit], want[~hit]), (cy, cx, relu)


@pytest.mark.gpu
@pytest.mark.parametrize("size", [(1, 1, 1), (2, 9, 33), (1, 5, 65)], ids=lambda s: "%dx%dx%d" % s)
@pytest.mark.parametrize("cout", R.COUTS)
def test_out_nan_reaches_exactly_its_pixel(lgu, cout, size):
    _need_gpu(lgu)
    conv, x, _, _ = out_case(cout, size)
    pack = _out_pack(lgu, conv)
    N, H, W = size
    clean = lgu.encconv.enc_out1x1(x.cuda(), pack).cpu()
    for k, (cy, cx) in enumerate(sorted({(0, 0), (H - 1, W - 1), (H // 2, W // 2), (H - 1, 0), (min(H - 1, 3), min(W - 1, 15))})):
        xn = x.clone()
        xn[N - 1, (37 * k + 5) % 128, cy, cx] = float("nan")
        hit = torch.zeros((N, cout, H, W), dtype=torch.bool)
        hit[N - 1, :, cy, cx] = True
        got = lgu.encconv.enc_out1x1(xn.cuda(), pack).cpu()
        assert torch.equal(torch.isnan(got), hit) and same_bits(got[~hit], clean[~hit])
        if cout == 256:
            net, inp = (t.cpu() for t in lgu.encconv.enc_out1x1(xn.cuda(), pack, split=True))
            assert torch.equal(torch.isnan(net), hit[:, :128]) and torch.equal(torch.isnan(inp), hit[:, 128:])


@pytest.mark.gpu
@pytest.mark.parametrize("size", [(9, 33), (10, 34), (17, 130)], ids=lambda s: "%dx%d" % s)
def test_an_image_does_not_depend_on_its_batch(lgu, size):
    _need_gpu(lgu)
    E = lgu.encconv
    conv = R.make_stem(46)
    pack = _stem_pack(lgu, conv)
    x3 = R.make_image(77, 3, *size).cuda()
    for relu in (False, True):
        whole = E.enc_stem7x7(x3, pack, relu=relu)
        for i in range(3):
            assert same_bits(whole[i:i + 1], E.enc_stem7x7(x3[i:i + 1].contiguous(), pack, relu=relu)), (i, relu)
    for cout in R.COUTS:
        conv = R.make_out(47, cout)
        pack = _out_pack(lgu, conv)
        f3 = R.make_features(78, 3, *size).half().cuda()
        whole = E.enc_out1x1(f3, pack)
        parts = E.enc_out1x1(f3, pack, split=True) if cout == 256 else None
        for i in range(3):
            one = f3[i:i + 1].contiguous()
            assert same_bits(whole[i:i + 1], E.enc_out1x1(one, pack)), (cout, i)
            if parts is not None:
                net, inp = E.enc_out1x1(one, pack, split=True)
                assert same_bits(parts[0][i:i + 1], net) and same_bits(parts[1][i:i + 1], inp)


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _stem_call(lgu, a, size, flags, cin=3, cout=32):
    args = lgu._lib.EncStemArgs(a["x"].data_ptr(), a["wpack"].data_ptr(), a["bias"].data_ptr(), a["out"].data_ptr(),
                                size[0], size[1], size[2], cin, cout, flags)
    rc = lgu._lib.load().lgu_encstem7x7_h16(args, _stream())
    torch.cuda.synchronize()
    return rc


def _out_call(lgu, a, size, flags, cin=128, cout=256):
    args = lgu._lib.EncOutArgs(a["x"].data_ptr(), a["wpack"].data_ptr(), a["bias"].data_ptr(), a["out"].data_ptr(),
                               a["inp"].data_ptr() if flags & lgu.encconv.SPLIT else None, size[0], size[1], size[2], cin, cout, flags)
    rc = lgu._lib.load().lgu_encout1x1_c128_h16(args, _stream())
    torch.cuda.synchronize()
    return rc


def _audit(lgu, base, written, call, want, shifts):
    """Every operand shifted off its 16-byte boundary in turn and all of them by one element: the aligned call's bits and
    intact guard bands, or for the pack a refusal that writes nothing."""
    from tests.alignment_cases import guards_intact, shifted
    variants = [([k], s) for k in base for s in shifts[base[k].dtype]]
    variants += [([k for k in base if k != "wpack"], None)]                    # everything at an odd element offset
    for keys, shift in variants:
        args = dict(base)
        for k in keys:
            args[k] = shifted(base[k], shift if shift is not None else base[k].element_size())
        for k in written:
            if k not in keys:
                args[k] = shifted(base[k], 0)
            args[k].fill_(float("nan"))
        before = {k: args[k].clone() for k in args}
        rc = call(args)
        if "wpack" in keys:
            assert rc == lgu._lib.LGU_E_UNSUPPORTED, (keys, shift, rc)
            assert all(same_bits(args[k], before[k]) for k in written), "refused, but an output changed"
        else:
            assert rc == 0, (keys, shift, rc)
            for k in written:
                assert same_bits(args[k], want[k]), "%s shifted by %s: %s differs from the aligned call" % (keys, shift, k)
        for k in base:
            if k not in written:
                assert same_bits(args[k], before[k]), "read-only operand %s changed" % k
        for k in set(keys) | set(written):
            assert guards_intact(args[k]), "%s, %s: a guard band of %s was written" % (keys, shift, k)


_SHIFTS = {torch.float32: (4, 8), torch.float16: (2, 4, 8)}


@pytest.mark.gpu
@pytest.mark.parametrize("half", [False, True], ids=["f32", "h16"])
@pytest.mark.parametrize("size", [(2, 9, 33), (2, 10, 34), (1, 16, 32)], ids=lambda s: "%dx%dx%d" % s)
def test_stem_guard_bands_and_alignment(lgu, size, half):
    """The alignment audit of DESIGN.md §4.1 for lgu_encstem7x7_h16: x, bias and out are served at element alignment with
    the aligned call's bits (by element where out is not 8-byte aligned or W_out % 4 != 0: W 33 and 34 give W_out 17, 1x16x32
    the 8-byte path), out inside a sentinel-filled buffer, a pack that is not 16-byte aligned is refused with nothing
    launched, and so are the other bad calls."""
    from tests.alignment_cases import guards_intact, shifted
    _need_gpu(lgu)
    E = lgu.encconv
    conv = R.make_stem(48)
    wpack, bias_h = _stem_pack(lgu, conv)
    x = R.make_image(5, *size).cuda()
    x = x.half() if half else x
    osz = (size[0], 32) + R.out_size(size[1], size[2])
    base = {"x": x, "wpack": wpack, "bias": bias_h, "out": torch.empty(osz, dtype=torch.float16, device="cuda")}
    assert all(t.data_ptr() % 16 == 0 for t in base.values())
    xf = E.X_HALF if half else 0
    for flags, relu in ((xf, False), (xf | E.STEM_RELU, True)):
        want = {"out": E.enc_stem7x7(x, (wpack, bias_h), relu=relu)}
        _audit(lgu, base, ["out"], lambda a: _stem_call(lgu, a, size, flags), want, _SHIFTS)
    # empty and bad calls launch nothing
    args = dict(base, out=shifted(base["out"], 0))
    args["out"].fill_(float("nan"))
    before = args["out"].clone()
    BAD, UNS = lgu._lib.LGU_E_BADARG, lgu._lib.LGU_E_UNSUPPORTED
    assert _stem_call(lgu, args, (0,) + size[1:], xf) == 0
    assert _stem_call(lgu, args, (-1,) + size[1:], xf) == BAD
    assert _stem_call(lgu, args, (size[0], 0, size[2]), xf) == BAD and _stem_call(lgu, args, (size[0], size[1], 0), xf) == BAD
    assert _stem_call(lgu, args, size, xf | 4) == BAD
    assert _stem_call(lgu, args, size, xf, cin=4) == UNS and _stem_call(lgu, args, size, xf, cout=64) == UNS
    a = lgu._lib.EncStemArgs(x.data_ptr(), wpack.data_ptr(), bias_h.data_ptr(), None, size[0], size[1], size[2], 3, 32, xf)
    assert lgu._lib.load().lgu_encstem7x7_h16(a, _stream()) == BAD              # a null output
    a.out, a.bias = args["out"].data_ptr(), None
    assert lgu._lib.load().lgu_encstem7x7_h16(a, _stream()) == BAD              # a null bias
    if not half:
        a.bias, a.x = bias_h.data_ptr(), x.data_ptr() + 2
        assert lgu._lib.load().lgu_encstem7x7_h16(a, _stream()) == BAD          # a float x below its element's alignment
    torch.cuda.synchronize()
    assert same_bits(args["out"], before) and guards_intact(args["out"])
    assert tuple(E.enc_stem7x7(x[:0], (wpack, bias_h)).shape) == (0,) + osz[1:]
    with pytest.raises(RuntimeError, match=r"enc_stem7x7: empty frame \(H\*W = 0\)"):
        E.enc_stem7x7(x[:, :, :0], (wpack, bias_h))


@pytest.mark.gpu
@pytest.mark.parametrize("cout", R.COUTS)
@pytest.mark.parametrize("size", [(2, 9, 33), (2, 10, 34), (1, 4, 8)], ids=lambda s: "%dx%dx%d" % s)
def test_out_guard_bands_and_alignment(lgu, size, cout):
    """The same audit for lgu_encout1x1_c128_h16: x, bias, out and inp at element alignment (by element where a pointer is
    not 8-byte aligned or H W % 4 != 0: 9x33 is odd, 10x34 and 4x8 take the 8-byte path), both outputs inside sentinel-filled
    buffers, a misaligned pack refused."""
    from tests.alignment_cases import guards_intact, shifted
    _need_gpu(lgu)
    E = lgu.encconv
    conv = R.make_out(49, cout)
    wpack, bias_h = _out_pack(lgu, conv)
    x = R.make_features(6, *size).half().cuda()
    osz = (size[0], cout) + size[1:]
    base = {"x": x, "wpack": wpack, "bias": bias_h, "out": torch.empty(osz, dtype=torch.float16, device="cuda")}
    _audit(lgu, base, ["out"], lambda a: _out_call(lgu, a, size, 0, cout=cout), {"out": E.enc_out1x1(x, (wpack, bias_h))}, _SHIFTS)
    psz = (size[0], 128) + size[1:]
    if cout == 256:
        net, inp = E.enc_out1x1(x, (wpack, bias_h), split=True)
        sbase = dict(base, out=torch.empty(psz, dtype=torch.float16, device="cuda"), inp=torch.empty(psz, dtype=torch.float16, device="cuda"))
        _audit(lgu, sbase, ["out", "inp"], lambda a: _out_call(lgu, a, size, E.SPLIT), {"out": net, "inp": inp}, _SHIFTS)
    # empty and bad calls launch nothing
    args = dict(base, out=shifted(base["out"], 0), inp=shifted(torch.empty(psz, dtype=torch.float16, device="cuda"), 0))
    for k in ("out", "inp"):
        args[k].fill_(float("nan"))
    before = {k: args[k].clone() for k in ("out", "inp")}
    BAD, UNS = lgu._lib.LGU_E_BADARG, lgu._lib.LGU_E_UNSUPPORTED
    call = lambda sz, flags, **kw: _out_call(lgu, args, sz, flags, **dict(dict(cout=cout), **kw))  # noqa: E731
    assert call((0,) + size[1:], 0) == 0
    assert call((-1,) + size[1:], 0) == BAD and call((size[0], 0, size[2]), 0) == BAD and call((size[0], size[1], 0), 0) == BAD
    assert call(size, 2) == BAD
    assert call(size, 0, cin=64) == UNS and call(size, 0, cout=192) == UNS and call(size, 0, cout=64) == UNS
    assert call(size, E.SPLIT, cout=128) == BAD                                # SPLIT is Cout 256's
    a = lgu._lib.EncOutArgs(x.data_ptr(), wpack.data_ptr(), bias_h.data_ptr(), args["out"].data_ptr(), args["inp"].data_ptr(),
                            size[0], size[1], size[2], 128, cout, 0)
    assert lgu._lib.load().lgu_encout1x1_c128_h16(a, _stream()) == BAD          # inp without the flag
    a.inp, a.Cout, a.flags = None, 256, E.SPLIT
    assert lgu._lib.load().lgu_encout1x1_c128_h16(a, _stream()) == BAD          # the flag without inp
    a.flags, a.Cout, a.out = 0, cout, None
    assert lgu._lib.load().lgu_encout1x1_c128_h16(a, _stream()) == BAD          # a null output
    torch.cuda.synchronize()
    assert all(same_bits(args[k], before[k]) and guards_intact(args[k]) for k in ("out", "inp"))
    assert tuple(E.enc_out1x1(x[:0], (wpack, bias_h)).shape) == (0,) + osz[1:]
    if cout == 256:
        net, inp = E.enc_out1x1(x[:0], (wpack, bias_h), split=True)
        assert tuple(net.shape) == tuple(inp.shape) == (0,) + psz[1:]
    with pytest.raises(RuntimeError, match=r"enc_out1x1: empty frame \(H\*W = 0\)"):
        E.enc_out1x1(x[:, :, :0], (wpack, bias_h))
