"""The fused residual-stage convolutions of the encoders (lgu_slam_amd.encconv, csrc/encconv.hip) against the float64
restatement of their rounding model, tests/encconv_restatement.py.

Numerics contract (include/lgu_corr.h):
- a single product is exact: impulses and the zero input are bit for bit, with stride 2 at even and odd rows and columns;
- every element of y: |y - epilogue(s64)| <= allowance(s64, S, 9 Cin + 2) of tests/conv3_restatement.py, widened for the
  residual epilogue by the one further half rounding, 2^-11 (|res + relu(s64)| + allowance) + 2^-25; every element of r:
  allowance(r64, Sr, Cin + 2);
- RELU and RESIDUAL are bit for bit torch's relu and relu(res + relu(.)) of the identity output on the device;
- r does not depend on the 3x3 pack, y not on the presence of the branch, an image not on its batch;
- NaN reaches exactly its stride-aware neighbourhood in y, its one pixel in r, and from res one element.
The alignment audit of lgu_encconv3x3_h16 (its operands travel in a parameter block) is test_guard_bands_and_alignment.
The GPU tests build their layers themselves and never read the reference tree.
"""
import ctypes
import os

import pytest

torch = pytest.importorskip("torch")

from tests import encconv_restatement as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = "lgu_encconv3x3_h16"
SHAPES = R.SHAPES
_NO_CPU = " must be a HIP device tensor: lgu_slam_amd has no CPU fallback"
_CASES = {}
_IDS = ["%d-%d-s%d" % s for s in SHAPES]


def same_bits(a, b):
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    iv = torch.int16 if a.dtype == torch.float16 else torch.int32
    return bool(torch.equal(a.view(iv), b.view(iv)))


def case(shape, size):
    """(c3, c1, x half, res half, s64, S, r64, Sr) on the CPU for one layer shape and input size, computed once and never
    changed."""
    if (shape, size) not in _CASES:
        cin, cout, st = shape
        c3, c1 = R.make_layer(70 + cin + cout, *shape)
        x = R.make_input(2000 + size[1] * size[2], *size, C=cin).half()
        res = R.make_residual(3000 + size[1] * size[2], (size[0], cout) + R.out_size(size[1], size[2], st))
        with torch.no_grad():
            _CASES[(shape, size)] = (c3, c1, x, res) + R.conv(x, c3, c1)
    return _CASES[(shape, size)]


# ---- CPU ------------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_entry(lgu):
    from tests.test_abi import declared_symbols
    lib = ctypes.CDLL(lgu._lib._build.SO_PATH)
    assert ENTRY in declared_symbols() and hasattr(lib, ENTRY)
    sig = lgu._lib.SIGNATURES[ENTRY]
    assert sig[0] is lgu._lib.EncConvArgs and issubclass(sig[0], ctypes.Structure) and sig[1] is ctypes.c_void_p
    assert [f[0] for f in sig[0]._fields_] == ["x", "wpack", "bias", "res", "out", "dpack", "dbias", "r", "N", "H", "W", "Cin",
                                              "Cout", "stride", "flags"]
    assert ctypes.sizeof(sig[0]) == 8 * 8 + 7 * 4 + 4
    assert "encconv.hip" in lgu._build.SOURCES
    assert lgu.ContextEncoder is lgu.context.ContextEncoder and lgu.enc_conv3x3 is lgu.encconv.enc_conv3x3
    assert lgu.pack_enc3 is lgu.encconv.pack_enc3 and lgu.pack_enc1 is lgu.encconv.pack_enc1
    text = open(os.path.join(ROOT, "include", "lgu_corr.h")).read()
    assert "#define LGU_ENCCONV_RELU %d " % lgu.encconv.RELU in text and "#define LGU_ENCCONV_RESIDUAL %d " % lgu.encconv.RESIDUAL in text
    assert lgu.encconv.SHAPES == SHAPES and set(lgu.encconv.MIN_FUSED_PIXELS) == set(SHAPES)
    assert lgu.__version__ == "0.8.0"


@pytest.mark.parametrize("shape", SHAPES, ids=_IDS)
def test_packs_put_every_weight_in_its_documented_slot_and_nothing_else(lgu, shape):
    cin, cout, st = shape
    g = torch.Generator().manual_seed(5)
    w = torch.randn((cout, cin, 3, 3), generator=g)
    b = torch.randn((cout,), generator=g)
    wpack, bias_h = lgu.encconv.pack_enc3(w, b)
    assert wpack.dtype == torch.float16 and wpack.is_contiguous() and wpack.numel() == 9 * cin * cout
    assert tuple(wpack.shape) == (9, cin // 32, cout // 16, 64, 8) and same_bits(bias_h, b.half())
    # a weight tensor that names its own index: the value at (co, c, ky, kx) is its flat index, exact in int32
    idx = torch.arange(cout * cin * 9, dtype=torch.int32).view(cout, cin, 3, 3)
    t, kc, ct, lane, j = torch.meshgrid(torch.arange(9), torch.arange(cin // 32), torch.arange(cout // 16), torch.arange(64),
                                        torch.arange(8), indexing="ij")
    co, c, ky, kx = 16 * ct + (lane & 15), 32 * kc + 8 * (lane >> 4) + j, t // 3, t % 3
    assert sorted(idx[co, c, ky, kx].flatten().tolist()) == list(range(cout * cin * 9))   # every weight once, nothing else
    assert same_bits(wpack, w.half()[co, c, ky, kx])
    for bad in (w[:, :16], torch.zeros(48, cin, 3, 3), torch.zeros(cout, cin, 1, 1), torch.zeros(32, 64, 3, 3)):
        with pytest.raises(RuntimeError, match="pack_enc3: weight must be"):
            lgu.encconv.pack_enc3(bad, b)
    with pytest.raises(RuntimeError, match="bias must be"):
        lgu.encconv.pack_enc3(w, b[:-1])
    if st == 2:
        w1 = torch.randn((cout, cin, 1, 1), generator=g)
        dpack, dbias_h = lgu.encconv.pack_enc1(w1, b)
        assert dpack.dtype == torch.float16 and dpack.is_contiguous() and tuple(dpack.shape) == (cin // 32, cout // 16, 64, 8)
        assert same_bits(dbias_h, b.half())
        idx = torch.arange(cout * cin, dtype=torch.int32).view(cout, cin)
        kc, ct, lane, j = torch.meshgrid(torch.arange(cin // 32), torch.arange(cout // 16), torch.arange(64), torch.arange(8),
                                         indexing="ij")
        co, c = 16 * ct + (lane & 15), 32 * kc + 8 * (lane >> 4) + j
        assert sorted(idx[co, c].flatten().tolist()) == list(range(cout * cin))
        assert same_bits(dpack, w1.half()[co, c, 0, 0])
        for bad in (w, torch.zeros(cout, cout, 1, 1), torch.zeros(cin, cin, 1, 1)):
            with pytest.raises(RuntimeError, match="pack_enc1: weight must be"):
                lgu.encconv.pack_enc1(bad, b)
        with pytest.raises(RuntimeError, match="bias must be"):
            lgu.encconv.pack_enc1(w1, b[:-1])


@pytest.mark.parametrize("size", [(1, 1, 1), (1, 2, 3), (2, 9, 33)])
@pytest.mark.parametrize("shape", SHAPES, ids=_IDS)
def test_restatement_equals_float64_conv2d_on_the_rounded_operands(shape, size):
    c3, c1, x, res, s64, S, r64, Sr = case(shape, size)
    cin, cout, st = shape
    F = torch.nn.functional
    xh, wh, bh = R.h64(x), R.h64(c3.weight), R.h64(c3.bias)
    s = F.conv2d(xh, wh, bh, stride=st, padding=1)
    Sc = F.conv2d(xh.abs(), wh.abs(), bh.abs(), stride=st, padding=1)
    # the operands are half values, so every product is exact in float64; the two sums differ in order only
    assert s.shape == s64.shape == (size[0], cout) + R.out_size(size[1], size[2], st)
    assert bool(((s - s64).abs() <= 2.0 ** -44 * S).all()) and bool(((Sc - S).abs() <= 2.0 ** -44 * S).all())
    assert bool((S >= s64.abs()).all()) and bool((R.allowance(s64, S, R.terms3(cin)) > 0).all())
    if st == 2:
        r = F.conv2d(xh, R.h64(c1.weight), R.h64(c1.bias), stride=2)
        assert r.shape == r64.shape == s64.shape
        assert bool(((r - r64).abs() <= 2.0 ** -44 * Sr).all()) and bool((Sr >= r64.abs()).all())
    else:
        assert r64 is None and Sr is None
    r64d = res.double()
    assert torch.equal(R.epilogue(s64, "identity"), s64) and torch.equal(R.epilogue(s64, "relu"), torch.relu(s64))
    assert torch.equal(R.epilogue(s64, "residual", r64d), torch.relu(r64d + torch.relu(s64)))
    a = R.allowance(s64, S, R.terms3(cin))
    assert torch.equal(R.allowed(s64, S, R.terms3(cin), "relu"), a)
    wide = R.allowed(s64, S, R.terms3(cin), "residual", r64d)
    assert torch.equal(wide, a + 2.0 ** -11 * ((r64d + torch.relu(s64)).abs() + a) + 2.0 ** -25)
    assert R.terms3(cin) == 9 * cin + 2 and R.terms1(cin) == cin + 2
    assert bool((x == 0).any()) and bool((res == 0).any()) and bool((res < 0).any())


def test_operator_refusals_in_their_order(lgu):
    """x's rank, stride, the pack, the bias's rank, the served shapes, the pack size, x's dtype, the residual, the branch,
    then contiguity, dtypes, no-grad and device: each refusal's text, and which of two defects is reported.  None of them
    touches a device."""
    f = lgu.encconv.enc_conv3x3
    H = torch.float16

    def z(*shape, dtype=H):
        return torch.zeros(shape, dtype=dtype)

    def nc(t):
        return torch.zeros(tuple(t.shape) + (2,), dtype=t.dtype)[..., 0]

    x, wp, bh = z(1, 32, 4, 6), z(9, 1, 4, 64, 8), z(64)
    dp, res = z(1, 4, 64, 8), z(1, 64, 2, 3)
    no_grad = "enc_conv3x3 has no autograd: its outputs would carry no gradient. Call it under torch.no_grad() or pass detached inputs"
    served = "enc_conv3x3 serves (Cin, Cout, stride) in %s, got " % (list(SHAPES),)
    k = dict(stride=2)
    cases = [
        ((x, (wp, bh)), k, "x" + _NO_CPU),
        ((z(32, 4, 6), (wp, bh)), k, "x must be (N,Cin,H,W), got (32, 4, 6)"),
        ((x, (wp, bh)), dict(stride=3), "stride must be 1 or 2, got 3"),
        ((x, wp), k, "pack must be (wpack, bias_h) of pack_enc3"),
        ((x, (wp, z(64, 1))), k, "bias_h must be (Cout,), got (64, 1)"),
        ((x, (wp, bh)), dict(stride=1), served + "(32, 64, 1)"),
        ((z(1, 48, 4, 6), (wp, bh)), k, served + "(48, 64, 2)"),
        ((x, (z(9, 1, 4, 64, 7), bh)), k, "wpack must hold 18432 halves (pack_enc3, 32 -> 64), got (9, 1, 4, 64, 7)"),
        ((x.float(), (wp, bh)), k, "expected scalar type Half but found Float (x)"),
        ((x, (wp, bh)), dict(stride=2, residual=z(1, 64, 4, 6)), "residual must be (1, 64, 2, 3), got (1, 64, 4, 6)"),
        ((x, (wp, bh)), dict(stride=2, residual=res.float()), "expected scalar type Half but found Float (residual)"),
        ((z(1, 32, 4, 6), (z(9, 1, 2, 64, 8), z(32))), dict(stride=1, down=(dp, bh)), "down (the 1x1 stride-2 branch) needs stride=2"),
        ((x, (wp, bh)), dict(stride=2, down=dp), "down must be (dpack, dbias_h) of pack_enc1"),
        ((x, (wp, bh)), dict(stride=2, down=(z(1, 4, 64, 7), bh)), "dpack must hold 2048 halves (pack_enc1, 32 -> 64), got (1, 4, 64, 7)"),
        ((x, (wp, bh)), dict(stride=2, down=(dp, z(32))), "dbias_h must be (64,), got (32,)"),
        ((nc(x), (wp, bh)), k, "x must be contiguous"),
        ((x, (nc(wp), bh)), k, "wpack must be contiguous"),
        ((x, (wp, nc(bh))), k, "bias_h must be contiguous"),
        ((x, (wp, bh)), dict(stride=2, residual=nc(res)), "residual must be contiguous"),
        ((x, (wp, bh)), dict(stride=2, down=(nc(dp), bh)), "dpack must be contiguous"),
        ((x, (wp.float(), bh)), k, "expected scalar type Half but found Float (wpack)"),
        ((x, (wp, bh.bfloat16())), k, "expected scalar type Half but found BFloat16 (bias_h)"),
        ((x, (wp, bh)), dict(stride=2, down=(dp, bh.float())), "expected scalar type Half but found Float (dbias_h)"),
        ((x.clone().requires_grad_(), (wp, bh)), k, no_grad),
        # two defects: the earlier check reports
        ((z(32, 4, 6), (wp, bh)), dict(stride=3), "x must be (N,Cin,H,W), got (32, 4, 6)"),
        ((x.float(), (z(5), bh)), k, "wpack must hold 18432 halves (pack_enc3, 32 -> 64), got (5,)"),
        ((x.float(), (wp, bh)), dict(stride=2, residual=z(1, 64, 4, 6)), "expected scalar type Half but found Float (x)"),
        ((nc(x), (wp, bh)), dict(stride=2, residual=res.float()), "expected scalar type Half but found Float (residual)"),
        ((nc(x), (wp, bh)), dict(stride=2, down=(dp, z(32))), "dbias_h must be (64,), got (32,)"),
        ((x.clone().requires_grad_(), (wp, bh.float())), k, "expected scalar type Half but found Float (bias_h)"),
        ((x, (wp, nc(bh))), dict(stride=2, residual=nc(res)), "bias_h must be contiguous"),
    ]
    for args, kw, message in cases:
        for relu in (False, True):
            with pytest.raises(RuntimeError) as info:
                f(*args, relu=relu, **kw)
            assert str(info.value) == message
            assert type(info.value) is (lgu._lib.UnsupportedShape if message.startswith(served) else RuntimeError)
    with torch.no_grad():      # grad mode off: the no-grad refusal does not apply, the device refusal is next
        with pytest.raises(RuntimeError) as info:
            f(x.clone().requires_grad_(), (wp, bh), stride=2)
        assert str(info.value) == "x" + _NO_CPU


# ---- GPU ------------------------------------------------------------------------------------------------------------
def _need_gpu(lgu):
    assert torch.cuda.is_available(), "these tests need the MI355X"
    assert os.path.exists(lgu._lib.so_path()), "liblgu_corr.so missing — run __graft_entry__.build()"


def _packed(lgu, c3, c1=None):
    p3 = lgu.encconv.pack_enc3(c3.weight.detach().cuda(), c3.bias.detach().cuda())
    return p3, (lgu.encconv.pack_enc1(c1.weight.detach().cuda(), c1.bias.detach().cuda()) if c1 is not None else None)


IMPULSE_AT = [(2, 2), (3, 3), (2, 3), (3, 2), (0, 0), (0, 5), (5, 0), (5, 5), (6, 6), (0, 6), (6, 1)]   # in a 7x7 image
IMPULSE_CH = [0, 31]


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES, ids=_IDS)
def test_impulses_give_the_weights_bit_for_bit(lgu, shape):
    """One input element = 1 in a 7x7 image (even and odd rows and columns, corners, the last row and column, first and
    last input channel), bias 0: a single product is exact, so output (y, x) is act(w_h[co, c, cy - s y + 1, cx - s x + 1])
    where that tap exists and 0 elsewhere, torch's rule; r is w'_h[co, c] at (cy / 2, cx / 2) for an even (cy, cx) only."""
    _need_gpu(lgu)
    cin, cout, st = shape
    c3, c1 = R.make_layer(43, *shape)
    with torch.no_grad():
        c3.bias.zero_()
        if c1 is not None:
            c1.bias.zero_()
    wh = c3.weight.detach().half()
    chans = IMPULSE_CH + [cin - 1]
    Ho, Wo = R.out_size(7, 7, st)
    x = torch.zeros((len(IMPULSE_AT) * len(chans), cin, 7, 7), dtype=torch.float16)
    want = torch.zeros((x.shape[0], cout, Ho, Wo), dtype=torch.float16)
    want_r = torch.zeros_like(want)
    for i, (cy, cx) in enumerate(IMPULSE_AT):
        for k, c in enumerate(chans):
            n = len(chans) * i + k
            x[n, c, cy, cx] = 1.0
            for ky in range(3):
                for kx in range(3):
                    ny, nx = cy - ky + 1, cx - kx + 1         # = st * y, st * x of the output that sees it through (ky, kx)
                    if ny % st == 0 and nx % st == 0 and 0 <= ny // st < Ho and 0 <= nx // st < Wo:
                        want[n, :, ny // st, nx // st] = wh[:, c, ky, kx]
            if st == 2 and cy % 2 == 0 and cx % 2 == 0:
                want_r[n, :, cy // 2, cx // 2] = c1.weight.detach().half()[:, c, 0, 0]
    ref = torch.nn.functional.conv2d(x.double(), wh.double(), stride=st, padding=1)
    assert torch.equal(ref, want.double())                       # torch's rule for which outputs an impulse reaches
    p3, p1 = _packed(lgu, c3, c1)
    res = R.make_residual(9, tuple(want.shape))
    for relu in (False, True):
        got = lgu.encconv.enc_conv3x3(x.cuda(), p3, stride=st, relu=relu, down=p1)
        got, r = got if st == 2 else (got, None)
        torch.cuda.synchronize()
        ref = torch.relu(want) if relu else want
        assert int((ref != 0).sum()) > 0.3 * int((want != 0).sum()) > 0
        assert same_bits(got, ref), "relu=%s: max |diff| %g" % (relu, float((got.cpu().float() - ref.float()).abs().max()))
        if st == 2:
            assert same_bits(r, want_r) and int((want_r != 0).sum()) == 4 * len(chans) * cout
    got = lgu.encconv.enc_conv3x3(x.cuda(), p3, stride=st, residual=res.cuda())
    assert same_bits(got, torch.relu(res + torch.relu(want)))


@pytest.mark.gpu
@pytest.mark.parametrize("size", [(1, 1, 1), (2, 9, 33), (1, 17, 130)])
@pytest.mark.parametrize("shape", SHAPES, ids=_IDS)
def test_zero_input_gives_act_of_the_bias_everywhere(lgu, shape, size):
    _need_gpu(lgu)
    cin, cout, st = shape
    c3, c1 = R.make_layer(44, *shape)
    p3, p1 = _packed(lgu, c3, c1)
    x = torch.zeros((size[0], cin, size[1], size[2]), dtype=torch.float16, device="cuda")
    osz = (size[0], cout) + R.out_size(size[1], size[2], st)
    bh = c3.bias.detach().half().view(1, -1, 1, 1).expand(osz)
    res = R.make_residual(10, osz)
    assert bool((bh < 0).any()) and bool((bh > 0).any())
    for relu in (False, True):
        got = lgu.encconv.enc_conv3x3(x, p3, stride=st, relu=relu, down=p1)
        got, r = got if st == 2 else (got, None)
        assert same_bits(got, torch.relu(bh) if relu else bh)
        if st == 2:
            assert same_bits(r, c1.bias.detach().half().view(1, -1, 1, 1).expand(osz))
    assert same_bits(lgu.encconv.enc_conv3x3(x, p3, stride=st, residual=res.cuda()), torch.relu(res + torch.relu(bh)))


def _size_cases():
    for shape, sid in zip(SHAPES, _IDS):
        for size in R.sizes(shape[0]):
            yield pytest.param(shape, size, id="%s-%dx%dx%d" % ((sid,) + size))


@pytest.mark.gpu
@pytest.mark.parametrize("shape,size", list(_size_cases()))
def test_every_element_is_within_the_derived_bound(lgu, shape, size):
    """The three epilogues (and, with stride 2, the branch) of one layer shape at one input size: every element within its
    allowance; RELU and RESIDUAL bit for bit torch's ops on the identity output of the same call; r the same bits with
    another 3x3 pack in the launch; y the same bits without the branch."""
    _need_gpu(lgu)
    cin, cout, st = shape
    c3, c1, x, res, s64, S, r64, Sr = case(shape, size)
    p3, p1 = _packed(lgu, c3, c1)
    xc, resc = x.cuda(), res.cuda()
    f = lgu.encconv.enc_conv3x3
    outs = {"identity": f(xc, p3, stride=st, down=p1), "relu": f(xc, p3, stride=st, relu=True, down=p1),
            "residual": f(xc, p3, stride=st, residual=resc, down=p1)}
    torch.cuda.synchronize()
    rs = {}
    if st == 2:
        rs = {k: v[1] for k, v in outs.items()}
        outs = {k: v[0] for k, v in outs.items()}
    y0 = outs["identity"]
    assert y0.dtype == torch.float16 and y0.is_contiguous() and tuple(y0.shape) == tuple(s64.shape)
    for kind in R.EPILOGUES:
        want = R.epilogue(s64, kind, res.double())
        allow = R.allowed(s64, S, R.terms3(cin), kind, res.double())
        err = (outs[kind].cpu().double() - want).abs()
        worst = float((err / allow).max())
        print("%s %s %s: max |err| %.3e, max err / allowance %.3f" % (shape, size, kind, float(err.max()), worst))
        assert bool((err <= allow).all()), (kind, worst)
    assert same_bits(outs["relu"], torch.relu(y0))
    assert same_bits(outs["residual"], torch.relu(resc + torch.relu(y0)))
    if st == 2:
        err = (rs["identity"].cpu().double() - r64).abs()
        allow = R.allowance(r64, Sr, R.terms1(cin))
        print("%s %s branch: max |err| %.3e, max err / allowance %.3f" % (shape, size, float(err.max()), float((err / allow).max())))
        assert bool((err <= allow).all())
        assert same_bits(rs["relu"], rs["identity"]) and same_bits(rs["residual"], rs["identity"])
        other, _ = R.make_layer(99, *shape)
        y_other, r_other = f(xc, _packed(lgu, other)[0], stride=2, down=p1)
        assert same_bits(r_other, rs["identity"]) and not same_bits(y_other, y0)
        for kind, kw in (("identity", {}), ("relu", dict(relu=True)), ("residual", dict(residual=resc))):
            assert same_bits(f(xc, p3, stride=2, **kw), outs[kind]), kind


NAN_SIZES = [(1, 1, 1), (1, 2, 3), (2, 9, 33), (2, 10, 34), (1, 5, 65)]


@pytest.mark.gpu
@pytest.mark.parametrize("size", NAN_SIZES)
@pytest.mark.parametrize("shape", SHAPES, ids=_IDS)
def test_nan_reaches_exactly_its_neighbourhood(lgu, shape, size):
    """NaNs at the corners, the last row and column and an interior even and odd position of x: y is NaN exactly where a
    float64 convolution of the NaN mask with ones is positive (torch's rule for stride and padding), r exactly at
    (cy / 2, cx / 2) of the even ones; one NaN in res reaches one element."""
    _need_gpu(lgu)
    cin, cout, st = shape
    c3, c1, x, res, *_ = case(shape, size)
    p3, p1 = _packed(lgu, c3, c1)
    N, H, W = size
    ats = sorted({(0, 0), (H - 1, W - 1), (0, W - 1), (H - 1, 0), (H // 2, W // 2), (H // 2 | 1 if H > 1 else 0, W // 2 | 1 if W > 1 else 0),
                  (min(H - 1, 2), min(W - 1, 31)), (min(H - 1, 3), min(W - 1, 32))})
    F = torch.nn.functional
    for cy, cx in ats:
        xn = x.clone()
        xn[N - 1, cin // 2, cy, cx] = float("nan")
        mask = torch.zeros((N, 1, H, W), dtype=torch.float64)
        mask[N - 1, 0, cy, cx] = 1.0
        hit = (F.conv2d(mask, torch.ones((1, 1, 3, 3), dtype=torch.float64), stride=st, padding=1) > 0).expand(-1, cout, -1, -1)
        for kw in (dict(), dict(relu=True), dict(residual=res.cuda())):
            got = lgu.encconv.enc_conv3x3(xn.cuda(), p3, stride=st, down=p1, **kw)
            got, r = got if st == 2 else (got, None)
            assert torch.equal(torch.isnan(got).cpu(), hit), (cy, cx, kw.keys())
            if st == 2:
                hit_r = (F.conv2d(mask, torch.ones((1, 1, 1, 1), dtype=torch.float64), stride=2) > 0).expand(-1, cout, -1, -1)
                assert torch.equal(torch.isnan(r).cpu(), hit_r) and int(hit_r.sum()) == (cout if cy % 2 == 0 and cx % 2 == 0 else 0)
    rn = res.clone()
    rn[N - 1, cout - 1, -1, -1] = float("nan")
    got = lgu.encconv.enc_conv3x3(x.cuda(), p3, stride=st, residual=rn.cuda())
    assert torch.equal(torch.isnan(got).cpu(), torch.isnan(rn)) and int(torch.isnan(got).sum()) == 1


@pytest.mark.gpu
@pytest.mark.parametrize("size", [(1, 9, 33), (1, 10, 34), (1, 17, 130)])
@pytest.mark.parametrize("shape", SHAPES, ids=_IDS)
def test_an_image_does_not_depend_on_its_batch(lgu, shape, size):
    _need_gpu(lgu)
    cin, cout, st = shape
    c3, c1 = R.make_layer(45, *shape)
    p3, p1 = _packed(lgu, c3, c1)
    x3 = R.make_input(77, 3, size[1], size[2], C=cin).half().cuda()
    res3 = R.make_residual(78, (3, cout) + R.out_size(size[1], size[2], st)).cuda()
    f = lgu.encconv.enc_conv3x3
    for kw3, kw1 in ((dict(), dict()), (dict(relu=True), dict(relu=True)), (dict(residual=res3), dict(residual=res3[1:2].contiguous()))):
        a = f(x3, p3, stride=st, down=p1, **kw3)
        b = f(x3[1:2].contiguous(), p3, stride=st, down=p1, **kw1)
        if st == 2:
            assert same_bits(a[1][1:2], b[1])
            a, b = a[0], b[0]
        assert same_bits(a[1:2], b)


# (shape, (H, W), workgroups of the large tile per image): the launcher takes the large tile of a shape class (32 x 4 output
# pixels, or 32 x 2 for (64,128,2), by 64 channels) when that gives at least two workgroups per CU; (32,32,1) has one tile
LARGE_GRID = [((32, 64, 2), (34, 130), 15), ((64, 64, 1), (17, 65), 15), ((64, 128, 2), (34, 130), 54), ((128, 128, 1), (17, 65), 30)]


@pytest.mark.gpu
@pytest.mark.parametrize("shape,hw,per_image", LARGE_GRID, ids=_IDS[1:])
def test_the_large_tile_gives_the_small_tiles_bits(lgu, shape, hw, per_image):
    """A batch whose grid crosses the launcher's threshold (two workgroups of the large tile per CU) against the same
    images one at a time, which take the small tile: bit for bit, every epilogue and the branch."""
    _need_gpu(lgu)
    cin, cout, st = shape
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    N = -(-2 * cus // per_image) + 1
    assert N * per_image >= 2 * cus > per_image
    c3, c1 = R.make_layer(47, *shape)
    p3, p1 = _packed(lgu, c3, c1)
    x = R.make_input(79, N, hw[0], hw[1], C=cin).half().cuda()
    res = R.make_residual(80, (N, cout) + R.out_size(hw[0], hw[1], st)).cuda()
    f = lgu.encconv.enc_conv3x3
    for kw in (dict(), dict(relu=True), dict(residual=res)):
        big = f(x, p3, stride=st, down=p1, **kw)
        for i in (0, N // 2, N - 1):
            kw1 = dict(kw, residual=res[i:i + 1].contiguous()) if "residual" in kw else kw
            one = f(x[i:i + 1].contiguous(), p3, stride=st, down=p1, **kw1)
            if st == 2:
                assert same_bits(big[1][i:i + 1], one[1]), (i, "r")
                assert same_bits(big[0][i:i + 1], one[0]), (i, list(kw))
            else:
                assert same_bits(big[i:i + 1], one), (i, list(kw))


def _c_call(lgu, a, shape, size, flags):
    cin, cout, st = shape
    args = lgu._lib.EncConvArgs(a["x"].data_ptr(), a["wpack"].data_ptr(), a["bias"].data_ptr(),
                                a["res"].data_ptr() if flags & lgu.encconv.RESIDUAL else None, a["out"].data_ptr(),
                                a["dpack"].data_ptr() if "dpack" in a else None, a["dbias"].data_ptr() if "dpack" in a else None,
                                a["r"].data_ptr() if "dpack" in a else None, size[0], size[1], size[2], cin, cout, st, flags)
    rc = lgu._lib.load().lgu_encconv3x3_h16(args, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc


@pytest.mark.gpu
@pytest.mark.parametrize("size", [(2, 9, 33), (2, 10, 34), (1, 16, 32)])
@pytest.mark.parametrize("shape", SHAPES, ids=_IDS)
def test_guard_bands_and_alignment(lgu, shape, size):
    """The alignment audit of DESIGN.md §4.1 for lgu_encconv3x3_h16: x, res, the biases, out and r are served at element
    alignment with the aligned call's bits (by element where a pointer is not 16-byte aligned or W_out % 8 != 0; W 33 and
    34 give W_out 33, 34 and 17, 1x16x32 the 16-byte paths), every written tensor inside a sentinel-filled buffer, a pack
    that is not 16-byte aligned is refused with nothing launched, and so are the other bad calls."""
    from tests.alignment_cases import guards_intact, shifted
    _need_gpu(lgu)
    cin, cout, st = shape
    c3, c1 = R.make_layer(46, *shape)
    (wpack, bias_h), p1 = _packed(lgu, c3, c1)
    osz = (size[0], cout) + R.out_size(size[1], size[2], st)
    x = R.make_input(5, *size, C=cin).half().cuda()
    res = R.make_residual(6, osz).cuda()
    base = {"x": x, "wpack": wpack, "bias": bias_h, "res": res, "out": torch.empty(osz, dtype=torch.float16, device="cuda")}
    if st == 2:
        base.update(dpack=p1[0], dbias=p1[1], r=torch.empty(osz, dtype=torch.float16, device="cuda"))
    assert all(t.data_ptr() % 16 == 0 for t in base.values())
    E = lgu.encconv
    written = [k for k in ("out", "r") if k in base]
    packs = [k for k in ("wpack", "dpack") if k in base]
    for flags, kw in ((0, {}), (E.RELU, dict(relu=True)), (E.RESIDUAL, dict(residual=res))):
        want = E.enc_conv3x3(x, (wpack, bias_h), stride=st, down=p1, **kw)
        want = dict(zip(written, want if st == 2 else (want,)))
        variants = [([k], s) for k in base for s in (2, 4, 8)]
        variants += [([k for k in base if k not in packs], 2)]             # everything at an odd element offset
        for keys, shift in variants:
            args = dict(base)
            for k in keys:
                args[k] = shifted(base[k], shift)
            for k in written:
                if k not in keys:
                    args[k] = shifted(base[k], 0)
            for k in written:
                args[k].fill_(float("nan"))
            before = {k: args[k].clone() for k in args}
            rc = _c_call(lgu, args, shape, size, flags)
            if set(keys) & set(packs):
                assert rc == lgu._lib.LGU_E_UNSUPPORTED, (keys, shift, rc)
                assert all(same_bits(args[k], before[k]) for k in written), "refused, but an output changed"
            else:
                assert rc == 0, (keys, shift, rc)
                for k in written:
                    assert same_bits(args[k], want[k]), "%s shifted by %d: %s differs from the aligned call" % (keys, shift, k)
            for k in base:
                if k not in written:
                    assert same_bits(args[k], before[k]), "read-only operand %s changed" % k
            for k in set(keys) | set(written):
                assert guards_intact(args[k]), "%s, %d: a guard band of %s was written" % (keys, shift, k)
    # empty and bad calls launch nothing
    args = dict(base)
    for k in written:
        args[k] = shifted(base[k], 0)
    before = {k: args[k].clone() for k in written}
    BAD, UNS = lgu._lib.LGU_E_BADARG, lgu._lib.LGU_E_UNSUPPORTED
    assert _c_call(lgu, args, shape, (0,) + size[1:], 0) == 0
    assert _c_call(lgu, args, shape, (-1,) + size[1:], 0) == BAD
    assert _c_call(lgu, args, shape, (size[0], 0, size[2]), 0) == BAD
    assert _c_call(lgu, args, shape, (size[0], size[1], 0), 0) == BAD
    assert _c_call(lgu, args, shape, size, 4) == BAD and _c_call(lgu, args, shape, size, E.RELU | E.RESIDUAL) == BAD
    assert _c_call(lgu, args, (cin, cout, 3 - st), size, 0) == (UNS if st == 1 else BAD)   # the branch with stride 1
    assert _c_call(lgu, args, (cin, 96, st), size, 0) == UNS and _c_call(lgu, args, (48, cout, st), size, 0) == UNS
    a = lgu._lib.EncConvArgs(x.data_ptr(), wpack.data_ptr(), bias_h.data_ptr(), None, args["out"].data_ptr(), None, None, None,
                             size[0], size[1], size[2], cin, cout, st, E.RESIDUAL)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert lgu._lib.load().lgu_encconv3x3_h16(a, stream) == BAD            # the flag without res
    a.flags, a.res = 0, res.data_ptr()
    assert lgu._lib.load().lgu_encconv3x3_h16(a, stream) == BAD            # res without the flag
    a.res, a.out = None, None
    assert lgu._lib.load().lgu_encconv3x3_h16(a, stream) == BAD            # a null output
    a.out, a.dbias = args["out"].data_ptr(), bias_h.data_ptr()
    assert lgu._lib.load().lgu_encconv3x3_h16(a, stream) == BAD            # an incomplete branch
    if st == 1:
        a.dpack, a.r = wpack.data_ptr(), args["out"].data_ptr()
        assert lgu._lib.load().lgu_encconv3x3_h16(a, stream) == BAD        # the branch with stride 1
    torch.cuda.synchronize()
    assert all(same_bits(args[k], before[k]) and guards_intact(args[k]) for k in written)
    assert tuple(E.enc_conv3x3(x[:0], (wpack, bias_h), stride=st).shape) == (0,) + osz[1:]
    if st == 2:
        y, r = E.enc_conv3x3(x[:0], (wpack, bias_h), stride=2, down=p1)
        assert tuple(y.shape) == tuple(r.shape) == (0,) + osz[1:]
    with pytest.raises(RuntimeError, match=r"enc_conv3x3: empty frame \(H\*W = 0\)"):
        E.enc_conv3x3(x[:, :, :0], (wpack, bias_h), stride=st)
