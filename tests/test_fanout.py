"""conv3.conv3x3_fanout (csrc/conv3.hip): two or three Conv2d(128, 128, 3, padding=1) of one input in one launch.

Contract (include/lgu_corr.h): output g has the bits of conv3x3(x, *packs[g], relu=relu).  Held here:
- bit for bit against conv3x3 for G in {2, 3}, relu on and off, float32 and half x, on the four shapes at which the tiles
  (the fan-out's 32 x 4, and the 64 x 2 and 32 x 4 of the conv3x3 it is held to) and the two store paths can go wrong;
  the packs are distinct per group, so a kernel that reads the wrong pack fails;
- one case against the float64 restatement with conv3_restatement.allowance(..., terms=1154), as tests/test_conv3.py holds
  conv3x3, so that the test does not rest on the sibling kernel alone;
- a NaN of x reaches exactly its 3x3 neighbourhood in every group, a NaN of one group's bias that group only;
- an image's outputs do not depend on its batch;
- through the C ABI: outputs embedded in sentinel-filled buffers, x and the biases at element alignment give the aligned
  call's bits with the bands intact; a wpack off 16 bytes is refused with nothing written.
The GPU tests build their modules themselves and never read the reference tree.
"""
import ctypes
import os

import pytest

torch = pytest.importorskip("torch")

from tests import conv3_restatement as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = "lgu_conv3x3_fanout_c128_h16"
SHAPES = [(1, 1, 1), (2, 9, 33), (2, 5, 65), (1, 6, 40)]
_NO_CPU = " must be a HIP device tensor: lgu_slam_amd has no CPU fallback"
_CONVS = {}


def same_bits(a, b):
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    return a.shape == b.shape and a.dtype == b.dtype and bool(torch.equal(a.view(torch.int16), b.view(torch.int16)))


def convs():
    """Three Conv2d(128, 128, 3, padding=1) with distinct seeded weights (CPU), made once and never changed."""
    if not _CONVS:
        _CONVS.update({g: R.make_conv(310 + g, 128) for g in range(3)})
    return [_CONVS[g] for g in range(3)]


# ---- CPU ------------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_entry(lgu):
    from tests.test_abi import declared_symbols
    lib = ctypes.CDLL(lgu._lib._build.SO_PATH)
    assert ENTRY in declared_symbols() and hasattr(lib, ENTRY)
    sig = lgu._lib.SIGNATURES[ENTRY]
    assert sig[0] is lgu._lib.Conv3FanoutArgs and issubclass(sig[0], ctypes.Structure) and sig[1] is ctypes.c_void_p
    assert [f[0] for f in sig[0]._fields_] == ["x", "wpack", "bias", "out", "N", "H", "W", "G", "flags"]
    assert ctypes.sizeof(sig[0]) == 10 * 8 + 5 * 4 + 4
    assert lgu.conv3x3_fanout is lgu.conv3.conv3x3_fanout and isinstance(lgu.conv3.MIN_FANOUT_PIXELS, int)
    text = open(os.path.join(ROOT, "include", "lgu_corr.h")).read()
    assert "int lgu_conv3x3_fanout_c128_h16(lgu_conv3_fanout_args args, void* stream);" in text
    assert lgu.__version__ == "0.8.0"


def test_operator_refusals_in_their_order(lgu):
    """Shape of x, number of packs, each pack's size and bias shape, contiguity, dtypes, no-grad, device: each refusal's
    text, and which of two defects is reported.  None of them touches a device."""
    f = lgu.conv3.conv3x3_fanout
    H = torch.float16

    def z(*shape, dtype=torch.float32):
        return torch.zeros(shape, dtype=dtype)

    def nc(t):
        return torch.zeros(tuple(t.shape) + (2,), dtype=t.dtype)[..., 0]

    x, wp, bh = z(1, 128, 2, 2), z(9, 4, 8, 64, 8, dtype=H), z(128, dtype=H)
    wp64 = z(9, 4, 4, 64, 8, dtype=H)
    ok = [(wp, bh), (wp, bh), (wp, bh)]
    no_grad = ("conv3x3_fanout has no autograd: its outputs would carry no gradient. Call it under torch.no_grad() or pass "
               "detached inputs")
    cases = [
        ((x, ok), "x" + _NO_CPU),
        ((x.half(), ok[:2]), "x" + _NO_CPU),
        ((z(1, 127, 2, 2), ok), "x must be (N,128,H,W), got (1, 127, 2, 2)"),
        ((z(128, 2, 2), ok), "x must be (N,128,H,W), got (128, 2, 2)"),
        ((x, ok[:1]), "packs must be two or three (wpack, bias_h) pairs (pack_conv3), got 1"),
        ((x, ok + ok[:1]), "packs must be two or three (wpack, bias_h) pairs (pack_conv3), got 4"),
        ((x, [(wp, bh), (wp64, z(64, dtype=H))]), "packs[1]: wpack must hold 147456 halves (pack_conv3, Cout 128), got (9, 4, 4, 64, 8)"),
        ((x, [(wp, bh), (wp, bh), (wp, z(64, dtype=H))]), "packs[2]: bias_h must be (128,), got (64,)"),
        ((nc(x), ok), "x must be contiguous"),
        ((x, [(wp, bh), (nc(wp), bh)]), "packs[1]: wpack must be contiguous"),
        ((x, [(wp, nc(bh)), (wp, bh)]), "packs[0]: bias_h must be contiguous"),
        ((x.double(), ok), "expected scalar type Float or Half but found Double (x)"),
        ((x, [(wp, bh), (wp.float(), bh)]), "expected scalar type Half but found Float (packs[1]: wpack)"),
        ((x, [(wp, bh), (wp, bh), (wp, bh.bfloat16())]), "expected scalar type Half but found BFloat16 (packs[2]: bias_h)"),
        ((x.clone().requires_grad_(), ok), no_grad),
        # two defects: the earlier check reports
        ((z(1, 127, 2, 2), ok[:1]), "x must be (N,128,H,W), got (1, 127, 2, 2)"),
        ((nc(x), ok[:1]), "packs must be two or three (wpack, bias_h) pairs (pack_conv3), got 1"),
        ((nc(x), [(wp, bh), (wp64, bh)]), "packs[1]: wpack must hold 147456 halves (pack_conv3, Cout 128), got (9, 4, 4, 64, 8)"),
        ((x.double(), [(wp, bh), (wp, nc(bh))]), "packs[1]: bias_h must be contiguous"),
        ((x.clone().requires_grad_(), [(wp, bh), (wp, bh.float())]), "expected scalar type Half but found Float (packs[1]: bias_h)"),
    ]
    for args, message in cases:
        for relu in (False, True):
            with pytest.raises(RuntimeError) as info:
                f(*args, relu=relu)
            assert type(info.value) is RuntimeError and str(info.value) == message
    with torch.no_grad():      # grad mode off: the no-grad refusal does not apply, the device refusal is next
        with pytest.raises(RuntimeError) as info:
            f(x.clone().requires_grad_(), ok)
        assert str(info.value) == "x" + _NO_CPU


# ---- GPU ------------------------------------------------------------------------------------------------------------
def _need_gpu(lgu):
    assert torch.cuda.is_available(), "these tests need the MI355X"
    assert os.path.exists(lgu._lib.so_path()), "liblgu_corr.so missing — run __graft_entry__.build()"


def _packs(lgu, G=3):
    return [lgu.conv3.pack_conv3(m.weight.detach().cuda(), m.bias.detach().cuda()) for m in convs()[:G]]


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES)
def test_every_output_has_the_bits_of_conv3x3(lgu, shape):
    _need_gpu(lgu)
    C = lgu.conv3
    packs = _packs(lgu)
    x32 = R.make_input(4000 + shape[1] * shape[2], *shape).cuda()
    for x in (x32, x32.half()):
        for relu in (False, True):
            want = [C.conv3x3(x, *p, relu=relu) for p in packs]
            assert not same_bits(want[0], want[1]) and not same_bits(want[1], want[2])
            for G in (2, 3):
                got = C.conv3x3_fanout(x, packs[:G], relu=relu)
                torch.cuda.synchronize()
                assert isinstance(got, tuple) and len(got) == G
                for g in range(G):
                    assert got[g].dtype == torch.float16 and got[g].is_contiguous()
                    assert same_bits(got[g], want[g]), (str(x.dtype), relu, G, g)
            # the order of the packs is the order of the outputs
            swapped = C.conv3x3_fanout(x, [packs[2], packs[0]], relu=relu)
            assert same_bits(swapped[0], want[2]) and same_bits(swapped[1], want[0])
    assert tuple(t.shape for t in C.conv3x3_fanout(x32[:0], packs)) == ((0, 128) + shape[1:],) * 3


@pytest.mark.gpu
def test_one_case_is_within_the_float64_bound(lgu):
    """|y - act(s64)| <= allowance(s64, S, 1154) for every group, relu on, shape (2, 9, 33)."""
    _need_gpu(lgu)
    shape = (2, 9, 33)
    x = R.make_input(4500, *shape)
    got = lgu.conv3.conv3x3_fanout(x.cuda(), _packs(lgu), relu=True)
    torch.cuda.synchronize()
    assert R.TERMS == 1154
    for g, m in enumerate(convs()):
        with torch.no_grad():
            s, S, _ = R.conv3(x, m.weight, m.bias, True)
        bound = R.allowance(s, S, R.TERMS)
        err = (got[g].cpu().double() - torch.relu(s)).abs()
        print("conv3x3_fanout group %d %s: worst error %.3g of its bound" % (g, shape, float((err / bound).max())))
        assert bool((err <= bound).all()), (g, float((err / bound).max()))


@pytest.mark.gpu
@pytest.mark.parametrize("shape,at", [((2, 9, 33), (1, 5, 3, 32)), ((2, 5, 65), (0, 127, 4, 64)), ((1, 6, 40), (0, 64, 0, 0))])
def test_nan_stays_where_it_belongs(lgu, shape, at):
    """A NaN at one pixel of x: exactly its 3x3 neighbourhood in every group, every other element with the clean bits.  A
    NaN in one group's bias: that group's channel everywhere, the other groups untouched."""
    _need_gpu(lgu)
    C = lgu.conv3
    packs = _packs(lgu)
    x = R.make_input(4600 + shape[2], *shape)
    clean = [t.cpu() for t in C.conv3x3_fanout(x.cuda(), packs, relu=True)]
    assert not any(bool(torch.isnan(t).any()) for t in clean)
    xn = x.clone()
    xn[at] = float("nan")
    n, _, cy, cx = at
    want = torch.zeros((shape[0], 1) + shape[1:], dtype=torch.bool)
    want[n, 0, max(cy - 1, 0):cy + 2, max(cx - 1, 0):cx + 2] = True
    for g, t in enumerate(C.conv3x3_fanout(xn.cuda(), packs, relu=True)):
        t = t.cpu()
        assert bool((torch.isnan(t) == want.expand_as(t)).all()), g
        assert bool((t.view(torch.int16) == clean[g].view(torch.int16))[~want.expand_as(t)].all()), g
    for bad in range(3):
        bias = packs[bad][1].clone()
        bias[17] = float("nan")
        mixed = [(p[0], bias) if g == bad else p for g, p in enumerate(packs)]
        for g, t in enumerate(C.conv3x3_fanout(x.cuda(), mixed, relu=True)):
            t = t.cpu()
            if g == bad:
                assert bool(torch.isnan(t[:, 17]).all()) and not bool(torch.isnan(t[:, :17]).any()) and not bool(torch.isnan(t[:, 18:]).any())
            else:
                assert same_bits(t, clean[g]), (bad, g)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(3, 9, 33), (3, 6, 40)])
def test_an_image_does_not_depend_on_its_batch(lgu, shape):
    _need_gpu(lgu)
    C = lgu.conv3
    packs = _packs(lgu)
    x = R.make_input(77, *shape).cuda()
    got = C.conv3x3_fanout(x, packs, relu=True)
    for k in range(shape[0]):
        alone = C.conv3x3_fanout(x[k:k + 1].contiguous(), packs, relu=True)
        assert all(same_bits(got[g][k:k + 1], alone[g]) for g in range(3)), k


def _c_call(lgu, x, packs, outs, flags, G=None, n=None):
    N, _, H, W = x.shape
    three = ctypes.c_void_p * 3
    flags |= lgu.conv3.X_HALF if x.dtype == torch.float16 else 0
    G = len(packs) if G is None else G
    args = lgu._lib.Conv3FanoutArgs(x.data_ptr(), three(*[p[0].data_ptr() for p in packs]), three(*[p[1].data_ptr() for p in packs]),
                                    three(*[o.data_ptr() for o in outs]), N if n is None else n, H, W, G, flags)
    rc = lgu._lib.load().lgu_conv3x3_fanout_c128_h16(args, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc


@pytest.mark.gpu
@pytest.mark.parametrize("half_x", (False, True))
@pytest.mark.parametrize("shape", [(2, 9, 33), (1, 6, 40)])
def test_guard_bands_and_alignment(lgu, shape, half_x):
    """lgu_conv3x3_fanout_c128_h16 through the C ABI (its operands travel in a parameter block, so the registry of
    tests/alignment_cases.py does not see it): every output embedded in a sentinel-filled buffer; x, the biases and the
    outputs at element alignment give the aligned call's bits with the bands intact; a wpack shifted by 8 bytes, a G outside
    {2, 3} are refused with nothing written; N == 0 launches nothing."""
    from tests.alignment_cases import guards_intact, shifted, shifts_for
    _need_gpu(lgu)
    C = lgu.conv3
    packs = _packs(lgu)
    x = R.make_input(4700 + shape[2], *shape).cuda()
    x = x.half() if half_x else x
    want = C.conv3x3_fanout(x, packs, relu=True)

    def fresh():
        return [shifted(torch.zeros_like(want[0]), 0) for _ in range(3)]
    outs = fresh()
    assert _c_call(lgu, x, packs, outs, C.RELU) == 0
    assert all(same_bits(o, w) and guards_intact(o) for o, w in zip(outs, want))
    variants = [("x", s) for s in shifts_for(x.dtype)] + [("bias", s) for s in (2, 4, 8)] + [("out", s) for s in (2, 4, 8)] + [("all", 0)]
    for key, shift in variants:
        xs = shifted(x, shift if key == "x" else x.element_size()) if key in ("x", "all") else x
        ps = [(p[0], shifted(p[1], shift if key == "bias" else 2)) if key in ("bias", "all") else p for p in packs]
        outs = [shifted(torch.zeros_like(want[0]), shift if key == "out" else 2) for _ in range(3)] if key in ("out", "all") else fresh()
        for G in (2, 3):
            for o in outs:
                o.zero_()
            assert _c_call(lgu, xs, ps[:G], outs[:G], C.RELU) == 0, (key, shift, G)
            assert all(same_bits(outs[g], want[g]) for g in range(G)), "%s shifted by %d, G %d: differs from the aligned call" % (key, shift, G)
            assert G == 3 or not bool(outs[2].any())      # the third output is not touched at G = 2
        assert all(guards_intact(t) for t in outs + [p[1] for p in ps if hasattr(p[1], "_lgu_guard")] + ([xs] if xs is not x else []))
        assert same_bits(xs, x) and all(same_bits(a[1], b[1]) for a, b in zip(ps, packs))
    # refusals: nothing written
    outs = fresh()
    for bad in range(3):
        ps = [(shifted(p[0], 8), p[1]) if g == bad else p for g, p in enumerate(packs)]
        assert _c_call(lgu, x, ps, outs, C.RELU) == lgu._lib.LGU_E_UNSUPPORTED, bad
    assert _c_call(lgu, x, packs, outs, C.RELU, G=1) == lgu._lib.LGU_E_UNSUPPORTED
    assert _c_call(lgu, x, packs, outs, C.RELU, G=4) == lgu._lib.LGU_E_UNSUPPORTED
    assert _c_call(lgu, x, packs, outs, 4) == lgu._lib.LGU_E_BADARG                # an unknown flag
    assert _c_call(lgu, x, packs, outs, C.RELU, n=-1) == lgu._lib.LGU_E_BADARG
    assert _c_call(lgu, x, packs, outs, C.RELU, n=0) == 0
    assert all(not bool(o.any()) and guards_intact(o) for o in outs)
    with pytest.raises(lgu._lib.UnsupportedShape):
        C.conv3x3_fanout(x, [(shifted(packs[0][0], 8), packs[0][1]), packs[1]], relu=True)
