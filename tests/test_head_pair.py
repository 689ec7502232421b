"""heads.head_pair (csrc/heads.hip): the reference's delta[2] and weight[2] + Sigmoid in one launch, edge-major, optionally
as the factor graph's float32 state (coords1 + delta.float(), weight.float()).

Contract (include/lgu_corr.h).  Held here:
- without coords, both results bit for bit to_edges(head_conv3x3(...)) of the separate launches, float32 and half inputs,
  on the four shapes at which the 32 x 4 tile can go wrong; with coords, torch.equal(target, coords + delta_h.float()) and
  torch.equal(weight_f, weight_h.float()).  The two heads have distinct weights and distinct inputs, so a kernel that
  swaps the heads, the packs or the activation fails;
- one case per input dtype against the float64 restatement, with heads_restatement.act_allowance as tests/test_heads.py's
  bound test, plus one fp32 rounding of the add in float32 mode: 2^-24 (|coords| + |delta64| + allowance);
- a NaN in d reaches exactly its 3x3 neighbourhood of delta and nothing of weight, and the other way round; a NaN or Inf in
  coords shows at its own element only;
- through the C ABI in both output modes: guard bands, x and biases at element alignment, outputs or coords off a whole
  pixel and a wpack off 16 bytes refused before the launch, a flag / coords mismatch LGU_E_BADARG.
The GPU tests build their modules themselves and never read the reference tree.
"""
import ctypes
import os

import pytest

torch = pytest.importorskip("torch")

from tests import conv3_restatement as R  # noqa: E402
from tests import heads_restatement as RH  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = "lgu_head3x3_pair_c128_h16"
SHAPES = [(1, 1, 1), (2, 9, 33), (2, 5, 65), (1, 6, 40)]
U24 = 2.0 ** -24
_NO_CPU = " must be a HIP device tensor: lgu_slam_amd has no CPU fallback"
_CASES = {}


def same_bits(a, b):
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    iv = torch.int16 if a.element_size() == 2 else torch.int32
    return bool(torch.equal(a.view(iv), b.view(iv)))


def case(shape):
    """(delta head, weight head, d, w, coords) on the CPU for one shape: distinct weights, distinct inputs, made once."""
    if shape not in _CASES:
        g = torch.Generator().manual_seed(900 + shape[1] * shape[2])
        N, H, W = shape
        ys, xs = torch.meshgrid(torch.arange(H).float(), torch.arange(W).float(), indexing="ij")
        coords = (torch.stack([xs, ys], -1)[None, None] + 3 * torch.randn((1, N, H, W, 2), generator=g)).contiguous()
        _CASES[shape] = (RH.make_head(81, 2), RH.make_head(82, 2), R.make_input(5000 + H * W, *shape), R.make_input(6000 + H * W, *shape),
                         coords)
    return _CASES[shape]


def to_edges(t):
    N, _, H, W = t.shape
    return t.view(1, N, -1, H, W).permute(0, 1, 3, 4, 2)[..., :2].contiguous()


# ---- CPU ------------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_entry(lgu):
    from tests.test_abi import declared_symbols
    lib = ctypes.CDLL(lgu._lib._build.SO_PATH)
    assert ENTRY in declared_symbols() and hasattr(lib, ENTRY)
    sig = lgu._lib.SIGNATURES[ENTRY]
    assert sig[0] is lgu._lib.HeadPairArgs and issubclass(sig[0], ctypes.Structure) and sig[1] is ctypes.c_void_p
    assert [f[0] for f in sig[0]._fields_] == ["x", "wpack", "bias", "out", "coords", "N", "H", "W", "flags"]
    assert ctypes.sizeof(sig[0]) == 9 * 8 + 4 * 4
    assert lgu.head_pair is lgu.heads.head_pair and isinstance(lgu.heads.MIN_PAIR_PIXELS, int)
    text = open(os.path.join(ROOT, "include", "lgu_corr.h")).read()
    assert "int lgu_head3x3_pair_c128_h16(lgu_head_pair_args args, void* stream);" in text
    assert "#define LGU_HEAD_PAIR_F32 %d " % lgu.heads.PAIR_F32 in text
    assert lgu.heads.PAIR_F32 not in (lgu.heads.X_HALF, lgu.heads.SIGMOID, lgu.heads.SOFTPLUS)
    assert lgu.__version__ == "0.8.0"


def test_operator_refusals_in_their_order(lgu):
    """Shapes of d and w, the packs' sizes and bias shapes, coords' shape, contiguity, dtypes, no-grad, device: each
    refusal's text, and which of two defects is reported.  None of them touches a device."""
    f = lgu.heads.head_pair
    H = torch.float16

    def z(*shape, dtype=torch.float32):
        return torch.zeros(shape, dtype=dtype)

    def nc(t):
        return torch.zeros(tuple(t.shape) + (2,), dtype=t.dtype)[..., 0]

    d, wp, bh, co = z(1, 128, 2, 3), z(4, 2, 64, 8, dtype=H), z(2, dtype=H), z(1, 1, 2, 3, 2)
    pk = (wp, bh)
    no_grad = "head_pair has no autograd: its outputs would carry no gradient. Call it under torch.no_grad() or pass detached inputs"
    cases = [
        ((d, d, pk, pk), {}, "d" + _NO_CPU),
        ((d.half(), d.half(), pk, pk), dict(coords=co), "d" + _NO_CPU),
        ((z(1, 127, 2, 3), d, pk, pk), {}, "d must be (N,128,H,W), got (1, 127, 2, 3)"),
        ((d, z(128, 2, 3), pk, pk), {}, "w must be (N,128,H,W), got (128, 2, 3)"),
        ((d, z(1, 128, 3, 2), pk, pk), {}, "w must be (1, 128, 2, 3), got (1, 128, 3, 2)"),
        ((d, d, (z(4, 1, 64, 8, dtype=H), bh), pk), {}, "pack_delta: wpack must hold 4096 halves (pack_head, Cout 2), got (4, 1, 64, 8)"),
        ((d, d, pk, (wp, z(1, dtype=H))), {}, "pack_weight: bias_h must be (2,), got (1,)"),
        ((d, d, pk, pk), dict(coords=z(1, 1, 2, 3)), "coords must be (1, 1, 2, 3, 2), got (1, 1, 2, 3)"),
        ((d, d, pk, pk), dict(coords=z(1, 2, 3, 2)), "coords must be (1, 1, 2, 3, 2), got (1, 2, 3, 2)"),
        ((nc(d), d, pk, pk), {}, "d must be contiguous"),
        ((d, nc(d), pk, pk), {}, "w must be contiguous"),
        ((d, d, pk, (nc(wp), bh)), {}, "pack_weight: wpack must be contiguous"),
        ((d, d, (wp, nc(bh)), pk), {}, "pack_delta: bias_h must be contiguous"),
        ((d, d, pk, pk), dict(coords=nc(co)), "coords must be contiguous"),
        ((d.double(), d.double(), pk, pk), {}, "expected scalar type Float or Half but found Double (d)"),
        ((d, d.half(), pk, pk), {}, "expected scalar type Float but found Half (w)"),
        ((d.half(), d, pk, pk), {}, "expected scalar type Half but found Float (w)"),
        ((d, d, (wp.float(), bh), pk), {}, "expected scalar type Half but found Float (pack_delta: wpack)"),
        ((d, d, pk, (wp, bh.bfloat16())), {}, "expected scalar type Half but found BFloat16 (pack_weight: bias_h)"),
        ((d, d, pk, pk), dict(coords=co.half()), "expected scalar type Float but found Half (coords)"),
        ((d, d, pk, pk), dict(coords=co.double()), "expected scalar type Float but found Double (coords)"),
        ((d.clone().requires_grad_(), d, pk, pk), {}, no_grad),
        ((d, d, pk, pk), dict(coords=co.clone().requires_grad_()), no_grad),
        # two defects: the earlier check reports
        ((z(1, 127, 2, 3), d, (z(5, dtype=H), bh), pk), {}, "d must be (N,128,H,W), got (1, 127, 2, 3)"),
        ((nc(d), d, (z(5, dtype=H), bh), pk), {}, "pack_delta: wpack must hold 4096 halves (pack_head, Cout 2), got (5,)"),
        ((nc(d), d, pk, pk), dict(coords=z(1, 1, 2, 3)), "coords must be (1, 1, 2, 3, 2), got (1, 1, 2, 3)"),
        ((d.double(), d.double(), pk, pk), dict(coords=nc(co)), "coords must be contiguous"),
        ((d.clone().requires_grad_(), d, pk, pk), dict(coords=co.half()), "expected scalar type Float but found Half (coords)"),
    ]
    for args, kw, message in cases:
        with pytest.raises(RuntimeError) as info:
            f(*args, **kw)
        assert type(info.value) is RuntimeError and str(info.value) == message
    with torch.no_grad():      # grad mode off: the no-grad refusal does not apply, the device refusal is next
        with pytest.raises(RuntimeError) as info:
            f(d.clone().requires_grad_(), d, pk, pk)
        assert str(info.value) == "d" + _NO_CPU


# ---- GPU ------------------------------------------------------------------------------------------------------------
def _need_gpu(lgu):
    assert torch.cuda.is_available(), "these tests need the MI355X"
    assert os.path.exists(lgu._lib.so_path()), "liblgu_corr.so missing — run __graft_entry__.build()"


def _packed(lgu, m):
    return lgu.heads.pack_head(m.weight.detach().cuda(), m.bias.detach().cuda())


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES)
def test_both_modes_have_the_bits_of_the_separate_launches(lgu, shape):
    _need_gpu(lgu)
    H = lgu.heads
    md, mw, d, w, coords = case(shape)
    pd, pw = _packed(lgu, md), _packed(lgu, mw)
    cc = coords.cuda()
    for dd, ww in ((d.cuda(), w.cuda()), (d.cuda().half(), w.cuda().half())):
        delta_h = to_edges(H.head_conv3x3(dd, *pd, act="none"))
        weight_h = to_edges(H.head_conv3x3(ww, *pw, act="sigmoid"))
        delta, weight = H.head_pair(dd, ww, pd, pw)
        target, weight_f = H.head_pair(dd, ww, pd, pw, coords=cc)
        torch.cuda.synchronize()
        for t in (delta, weight, target, weight_f):
            assert tuple(t.shape) == (1,) + shape + (2,) and t.is_contiguous()
        assert delta.dtype == weight.dtype == torch.float16 and target.dtype == weight_f.dtype == torch.float32
        assert same_bits(delta, delta_h) and same_bits(weight, weight_h), str(dd.dtype)
        assert torch.equal(target, cc + delta_h.to(dtype=torch.float)) and torch.equal(weight_f, weight_h.to(dtype=torch.float))
        assert same_bits(cc, coords)
        # swapped operands are another result: the heads are told apart
        if shape != (1, 1, 1):
            other = H.head_pair(ww, dd, pw, pd)
            assert not same_bits(other[0], delta) and not same_bits(other[1], weight)
    assert tuple(H.head_pair(d.cuda()[:0], w.cuda()[:0], pd, pw)[0].shape) == (1, 0) + shape[1:] + (2,)


@pytest.mark.gpu
@pytest.mark.parametrize("half_x", (False, True))
def test_one_case_per_dtype_is_within_the_float64_bound(lgu, half_x):
    """delta: |h - s64| <= allowance(s64, S, 1154); weight: the sigmoid's act_allowance on top; float32 mode: weight
    unchanged (the conversion is exact), target within the allowance plus one fp32 rounding of the add,
    2^-24 (|coords| + |s64| + allowance)."""
    _need_gpu(lgu)
    shape = (2, 9, 33)
    md, mw, d, w, coords = case(shape)
    pd, pw = _packed(lgu, md), _packed(lgu, mw)
    dd, ww = (d.half(), w.half()) if half_x else (d, w)
    delta, weight = lgu.heads.head_pair(dd.cuda(), ww.cuda(), pd, pw)
    target, weight_f = lgu.heads.head_pair(dd.cuda(), ww.cuda(), pd, pw, coords=coords.cuda())
    torch.cuda.synchronize()
    with torch.no_grad():
        (sd, Sd), (sw, Sw) = RH.head(dd, md.weight, md.bias), RH.head(ww, mw.weight, mw.bias)
    planar = lambda t: t[0].permute(0, 3, 1, 2).cpu().double()      # noqa: E731
    ad = R.allowance(sd, Sd, RH.TERMS)
    yw = RH.act64(sw, "sigmoid")
    aw = RH.act_allowance(yw, R.allowance(sw, Sw, RH.TERMS), "sigmoid")
    c64 = planar(coords)
    at = ad + U24 * (c64.abs() + sd.abs() + ad)
    for name, got, ref, bound in (("delta", delta, sd, ad), ("weight", weight, yw, aw), ("target", target, c64 + sd, at),
                                  ("weight float32", weight_f, yw, aw)):
        err = (planar(got) - ref).abs()
        print("head_pair %s %s half_x=%s: worst error %.3g of its bound" % (name, shape, half_x, float((err / bound).max())))
        assert bool((err <= bound).all()), (name, float((err / bound).max()))


@pytest.mark.gpu
@pytest.mark.parametrize("shape,at", [((2, 9, 33), (1, 5, 3, 32)), ((2, 5, 65), (0, 127, 4, 64)), ((1, 6, 40), (0, 64, 0, 0))])
def test_nan_locality(lgu, shape, at):
    _need_gpu(lgu)
    H = lgu.heads
    md, mw, d, w, coords = case(shape)
    pd, pw = _packed(lgu, md), _packed(lgu, mw)
    cc = coords.cuda()
    clean = [t.cpu() for t in H.head_pair(d.cuda(), w.cuda(), pd, pw) + H.head_pair(d.cuda(), w.cuda(), pd, pw, coords=cc)]
    assert not any(bool(torch.isnan(t).any()) for t in clean)
    n, _, cy, cx = at
    want = torch.zeros((1,) + shape + (1,), dtype=torch.bool)
    want[0, n, max(cy - 1, 0):cy + 2, max(cx - 1, 0):cx + 2] = True
    for which in (0, 1):
        ins = [d.clone(), w.clone()]
        ins[which][at] = float("nan")
        got = [t.cpu() for t in H.head_pair(ins[0].cuda(), ins[1].cuda(), pd, pw) + H.head_pair(ins[0].cuda(), ins[1].cuda(), pd, pw, coords=cc)]
        for k, t in enumerate(got):
            if k % 2 == which:      # the head that read the NaN: exactly the 3x3 neighbourhood, both channels
                assert bool((torch.isnan(t) == want.expand_as(t)).all()), (which, k)
                assert bool((t == clean[k])[~want.expand_as(t)].all()), (which, k)
            else:
                assert same_bits(t, clean[k]), (which, k)
    # coords: a NaN and an Inf show at their own element only, and the weight does not see them
    e_nan, e_inf = (0, n, cy, cx, 1), (0, shape[0] - 1, shape[1] - 1, shape[2] - 1, 0)
    cn = coords.clone()
    cn[e_nan], cn[e_inf] = float("nan"), float("inf")
    target, weight_f = (t.cpu() for t in H.head_pair(d.cuda(), w.cuda(), pd, pw, coords=cn.cuda()))
    moved = torch.zeros_like(target, dtype=torch.bool)
    moved[e_nan] = moved[e_inf] = True
    if e_nan != e_inf:
        assert bool(torch.isnan(target[e_nan])) and float(target[e_inf]) == float("inf")
    assert bool((target == clean[2])[~moved].all()) and not bool(torch.isfinite(target[moved]).any())
    assert same_bits(weight_f, clean[3])


def _c_call(lgu, d, w, pd, pw, outs, coords, flags, n=None):
    N, _, H, W = d.shape
    two = ctypes.c_void_p * 2
    flags |= lgu.heads.X_HALF if d.dtype == torch.float16 else 0
    args = lgu._lib.HeadPairArgs(two(d.data_ptr(), w.data_ptr()), two(pd[0].data_ptr(), pw[0].data_ptr()),
                                 two(pd[1].data_ptr(), pw[1].data_ptr()), two(outs[0].data_ptr(), outs[1].data_ptr()),
                                 None if coords is None else coords.data_ptr(), N if n is None else n, H, W, flags)
    rc = lgu._lib.load().lgu_head3x3_pair_c128_h16(args, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc


@pytest.mark.gpu
@pytest.mark.parametrize("f32", (False, True))
@pytest.mark.parametrize("half_x", (False, True))
@pytest.mark.parametrize("shape", [(2, 9, 33), (1, 6, 40)])
def test_guard_bands_and_alignment(lgu, shape, half_x, f32):
    """lgu_head3x3_pair_c128_h16 through the C ABI (its operands travel in a parameter block, so the registry of
    tests/alignment_cases.py does not see it), in both output modes."""
    from tests.alignment_cases import guards_intact, shifted, shifts_for
    _need_gpu(lgu)
    H, L = lgu.heads, lgu._lib
    md, mw, d, w, coords = case(shape)
    pd, pw = _packed(lgu, md), _packed(lgu, mw)
    dd, ww = (d.cuda().half(), w.cuda().half()) if half_x else (d.cuda(), w.cuda())
    cc = coords.cuda() if f32 else None
    flag = H.PAIR_F32 if f32 else 0
    want = H.head_pair(dd, ww, pd, pw, coords=cc)
    pixel = 8 if f32 else 4

    def fresh(shift=0):
        return [shifted(torch.zeros_like(want[0]), shift) for _ in range(2)]
    outs = fresh()
    assert _c_call(lgu, dd, ww, pd, pw, outs, cc, flag) == 0
    assert all(same_bits(o, t) and guards_intact(o) for o, t in zip(outs, want))
    # x and the biases at element alignment, the outputs and coords at every whole-pixel shift: the aligned call's bits
    served = [("x", s) for s in shifts_for(dd.dtype)] + [("bias", s) for s in (2, 4, 8)] + [("out", s) for s in (4, 8) if s % pixel == 0]
    served += [("coords", 8)] if f32 else []
    for key, shift in served + [("all", 0)]:
        xs = [shifted(t, shift if key == "x" else t.element_size()) for t in (dd, ww)] if key in ("x", "all") else [dd, ww]
        ps = [(p[0], shifted(p[1], shift if key == "bias" else 2)) for p in (pd, pw)] if key in ("bias", "all") else [pd, pw]
        outs = fresh(shift if key == "out" else pixel % 16) if key in ("out", "all") else fresh()
        cs = shifted(cc, shift if key == "coords" else 8) if f32 and key in ("coords", "all") else cc
        assert _c_call(lgu, xs[0], xs[1], ps[0], ps[1], outs, cs, flag) == 0, (key, shift)
        assert all(same_bits(o, t) for o, t in zip(outs, want)), "%s shifted by %d: differs from the aligned call" % (key, shift)
        assert all(guards_intact(t) for t in outs + [t for t in xs + [ps[0][1], ps[1][1], cs] if hasattr(t, "_lgu_guard")])
        assert same_bits(xs[0], dd) and same_bits(xs[1], ww) and (cs is None or same_bits(cs, cc))
    # refused before the launch, nothing written: a wpack off 16 bytes, an output or coords off a whole pixel
    outs = fresh()
    for k in range(2):
        ps = [(shifted(p[0], 8), p[1]) if i == k else p for i, p in enumerate((pd, pw))]
        assert _c_call(lgu, dd, ww, ps[0], ps[1], outs, cc, flag) == L.LGU_E_UNSUPPORTED
        for shift in [s for s in ((4, 8) if f32 else (2, 4, 8)) if s % pixel]:
            bad = fresh()
            bad[k] = shifted(torch.zeros_like(want[0]), shift)
            assert _c_call(lgu, dd, ww, pd, pw, bad, cc, flag) == L.LGU_E_UNSUPPORTED, (k, shift)
            assert all(not bool(o.any()) and guards_intact(o) for o in bad)
    if f32:
        assert _c_call(lgu, dd, ww, pd, pw, outs, shifted(cc, 4), flag) == L.LGU_E_UNSUPPORTED
    # a flag / coords mismatch, an unknown flag, a negative N: LGU_E_BADARG; N == 0: nothing launched
    assert _c_call(lgu, dd, ww, pd, pw, outs, None if f32 else coords.cuda(), flag) == L.LGU_E_BADARG
    assert _c_call(lgu, dd, ww, pd, pw, outs, cc, flag | H.SIGMOID) == L.LGU_E_BADARG
    assert _c_call(lgu, dd, ww, pd, pw, outs, cc, flag, n=-1) == L.LGU_E_BADARG
    assert _c_call(lgu, dd, ww, pd, pw, outs, cc, flag, n=0) == 0
    assert all(not bool(o.any()) and guards_intact(o) for o in outs)
