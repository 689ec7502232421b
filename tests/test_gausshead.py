"""The Gaussian mask's fused parameter head (lgu_slam_amd.gaussian_mask.gaussian_head / install, csrc/gausshead.hip) against
the float64 restatement tests/gausshead_restatement.py.

Numerics contract (include/lgu_corr.h lgu_gaussian_head):
- every element of mean_ofs, cov_raw and the hidden tt is within the bound gausshead_restatement.bounds derives from the
  arithmetic (half mode: exact products, fp32 accumulation, one half rounding after each bias and after tanh; fp32 mode:
  fp32 fused multiply-add chains), on half x, on fp32 x (rounded to half exactly once) and in fp32 mode;
- the reference's own half run (the committed autocast fixture) lies within the same bound, so kernel and fixture are
  within twice the bound of each other;
- the bits of a pixel depend on its own 256 inputs only; a NaN reaches exactly its pixel; nothing outside the outputs is
  written; an x that is not 16-byte aligned is refused before a launch.
The module's own autocast forward is not held to the bound; the bound test prints where it sits.
The GPU tests never read the reference tree.
"""
import ctypes
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import gausshead_restatement as R  # noqa: E402
from tests.test_glue_reference import GOLD, REF, T, _gen, build_heads, gold  # noqa: E402
from tests.test_upmask import same_bits  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = "lgu_gaussian_head"
TILE = 16           # pixels per MFMA tile of csrc/gausshead.hip
needs_ref = pytest.mark.skipif(not os.path.isdir(REF), reason="reference checkout not present on this machine")
# the issue's shapes: one pixel; 42 pixels (a ragged last tile, a sample boundary inside a tile); 65 (one past a tile
# boundary); the fixture's shape; 2304 tiles, more than the 8 x 256 waves of a launch on an MI355X, so that a wave runs a
# second tile on the prefetched registers
SHAPES = [(1, 1, 1), (2, 3, 7), (1, 5, 13), (3, 16, 16), (12, 48, 64)]
assert (12 * 48 * 64) // TILE > 8 * 256
MODES = ["half", "half_x32", "fp32"]      # half x in half mode; fp32 x in half mode; fp32 mode
_NO_CPU = " must be a HIP device tensor: lgu_slam_amd has no CPU fallback"
_CASES = {}
W = R.make_weights(7)


def case(shape, half):
    """(x, chain, bounds) on the CPU for one shape and arithmetic mode, computed once and never changed."""
    key = (shape, half)
    if key not in _CASES:
        x = R.make_input(900 + shape[0] * shape[1] * shape[2], *shape)
        c = R.chain(x, *W, half=half)
        _CASES[key] = (x, c, R.bounds(c, half))
    return _CASES[key]


def make_ga(lgu, h, w, weights=W):
    return R.load(lgu.GaussianMask(h, w), *weights).eval()


def fixture():
    """(x (3,16,16,256) half, (W1,b1,W2,b2), raw_map, raw_mean_ofs, raw_cov) of the committed glue fixtures: blocks A
    (edges 0..1) and B (edge 2) joined."""
    z, zh = gold("glue_corrblock_16x16"), gold("glue_heads")
    za = np.load(os.path.join(GOLD, "glue_corrblock_autocast_16x16_heads.npz"), allow_pickle=False)
    x = torch.cat((T(z["fmap1"])[0], T(z["fmap2"])[0]), dim=1).permute(0, 2, 3, 1).contiguous()
    assert x.dtype == torch.float16 and tuple(x.shape) == (3, 16, 16, 256) and int(z["E_a"]) == 2
    W2 = torch.cat((T(zh["w:GA.meanMap.weight"]), T(zh["w:GA.covMap.weight"])))
    b2 = torch.cat((T(zh["w:GA.meanMap.bias"]), T(zh["w:GA.covMap.bias"])))
    weights = (T(zh["w:GA.map.weight"]), T(zh["w:GA.map.bias"]), W2, b2)
    raw = [torch.cat((T(za["A_" + k]), T(za["B_" + k]))) for k in ("raw_map", "raw_mean_ofs", "raw_cov")]
    assert all(r.dtype == torch.float16 for r in raw)
    return (x, weights) + tuple(raw)


# ---- CPU ------------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_entry(lgu):
    from tests.test_abi import declared_symbols
    lib = ctypes.CDLL(lgu._lib._build.SO_PATH)
    L, M = lgu._lib, lgu.gaussian_mask
    assert ENTRY in declared_symbols() and hasattr(lib, ENTRY) and ENTRY in L.SIGNATURES
    sig = L.SIGNATURES[ENTRY]
    assert sig[0] is L.GaussHeadArgs and issubclass(sig[0], ctypes.Structure) and sig[1] is ctypes.c_void_p
    assert [f[0] for f in sig[0]._fields_] == ["x", "wpack", "bias", "mean_ofs", "cov_raw", "hidden", "E", "H", "W", "flags"]
    assert ctypes.sizeof(sig[0]) == 6 * 8 + 4 * 4
    assert "gausshead.hip" in lgu._build.SOURCES
    assert lgu.gaussian_head is M.gaussian_head and lgu.pack_gaussian_head is M.pack_gaussian_head and lgu.GaussianHead is M.GaussianHead
    text = open(os.path.join(ROOT, "include", "lgu_corr.h")).read()
    assert M.WPACK_ELEMS == 256 * 16 + 64 * 4 == 4352 and M.BIAS_ELEMS == 20 and (M.CIN, M.HIDDEN) == (256, 16)
    for name, val in (("WPACK_ELEMS", M.WPACK_ELEMS), ("BIAS_ELEMS", M.BIAS_ELEMS), ("CIN", M.CIN), ("HIDDEN", M.HIDDEN)):
        assert "#define LGU_GAUSSHEAD_%s %d\n" % (name, val) in text
    assert "#define LGU_GAUSSHEAD_X_HALF %d " % M.X_HALF in text and "#define LGU_GAUSSHEAD_FP32 %d " % M.FP32 in text
    assert M.X_HALF & M.FP32 == 0 and isinstance(M.MIN_FUSED_PIXELS, int) and M.MIN_FUSED_PIXELS >= 0


@pytest.mark.parametrize("half", (True, False))
def test_pack_puts_every_weight_in_its_documented_slot_and_zero_elsewhere(lgu, half):
    """The docstring's index formula as a plain loop: each of the 256*16 + 16*4 weights and 20 biases exactly once, the
    padded rows of the second operand zero."""
    ga = make_ga(lgu, 2, 2)
    W1, b1, W2, b2 = W
    assert bool((W1 != 0).all()) and bool((W2 != 0).all()) and bool((b2 != 0).all())
    wpack, bias = lgu.gaussian_mask.pack_gaussian_head(ga.map, ga.meanMap, ga.covMap, half)
    dt = torch.float16 if half else torch.float32
    assert wpack.dtype == dt == bias.dtype and wpack.is_contiguous() and tuple(wpack.shape) == (4352,) and tuple(bias.shape) == (20,)
    assert same_bits(bias, torch.cat((b1, b2)).to(dt))
    want = torch.zeros(4352, dtype=dt)
    named = []                                   # which weight each live slot names
    W1r, W2r = W1.to(dt), W2.to(dt)
    for lane in range(64):
        r, g = lane & 15, lane >> 4
        if half:
            for kc in range(8):
                for j in range(8):
                    want[(kc * 64 + lane) * 8 + j] = W1r[r, 32 * kc + 8 * g + j]
                    named.append(("W1", r, 32 * kc + 8 * g + j))
            for j in range(4):
                if r < 4:
                    want[4096 + 4 * lane + j] = W2r[r, 4 * g + j]
                    named.append(("W2", r, 4 * g + j))
        else:
            for s in range(64):
                want[s * 64 + lane] = W1r[r, 16 * (s >> 2) + 4 * g + (s & 3)]
                named.append(("W1", r, 16 * (s >> 2) + 4 * g + (s & 3)))
            for i in range(4):
                if r < 4:
                    want[4096 + 64 * i + lane] = W2r[r, 4 * g + i]
                    named.append(("W2", r, 4 * g + i))
    assert sorted(named) == sorted([("W1", r, c) for r in range(16) for c in range(256)] + [("W2", r, k) for r in range(4) for k in range(16)])
    assert same_bits(wpack, want)
    assert int((wpack[4096:] == 0).sum()) == 256 - 64 and int((wpack[:4096] == 0).sum()) == 0


@pytest.mark.parametrize("half", (True, False))
def test_restatement_equals_this_builds_modules_in_float64(lgu, half):
    x, c, (a1, a2, a3) = case((2, 3, 7), half)
    r = R.h64 if half else R.f64
    ga = make_ga(lgu, 3, 7, tuple(r(t) for t in W)).double()
    with torch.no_grad():
        u = ga.map(r(x))
        tt = ga.mapA(r(x))
        m, cv = ga.meanMap(tt), ga.covMap(tt)
    tol = 2.0 ** -44
    assert bool(((u - c["s1"]).abs() <= tol * c["S1"]).all()) and bool(((tt - c["tt"]).abs() <= tol * (1 + c["S1"])).all())
    mean, cov = R.split(c["s2"])
    assert bool(((m - mean).abs() <= tol * (1 + c["S2"][..., :2])).all())
    assert bool(((cv.reshape(2, 21, 2) - cov).abs() <= tol * (1 + c["S2"][..., 2:].reshape(2, 21, 2))).all())
    assert bool((c["S1"] >= c["s1"].abs()).all()) and bool((a1 > 0).all()) and bool((a2 > a1).all()) and bool((a3 > 0).all())
    assert R.TERMS1 == 258 and R.TERMS2 == 18


@needs_ref
def test_restatement_equals_the_references_own_modules_in_float64():
    ref_ga = _gen().load_reference_glue()[1]
    x, c, _ = case((2, 3, 7), True)
    ga = R.load(ref_ga.GaussianMask(3, 7), *(R.h64(t) for t in W)).double()
    with torch.no_grad():
        u = ga.map(R.h64(x))
        tt = ga.mapA(R.h64(x))
        m, cv = ga.meanMap(tt), ga.covMap(tt)
    tol = 2.0 ** -44
    assert bool(((u - c["s1"]).abs() <= tol * c["S1"]).all()) and bool(((tt - c["tt"]).abs() <= tol * (1 + c["S1"])).all())
    assert bool(((torch.cat((m, cv), dim=-1) - c["s2"]).abs() <= tol * (1 + c["S2"])).all())


def test_the_references_own_half_run_stays_inside_the_bound():
    """The committed autocast fixture (the reference's unchanged modules under float16 autocast) against the float64 chain
    on the committed inputs and weights: map within a1, the two heads within the output bound."""
    x, weights, raw_map, raw_mean, raw_cov = fixture()
    c = R.chain(x, *weights, half=True)
    a1, a2, a3 = R.bounds(c, True)
    e1 = (raw_map.double() - c["s1"]).abs() / a1
    e3 = (torch.cat((raw_mean, raw_cov), dim=-1).double() - c["s2"]).abs() / a3
    print("the reference's half run: map worst %.3g of a1, heads worst %.3g of the output bound" % (float(e1.max()), float(e3.max())))
    assert float(e1.max()) <= 1.0 and float(e3.max()) <= 1.0
    assert bool((weights[2][:2] != 0).any()), "the fixture's mean head is not zero"


def test_operator_refusals_come_before_any_launch(lgu, monkeypatch):
    M = lgu.gaussian_mask
    launched = []
    monkeypatch.setattr(M, "launch", lambda *a, **k: launched.append(a))
    H = torch.float16

    def z(*shape, dtype=torch.float32):
        return torch.zeros(shape, dtype=dtype)

    def nc(t):
        return torch.zeros(tuple(t.shape) + (2,), dtype=t.dtype)[..., 0]

    x, wp, b = z(2, 3, 5, 256), z(4352, dtype=H), z(20, dtype=H)
    no_grad = "gaussian_head has no autograd: its outputs would carry no gradient. Call it under torch.no_grad() or pass detached inputs"
    table = [
        ((x, wp, b), {"half": True}, "x" + _NO_CPU),
        ((x, wp.float(), b.float()), {"half": False}, "x" + _NO_CPU),
        ((x, wp.float(), b.float()), {}, "x" + _NO_CPU),                    # half=None without autocast: fp32 mode
        ((z(3, 5, 256), wp, b), {"half": True}, "x must be (E,h,w,256), got (3, 5, 256)"),
        ((z(2, 3, 5, 128), wp, b), {"half": True}, "x must be (E,h,w,256), got (2, 3, 5, 128)"),
        ((x, z(4351, dtype=H), b), {"half": True}, "wpack must hold 4352 elements (pack_gaussian_head), got (4351,)"),
        ((x, wp, z(16, dtype=H)), {"half": True}, "bias must be (20,), got (16,)"),
        ((nc(x), wp, b), {"half": True}, "x must be contiguous"),
        ((x, nc(wp), b), {"half": True}, "wpack must be contiguous"),
        ((x.double(), wp, b), {"half": True}, "expected scalar type Float or Half but found Double (x)"),
        ((x.half(), wp.float(), b.float()), {"half": False}, "expected scalar type Float but found Half (x)"),
        ((x, wp.float(), b), {"half": True}, "expected scalar type Half but found Float (wpack)"),
        ((x, wp.float(), b), {"half": False}, "expected scalar type Float but found Half (bias)"),
        ((x.clone().requires_grad_(), wp, b), {"half": True}, no_grad),
        ((z(2, 0, 5, 256), wp, b), {"half": True}, "x" + _NO_CPU),           # the empty sample is refused after the device
    ]
    for args, kw, message in table:
        with pytest.raises(RuntimeError) as info:
            M.gaussian_head(*args, **kw)
        assert type(info.value) is RuntimeError and str(info.value) == message
    assert launched == []
    nn = torch.nn
    for bad in ((nn.Linear(128, 16), nn.Linear(16, 2), nn.Linear(16, 2)), (nn.Linear(256, 16), nn.Linear(16, 3), nn.Linear(16, 2)),
                (nn.Linear(256, 16), nn.Linear(16, 2), nn.Linear(16, 2, bias=False)), (nn.Linear(256, 8), nn.Linear(8, 2), nn.Linear(8, 2)),
                (nn.Conv2d(256, 16, 1), nn.Linear(16, 2), nn.Linear(16, 2))):
        for half in (True, False):
            with pytest.raises(RuntimeError, match="pack_gaussian_head: map must be Linear"):
                M.pack_gaussian_head(*bad, half)


def test_install_binds_one_wrapper_and_cpu_inputs_take_the_modules_path(lgu):
    M = lgu.gaussian_mask
    ga = make_ga(lgu, 3, 7)
    keys = list(ga.state_dict().keys())
    x = R.make_input(3, 2, 3, 7)
    with torch.no_grad():
        want = ga.gaussian_parameters(x)
        wr = M.install(ga)
        assert isinstance(wr, M.GaussianHead) and ga.gaussian_parameters is wr and M.install(ga) is wr
        assert list(ga.state_dict().keys()) == keys and len(list(ga.parameters())) == 6
        got = ga.gaussian_parameters(x)
    assert wr.fused_calls == 0 and all(same_bits(a, b) for a, b in zip(got, want))
    # the cache follows the parameters, one pack per mode
    p = wr.packed(True)
    assert wr.packed(True) is p and wr.packed(False) is not p and wr.packed(False)[0].dtype == torch.float32
    with torch.no_grad():
        ga.map.weight.mul_(2.0)
    assert wr.packed(True) is not p and same_bits(wr.packed(True)[0], M.pack_gaussian_head(ga.map, ga.meanMap, ga.covMap, True)[0])
    M.uninstall(ga)
    assert "gaussian_parameters" not in ga.__dict__ and ga.gaussian_parameters.__func__ is M.GaussianMask.gaussian_parameters
    M.uninstall(ga)                       # nothing bound: nothing happens
    for bad in (torch.nn.Linear(256, 16), torch.nn.Sequential(ga), object(), None):
        with pytest.raises(RuntimeError, match="gaussian_mask.install: the module must be"):
            M.install(bad)
        with pytest.raises(RuntimeError, match="GaussianHead: the module must be"):
            M.GaussianHead(bad)


# ---- GPU ------------------------------------------------------------------------------------------------------------
def _need_gpu(lgu):
    assert torch.cuda.is_available(), "these tests need the MI355X"
    assert os.path.exists(lgu._lib.so_path()), "liblgu_corr.so missing — run __graft_entry__.build()"


@pytest.fixture
def no_threshold(lgu, monkeypatch):
    """The wrapper's routing by size follows a measurement (MIN_FUSED_PIXELS); these tests are about the fused path."""
    monkeypatch.setattr(lgu.gaussian_mask, "MIN_FUSED_PIXELS", 0)


def _packed(lgu, half, weights=W, h=1, w=1):
    ga = make_ga(lgu, h, w, weights).cuda()
    return lgu.gaussian_mask.pack_gaussian_head(ga.map, ga.meanMap, ga.covMap, half)


def _x_of(x, mode):
    xc = x.cuda()
    return xc.half() if mode == "half" else xc


def _check_bound(got, c, bnd, what):
    """mean_ofs, cov_raw, tt of one call against the chain; returns the worst fractions (heads, hidden)."""
    mean, cov, tt = got
    a1, a2, a3 = bnd
    ref_mean, ref_cov = R.split(c["s2"])
    am, ac = R.split(a3)
    em = (mean.cpu().double() - ref_mean).abs() / am
    ec = (cov.cpu().double() - ref_cov).abs() / ac
    et = (tt.cpu().double() - c["tt"]).abs() / a2
    worst = max(float(em.max()), float(ec.max()))
    assert worst <= 1.0 and float(et.max()) <= 1.0, (what, worst, float(et.max()))
    return worst, float(et.max())


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", SHAPES)
def test_every_element_is_within_the_derived_bound(lgu, shape, mode):
    """mean_ofs, cov_raw and tt within gausshead_restatement.bounds of the float64 chain; prints where the module's own
    forward (autocast for the half modes) sits and what share of its elements has the kernel's bits."""
    _need_gpu(lgu)
    M = lgu.gaussian_mask
    half = mode != "fp32"
    x, c, bnd = case(shape, half)
    E, h, w = shape
    xc = _x_of(x, mode)
    wpack, bias = _packed(lgu, half)
    got = M.gaussian_head(xc, wpack, bias, half=half, hidden=True)
    ga = make_ga(lgu, h, w).cuda()
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16, enabled=half):
        tt_own = ga.mapA(xc)
        own = (ga.meanMap(tt_own), ga.covMap(tt_own).view(E, h * w, 2), tt_own)
    torch.cuda.synchronize()
    dt = torch.float16 if half else torch.float32
    assert [tuple(t.shape) for t in got] == [(E, h, w, 2), (E, h * w, 2), (E, h, w, 16)] and all(t.dtype == dt and t.is_contiguous() for t in got)
    assert all(o.dtype == dt for o in own)
    worst, worst_tt = _check_bound(got, c, bnd, (shape, mode))
    a1, a2, a3 = bnd
    own_frac = max(float(((o.cpu().double() - r).abs() / a).max())
                   for o, r, a in zip(own, R.split(c["s2"]) + (c["tt"],), R.split(a3) + (a2,)))
    ident = float(torch.cat([(o.reshape(-1) == g.reshape(-1)) for o, g in zip(own, got)]).double().mean())
    print("gaussian_head %s %s: heads worst %.3g, tt worst %.3g of the bound; the module's own forward: worst %.3g of the bound, "
          "%.4f bit-identical to the kernel" % (shape, mode, worst, worst_tt, own_frac, ident))


@pytest.mark.gpu
def test_fixture_inputs_within_the_bound_of_the_chain_and_twice_of_the_references_half_run(lgu):
    _need_gpu(lgu)
    M = lgu.gaussian_mask
    x, weights, raw_map, raw_mean, raw_cov = fixture()
    c = R.chain(x, *weights, half=True)
    a1, a2, a3 = R.bounds(c, True)
    ga = make_ga(lgu, 16, 16, weights).cuda()
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        got = M.gaussian_head(x.cuda(), *M.pack_gaussian_head(ga.map, ga.meanMap, ga.covMap, True), hidden=True)   # half=None: autocast
    torch.cuda.synchronize()
    assert all(t.dtype == torch.float16 for t in got)
    _check_bound(got, c, (a1, a2, a3), "fixture")
    mean, cov, tt = (t.cpu().double() for t in got)
    am, ac = R.split(a3)
    em = ((mean - raw_mean.double()).abs() / (2 * am)).max()
    ec = ((cov - raw_cov.double().reshape(3, 256, 2)).abs() / (2 * ac)).max()
    et = ((tt - torch.tanh(raw_map.double())).abs() / (2 * a2)).max()
    print("kernel against the reference's half run: mean_ofs %.3g, cov_raw %.3g, tt %.3g of twice the bound" % (float(em), float(ec), float(et)))
    assert float(em) <= 1.0 and float(ec) <= 1.0 and float(et) <= 1.0


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(2, 3, 7), (3, 16, 16), (12, 48, 64)])
def test_same_bits_across_call_forms(lgu, shape):
    """Whole or one sample at a time; under autocast fp32 x gives the bits of x.half(); hidden=True changes no output."""
    _need_gpu(lgu)
    M = lgu.gaussian_mask
    x, _, _ = case(shape, True)
    xc = x.cuda()
    for half in (True, False):
        wpack, bias = _packed(lgu, half)
        whole = M.gaussian_head(xc, wpack, bias, half=half, hidden=True)
        plain = M.gaussian_head(xc, wpack, bias, half=half)
        assert len(plain) == 2 and same_bits(plain[0], whole[0]) and same_bits(plain[1], whole[1])
        parts = [M.gaussian_head(xc[k:k + 1].contiguous(), wpack, bias, half=half, hidden=True) for k in range(shape[0])]
        for i in range(3):
            assert same_bits(torch.cat([p[i] for p in parts]), whole[i]), (half, i)
        back = M.gaussian_head(torch.flip(xc, dims=(0,)).contiguous(), wpack, bias, half=half, hidden=True)
        assert all(same_bits(torch.flip(b, dims=(0,)), a) for a, b in zip(whole, back))
    wpack, bias = _packed(lgu, True)
    with torch.autocast("cuda", dtype=torch.float16):
        a = M.gaussian_head(xc, wpack, bias, hidden=True)
        b = M.gaussian_head(xc.half(), wpack, bias, hidden=True)
        c = M.gaussian_head(xc.half().float(), wpack, bias, hidden=True)
    assert all(t.dtype == torch.float16 for t in a)
    assert all(same_bits(p, q) and same_bits(p, r) for p, q, r in zip(a, b, c))


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_nan_reaches_exactly_its_pixel(lgu, mode):
    """One NaN in one channel of one pixel: that pixel's 4 outputs and 16 hidden values, every other element keeps its
    bits.  (2,3,7): pixels 15 and 16 lie on either side of a tile boundary, 21 is the first of sample 1, 41 the last of
    the ragged tile; channels include the first and the last."""
    _need_gpu(lgu)
    M = lgu.gaussian_mask
    shape, half = (2, 3, 7), mode != "fp32"
    x, _, _ = case(shape, half)
    wpack, bias = _packed(lgu, half)
    clean = [t.cpu() for t in M.gaussian_head(_x_of(x, mode), wpack, bias, half=half, hidden=True)]
    assert not any(bool(torch.isnan(t).any()) for t in clean)
    iv = torch.int16 if half else torch.int32
    for pix, ch in ((15, 255), (16, 0), (21, 31), (41, 100), (0, 7)):
        xn = x.clone()
        xn.view(-1, 256)[pix, ch] = float("nan")
        got = [t.cpu() for t in M.gaussian_head(_x_of(xn, mode), wpack, bias, half=half, hidden=True)]
        for g, cl in zip(got, clean):
            g2, c2 = g.reshape(42, -1), cl.reshape(42, -1)
            want = torch.zeros_like(g2, dtype=torch.bool)
            want[pix] = True
            assert bool((torch.isnan(g2) == want).all()), (pix, ch, mode)
            assert bool((g2.view(iv) == c2.view(iv))[~want].all()), (pix, ch, mode)


def _c_entry(lgu, x, wpack, bias, mean, cov, hidden, flags, e=None):
    E, h, w, _ = x.shape
    args = lgu._lib.GaussHeadArgs(x.data_ptr(), wpack.data_ptr(), bias.data_ptr(), mean.data_ptr(), cov.data_ptr(),
                                  hidden.data_ptr() if hidden is not None else None, E if e is None else e, h, w, flags)
    rc = getattr(lgu._lib.load(), ENTRY)(args, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", [(2, 3, 7), (1, 5, 13)])
def test_guard_bands_through_the_c_entry(lgu, shape, mode):
    """Outputs carved out of sentinel-filled buffers, at 16-byte alignment and one element past it, with and without
    hidden: the Python call's bits, no byte outside the three tensors; every refusal writes nothing."""
    from tests.alignment_cases import guards_intact, shifted
    _need_gpu(lgu)
    M, L = lgu.gaussian_mask, lgu._lib
    half = mode != "fp32"
    x, _, _ = case(shape, half)
    xc = _x_of(x, mode)
    wpack, bias = _packed(lgu, half)
    want = M.gaussian_head(xc, wpack, bias, half=half, hidden=True)
    flags = (0 if half else M.FP32) | (M.X_HALF if xc.dtype == torch.float16 else 0)
    es = want[0].element_size()
    for shift in (0, es):
        for with_hidden in (True, False):
            outs = [shifted(torch.zeros_like(t), shift) for t in want]
            before = outs[2].clone()
            b = shifted(bias, shift)
            assert _c_entry(lgu, xc, wpack, b, outs[0], outs[1], outs[2] if with_hidden else None, flags) == 0
            assert same_bits(outs[0], want[0]) and same_bits(outs[1], want[1])
            assert same_bits(outs[2], want[2] if with_hidden else before)
            assert all(guards_intact(t) for t in outs) and guards_intact(b)
    outs = [shifted(torch.full_like(t, 0.25), 0) for t in want]
    for rc, kw in ((L.LGU_E_BADARG, dict(flags=flags | 4)), (L.LGU_E_BADARG, dict(flags=M.FP32 | M.X_HALF)), (L.LGU_E_BADARG, dict(flags=flags, e=-1)),
                   (0, dict(flags=flags, e=0))):
        assert _c_entry(lgu, xc, wpack, bias, *outs, **kw) == rc, kw
    assert _c_entry(lgu, shifted(xc, xc.element_size()), wpack, bias, *outs, flags=flags) == L.LGU_E_UNSUPPORTED
    assert _c_entry(lgu, xc, shifted(wpack, 8), bias, *outs, flags=flags) == L.LGU_E_UNSUPPORTED
    assert all(bool((t == 0.25).all()) and guards_intact(t) for t in outs)


@pytest.mark.gpu
def test_a_misaligned_x_is_refused_before_any_launch(lgu, monkeypatch):
    from tests.alignment_cases import shifted
    _need_gpu(lgu)
    M = lgu.gaussian_mask
    x, _, _ = case((2, 3, 7), True)
    launched = []
    real = M.launch
    monkeypatch.setattr(M, "launch", lambda *a, **k: (launched.append(a[0]), real(*a, **k)))
    for half, xin in ((True, x.cuda().half()), (True, x.cuda()), (False, x.cuda())):
        wpack, bias = _packed(lgu, half)
        view = torch.zeros(xin.numel() + 8, dtype=xin.dtype, device="cuda")[1:1 + xin.numel()].view(xin.shape)
        view.copy_(xin)
        assert view.is_contiguous() and view.data_ptr() % 16 == xin.element_size()
        with pytest.raises(lgu._lib.UnsupportedShape):
            M.gaussian_head(view, wpack, bias, half=half)
        with pytest.raises(lgu._lib.UnsupportedShape):
            M.gaussian_head(shifted(xin, 8), wpack, bias, half=half)
        assert launched == []
        M.gaussian_head(shifted(xin, 0), wpack, bias, half=half)
        assert launched == [ENTRY]
        del launched[:]
    assert tuple(M.gaussian_head(x.cuda()[:0], *_packed(lgu, True), half=True)[1].shape) == (0, 21, 2)
    with pytest.raises(RuntimeError, match="empty sample"):
        M.gaussian_head(x.cuda()[:, :0], *_packed(lgu, True), half=True)


def _count_class_calls(monkeypatch, lgu):
    cls, seen = lgu.gaussian_mask.GaussianMask, []
    orig = cls.gaussian_parameters

    def gaussian_parameters(self, x):
        seen.append(self)
        return orig(self, x)
    monkeypatch.setattr(cls, "gaussian_parameters", gaussian_parameters)
    return seen


@pytest.mark.gpu
def test_installed_route_is_the_head_then_the_tail_and_uninstall_restores(lgu, no_threshold, monkeypatch):
    _need_gpu(lgu)
    M = lgu.gaussian_mask
    shape = (2, 3, 7)
    x, _, _ = case(shape, True)
    xc = x.cuda()
    ga = make_ga(lgu, 3, 7).cuda()
    forms = [(xc.half(), True, True), (xc, True, True), (xc, False, False)]      # x, autocast, half mode
    with torch.no_grad():
        before = []
        for xin, ac, _ in forms:
            with torch.autocast("cuda", dtype=torch.float16, enabled=ac):
                before.append(ga.gaussian_parameters(xin))
        wr = M.install(ga)
        seen = _count_class_calls(monkeypatch, lgu)
        for n, (xin, ac, half) in enumerate(forms):
            with torch.autocast("cuda", dtype=torch.float16, enabled=ac):
                got = ga.gaussian_parameters(xin)
                want = lgu.ops.gaussian_params(*M.gaussian_head(xin, *wr.packed(half)), 3, 7)
            assert wr.fused_calls == n + 1 and seen == []
            assert len(got) == 3 and all(same_bits(a, b) for a, b in zip(got, want))
            assert [t.dtype for t in got] == [t.dtype for t in before[n]] and [t.shape for t in got] == [t.shape for t in before[n]]
            assert got[0].dtype == torch.float32 and tuple(got[0].shape) == (2, 3, 7, 2) and tuple(got[2].shape) == (2, 21)
        # a view that is not contiguous is served through its contiguous copy
        wide = torch.zeros((2, 3, 7, 512), device="cuda")
        wide[..., :256] = xc
        assert all(same_bits(a, b) for a, b in zip(ga.gaussian_parameters(wide[..., :256]), ga.gaussian_parameters(xc)))
        assert wr.fused_calls == 5 and seen == []
        M.uninstall(ga)
        for (xin, ac, _), want in zip(forms, before):
            with torch.autocast("cuda", dtype=torch.float16, enabled=ac):
                got = ga.gaussian_parameters(xin)
            assert all(same_bits(a, b) for a, b in zip(got, want))
    assert wr.fused_calls == 5 and len(seen) == 3


@pytest.mark.gpu
def test_other_calls_take_the_modules_own_path(lgu, no_threshold, monkeypatch):
    """CPU x, an x that requires grad, a bfloat16 autocast, a coord of another size, a raised MIN_FUSED_PIXELS and a
    misaligned x: the class's own gaussian_parameters, its bits, and the counter stays."""
    from tests.alignment_cases import shifted
    _need_gpu(lgu)
    M = lgu.gaussian_mask
    x, _, _ = case((2, 3, 7), True)
    xc = x.cuda()
    ga, twin = make_ga(lgu, 3, 7).cuda(), make_ga(lgu, 3, 7).cuda()
    wr = M.install(ga)
    seen = _count_class_calls(monkeypatch, lgu)

    def old_path(fn, n_seen):
        got, want = fn(ga), fn(twin)
        assert all(same_bits(a, b) for a, b in zip(got, want))
        assert wr.fused_calls == 0 and [s for s in seen if s is ga] == [ga] * n_seen
        return got

    cpu_ga = make_ga(lgu, 3, 7)
    cpu_wr = M.install(cpu_ga)
    with torch.no_grad():
        assert all(same_bits(a, b) for a, b in zip(cpu_ga.gaussian_parameters(x), make_ga(lgu, 3, 7).gaussian_parameters(x)))
    assert cpu_wr.fused_calls == 0

    def with_grad(m):
        with torch.autocast("cuda", dtype=torch.float16):
            return m.gaussian_parameters(xc.clone().requires_grad_())
    assert old_path(with_grad, 1)[0].requires_grad

    def bf16(m):
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
            return m.gaussian_parameters(xc)
    old_path(bf16, 2)

    def misaligned(m):
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
            return m.gaussian_parameters(shifted(xc, 4))
    old_path(misaligned, 3)

    monkeypatch.setattr(M, "MIN_FUSED_PIXELS", 43)

    def small(m):
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
            return m.gaussian_parameters(xc)
    old_path(small, 4)
    monkeypatch.setattr(M, "MIN_FUSED_PIXELS", 42)
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        ga.gaussian_parameters(xc)
    assert wr.fused_calls == 1
    wr.fused_calls = 0

    # a coord that is not (h, w): GaussianMask(1, 1) broadcasts its one grid point in the torch composition
    ga, twin = make_ga(lgu, 1, 1).cuda(), make_ga(lgu, 1, 1).cuda()
    wr = M.install(ga)

    def other_coord(m):
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
            return m.gaussian_parameters(xc)
    old_path(other_coord, 1)


@pytest.mark.gpu
def test_corrblock_with_an_installed_ga(lgu, no_threshold, monkeypatch):
    """A CorrBlock built under autocast with an installed GA: mean_n and theta are that call's results, and its pyramid is,
    bit for bit, that of a block whose uninstalled GA returns the fused parameters."""
    _need_gpu(lgu)
    M = lgu.gaussian_mask
    z = gold("glue_corrblock_16x16")
    ofsMap, ofs_residual, GA = build_heads(lgu, 16, 16, "cuda")
    f1, f2 = T(z["fmap1"], "cuda"), T(z["fmap2"], "cuda")
    wr = M.install(GA)
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        blk = lgu.CorrBlock(ofsMap, ofs_residual, GA, f1, f2)
        assert wr.fused_calls == 1
        mean, cov, det = wr(blk.t)
        assert same_bits(blk.mean_n, mean.view(1, 3, 16, 16, 2)) and same_bits(blk.theta, 2 * det.view(1, 3, 16, 16))
        pyr = [lv.clone() for lv in blk.corr_pyramid]
        M.uninstall(GA)
        monkeypatch.setattr(GA, "gaussian_parameters", lambda x: (mean, cov, det), raising=False)
        twin = lgu.CorrBlock(ofsMap, ofs_residual, GA, f1, f2)
        assert same_bits(twin.mean_n, blk.mean_n) and same_bits(twin.theta, blk.theta)
        assert len(pyr) == 4 == len(twin.corr_pyramid)
        for a, b in zip(pyr, twin.corr_pyramid):
            assert same_bits(a, b)
    assert wr.fused_calls == 2
