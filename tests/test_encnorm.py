"""The feature encoder's instance norms folded into its residual-stage convolutions (lgu_slam_amd.encconv.enc_conv3x3_norm,
new_stats, stats_mean_rstd; features.FeatureEncoder(norms=True); csrc/encconv.hip, csrc/encstats.hpp) against the
restatement tests/encnorm_restatement.py.

Numerics contract (include/lgu_corr.h):
- the accumulators summed over their R slots are the Python-integer sums of the stored half output, exactly;
- (mean, rstd) is bit for bit the double lines in numpy; against the float64 two-pass values it is within one fp32 rounding:
  |got - ref| <= (2^-24 + 2^-36) |ref| + 2^-48 mean|x| (the rounding to float, the 1.3e-12 of the double lines, and the
  two-pass reference's own summation error);
- the staged tensor h is bit for bit the restated float32 steps with the (mean, rstd) read back from the device, and out and
  r are bit for bit enc_conv3x3's on h; against the float64 instance norm h stays within §3.13's half bound
  ulp_half(|ref| + E) / 2 + E with L = 2 in E;
- an image's bits do not depend on its batch or on the tile, two runs are identical, and a plane with BAD != 0 makes NaN
  exactly what reads it;
- the whole encoder with norms=True is the chain of restated steps bit for bit and follows §3.13's whole-encoder rule
  against the route it replaces: rms(folded - ref64) <= 1.25 rms(convs=True, ends=True - ref64).
The tile independence is tested as tests/test_encconv.py tests it: a batch whose grid crosses the launcher's threshold takes
the large tile, the same images one at a time the small one.  The GPU tests never read the reference tree.
"""
import ctypes
import functools
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import encconv_restatement as EC  # noqa: E402
from tests import encnorm_restatement as R  # noqa: E402
from tests import features_restatement as FR  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("lgu_encconv3x3_norm_h16", "lgu_encstats_finalize", "lgu_encstats_replicas")
SHAPES = EC.SHAPES
SIZES = EC.EDGE_SIZES
_IDS = ["%d-%d-s%d" % s for s in SHAPES]
_NO_CPU = " must be a HIP device tensor: lgu_slam_amd has no CPU fallback"
EPS = 1e-5
DEV = "cuda"


def same_bits(a, b):
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    iv = {torch.float16: torch.int16, torch.float32: torch.int32, torch.int64: torch.int64}[a.dtype]
    return bool(torch.equal(a.view(iv), b.view(iv)))


def same_words(got, want):
    return all(got[k].shape == want[k].shape and bool(np.all(got[k] == want[k])) for k in R.WORDS)


@functools.lru_cache(maxsize=None)
def operands(cin, size):
    """(x, y) half (N,cin,H,W) on the CPU, cached and never written: per-channel means of alternating sign far from zero
    (a zero padded BEFORE the prologue would become relu((0 - mean) * rstd) > 0 on the planes of negative mean), exact
    zeros and both signs in y."""
    N, H, W = size
    g = torch.Generator().manual_seed(4000 + 131 * cin + H * W)
    mean = (3.0 + torch.arange(cin, dtype=torch.float32) % 5) * (1.0 - 2.0 * (torch.arange(cin) % 2))
    x = (torch.randn((N, cin, H, W), generator=g) * 0.7 + mean.view(1, -1, 1, 1)).half()
    y = (torch.randn((N, cin, H, W), generator=g) * 1.5 - mean.view(1, -1, 1, 1) * 0.5).half()
    y[torch.rand((N, cin, H, W), generator=g) < 0.2] = 0.0
    return x, y


@functools.lru_cache(maxsize=None)
def operand_sums(cin, size):
    x, y = operands(cin, size)
    return R.int_sums(x), R.int_sums(y)


# ---- CPU ------------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_entries(lgu):
    from tests.test_abi import declared_symbols
    syms = declared_symbols()
    lib = ctypes.CDLL(lgu._lib._build.SO_PATH)
    for s in ENTRIES:
        assert s in syms and s in lgu._lib.SIGNATURES and hasattr(lib, s), s
    sig = lgu._lib.SIGNATURES["lgu_encconv3x3_norm_h16"]
    assert sig[0] is lgu._lib.EncConvNormArgs and sig[1] is ctypes.c_void_p
    assert [f[0] for f in sig[0]._fields_] == ["x", "wpack", "bias", "out", "dpack", "dbias", "r", "y", "stats_x", "stats_y", "keep",
                                              "stats_out", "stats_r", "eps", "N", "H", "W", "Cin", "Cout", "stride", "mode", "flags"]
    assert ctypes.sizeof(sig[0]) == 13 * 8 + 9 * 4 + 4
    assert ctypes.sizeof(lgu._lib.EncStatsArgs) == 2 * 8 + 2 * ctypes.sizeof(ctypes.c_long) + 8
    assert ctypes.sizeof(lgu._lib.EncConvArgs) == 8 * 8 + 7 * 4 + 4                    # lgu_encconv_args is unchanged
    lib.lgu_encstats_replicas.restype = ctypes.c_int
    assert lib.lgu_encstats_replicas() == lgu.encconv.stats_replicas() and lgu.encconv.stats_replicas() in (1, 2, 4, 8)
    text = open(os.path.join(ROOT, "include", "lgu_corr.h")).read()
    for name, val in (("NORM", lgu.encconv.NORM), ("RES", lgu.encconv.RES), ("RES_NORM", lgu.encconv.RES_NORM), ("EMIT", lgu.encconv.EMIT)):
        assert "#define LGU_ENCNORM_%s %d" % (name, val) in text
    assert "extractor.py:49-50" in text and "global_atomic_add_x2" in text
    assert os.path.exists(os.path.join(lgu._build.CSRC, "encstats.hpp"))
    assert lgu.enc_conv3x3_norm is lgu.encconv.enc_conv3x3_norm and lgu.encconv.MAX_STATS_PLANE == R.MAX_PLANE
    assert isinstance(lgu.encconv.MIN_NORMS_PIXELS, int) and lgu.encconv.MIN_NORMS_PIXELS >= 0


def test_install_accepts_norms_and_keeps_the_defaults(lgu):
    m = FR.set_weights(FR.RefEncoder(), 3)
    wr = lgu.features.install(m, convs=True, ends=True, norms=True)
    try:
        assert wr.norms is True and wr.convs is True and wr.ends is True and wr.folded_calls == 0 and wr.fused_calls == 0
        assert lgu.features.install(m) is wr
        x = torch.zeros((1, 1, 3, 16, 16))
        with torch.no_grad():
            assert same_bits(m(x), type(m).forward(m, x))              # a CPU call is the module's own forward
        assert wr.folded_calls == 0 and wr.fused_calls == 0
    finally:
        lgu.features.uninstall(m)
    wr = lgu.features.FeatureEncoder(FR.RefEncoder())
    assert wr.norms is False and wr.folded_calls == 0
    assert lgu.features.FeatureEncoder(FR.RefEncoder(), True, True, True).norms is True     # positional, after convs and ends
    assert wr._stat_planes() == 4 * 32 + 5 * 64 + 4 * 128


def test_every_finite_half_is_an_integer_below_2_40_after_scaling():
    """The representation the 64-bit bounds rest on, over all 63488 finite halves: h = +-m 2^(k-24), m < 2048, k <= 29."""
    bits = np.arange(1 << 16, dtype=np.uint16)
    h = bits.view(np.float16)
    h = h[np.isfinite(h)]
    m, k = R.decompose(h)
    assert h.size == 63488 and int(m.max()) == 2047 and int(k.max()) == 29 and int(m.min()) == 0 and int(k.min()) == 0
    assert bool(np.all(np.abs(h.astype(np.float64)) * 2.0 ** 24 == (m << k).astype(np.float64)))
    s = R.int_sums(torch.from_numpy(h.copy()).view(1, -1))
    assert int(s["BAD"]) == 0 and int(s["S1"]) == 0                    # every value with its negative
    want = sum(int(a) ** 2 << (2 * int(b)) for a, b in zip(m, k))
    assert (int(s["HI"]) << 40) + int(s["LO"]) == want
    assert 49152 * ((2047 << 29) ** 2 >> 40) < 1 << 62 and R.MAX_PLANE * ((1 << 40) - 1) < 1 << 62 and R.MAX_PLANE * (2047 << 29) < 1 << 62
    bad = R.int_sums(torch.tensor([[1.0, float("inf"), float("nan"), -2.0]], dtype=torch.float16).view(1, 1, 4))
    assert int(bad["BAD"][0]) == 2 and int(bad["S1"][0]) == -(1 << 24)
    acc = R.acc_from(s, 4)
    assert tuple(acc.shape) == (4, 4) and same_words(R.words_of(acc.view(1, 1, 4, 4)), {k: v.reshape(1, 1) for k, v in s.items()})


HALF_FAMILIES = [f for f, (_, _, dts) in FR.FAMILIES.items() if "h16" in dts]
PLANE_SIZES = (2, 35, 3072, 49152)


@functools.lru_cache(maxsize=None)
def family(name, hw):
    a, b = FR.family_inputs(name, torch.float16, 6, hw)
    return a, b, R.int_sums(a.view(6, 1, hw)), R.int_sums(b.view(6, 1, hw))


@pytest.mark.parametrize("name", HALF_FAMILIES)
def test_restated_mean_rstd_is_within_one_fp32_rounding_of_float64(name):
    worst = 0.0
    for hw in PLANE_SIZES:
        a, _, sa, _ = family(name, hw)
        got = R.mean_rstd_table(sa, hw, EPS).double()
        x = a.double()
        mean = x.mean(-1)
        var = ((x - mean[:, None]) ** 2).mean(-1)
        ref = torch.stack([mean, 1.0 / torch.sqrt(var + float(np.float32(EPS)))], -1)
        slack = 2.0 ** -48 * x.abs().mean(-1)
        allow = (2.0 ** -24 + 2.0 ** -36) * ref.abs() + torch.stack([slack, torch.zeros_like(slack)], -1)
        err = (got - ref).abs()
        worst = max(worst, float((err / allow).max()))
        assert bool((err <= allow).all()), (name, hw, float((err / allow).max()))
    print("%s: (mean, rstd) reaches %.3f of one fp32 rounding" % (name, worst))


@pytest.mark.parametrize("mode", R.MODES)
def test_restated_prologues_stay_within_the_half_bound(mode):
    worst = 0.0
    for name in HALF_FAMILIES:
        for hw in PLANE_SIZES:
            a, b, sa, sb = family(name, hw)
            mra, mrb = R.mean_rstd_table(sa, hw, EPS).view(6, 1, 2), R.mean_rstd_table(sb, hw, EPS).view(6, 1, 2)
            h = R.prologue(mode, a.view(6, 1, 1, hw), mra, b.view(6, 1, 1, hw), mrb).view(6, hw)
            ref, E = R.reference(mode, a, b, EPS)
            ratio = float(((h.double() - ref).abs() / FR.bound(ref, E, torch.float16)).max())
            worst = max(worst, ratio)
            assert ratio <= 1.0, (mode, name, hw, ratio)
    print("%s: the restated prologue reaches %.3f of the half bound" % (mode, worst))


def test_operator_refusals_in_their_order(lgu):
    """enc_conv3x3's refusals first, then pre, keep, eps, the statistics and y, stats_out, then contiguity, dtypes, no-grad
    and device; and stats_mean_rstd's.  None of them touches a device."""
    f = lgu.encconv.enc_conv3x3_norm
    H, I = torch.float16, torch.int64
    Rn = lgu.encconv.stats_replicas()

    def z(*shape, dtype=H):
        return torch.zeros(shape, dtype=dtype)

    def nc(t):
        return torch.zeros(tuple(t.shape) + (2,), dtype=t.dtype)[..., 0]

    x, wp, bh, dp = z(1, 32, 4, 6), z(9, 1, 4, 64, 8), z(64), z(1, 4, 64, 8)
    sx, y, so = z(1, 32, Rn, 4, dtype=I), z(1, 32, 4, 6), z(1, 64, Rn, 4, dtype=I)
    pre_text = 'pre must be None, ("norm", sx), ("res", sx, y) or ("res_norm", sx, y, sy)'
    served = "enc_conv3x3_norm serves (Cin, Cout, stride) in %s, got " % (list(SHAPES),)
    no_grad = "enc_conv3x3_norm has no autograd: its outputs would carry no gradient. Call it under torch.no_grad() or pass detached inputs"
    k = dict(stride=2)
    cases = [
        ((x, (wp, bh)), dict(k, emit=True), "x" + _NO_CPU),
        ((x, (wp, bh)), k, "x" + _NO_CPU),
        ((z(32, 4, 6), (wp, bh)), k, "x must be (N,Cin,H,W), got (32, 4, 6)"),
        ((x, (wp, bh)), dict(stride=3), "stride must be 1 or 2, got 3"),
        ((x, wp), k, "pack must be (wpack, bias_h) of pack_enc3"),
        ((x, (wp, z(64, 1))), k, "bias_h must be (Cout,), got (64, 1)"),
        ((x, (wp, bh)), dict(stride=1), served + "(32, 64, 1)"),
        ((x, (z(5), bh)), k, "wpack must hold 18432 halves (pack_enc3, 32 -> 64), got (5,)"),
        ((x.float(), (wp, bh)), k, "expected scalar type Half but found Float (x)"),
        ((x, (wp, bh)), dict(k, down=dp), "down must be (dpack, dbias_h) of pack_enc1"),
        ((x, (wp, bh)), dict(k, down=(dp, z(32))), "dbias_h must be (64,), got (32,)"),
        ((x, (wp, bh)), dict(k, pre=("norm",)), pre_text),
        ((x, (wp, bh)), dict(k, pre=("res", sx)), pre_text),
        ((x, (wp, bh)), dict(k, pre=("other", sx)), pre_text),
        ((x, (wp, bh)), dict(k, pre=sx), pre_text),
        ((x, (wp, bh)), dict(k, keep=True), "keep=True needs a prologue (pre): without one the staged tensor is x"),
        ((x, (wp, bh)), dict(k, pre=("norm", sx), eps=-1.0), "eps must be >= 0, got -1.0"),
        ((x, (wp, bh)), dict(k, pre=("norm", sx[:, :16])), "sx must be (1, 32, %d, 4), got (1, 16, %d, 4)" % (Rn, Rn)),
        ((x, (wp, bh)), dict(k, pre=("norm", sx.int())), "expected scalar type Long but found Int (sx)"),
        ((x, (wp, bh)), dict(k, pre=("res", sx, y[:, :, :2])), "y must be (1, 32, 4, 6), got (1, 32, 2, 6)"),
        ((x, (wp, bh)), dict(k, pre=("res", sx, y.float())), "expected scalar type Half but found Float (y)"),
        ((x, (wp, bh)), dict(k, pre=("res_norm", sx, y, sx[0])), "sy must be (1, 32, %d, 4), got (32, %d, 4)" % (Rn, Rn)),
        ((x, (wp, bh)), dict(k, stats_out=so), "stats_out needs emit=True"),
        ((x, (wp, bh)), dict(k, emit=True, stats_out=(so, so)), "stats_out must be one accumulator tensor (N,Cout,R,4) without down"),
        ((x, (wp, bh)), dict(k, emit=True, down=(dp, bh), stats_out=so), "stats_out must be (out_stats, r_stats) with down"),
        ((x, (wp, bh)), dict(k, emit=True, stats_out=so[:, :32]), "out_stats must be (1, 64, %d, 4), got (1, 32, %d, 4)" % (Rn, Rn)),
        ((x, (wp, bh)), dict(k, emit=True, down=(dp, bh), stats_out=(so, so.float())), "expected scalar type Long but found Float (r_stats)"),
        ((nc(x), (wp, bh)), dict(k, emit=True), "x must be contiguous"),
        ((x, (wp, bh)), dict(k, pre=("norm", nc(sx))), "sx must be contiguous"),
        ((x, (wp, bh)), dict(k, pre=("res", sx, nc(y))), "y must be contiguous"),
        ((x, (wp, bh)), dict(k, emit=True, stats_out=nc(so)), "out_stats must be contiguous"),
        ((x, (wp.float(), bh)), dict(k, emit=True), "expected scalar type Half but found Float (wpack)"),
        ((x.clone().requires_grad_(), (wp, bh)), dict(k, emit=True), no_grad),
        # two defects: the earlier check reports
        ((x.float(), (wp, bh)), dict(k, pre=("norm",)), "expected scalar type Half but found Float (x)"),
        ((x, (wp, bh)), dict(k, pre=("norm",), keep=True), pre_text),
        ((x, (wp, bh)), dict(k, keep=True, eps=-1.0), "keep=True needs a prologue (pre): without one the staged tensor is x"),
        ((nc(x), (wp, bh)), dict(k, pre=("norm", sx.int())), "expected scalar type Long but found Int (sx)"),
        ((nc(x), (wp, bh)), dict(k, stats_out=so), "stats_out needs emit=True"),
        ((x, (nc(wp), bh)), dict(k, pre=("norm", nc(sx))), "wpack must be contiguous"),
    ]
    for args, kw, message in cases:
        with pytest.raises((RuntimeError, ValueError)) as info:
            f(*args, **kw)
        assert str(info.value) == message
        assert type(info.value) is (lgu._lib.UnsupportedShape if message.startswith(served) else ValueError if message.startswith("eps") else RuntimeError)
    big = torch.zeros((1, 32, 2049, 2048), dtype=H, device="meta")          # a plane of 2^22 + 2048 pixels: shapes only
    with pytest.raises(lgu._lib.UnsupportedShape, match=r"planes of at most 2\^22 pixels, got 2049 x 2048"):
        f(big, (z(9, 1, 2, 64, 8), z(32)), emit=True)
    g = lgu.encconv.stats_mean_rstd
    acc = z(2, 3, Rn, 4, dtype=I)
    for args, message, kind in [((z(2, 3, Rn + 1, 4, dtype=I), 5), "acc must be (N,C,%d,4), got (2, 3, %d, 4)" % (Rn, Rn + 1), RuntimeError),
                                ((acc.int(), 5), "expected scalar type Long but found Int (acc)", RuntimeError),
                                ((acc, 0), "cnt must be >= 1, got 0", RuntimeError),
                                ((acc, (1 << 22) + 1), "stats_mean_rstd serves planes of at most 2^22 pixels, got 4194305", lgu._lib.UnsupportedShape),
                                ((acc, 5, -1e-5), "eps must be >= 0, got -1e-05", ValueError),
                                ((nc(acc), 5), "acc must be contiguous", RuntimeError),
                                ((acc, 5), "acc" + _NO_CPU, RuntimeError)]:
        with pytest.raises((RuntimeError, ValueError)) as info:
            g(*args)
        assert str(info.value) == message and type(info.value) is kind


# ---- GPU ------------------------------------------------------------------------------------------------------------
def _need_gpu(lgu):
    assert torch.cuda.is_available(), "these tests need the MI355X"
    assert os.path.exists(lgu._lib.so_path()), "liblgu_corr.so missing — run __graft_entry__.build()"


def _packed(lgu, c3, c1=None):
    p3 = lgu.encconv.pack_enc3(c3.weight.detach().cuda(), c3.bias.detach().cuda())
    return p3, (lgu.encconv.pack_enc1(c1.weight.detach().cuda(), c1.bias.detach().cuda()) if c1 is not None else None)


def _plain(lgu, x, p3, st, p1):
    got = lgu.encconv.enc_conv3x3(x, p3, stride=st, down=p1)
    return got if p1 is not None else (got, None)


def _pre(mode, sx, y, sy):
    return {"norm": ("norm", sx), "res": ("res", sx, y), "res_norm": ("res_norm", sx, y, sy)}[mode]


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES, ids=_IDS)
def test_emit_changes_no_bit_and_its_sums_are_exact(lgu, shape):
    _need_gpu(lgu)
    cin, cout, st = shape
    c3, c1 = EC.make_layer(81, *shape)
    p3, p1 = _packed(lgu, c3, c1)
    E = lgu.encconv
    for size in SIZES:
        x = EC.make_input(2100 + size[1] * size[2], *size, C=cin).half().cuda()
        want, want_r = _plain(lgu, x, p3, st, p1)
        out, r, kept, so, sr = E.enc_conv3x3_norm(x, p3, stride=st, down=p1, emit=True)
        assert kept is None and same_bits(out, want) and (sr is None) == (r is None) == (st == 1)
        assert so.dtype == torch.int64 and tuple(so.shape) == (size[0], cout, E.stats_replicas(), 4)
        assert same_words(R.words_of(so), R.int_sums(want)), size
        if st == 2:
            assert same_bits(r, want_r) and same_words(R.words_of(sr), R.int_sums(want_r)), size
        # a second launch adds to the caller's accumulators: twice the sums, and the launch without the branch the same
        out2, _, _, so2, _ = E.enc_conv3x3_norm(x, p3, stride=st, emit=True, stats_out=so)
        assert so2 is so and same_bits(out2, want)
        assert same_words(R.words_of(so), {k: 2 * v for k, v in R.int_sums(want).items()}), size
    # an infinite bias makes one output plane infinite: only that plane's BAD counts, and its other words stay zero
    size = (2, 9, 33)
    x = EC.make_input(7, *size, C=cin).half().cuda()
    bias = p3[1].clone()
    bias[cout - 3] = float("inf")
    out, _, _, so, _ = E.enc_conv3x3_norm(x, (p3[0], bias), stride=st, emit=True)
    words, want = R.words_of(so), R.int_sums(out)
    Ho, Wo = EC.out_size(size[1], size[2], st)
    assert same_words(words, want) and int(words["BAD"].sum()) == 2 * Ho * Wo
    assert all(int(words["BAD"][n, cout - 3]) == Ho * Wo and int(words["HI"][n, cout - 3]) == 0 for n in range(2))
    assert int((words["HI"] > 0).sum()) == 2 * (cout - 1)


@pytest.mark.gpu
def test_finalise_is_the_numpy_lines_bit_for_bit(lgu):
    """Crafted planes: the half families of §3.13 at 35 and 3072 pixels, a constant plane, a plane of one pixel, planes
    with an infinity or a NaN; sums spread over the slots; and every eps."""
    _need_gpu(lgu)
    E = lgu.encconv
    Rn = E.stats_replicas()
    for hw in (1, 2, 35, 3072):
        planes = [FR.family_inputs(f, torch.float16, 6, hw)[0] for f in HALF_FAMILIES]
        planes.append(torch.full((6, hw), -7.25, dtype=torch.float16))
        t = torch.stack(planes, 1).contiguous()                              # (6, F + 1, hw)
        t[5, 0, 0] = float("inf")
        t[4, 1, hw - 1] = float("nan")
        sums = R.int_sums(t.view(6, -1, 1, hw))
        acc = R.acc_from(sums, Rn, DEV)
        for eps in (EPS, 0.0, 1e-3):
            got = E.stats_mean_rstd(acc, hw, eps)
            want = R.mean_rstd_table(sums, hw, eps)
            assert got.dtype == torch.float32 and tuple(got.shape) == (6, len(planes), 2)
            assert same_bits(got, want), (hw, eps)
            assert bool(torch.isnan(got[5, 0]).all()) and bool(torch.isnan(got[4, 1]).all()) and int(torch.isnan(got).sum()) == 4
        const = E.stats_mean_rstd(acc, hw, EPS)[0, -1].cpu()
        assert float(const[0]) == -7.25 and float(const[1]) == float(np.float32(1.0 / np.sqrt(np.float64(np.float32(EPS)))))
    assert tuple(E.stats_mean_rstd(acc[:0], 5).shape) == (0, len(planes), 2)
    assert same_bits(E.new_stats(2, 3, DEV), torch.zeros((2, 3, Rn, 4), dtype=torch.int64))


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES, ids=_IDS)
def test_emitted_statistics_finalise_to_the_numpy_lines(lgu, shape):
    _need_gpu(lgu)
    cin, cout, st = shape
    c3, c1 = EC.make_layer(82, *shape)
    p3, p1 = _packed(lgu, c3, c1)
    for size in SIZES:
        x = operands(cin, size)[0].cuda()
        out, r, _, so, sr = lgu.encconv.enc_conv3x3_norm(x, p3, stride=st, down=p1, emit=True)
        cnt = out.shape[2] * out.shape[3]
        assert same_bits(lgu.encconv.stats_mean_rstd(so, cnt, EPS), R.mean_rstd_table(R.int_sums(out), cnt, EPS)), size
        if st == 2:
            assert same_bits(lgu.encconv.stats_mean_rstd(sr, cnt, EPS), R.mean_rstd_table(R.int_sums(r), cnt, EPS)), size


@pytest.mark.gpu
@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("shape", SHAPES, ids=_IDS)
def test_prologue_is_the_restated_steps_and_the_convolution_sees_it(lgu, shape, mode):
    _need_gpu(lgu)
    cin, cout, st = shape
    c3, c1 = EC.make_layer(83, *shape)
    p3, p1 = _packed(lgu, c3, c1)
    E = lgu.encconv
    Rn = E.stats_replicas()
    for size in SIZES:
        x, y = operands(cin, size)
        cnt = size[1] * size[2]
        sx, sy = (R.acc_from(s, Rn, DEV) for s in operand_sums(cin, size))
        mrx, mry = E.stats_mean_rstd(sx, cnt, EPS).cpu(), E.stats_mean_rstd(sy, cnt, EPS).cpu()
        h = R.prologue(mode, x, mrx, y, mry)
        assert cnt == 1 or (bool((h[:, 1::2] > 0).any()) and bool((h == 0).any()))
        pre = _pre(mode, sx, y.cuda(), sy)
        out, r, kept, so, sr = E.enc_conv3x3_norm(x.cuda(), p3, stride=st, down=p1, pre=pre, keep=True, eps=EPS)
        assert so is None and sr is None and same_bits(kept, h), (size, float((kept.cpu().float() - h.float()).abs().max()))
        want, want_r = _plain(lgu, h.cuda(), p3, st, p1)
        assert same_bits(out, want), size
        # zeros padded before the prologue instead of after it would differ
        hp = R.prologue(mode, torch.nn.functional.pad(x, (1, 1, 1, 1)), mrx, torch.nn.functional.pad(y, (1, 1, 1, 1)), mry)
        assert bool((hp[:, :, 0, :] != 0).any())
        if st == 2:
            assert same_bits(r, want_r), size
        out2, r2, kept2, so2, _ = E.enc_conv3x3_norm(x.cuda(), p3, stride=st, down=p1, pre=pre, emit=True, eps=EPS)
        assert kept2 is None and same_bits(out2, want) and (st == 1 or same_bits(r2, want_r))
        assert same_words(R.words_of(so2), R.int_sums(want)), size
        out3 = E.enc_conv3x3_norm(x.cuda(), p3, stride=st, pre=pre, keep=True, emit=True, eps=1e-3)
        h3 = R.prologue(mode, x, E.stats_mean_rstd(sx, cnt, 1e-3).cpu(), y, E.stats_mean_rstd(sy, cnt, 1e-3).cpu())
        assert same_bits(out3[2], h3) and out3[1] is None and (cnt == 1 or not same_bits(h3, h))


# (shape, (H, W) of the input, workgroups of the large tile per image), as tests/test_encconv.py LARGE_GRID
LARGE_GRID = [((32, 64, 2), (34, 130), 15), ((64, 64, 1), (17, 65), 15), ((64, 128, 2), (34, 130), 54), ((128, 128, 1), (17, 65), 30)]
_BATCHES = [((32, 32, 1), (17, 130), 0)] + LARGE_GRID


@pytest.mark.gpu
@pytest.mark.parametrize("shape,hw,per_image", _BATCHES, ids=_IDS)
def test_an_image_depends_neither_on_its_batch_nor_on_the_tile(lgu, shape, hw, per_image):
    """A batch whose grid crosses the launcher's threshold (two workgroups of the large tile per CU; (32,32,1) has one
    tile) against the same images one at a time: out, r, kept and the summed accumulators bit for bit, every mode; two
    runs identical; a plane whose BAD is not zero makes NaN exactly its own plane of h and every output of its image."""
    _need_gpu(lgu)
    cin, cout, st = shape
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    N = (-(-2 * cus // per_image) + 1) if per_image else 3
    c3, c1 = EC.make_layer(84, *shape)
    p3, p1 = _packed(lgu, c3, c1)
    E = lgu.encconv
    g = torch.Generator().manual_seed(85)
    x = (torch.randn((N, cin, hw[0], hw[1]), generator=g) * 0.7 - 2.0).half().cuda()
    y = (torch.randn((N, cin, hw[0], hw[1]), generator=g) * 1.5).half().cuda()
    # the accumulators of x and y from an emitting launch whose output is its input: the centre tap is the identity matrix
    eye = torch.zeros((cin, cin, 3, 3), device=DEV)
    eye[torch.arange(cin), torch.arange(cin), 1, 1] = 1.0
    ident = E.pack_enc3(eye, torch.zeros(cin, device=DEV))
    (xi, _, _, sx, _), (yi, _, _, sy, _) = E.enc_conv3x3_norm(x, ident, emit=True), E.enc_conv3x3_norm(y, ident, emit=True)
    assert same_bits(xi, x) and same_bits(yi, y)
    assert same_words(R.words_of(sx[:1]), R.int_sums(x[:1])) and same_words(R.words_of(sy[-1:]), R.int_sums(y[-1:]))
    picks = (0, N // 2, N - 1)
    for mode in R.MODES:
        big = E.enc_conv3x3_norm(x, p3, stride=st, down=p1, pre=_pre(mode, sx, y, sy), keep=True, emit=True, eps=EPS)
        again = E.enc_conv3x3_norm(x, p3, stride=st, down=p1, pre=_pre(mode, sx, y, sy), keep=True, emit=True, eps=EPS)
        for a, b in zip(big, again):
            assert (a is None and b is None) or same_bits(a, b), mode
        for i in picks:
            s = slice(i, i + 1)
            one = E.enc_conv3x3_norm(x[s].contiguous(), p3, stride=st, down=p1,
                                     pre=_pre(mode, sx[s].contiguous(), y[s].contiguous(), sy[s].contiguous()), keep=True, emit=True, eps=EPS)
            for k in (0, 1, 2):
                assert (big[k] is None and one[k] is None) or same_bits(big[k][s], one[k]), (mode, i, k)
            for k in (3, 4):
                assert (big[k] is None and one[k] is None) or same_bits(big[k][s].sum(2), one[k].sum(2)), (mode, i, k)
    # BAD != 0 in one plane of image 1
    bad = sx.clone()
    bad[1, 5, E.stats_replicas() - 1, 3] = 2
    clean = E.enc_conv3x3_norm(x, p3, stride=st, down=p1, pre=("res", sx, y), keep=True, eps=EPS)
    out, r, kept, _, _ = E.enc_conv3x3_norm(x, p3, stride=st, down=p1, pre=("res", bad, y), keep=True, eps=EPS)
    nan_kept = torch.zeros_like(kept, dtype=torch.bool)
    nan_kept[1, 5] = True
    assert bool(torch.equal(torch.isnan(kept), nan_kept))
    keep_rows = [i for i in range(N) if i != 1]
    for got, ref in ((out, clean[0]), (r, clean[1]), (kept, clean[2])):
        if got is not None:
            assert same_bits(got[keep_rows], ref[keep_rows])
    assert bool(torch.isnan(out[1]).all()) and (r is None or bool(torch.isnan(r[1]).all())) and not bool(torch.isnan(clean[0]).any())


def _c_call(lgu, a, shape, size, mode, flags, eps=EPS):
    cin, cout, st = shape

    def p(k):
        return a[k].data_ptr() if a.get(k) is not None else None
    args = lgu._lib.EncConvNormArgs(p("x"), p("wpack"), p("bias"), p("out"), p("dpack"), p("dbias"), p("r"), p("y"), p("stats_x"), p("stats_y"),
                                    p("keep"), p("stats_out"), p("stats_r"), eps, size[0], size[1], size[2], cin, cout, st, mode, flags)
    rc = lgu._lib.load().lgu_encconv3x3_norm_h16(args, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc


@pytest.mark.gpu
@pytest.mark.parametrize("size", [(2, 9, 33), (2, 10, 34), (1, 16, 32)])
@pytest.mark.parametrize("shape", SHAPES, ids=_IDS)
def test_guard_bands_and_alignment(lgu, shape, size):
    """RES_NORM with keep and emit, every pointer operand of lgu_encconv3x3_norm_h16: x, y, the biases, out, r and keep at
    element alignment, the accumulators at 8 bytes, each inside a sentinel-filled buffer, give the aligned call's bits and
    leave their guard bands alone; a pack off 16 bytes is refused with nothing written; the accumulators take exactly the
    sums.  Then the bad calls, and lgu_encstats_finalize's operands."""
    from tests.alignment_cases import guards_intact, shifted
    _need_gpu(lgu)
    cin, cout, st = shape
    E = lgu.encconv
    Rn = E.stats_replicas()
    c3, c1 = EC.make_layer(86, *shape)
    (wpack, bias_h), p1 = _packed(lgu, c3, c1)
    osz = (size[0], cout) + EC.out_size(size[1], size[2], st)
    x, y = (t.cuda() for t in operands(cin, size))
    sx, sy = (R.acc_from(s, Rn, DEV) for s in operand_sums(cin, size))
    base = {"x": x, "y": y, "wpack": wpack, "bias": bias_h, "stats_x": sx, "stats_y": sy,
            "out": torch.empty(osz, dtype=torch.float16, device=DEV), "keep": torch.empty_like(x),
            "stats_out": torch.zeros((size[0], cout, Rn, 4), dtype=torch.int64, device=DEV)}
    if st == 2:
        base.update(dpack=p1[0], dbias=p1[1], r=torch.empty(osz, dtype=torch.float16, device=DEV), stats_r=torch.zeros_like(base["stats_out"]))
    want = E.enc_conv3x3_norm(x, (wpack, bias_h), stride=st, down=p1, pre=("res_norm", sx, y, sy), keep=True, emit=True, eps=EPS)
    want = dict(zip(("out", "r", "keep", "stats_out", "stats_r"), want))
    written = [k for k in ("out", "r", "keep") if k in base]
    accs = [k for k in ("stats_out", "stats_r") if k in base]
    packs = [k for k in ("wpack", "dpack") if k in base]
    variants = [([k], s) for k in base for s in ((8,) if base[k].dtype == torch.int64 else (2, 4, 8))]
    variants += [([k for k in base if k not in packs and base[k].dtype == torch.float16], 2)]
    for keys, shift in variants:
        args = dict(base)
        for k in keys:
            args[k] = shifted(base[k], shift)
        for k in written + accs:
            if k not in keys:
                args[k] = shifted(base[k], 0)
        for k in written:
            args[k].fill_(float("nan"))
        for k in accs:
            args[k].zero_()
        before = {k: args[k].clone() for k in args}
        rc = _c_call(lgu, args, shape, size, E.RES_NORM, E.EMIT)
        if set(keys) & set(packs):
            assert rc == lgu._lib.LGU_E_UNSUPPORTED, (keys, shift, rc)
            assert all(same_bits(args[k], before[k]) for k in written + accs), "refused, but an output changed"
        else:
            assert rc == 0, (keys, shift, rc)
            for k in written:
                assert same_bits(args[k], want[k]), "%s shifted by %d: %s differs from the aligned call" % (keys, shift, k)
            for k in accs:
                assert same_bits(args[k].sum(2), want[k].sum(2)), (keys, shift, k)
        for k in base:
            if k not in written + accs:
                assert same_bits(args[k], before[k]), "read-only operand %s changed" % k
        for k in set(keys) | set(written) | set(accs):
            assert guards_intact(args[k]), "%s, %d: a guard band of %s was written" % (keys, shift, k)
    # bad calls launch nothing
    args = dict(base)
    for k in written + accs:
        args[k] = shifted(base[k], 0)
    before = {k: args[k].clone() for k in written + accs}
    BAD, UNS = lgu._lib.LGU_E_BADARG, lgu._lib.LGU_E_UNSUPPORTED
    call = functools.partial(_c_call, lgu)
    assert call(args, shape, (0,) + size[1:], E.RES_NORM, E.EMIT) == 0
    assert call(args, shape, (-1,) + size[1:], E.RES_NORM, E.EMIT) == BAD and call(args, shape, (size[0], 0, size[2]), E.RES_NORM, E.EMIT) == BAD
    assert call(args, shape, size, 4, E.EMIT) == BAD and call(args, shape, size, -1, E.EMIT) == BAD and call(args, shape, size, E.RES_NORM, 2) == BAD
    assert call(args, shape, size, E.RES_NORM, E.EMIT, eps=-1.0) == BAD and call(args, shape, size, E.RES_NORM, E.EMIT, eps=float("nan")) == BAD
    assert call(args, shape, size, E.RES, E.EMIT) == BAD and call(args, shape, size, E.NORM, E.EMIT) == BAD   # operands the mode does not read
    assert call(args, shape, size, E.RES_NORM, 0) == BAD                                                  # accumulators without EMIT
    assert call(dict(args, stats_out=None), shape, size, E.RES_NORM, E.EMIT) == BAD
    assert call(dict(args, stats_y=None), shape, size, E.RES_NORM, E.EMIT) == BAD
    assert call(dict(args, y=None, stats_y=None, stats_x=None), shape, size, 0, E.EMIT) == BAD            # keep without a prologue
    assert call(dict(args, y=None, stats_y=None, stats_x=None, keep=None, stats_out=None, stats_r=None), shape, size, 0, 0) == BAD
    assert call(dict(args, out=None), shape, size, E.RES_NORM, E.EMIT) == BAD
    assert call(args, (cin, 96, st), size, E.RES_NORM, E.EMIT) == UNS and call(args, (48, cout, st), size, E.RES_NORM, E.EMIT) == UNS
    assert call(args, shape, (1, 2049, 2048), E.RES_NORM, E.EMIT) == UNS                                 # a plane above 2^22 pixels
    if st == 2:
        assert call(dict(args, stats_r=None), shape, size, E.RES_NORM, E.EMIT) == BAD
        assert call(dict(args, dbias=None), shape, size, E.RES_NORM, E.EMIT) == BAD
    assert all(same_bits(args[k], before[k]) and guards_intact(args[k]) for k in written + accs)
    # the finalise entry: acc at 8 bytes, the table at 4, 8 and 12
    lib, stream = lgu._lib.load(), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    cnt = size[1] * size[2]
    ref = E.stats_mean_rstd(sx, cnt, EPS)
    for a_shift, o_shift in ((8, 0), (0, 4), (0, 8), (8, 12)):
        acc, tab = shifted(sx, a_shift), shifted(torch.full_like(ref, float("nan")), o_shift)
        rc = lib.lgu_encstats_finalize(lgu._lib.EncStatsArgs(acc.data_ptr(), tab.data_ptr(), sx.shape[0] * cin, cnt, EPS), stream)
        torch.cuda.synchronize()
        assert rc == 0 and same_bits(tab, ref) and guards_intact(tab) and guards_intact(acc) and same_bits(acc, sx)
    tab = shifted(torch.full_like(ref, float("nan")), 0)
    keep = tab.clone()
    A = lgu._lib.EncStatsArgs
    assert lib.lgu_encstats_finalize(A(sx.data_ptr(), tab.data_ptr(), 0, cnt, EPS), stream) == 0
    assert lib.lgu_encstats_finalize(A(sx.data_ptr(), tab.data_ptr(), -1, cnt, EPS), stream) == BAD
    assert lib.lgu_encstats_finalize(A(sx.data_ptr(), tab.data_ptr(), 2, 0, EPS), stream) == BAD
    assert lib.lgu_encstats_finalize(A(sx.data_ptr(), tab.data_ptr(), 2, cnt, -1.0), stream) == BAD
    assert lib.lgu_encstats_finalize(A(None, tab.data_ptr(), 2, cnt, EPS), stream) == BAD
    assert lib.lgu_encstats_finalize(A(sx.data_ptr() + 4, tab.data_ptr(), 2, cnt, EPS), stream) == BAD
    assert lib.lgu_encstats_finalize(A(sx.data_ptr(), tab.data_ptr() + 2, 2, cnt, EPS), stream) == BAD
    assert lib.lgu_encstats_finalize(A(sx.data_ptr(), tab.data_ptr(), 2, (1 << 22) + 1, EPS), stream) == UNS
    torch.cuda.synchronize()
    assert same_bits(tab, keep) and guards_intact(tab)


# ---- the whole encoder ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def encoder_case(name):
    """(device module, device images, float64 CPU forward of the same module); cached and never written."""
    m, images = FR.make_case(name)
    m64 = FR.RefEncoder().double()
    m64.load_state_dict(m.state_dict())
    with torch.no_grad():
        ref = m64.eval()(images.double())
    return m.to(DEV), images.to(DEV), ref


def rms(x, ref):
    return float(((x.double().cpu() - ref) ** 2).mean().sqrt())


def restated_chain(lgu, m, images):
    """The folded forward, step by step: the stem, norm1's call, and for every convolution the statistics of its stored
    input planes as Python integers, (mean, rstd) by the numpy lines, the prologue in float32 torch steps on the CPU and
    enc_conv3x3 on the staged tensor; the last block's norm call; the output layer."""
    E, F = lgu.encconv, lgu.features
    b, n, c, hh, ww = images.shape
    y = E.enc_stem7x7(images.view(b * n, c, hh, ww), E.pack_stem(m.conv1.weight, m.conv1.bias))
    y = F.instance_norm_relu(y, eps=m.norm1.eps)
    blocks = [blk for layer in (m.layer1, m.layer2, m.layer3) for blk in layer]

    def table(t, eps):
        return R.mean_rstd_table(R.int_sums(t), t.shape[2] * t.shape[3], eps)
    h, t2, r = y, None, None          # the block's input; the previous block's second output and branch
    for i, blk in enumerate(blocks):
        if i > 0:
            prev = blocks[i - 1]
            if prev.downsample is None:
                h = R.prologue("res", t2.cpu(), table(t2, prev.norm2.eps), h.cpu()).cuda()
            else:
                h = R.prologue("res_norm", t2.cpu(), table(t2, prev.norm2.eps), r.cpu(), table(r, prev.norm2.eps)).cuda()
        p1 = E.pack_enc3(blk.conv1.weight, blk.conv1.bias)
        if blk.downsample is None:
            t1 = E.enc_conv3x3(h, p1)
        else:
            t1, r = E.enc_conv3x3(h, p1, stride=2, down=E.pack_enc1(blk.downsample[0].weight, blk.downsample[0].bias))
        a = R.prologue("norm", t1.cpu(), table(t1, blk.norm1.eps)).cuda()
        t2 = E.enc_conv3x3(a, E.pack_enc3(blk.conv2.weight, blk.conv2.bias))
    y = F.instance_norm_relu(t2, h, eps=blocks[-1].norm2.eps)
    y = E.enc_out1x1(y, E.pack_out1(m.conv2.weight, m.conv2.bias))
    return y.view(b, n, *y.shape[1:])


@pytest.fixture
def count_calls(lgu, monkeypatch):
    """Every library launch of the encoder's modules and every accumulator fill, in order."""
    calls = []
    for mod in (lgu.encconv, lgu.features):
        own = mod.launch
        monkeypatch.setattr(mod, "launch", (lambda own: lambda symbol, *a: (calls.append(symbol), own(symbol, *a))[1])(own))
    own_new = lgu.encconv.new_stats
    monkeypatch.setattr(lgu.encconv, "new_stats", lambda *a: (calls.append("fill"), own_new(*a))[1])
    return calls


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(FR.CASES))
def test_folded_encoder_is_the_restated_chain_and_as_close_to_float64_as_the_parent_route(lgu, monkeypatch, count_calls, name):
    _need_gpu(lgu)
    monkeypatch.setattr(lgu.encconv, "MIN_NORMS_PIXELS", 0)          # the routing follows a measurement; this is about the route
    monkeypatch.setattr(lgu.encconv, "MIN_FUSED_PIXELS", {s: 0 for s in lgu.encconv.SHAPES})
    monkeypatch.setattr(lgu.encconv, "MIN_STEM_PIXELS", 0)
    monkeypatch.setattr(lgu.encconv, "MIN_OUT_PIXELS", {128: 0, 256: 0})
    m, images, ref = encoder_case(name)
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        wr = lgu.features.install(m, convs=True, ends=True)
        try:
            parent = m(images)
            assert wr.fused_calls == 1 and wr.folded_calls == 0 and len(count_calls) == 27
        finally:
            lgu.features.uninstall(m)
        del count_calls[:]
        wr = lgu.features.install(m, convs=True, ends=True, norms=True)
        try:
            got = m(images)
            assert wr.fused_calls == 1 and wr.folded_calls == 17 and len(count_calls) == 17
            seq = list(count_calls)
            again = m(images)
            assert wr.folded_calls == 34 and same_bits(got, again)
        finally:
            lgu.features.uninstall(m)
        want = restated_chain(lgu, m, images)
    assert seq == ["lgu_encstem7x7_h16", "lgu_instnorm_relu_h16", "fill"] + ["lgu_encconv3x3_norm_h16"] * 12 + [
        "lgu_instnorm_relu_h16", "lgu_encout1x1_c128_h16"]
    assert got.dtype == torch.float16 and got.shape == parent.shape == ref.shape and same_bits(got, want)
    r_got, r_parent = rms(got, ref), rms(parent, ref)
    print("%s: rms folded %.4g, convs=True ends=True %.4g, ratio %.3f" % (name, r_got, r_parent, r_got / r_parent))
    assert r_got <= 1.25 * r_parent


@pytest.mark.gpu
def test_other_inputs_and_norms_false_give_todays_results(lgu, monkeypatch, count_calls):
    """fp32, CPU and grad inputs, a call below MIN_NORMS_PIXELS and norms=False with norms=True installed or not: the
    same route as today, the same bits, and no folded launch."""
    _need_gpu(lgu)
    m, images, _ = encoder_case("features_fnet_1x64x48")
    twin = FR.make_case("features_fnet_1x64x48")[0].to(DEV)
    wr = lgu.features.install(m, convs=True, ends=True, norms=True)
    wt = lgu.features.install(twin, convs=True, ends=True)
    try:
        with torch.no_grad():
            assert same_bits(m(images), twin(images))                                  # fp32: the per-site route, library convolutions
            with torch.autocast("cuda", dtype=torch.float16):
                monkeypatch.setattr(lgu.encconv, "MIN_NORMS_PIXELS", 64 * 48 + 1)
                del count_calls[:]
                a, b = m(images), twin(images)                                         # below the threshold: today's 27 launches
                assert same_bits(a, b) and count_calls[:27] == count_calls[27:] and "lgu_encconv3x3_norm_h16" not in count_calls
                monkeypatch.setattr(lgu.encconv, "MIN_NORMS_PIXELS", 0)
                wr.norms = False
                assert same_bits(m(images), b)
                wr.norms, wr.convs = True, False                                       # norms needs convs
                del count_calls[:]
                m(images)
                assert "lgu_encconv3x3_norm_h16" not in count_calls and "fill" not in count_calls
                wr.convs = True
            cpu = FR.make_case("features_fnet_1x64x48")[0]
            wc = lgu.features.install(cpu, convs=True, ends=True, norms=True)
            assert same_bits(cpu(images.cpu()), type(cpu).forward(cpu, images.cpu())) and wc.fused_calls == 0
        assert wr.folded_calls == 0 and wt.folded_calls == 0
        x = images.clone().requires_grad_()
        with torch.autocast("cuda", dtype=torch.float16):
            before = wr.fused_calls
            assert m(x).requires_grad and wr.fused_calls == before and wr.folded_calls == 0
    finally:
        lgu.features.uninstall(m)
        lgu.features.uninstall(twin)
