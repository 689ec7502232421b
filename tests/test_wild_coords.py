"""Every lookup kernel at wild coordinates: the ladder of tests/wild_coords.py (map edge, int16 rails and aliases, 24-bit
aliases, int32 rails, non-finite) through every kernel family, against tests/sampler_restatement.py — the reference's
samplers with the device's float -> int conversion.

The unmarked part runs anywhere: the restatement against the C oracle where C defines the conversion, the properties the
inputs exist for (an alias row is all zero, its in-map twin is not, NaN appears exactly where the reference puts it) and
the coverage of the ladder.  The `gpu` part runs the same placement through each family and asserts equal NaN positions,
finite values within the suite's bound for that kernel, the offsets' in-place state, bitwise agreement between layouts
and scheduling modes, an untouched ordinary edge, and intact guard bands around every written tensor.
"""
import functools
import os

import numpy as np
import pytest

from tests import sampler_restatement as S
from tests import wild_coords as W

torch = pytest.importorskip("torch")

H1, W1 = W.H1, W.W1


# ---- shared inputs and references (computed once, never modified: every user copies what it hands to an operator) -----------
@functools.lru_cache(maxsize=None)
def vcase(R):
    return W.volume_case(R)


@functools.lru_cache(maxsize=None)
def mcase(C, R=3):
    return W.map_case(C, R)


def _copies(offs):
    return [o.copy() if o is not None else None for o in offs]


@functools.lru_cache(maxsize=None)
def vref(R, L, dense, probe, plain=False):
    """Restatement of the fused volume lookup: (out, offsets after the call)."""
    case = vcase(R)
    offs = _copies(case["offsets"][:L] if dense else case["offsets"][:2] + [None] * (L - 2))
    out = S.defcorr_pyramid(case["volumes"][:L], case["plain" if plain else "coords"], offs, R, probe)
    return out, offs


@functools.lru_cache(maxsize=None)
def mref(C, R, L=4, noff=2, half=False):
    """Restatement of the fused low-memory lookup on the (half-rounded) maps: (out, offsets after the call)."""
    case = mcase(C, R)
    rnd = (lambda a: a.astype(np.float16).astype(np.float32)) if half else (lambda a: a)
    offs = _copies(case["offsets"][:noff] + [None] * (L - noff))
    out = S.lowmem_pyramid(rnd(case["fmap1"]), [rnd(f) for f in case["fmap2s"][:L]], case["coords"], offs, R)
    return out, offs


def agree(got, want, tol, ctx=""):
    """Equal NaN positions; finite values within tol."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (ctx, got.shape, want.shape)
    gn, wn = np.isnan(got), np.isnan(want)
    if not np.array_equal(gn, wn):
        k = np.argwhere(gn != wn)
        pytest.fail("%s: NaN positions differ at %d of %d places, first %s: got %r want %r"
                    % (ctx, len(k), got.size, tuple(k[0]), got[tuple(k[0])], want[tuple(k[0])]))
    err = np.abs(got - want)[~wn]
    worst = float(err.max()) if err.size else 0.0
    print("WILD %s: max |err| %.3g (bound %.3g), %d NaN of %d" % (ctx, worst, tol, int(wn.sum()), want.size))
    assert worst <= tol, (ctx, worst, tol)
    return worst


def pixels_of(cls, want_axis=None):
    """(edge, pixel, ladder index, axis, level) of every slot whose entry is of class cls."""
    return [s for s in W.schedule(H1, W1) if W.LADDER[s[2]][0] == cls and (want_axis is None or s[3] == want_axis)]


# =============================================================== CPU ===============================================================
def test_ladder_coverage():
    """Table check: every class at every level and on x alone, y alone and both; every entry on all three axis modes; the
    wild offsets sit on ordinary pixels; edge 2 receives nothing."""
    sched = W.schedule(H1, W1)
    assert len(sched) == len(W.slots(H1, W1)) == 39 + 192
    for cls in W.CLASSES:
        rows = [s for s in sched if W.LADDER[s[2]][0] == cls]
        assert {s[4] for s in rows} == {0, 1, 2, 3}, cls
        assert {s[3] for s in rows} == set(W.AXES), cls
        assert {s[0] for s in rows} == {0, 1}, cls            # among ordinary pixels and in the all-wild edge
    for k in range(len(W.LADDER)):
        assert {s[3] for s in sched if s[2] == k} == set(W.AXES), W.LADDER[k][1]
    labels = {e[1] for e in W.LADDER}
    for must in ("-(R+2)", "-(R+1)", "-R", "-1", "-0.0", "0", "n-1", "n", "n+R", "n+R+1", "n+2^-10", "0-2^-10", "32760", "32767",
                 "32767.5", "32768", "32768+R+1", "-32768", "-32769-R", "65536+5.25", "-65536+5.25", "131072+5.25", "2^23+5",
                 "2^24+6", "-2^24+6", "2^25+8", "2^30", "2^31-128", "2^31", "-2^31", "-2^31-256", "3e9", "2^32+1024", "1e20",
                 "FLT_MAX", "+inf", "-inf", "nan", "1e-40", "-1e-40"):
        assert must in labels, must
    assert all(s[0] != 2 for s in sched)
    wild_pixels = {s[1] for s in sched if s[0] == 0}
    off = np.zeros((1, H1, W1, 7, 7, 2), np.float32)
    assert not set(W.apply_wild_offsets(off, 3)) & wild_pixels and not set(W.apply_wild_offsets(off, 3, 5)) & wild_pixels
    assert np.isnan(off[0, 4, 13, 3, 3]).all() and np.isnan(off[0, 4, 10, 0, 1, 0]) and off[0, 4, 11, 6, 0, 0] == 1e6
    # -0.0 and the subnormals survive the float32 round trip
    assert np.signbit(W.written(W.LADDER.index(next(e for e in W.LADDER if e[1] == "-0.0")), 32, 3, 2))
    case = vcase(3)
    assert np.array_equal(case["coords"][2], case["plain"][2]) and np.isfinite(case["plain"]).all()
    assert (case["coords"][1] != case["plain"][1]).any(axis=0).all()           # edge 1: every pixel carries an entry


@pytest.mark.parametrize("R", [1, 2, 3])
def test_restatement_equals_the_c_oracle_volume_samplers(oracle, R):
    """Where C defines the conversion (finite, |c| <= 2^30; the other entries moved off the map, NaN offsets made ordinary)
    the restatement and the C oracle evaluate the same float32 expressions: bit for bit."""
    case = vcase(R)
    c = W.tame(case["coords"])
    for l in range(4):
        cl = (c / np.float32(2 ** l)).astype(np.float32)
        off = np.nan_to_num(case["offsets"][l], nan=0.5)
        oa, ob = off.copy(), off.copy()
        a, = oracle.defCorr_index_forward(case["volumes"][l], cl, oa, R)
        b, = S.defCorr_index_forward(case["volumes"][l], cl, ob, R)
        assert np.array_equal(a, b) and np.array_equal(oa, ob), (l, float(np.abs(a - b).max()))
        pa, = oracle.corr_index_forward(case["volumes"][l], cl, R)
        pb, = S.corr_index_forward(case["volumes"][l], cl, R)
        assert np.array_equal(pa, pb), (l, float(np.abs(pa - pb).max()))
        assert 0.05 < float((a != 0).mean()) < 0.9                              # both in-map and off-map taps
    po, pr = _copies(case["offsets"][:2]), _copies(case["offsets"][:2])
    po, pr = [np.nan_to_num(o, nan=0.5) for o in po] + [None, None], [np.nan_to_num(o, nan=0.5) for o in pr] + [None, None]
    a = oracle.defcorr_pyramid_forward(case["volumes"], c, po, R, probe=True)
    b = S.defcorr_pyramid(case["volumes"], c, pr, R, probe=True)
    assert np.abs(a - b).max() <= 2e-5 and np.abs(po[1] - pr[1]).max() <= 1e-6   # the mask is float32 there, float64 here


@pytest.mark.parametrize("C", [64, 128])
def test_restatement_equals_the_c_oracle_lowmem_altcorr(oracle, C):
    case = mcase(C)
    c = W.tame(case["coords"])
    worst = 0.0
    for l in range(4):
        cl = (c / np.float32(2 ** l)).astype(np.float32)
        off = np.nan_to_num(case["offsets"][l], nan=0.5) if l < 2 else np.zeros_like(case["offsets"][0])
        oa, ob = off.copy(), off.copy()
        a, = oracle.lowMem_defSample(case["fmap1"], case["fmap2s"][l], cl, oa, 3)
        b, = S.lowMem_defSample(case["fmap1"], case["fmap2s"][l], cl, ob, 3)
        worst = max(worst, float(np.abs(a - b).max()))
        assert np.array_equal(oa, ob)
        for r in (1, 3):
            a, = oracle.altcorr_forward(case["fmap1"], case["fmap2s"][l], cl, r)
            b, = S.altcorr_forward(case["fmap1"], case["fmap2s"][l], cl, r)
            worst = max(worst, float(np.abs(a - b).max()))
    print("WILD restatement vs C oracle, low-memory family, C=%d: max |err| %.3g" % (C, worst))
    assert worst <= 1e-5
    g = np.random.default_rng(3).standard_normal((3, 1, 9, H1, W1)).astype(np.float32)
    cl = (c / np.float32(2)).astype(np.float32)
    ga = oracle.altcorr_backward(case["fmap1"], case["fmap2s"][1], cl, g, 1)
    gb = S.altcorr_backward(case["fmap1"], case["fmap2s"][1], cl, g, 1)
    for x, y in zip(ga, gb):
        assert np.abs(x - y).max() <= 1e-5 * max(1.0, float(np.abs(y).max()))


@pytest.mark.parametrize("W2", [32, 30])
def test_restatement_equals_the_c_oracle_gaussian_mask(oracle, W2):
    case = W.gauss_case(W2)
    m = W.tame(case["means"])
    a, = oracle.gaussianMask(m, case["covs"], case["volume"], 4)
    b, = S.gaussianMask(m, case["covs"], case["volume"], 4)
    assert np.abs(a - b).max() <= 1e-5 and float((a != 0).mean()) > 0.01
    ga = oracle.gaussianMask_backward(m, case["covs"], case["volume"], case["grad"], 4)
    gb = S.gaussianMask_backward(m, case["covs"], case["volume"], case["grad"], 4)
    for x, y in zip(ga, gb):
        assert np.abs(x - y).max() <= 1e-5 * max(1.0, float(np.abs(y).max()))
    la, lb = oracle.volume_pyramid(m, case["covs"], case["volume"], 3, 4), S.volume_pyramid(m, case["covs"], case["volume"], 3, 4)
    for x, y in zip(la, lb):
        assert np.abs(x - y).max() <= 1e-5


def test_the_inputs_do_what_they_are_for():
    """Properties of the REFERENCE, on the restatement: a kernel that packed an alias row into 16 bits, or multiplied its
    row in 24, would return the twin's non-zero values for it."""
    R = 3
    case = vcase(R)
    out, _ = vref(R, 4, False, False)                        # (3, 196, 8, 24)
    lout, _ = mref(64, R)                                    # (3, 1, 196, 8, 24)
    px = lambda a, e, p: a[e, :, p // W1, p % W1]
    # with one sample per pixel the low-memory sampler reads offset row b * n = 0 for EVERY edge (lowMem_defSample.cu:80-83):
    # the wild offset taps of edge 0 reach the same pixels of edges 1 and 2 there
    shared = {q[0] for q in W.WILD_OFFSETS} | {q[0] + 5 for q in W.WILD_OFFSETS}
    for cls in ("alias", "m24", "i16", "i32"):
        for e, p, k, axis, lv in pixels_of(cls):
            assert not px(out, e, p).any(), (W.LADDER[k][1], axis, lv)                       # all zero, never NaN
            assert p in shared or not px(lout[:, 0], e, p).any(), (W.LADDER[k][1], axis, lv)
    seen = set()
    for e, p, k, axis, lv in pixels_of("twin"):
        v = W.value(k, 0, R)
        for ext, o in ((W.VOL_EXTENTS, out), (W.MAP_EXTENTS, lout[:, 0])):
            h2, w2 = ext[lv]
            inside = (axis == "y" or np.floor(v) - R + (4 if lv < 2 else 0) <= w2 - 1 - 4) and \
                     (axis == "x" or np.floor(v) - R + (4 if lv < 2 else 0) <= h2 - 1 - 4)
            if inside:
                assert px(o, e, p)[49 * lv:49 * (lv + 1)].any(), (W.LADDER[k][1], axis, lv)
                seen.add((W.LADDER[k][1], ext is W.VOL_EXTENTS))
    assert {s[0] for s in seen if s[1]} == {"5.25", "5", "6", "8"} and {s[0] for s in seen if not s[1]} >= {"5"}
    # NaN rows of the volume samplers: NaN exactly at the taps whose x1 (y1) lies in the slice, zero elsewhere; inf rows: zeros
    nan_k = next(k for k, e in enumerate(W.LADDER) if e[1] == "nan")
    inf_k = [k for k, e in enumerate(W.LADDER) if e[1] in ("+inf", "-inf")]
    checked = 0
    for l, (h2, w2) in enumerate(W.VOL_EXTENTS):
        cl = (case["coords"] / np.float32(2 ** l)).astype(np.float32)
        pr, = S.corr_index_forward(case["volumes"][l], cl, R)                                # (3, rd, rd, 8, 24) [i][j]
        for e, p, k, axis, lv in W.schedule(H1, W1):
            y, x = p // W1, p % W1
            taps = pr[e, :, :, y, x]
            if k == nan_k:
                fx = 0 if axis in ("x", "both") else int(np.floor(cl[e, 0, y, x]))
                fy = 0 if axis in ("y", "both") else int(np.floor(cl[e, 1, y, x]))
                i, j = np.arange(7).reshape(7, 1), np.arange(7).reshape(1, 7)
                inmap = (fx - R + i >= 0) & (fx - R + i < w2) & (fy - R + j >= 0) & (fy - R + j < h2)
                assert np.array_equal(np.isnan(taps), inmap) and not taps[~inmap].any(), (l, axis)
                checked += int(inmap.any())
            elif k in inf_k:
                assert not taps.any(), (l, axis)                                             # zeros, not NaN
    assert checked >= 8
    # the low-memory sampler and altcorr test every corner alone and multiply a padded zero by the weight: a NaN or infinite
    # coordinate (inf - floor(inf) is NaN) makes every tap of the pixel NaN there; see tests/sampler_restatement.py
    for e, p, k, axis, lv in pixels_of("nonfin"):
        if W.LADDER[k][1] in ("nan", "+inf", "-inf"):
            assert np.isnan(px(lout[:, 0], e, p)).all(), (W.LADDER[k][1], axis)
    # the wild offsets: the NaN tap alone is NaN (if its other axis is in range), the centre tap is zeroed and finite
    p = W.WILD_OFFSETS[3][0]
    assert np.isfinite(px(out, 0, p)[:49]).all() and px(out, 0, p)[:49].any()
    p = W.WILD_OFFSETS[1][0]
    assert px(out, 0, p)[6 * 7 + 0] == 0 and np.count_nonzero(px(out, 0, p)[:49]) >= 20       # the 1e6 tap alone is lost
    # edge 2 is ordinary: no pixel without a non-zero tap, nothing NaN
    assert np.isfinite(out[2]).all() and out[2].any(axis=0).all()
    keep = np.ones(H1 * W1, bool)
    keep[sorted(shared)] = False
    assert np.isfinite(lout[2, 0].reshape(196, -1)[:, keep]).all() and lout[2, 0].any(axis=0).all()
    plain, _ = vref(R, 4, False, False, True)
    assert np.array_equal(plain[2], out[2])


def test_a_nan_probe_poisons_level_one_offsets_persistently():
    """corr.py:94-99: offset[1] *= sigmoid(var(probe)).  A NaN probe leaves NaN offsets, which every later call reads."""
    out, offs = vref(3, 4, False, True)
    nan_px = [(e, p) for e, p, k, axis, lv in pixels_of("nonfin") if W.LADDER[k][1] == "nan"]
    hit = 0
    for e, p in nan_px:
        o = offs[1][e, p // W1, p % W1]
        if np.isnan(o).any():
            hit += 1
            assert np.isnan(np.delete(o.reshape(49, 2), 24, 0)).all() and not o[3, 3].any()    # all but the zeroed centre
    assert hit >= 2
    assert np.isfinite(offs[1][2]).all()


# =============================================================== GPU ===============================================================
gpu = pytest.mark.gpu
_SENT = 1234.5


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def banded(shape, dtype=None, guard=4096):
    """A tensor in the middle of a sentinel-filled buffer: a stray write of a kernel lands in the bands."""
    n = int(np.prod(shape))
    big = torch.full((n + 2 * guard,), _SENT, dtype=dtype or torch.float32, device="cuda")
    return big, big[guard:guard + n].view(shape), guard


def banded_copy(a):
    big, view, g = banded(tuple(a.shape))
    view.copy_(dev(a))
    return big, view, g


def intact(big, guard):
    return bool((big[:guard] == _SENT).all()) and bool((big[-guard:] == _SENT).all())


def cabi(lgu, name, *args):
    """A C-ABI entry called directly: its outputs are then tensors of the caller's choosing — banded ones here — where the
    Python operator of the same name allocates them itself."""
    lgu._lib.check(getattr(lgu._lib.load(), name)(*args), name)


def same_bits(a, b):
    """Bitwise agreement of two device results that may hold NaN."""
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(torch.isnan(a), torch.isnan(b)) \
        and torch.equal(torch.nan_to_num(a, nan=7.0), torch.nan_to_num(b, nan=7.0))


@pytest.fixture
def native(lgu):
    assert torch.cuda.is_available(), "these tests need the MI355X"
    assert os.path.exists(lgu._lib.so_path()), "liblgu_corr.so missing"
    lgu._lib.load()
    return lgu


def offsets_agree(got, want, tol=0.0, ctx=""):
    for l, (a, b) in enumerate(zip(got, want)):
        if a is None:
            assert b is None
            continue
        a = host(a)
        if tol == 0.0:
            assert np.array_equal(a, b, equal_nan=True), "%s: offsets[%d] in-place state differs" % (ctx, l)
        else:
            agree(a, b, tol, "%s offsets[%d]" % (ctx, l))


def volume_operands(lgu, R, L, dense, tiled=False, slots=False):
    case = vcase(R)
    vols = [dev(v) for v in case["volumes"][:L]]
    hw = [tuple(v.shape[3:]) for v in vols]
    slot_t = None
    if slots:
        perm = torch.tensor([3, 0, 4], dtype=torch.int32, device="cuda")
        big = []
        for v in vols:
            b = torch.randn((5,) + tuple(v.shape[1:]), device="cuda")
            b[perm.long()] = v
            big.append(b)
        vols, slot_t = big, perm
    if tiled:
        vols = [lgu.ops.volume_retile(v.contiguous()) for v in vols]
    offs_np = case["offsets"][:L] if dense else case["offsets"][:2] + [None] * (L - 2)
    bands, offs = [], []
    for o in offs_np:
        if o is None:
            offs.append(None)
        else:
            big, view, g = banded_copy(o)
            bands.append((big, g))
            offs.append(view)
    return case, vols, hw, slot_t, offs, bands


@gpu
@pytest.mark.parametrize("mode", ["plain", "coords_last", "slots"])
@pytest.mark.parametrize("tiled", [False, True])
@pytest.mark.parametrize("probe", [False, True])
def test_metric_kernel(native, probe, tiled, mode):
    """csrc/defcorr_lean.hip in its four instantiations <PROBE, TILED>, with planar / interleaved coords and slots."""
    lgu, R = native, 3
    case, vols, hw, slot_t, offs, bands = volume_operands(lgu, R, 4, False, tiled, mode == "slots")
    obig, out, og = banded((3, 196, H1, W1))
    bands.append((obig, og))
    plan = lgu.ops.DefcorrPyramidPlan(vols, offs, R, probe=probe, tiled=tiled, level_hw=hw if tiled else None,
                                      coords_last=(mode == "coords_last"), slots=slot_t)
    shape = (lambda c: dev(c).permute(0, 2, 3, 1).contiguous()) if mode == "coords_last" else dev
    got = plan(shape(case["coords"]), out=out)
    torch.cuda.synchronize()
    want, want_offs = vref(R, 4, False, probe)
    ctx = "metric probe=%d tiled=%d %s" % (probe, tiled, mode)
    agree(host(got), want, 2e-5 if probe else 1e-5, ctx)
    offsets_agree(offs[:1], want_offs[:1], 0.0, ctx)
    offsets_agree(offs[1:2], want_offs[1:2], 1e-5 if probe else 0.0, ctx)
    assert not bool((got == _SENT).any()) and all(intact(b, g) for b, g in bands), ctx + ": a write outside the tensors"
    # edge 2 is ordinary: bitwise what the call returns when edges 0 and 1 are ordinary too
    _, _, _, _, offs2, _ = volume_operands(lgu, R, 4, False)
    plan2 = lgu.ops.DefcorrPyramidPlan(vols, offs2, R, probe=probe, tiled=tiled, level_hw=hw if tiled else None,
                                       coords_last=(mode == "coords_last"), slots=slot_t)
    assert torch.equal(plan2(shape(case["plain"]))[2], got[2]), ctx


@gpu
@pytest.mark.parametrize("fmt", ["nhwc", "nhwc_f16"])
@pytest.mark.parametrize("probe", [False, True])
def test_metric_kernel_output_formats(native, probe, fmt):
    lgu, R = native, 3
    case, tv, hw, _, offs_a, _ = volume_operands(lgu, R, 4, False, True)
    _, _, _, _, offs_b, bands = volume_operands(lgu, R, 4, False, True)
    coords = dev(case["coords"])
    planar = lgu.ops.defcorr_pyramid_forward(tv, coords, offs_a, R, probe=probe, tiled=True, level_hw=hw)
    big, view, g = banded((3, H1, W1, 196), torch.float16 if fmt == "nhwc_f16" else torch.float32)
    got = lgu.ops.defcorr_pyramid_forward(tv, coords, offs_b, R, probe=probe, tiled=True, level_hw=hw, out_format=fmt,
                                          out=view.permute(0, 3, 1, 2))
    torch.cuda.synchronize()
    assert same_bits(got, planar.half() if fmt == "nhwc_f16" else planar)
    assert bool(torch.isnan(planar).any()) and intact(big, g) and all(intact(b, gg) for b, gg in bands)
    for a, b in zip(offs_a, offs_b):
        assert a is None or same_bits(a, b)


@gpu
@pytest.mark.parametrize("probe", [False, True])
def test_metric_kernel_fused_encoder_layer(native, probe):
    """lookup + first corr_encoder layer in one launch == relu(W x + b) on the half lookup, NaN rows included (tolerance of
    test_randomized_differential_pyramid: 2^-10 relative + 1e-4)."""
    lgu, R = native, 3
    case, tv, hw, _, offs_a, _ = volume_operands(lgu, R, 4, False, True)
    _, _, _, _, offs_b, bands = volume_operands(lgu, R, 4, False, True)
    coords = dev(case["coords"])
    g = torch.Generator(device="cuda")
    g.manual_seed(17)
    w, b = lgu.ops.pack_encoder_layer(torch.randn(128, 196, 1, 1, device="cuda", generator=g) * 0.5,
                                      torch.randn(128, device="cuda", generator=g) * 0.1)
    x = lgu.ops.defcorr_pyramid_forward(tv, coords, offs_a, R, probe=probe, tiled=True, level_hw=hw, out_format="nhwc_f16")
    ebig, eview, eg = banded((3, H1, W1, 128), torch.float16)
    got = lgu.ops.DefcorrPyramidPlan(tv, offs_b, R, probe=probe, tiled=True, level_hw=hw, encoder=(w, b))(coords, out=eview.permute(0, 3, 1, 2))
    torch.cuda.synchronize()
    assert got.data_ptr() == eview.data_ptr() and intact(ebig, eg) and not bool((got == _SENT).any())
    want = torch.relu(x.permute(0, 2, 3, 1).float() @ w[:, :196].float().t() + b.float()).permute(0, 3, 1, 2)
    assert bool(torch.isnan(want).any()) and float(torch.nan_to_num(want).max()) > 0.05
    gn, wn = torch.isnan(got), torch.isnan(want)
    assert torch.equal(gn, wn), "NaN positions differ at %d places" % int((gn != wn).sum())
    err = (got.float() - want).abs()[~wn]
    assert bool((err <= want[~wn].abs() * 2.0 ** -10 + 1e-4).all()), float(err.max())
    assert all(intact(bb, gg) for bb, gg in bands)
    for a_, b_ in zip(offs_a, offs_b):
        assert a_ is None or same_bits(a_, b_)


@gpu
@pytest.mark.parametrize("variant", [0, 1, 2, 3, 4, 5])
@pytest.mark.parametrize("R", [1, 2, 3])
@pytest.mark.parametrize("L", [2, 3])
def test_general_volume_kernels(native, monkeypatch, L, R, variant):
    """csrc/defcorr.hip, LGU_DEFCORR_VARIANT 0-5, dense offsets."""
    lgu = native
    monkeypatch.setenv("LGU_DEFCORR_VARIANT", str(variant))
    case, vols, hw, _, offs, bands = volume_operands(lgu, R, L, True)
    rd = 2 * R + 1
    obig, out, og = banded((3, L * rd * rd, H1, W1))
    got = lgu.ops.defcorr_pyramid_forward(vols, dev(case["coords"]), offs, R, out=out)
    torch.cuda.synchronize()
    want, want_offs = vref(R, L, True, False)
    ctx = "general variant=%d L=%d R=%d" % (variant, L, R)
    agree(host(got), want, 1e-6, ctx)
    offsets_agree(offs, want_offs, 0.0, ctx)
    assert not bool((got == _SENT).any()) and intact(obig, og) and all(intact(b, g) for b, g in bands), ctx
    _, _, _, _, offs2, _ = volume_operands(lgu, R, L, True)
    assert torch.equal(lgu.ops.defcorr_pyramid_forward(vols, dev(case["plain"]), offs2, R)[2], got[2]), ctx


@gpu
@pytest.mark.parametrize("R", [1, 2, 3])
def test_volume_operators(native, R):
    """corr_index_forward / defCorr_index_forward, level by level as the reference calls them."""
    lgu = native
    case, vols, hw, _, offs, bands = volume_operands(lgu, R, 4, True)
    for l in range(4):
        cl = (case["coords"] / np.float32(2 ** l)).astype(np.float32)
        o = case["offsets"][l].copy()
        want, = S.defCorr_index_forward(case["volumes"][l], cl, o, R)
        got, = lgu.ops.defCorr_index_forward(vols[l], dev(cl), offs[l], R)
        agree(host(got), want, 1e-6, "defCorr_index_forward R=%d l=%d" % (R, l))
        assert np.array_equal(host(offs[l]), o, equal_nan=True)
        want, = S.corr_index_forward(case["volumes"][l], cl, R)
        gotp, = lgu.ops.corr_index_forward(vols[l], dev(cl), R)
        agree(host(gotp), want, 1e-6, "corr_index_forward R=%d l=%d" % (R, l))
        # the same two kernels writing into banded outputs
        P, st, cd = lgu.ops._ptr, lgu.ops._stream(vols[l]), dev(cl)
        h2, w2 = hw[l]
        for name, ref_out, extra in (("lgu_defcorr_fwd_f32", got, (P(offs[l]),)), ("lgu_corridx_fwd_f32", gotp, ())):
            big, out, g = banded(tuple(ref_out.shape))
            cabi(lgu, name, P(vols[l]), P(cd), *extra, P(out), 3, H1, W1, h2, w2, R, st)
            torch.cuda.synchronize()
            assert same_bits(out, ref_out) and intact(big, g), (name, l)
    torch.cuda.synchronize()
    assert all(intact(b, g) for b, g in bands)


def map_operands(C, R, half, L=4, noff=2):
    case = mcase(C, R)
    cast = (lambda t: t.half()) if half else (lambda t: t)
    f1, f2s = cast(dev(case["fmap1"])), [cast(dev(f)) for f in case["fmap2s"][:L]]
    bands, offs = [], []
    for l in range(L):
        if l < noff:
            big, view, g = banded_copy(case["offsets"][l])
            bands.append((big, g))
            offs.append(view)
        else:
            offs.append(None)
    return case, f1, f2s, offs, bands


@gpu
@pytest.mark.parametrize("C", [64, 128])
def test_cooperative_lowmem_kernel(native, monkeypatch, C):
    """csrc/lowmem_coop.hip (half maps, four levels, offsets on levels 0-1): default / all fused / all split scheduling and
    chunk-planar maps bitwise equal, the one-wave kernel (LGU_LOWMEM_COOP=0) and the restatement to 1e-5."""
    lgu, R = native, 3
    want, want_offs = mref(C, R, half=True)
    rd2 = 49

    def run(chunked=False, coords=None, **env):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        case, f1, f2s, offs, bands = map_operands(C, R, True)
        obig, out, og = banded((3, 1, 4 * rd2, H1, W1))
        if chunked:
            f2s = [lgu.ops.lowmem_chunked(f) for f in f2s]
        got = lgu.ops.lowmem_pyramid_forward_mixed(f1, f2s, dev(case["coords"] if coords is None else coords), offs, R, out=out,
                                                   chunked=chunked)
        torch.cuda.synchronize()
        for k in env:
            monkeypatch.delenv(k)
        assert not bool((got == _SENT).any()) and intact(obig, og) and all(intact(b, g) for b, g in bands), env
        return got, offs

    default, offs = run()
    agree(host(default), want, 1e-5, "coop default C=%d" % C)
    offsets_agree(offs, want_offs, 0.0, "coop default")
    for env in (dict(LGU_LOWMEM_COOP_SPLIT="0"), dict(LGU_LOWMEM_COOP_SPLIT="1")):
        got, o = run(**env)
        assert same_bits(got, default), env
        offsets_agree(o, want_offs, 0.0, str(env))
    got, o = run(chunked=True)
    assert same_bits(got, default), "chunk-planar maps"
    old, o = run(LGU_LOWMEM_COOP="0")
    agree(host(old), want, 1e-5, "one-wave kernel C=%d" % C)
    offsets_agree(o, want_offs, 0.0, "one-wave kernel")
    plain, _ = run(coords=mcase(C, R)["plain"])
    assert same_bits(plain[2], default[2])      # edge 2 reads offset row 0 too: its NaN tap is there in both runs


@gpu
def test_cooperative_lowmem_kernel_frame_indirection_and_calls(native):
    """The ii / jj form reads frame buffers in place; the `calls` entry (off_row) serves several reference calls in one
    launch — here the ordinary edge as call 0 and the two wild edges as call 1, each with its own offset row."""
    lgu, R, C = native, 3, 64
    case, f1, f2s, _, _ = map_operands(C, R, True)
    coords = dev(case["coords"])
    # frames: fmap1 of edge b is frame ii[b] of buffer 0, fmap2 of edge b is frame jj[b]
    ii = torch.tensor([2, 0, 1], device="cuda")
    jj = torch.tensor([3, 1, 0], device="cuda")
    frames = [(torch.randn(4, 8 >> l, 24 >> l, C, device="cuda") * 0.125).half() for l in range(4)]
    o_np = case["offsets"]
    oa, ob = [dev(o_np[0]), dev(o_np[1]), None, None], [dev(o_np[0]), dev(o_np[1]), None, None]
    got = lgu.ops.lowmem_pyramid_forward_mixed(frames[0], frames, coords, oa, R, ii=ii, jj=jj)
    per_edge = lgu.ops.lowmem_pyramid_forward_mixed(frames[0][ii].contiguous(), [f[jj].contiguous() for f in frames], coords, ob, R)
    assert same_bits(got, per_edge) and same_bits(oa[0], ob[0]) and same_bits(oa[1], ob[1])
    ro = _copies(o_np[:2]) + [None, None]
    want = S.lowmem_pyramid(host(frames[0][ii].float()), [host(f[jj].float()) for f in frames], case["coords"], ro, R)
    agree(host(got), want, 1e-5, "frame indirection")
    offsets_agree(oa, ro, 0.0, "frame indirection")
    # calls: edge order [2, 0, 1], rows [0, 1, 1]; row 0 = edge 2's ordinary offsets, row 1 = edge 0's (with the wild taps)
    order = [2, 0, 1]
    rows = torch.tensor([0, 1, 1], dtype=torch.int32, device="cuda")
    k0 = np.stack([o_np[0][2], o_np[0][0]])
    k1 = np.stack([o_np[1][2], o_np[1][0]])
    b0, v0, g0 = banded_copy(k0)
    b1, v1, g1 = banded_copy(k1)
    obig, out, og = banded((3, 1, 196, H1, W1))
    sel = torch.tensor(order, device="cuda")
    got = lgu.ops.lowmem_pyramid_forward_mixed(f1[sel].contiguous(), [f[sel].contiguous() for f in f2s], coords[sel].contiguous(),
                                               [v0, v1, None, None], R, off_row=rows, out=out)
    torch.cuda.synchronize()
    rnd = lambda a: a.astype(np.float16).astype(np.float32)
    wo0, wo1 = [k0[0:1].copy(), k1[0:1].copy(), None, None], [k0[1:2].copy(), k1[1:2].copy(), None, None]
    want0 = S.lowmem_pyramid(rnd(case["fmap1"][2:3]), [rnd(f[2:3]) for f in case["fmap2s"]], case["coords"][2:3], wo0, R)
    want1 = S.lowmem_pyramid(rnd(case["fmap1"][0:2]), [rnd(f[0:2]) for f in case["fmap2s"]], case["coords"][0:2], wo1, R)
    agree(host(got), np.concatenate([want0, want1]), 1e-5, "calls entry")
    assert np.array_equal(host(v0), np.concatenate([wo0[0], wo1[0]]), equal_nan=True)
    assert np.array_equal(host(v1), np.concatenate([wo0[1], wo1[1]]), equal_nan=True)
    assert not bool((got == _SENT).any()) and intact(obig, og) and intact(b0, g0) and intact(b1, g1)


@gpu
@pytest.mark.parametrize("zo", [None, "0"])
@pytest.mark.parametrize("R", [1, 2, 3])
@pytest.mark.parametrize("half", [False, True])
def test_matrix_core_lowmem_pyramid(native, monkeypatch, half, R, zo):
    """csrc/lowmem_mfma.hip through the pyramid entry (the cooperative kernel switched off for the half maps), with and
    without the zero-offset levels' shared floors (LGU_LOWMEM_ZO)."""
    lgu, C = native, 128
    if zo is not None:
        monkeypatch.setenv("LGU_LOWMEM_ZO", zo)
    if half:
        monkeypatch.setenv("LGU_LOWMEM_COOP", "0")
    case, f1, f2s, offs, bands = map_operands(C, R, half)
    rd2 = (2 * R + 1) ** 2
    obig, out, og = banded((3, 1, 4 * rd2, H1, W1))
    got = lgu.ops.lowmem_pyramid_forward_mixed(f1, f2s, dev(case["coords"]), offs, R, out=out)
    torch.cuda.synchronize()
    want, want_offs = mref(C, R, half=half)
    ctx = "mfma pyramid half=%d R=%d zo=%s" % (half, R, zo)
    agree(host(got), want, 1e-5, ctx)
    offsets_agree(offs, want_offs, 0.0, ctx)
    assert not bool((got == _SENT).any()) and intact(obig, og) and all(intact(b, g) for b, g in bands), ctx
    _, _, _, offs2, _ = map_operands(C, R, half)
    assert same_bits(lgu.ops.lowmem_pyramid_forward_mixed(f1, f2s, dev(case["plain"]), offs2, R)[2], got[2]), ctx


@gpu
@pytest.mark.parametrize("kernel", ["f32_v0", "f32_v1", "f32_v2", "h16_v0", "h16_v1"])
@pytest.mark.parametrize("R", [1, 2, 3])
def test_lowmem_per_level_operators(native, monkeypatch, R, kernel):
    """lowMem_defSample (LGU_LOWMEM_VARIANT 0 = fp32 matrix cores, 2 = VALU tile kernel, 1 = wave per pixel) and
    lowMem_defSample_mixed (LGU_LOWMEM_H16_VARIANT 0 = matrix cores, 1 = VALU tile kernel), level by level."""
    lgu, C = native, 64
    half = kernel.startswith("h16")
    monkeypatch.setenv("LGU_LOWMEM_H16_VARIANT" if half else "LGU_LOWMEM_VARIANT", kernel[-1])
    case, f1, f2s, offs, bands = map_operands(C, R, half, noff=2)
    rnd = (lambda a: a.astype(np.float16).astype(np.float32)) if half else (lambda a: a)
    op = lgu.ops.lowMem_defSample_mixed if half else lgu.ops.lowMem_defSample
    rd = 2 * R + 1
    for l in range(4):
        cl = (case["coords"] / np.float32(2 ** l)).astype(np.float32)
        o = case["offsets"][l].copy() if l < 2 else np.zeros((3, H1, W1, rd, rd, 2), np.float32)
        od = offs[l] if l < 2 else dev(o)
        want, = S.lowMem_defSample(rnd(case["fmap1"]), rnd(case["fmap2s"][l]), cl, o, R)
        got, = op(f1, f2s[l], dev(cl), od, R)
        agree(host(got), want, 1e-5, "%s R=%d l=%d" % (kernel, R, l))
        assert np.array_equal(host(od), o, equal_nan=True), (kernel, l)
        big, out, g = banded(tuple(got.shape))      # the same kernel writing into a banded output
        P, cd = lgu.ops._ptr, dev(cl)
        cabi(lgu, "lgu_lowmem_defsample_fwd_h16" if half else "lgu_lowmem_defsample_fwd_f32", P(f1), P(f2s[l]), P(cd), P(od),
             P(out), 3, 1, H1, W1, f2s[l].shape[1], f2s[l].shape[2], C, od.shape[0], R, lgu.ops._stream(f1))
        torch.cuda.synchronize()
        assert same_bits(out, got) and intact(big, g), (kernel, l)
    torch.cuda.synchronize()
    assert all(intact(b, g) for b, g in bands)


def _altcorr_bounds(case_f1, case_f2, cl, g, r):
    """The elementwise bounds of tests/test_backward.py (k_f1 * u * A1, (N + 8) * u * A2): A = the same sums over absolute
    values, N = contributions per fmap2 position."""
    from tests import backward_restatement as BR
    A1, A2, _ = S.altcorr_backward(np.abs(case_f1), np.abs(case_f2), cl, np.abs(g), r)
    H2, W2 = case_f2.shape[1:3]
    _, _, h2, w2, ok = S._alt_geometry(cl, r, H2, W2)
    N = np.zeros(case_f2.shape[:3])
    B = cl.shape[0]
    for iy in range(2 * r + 2):
        for ix in range(2 * r + 2):
            o = ok[:, 0, :, :, iy, ix]
            y, x = np.clip(h2[:, 0, :, :, iy], 0, H2 - 1), np.clip(w2[:, 0, :, :, ix], 0, W2 - 1)
            np.add.at(N, (np.broadcast_to(np.arange(B).reshape(B, 1, 1), y.shape), y, x), o.astype(np.float64))
    return BR.k_f1(1, r) * BR.U * A1, (N[..., None] + 8) * BR.U * A2


@gpu
@pytest.mark.parametrize("variant", [0, 1, 2])
@pytest.mark.parametrize("r", [1, 3])
def test_altcorr_forward_and_backward(native, monkeypatch, r, variant):
    lgu, C = native, 64
    monkeypatch.setenv("LGU_LOWMEM_VARIANT", str(variant))
    case, f1, f2s, _, _ = map_operands(C, 3, False)
    l = 1
    cl = (case["coords"] / np.float32(2 ** l)).astype(np.float32)
    want, = S.altcorr_forward(case["fmap1"], case["fmap2s"][l], cl, r)
    got, = lgu.ops.altcorr_forward(f1, f2s[l], dev(cl), r)
    agree(host(got), want, 1e-5, "altcorr_forward r=%d variant=%d" % (r, variant))
    plain, = lgu.ops.altcorr_forward(f1, f2s[l], dev((case["plain"] / np.float32(2)).astype(np.float32)), r)
    assert torch.equal(plain[2], got[2])
    P, st, cd = lgu.ops._ptr, lgu.ops._stream(f1), dev(cl)
    fh, fw = f2s[l].shape[1:3]
    big, out, bg = banded(tuple(got.shape))          # the same kernel writing into a banded output
    cabi(lgu, "lgu_altcorr_fwd_f32", P(f1), P(f2s[l]), P(cd), P(out), 3, 1, H1, W1, fh, fw, C, r, st)
    torch.cuda.synchronize()
    assert same_bits(out, got) and intact(big, bg)
    if variant:
        return          # the backward has one kernel
    g = np.random.default_rng(70 + r).standard_normal(want.shape).astype(np.float32)
    w1, w2, _ = S.altcorr_backward(case["fmap1"], case["fmap2s"][l], cl, g, r)
    b1, b2 = _altcorr_bounds(case["fmap1"], case["fmap2s"][l], cl, g, r)
    # the backward scatters into fmap2_grad at positions formed from coords: both gradients are banded (C entry; the operator
    # allocates fmap1_grad and a zeroed fmap2_grad itself and returns an all-zero coords_grad)
    big1, g1, bg1 = banded(tuple(f1.shape))
    big2, g2, bg2 = banded(tuple(f2s[l].shape))
    g2.zero_()
    gd = dev(g)
    cabi(lgu, "lgu_altcorr_bwd_f32", P(f1), P(f2s[l]), P(cd), P(gd), P(g1), P(g2), 3, 1, H1, W1, fh, fw, C, r, st)
    torch.cuda.synchronize()
    assert intact(big1, bg1) and intact(big2, bg2) and not bool((g1 == _SENT).any())
    cg = lgu.ops.altcorr_backward(f1, f2s[l], dev(cl), dev(g), r)[2]
    for name, got_, want_, bound in (("fmap1_grad", host(g1), w1, b1), ("fmap2_grad", host(g2), w2, b2)):
        gn, wn = np.isnan(got_), np.isnan(want_)
        assert wn.any() and np.array_equal(gn, wn), "%s: NaN positions differ at %d places" % (name, int((gn != wn).sum()))
        err = np.abs(got_ - want_)
        bad = ~wn & ~(err <= bound)
        print("WILD altcorr_backward %s r=%d: worst err/bound %.3f" % (name, r, float(np.nanmax(np.where(wn | (bound == 0), 0, err / np.where(bound == 0, 1, bound))))))
        assert not bad.any(), (name, int(bad.sum()), float(err[bad].max()))
    assert not bool(cg.any())


@gpu
@pytest.mark.parametrize("W2", [32, 30])
def test_gaussian_mask_kernels(native, W2):
    """gaussianMask / gaussianMask_backward / volume_pyramid (row-major and tiled) with the ladder on the means; W2 = 32 takes
    the vector kernel, W2 = 30 the generic one."""
    lgu = native
    case = W.gauss_case(W2)
    means, covs, vol, grad = dev(case["means"]), dev(case["covs"]), dev(case["volume"]), dev(case["grad"])
    want, = S.gaussianMask(case["means"], case["covs"], case["volume"], 4)
    got, = lgu.ops.gaussianMask(means, covs, vol, 4)
    agree(host(got), want, 1e-5, "gaussianMask W2=%d" % W2)
    assert np.isnan(want).any()
    plain, = lgu.ops.gaussianMask(dev(case["plain"]), covs, vol, 4)
    assert torch.equal(plain[2], got[2])
    wm, wc = S.gaussianMask_backward(case["means"], case["covs"], case["volume"], case["grad"], 4)
    gm, gc = lgu.ops.gaussianMask_backward(means, covs, vol, grad, 4)
    agree(host(gm), wm, 1e-5 * max(1.0, float(np.nanmax(np.abs(wm)))), "gaussianMask_backward means W2=%d" % W2)
    agree(host(gc), wc, 1e-5 * max(1.0, float(np.nanmax(np.abs(wc)))), "gaussianMask_backward covs W2=%d" % W2)
    # the kernels store at positions formed from `means`: the same calls with every output between sentinel bands
    P, st = lgu.ops._ptr, lgu.ops._stream(vol)
    dims = (3, H1, W1, 24, W2, 4, st)
    bigv, outv, gv = banded(tuple(vol.shape))
    cabi(lgu, "lgu_gaussmask_fwd_f32", P(means), P(covs), P(vol), P(outv), *dims)
    bigm, outm, gmb = banded(tuple(means.shape))
    bigc, outc, gcb = banded(tuple(covs.shape))
    cabi(lgu, "lgu_gaussmask_bwd_f32", P(means), P(covs), P(vol), P(grad), P(outm), P(outc), *dims)
    torch.cuda.synchronize()
    assert same_bits(outv, got) and same_bits(outm, gm) and same_bits(outc, gc)
    assert intact(bigv, gv) and intact(bigm, gmb) and intact(bigc, gcb)
    L = 3
    wl = S.volume_pyramid(case["means"], case["covs"], case["volume"], L, 4)
    for tiled in (False, True):
        if W2 % 4 != 0:                        # the fused builder serves slices of whole float4 rows only: an explicit refusal
            with pytest.raises(lgu._lib.UnsupportedShape):
                lgu.ops.volume_pyramid(means, covs, vol, L, 4, inplace=False, tiled=tiled)
            continue
        levels = lgu.ops.volume_pyramid(means, covs, vol, L, 4, inplace=False, tiled=tiled)
        for l in range(L):
            lv = lgu.ops.volume_retile(levels[l], to_tiled=False, hw=(24 >> l, W2 >> l)) if tiled else levels[l]
            agree(host(lv), wl[l], 1e-5, "volume_pyramid tiled=%d W2=%d l=%d" % (tiled, W2, l))
        # every level between sentinel bands (C entry: the operator allocates the levels itself)
        lb = [banded(tuple(t.shape)) for t in levels]
        lp = (lgu.ops._vp * L)(*[b[1].data_ptr() for b in lb])
        cabi(lgu, "lgu_volume_pyramid_tiled_f32" if tiled else "lgu_volume_pyramid_f32", P(means), P(covs), P(vol), lp, L, 3, H1, W1,
             24, W2, 4, st)
        torch.cuda.synchronize()
        for l, (big, view, g) in enumerate(lb):
            assert same_bits(view, levels[l]) and intact(big, g), (tiled, l)


@gpu
def test_fused_pyramid_builder(native):
    """lgu_volume_build_pyramid_f32 through volume_build_pyramid: the all-pairs volume of 8 x 32 maps formed on the matrix
    cores and written as the tiled pyramid, the ladder on the means; 1e-5 of the level's scale as
    test_volume_built_on_the_matrix_cores_equals_matmul_plus_fused_builder."""
    lgu = native
    case = W.build_case()
    E, C, H, Wd = case["fmap1"].shape
    f1, f2 = dev(case["fmap1"]), dev(case["fmap2"])
    got = lgu.ops.volume_build_pyramid(f1, f2, dev(case["means"]), dev(case["covs"]))
    torch.cuda.synchronize()
    raw = np.einsum("ecp,ecq->epq", case["fmap1"].reshape(E, C, -1).astype(np.float64) / 4,
                    case["fmap2"].reshape(E, C, -1).astype(np.float64) / 4).reshape(E, H, Wd, H, Wd)
    want = S.volume_pyramid(case["means"], case["covs"], raw, 4, 4)
    assert np.isnan(want[0]).any()
    for l in range(4):
        lv = lgu.ops.volume_retile(got[l], to_tiled=False, hw=(H >> l, Wd >> l))
        agree(host(lv), want[l], 1e-5 * float(np.nanmax(np.abs(want[l]))), "volume_build_pyramid l=%d" % l)
    # the four tiled levels between sentinel bands (C entry, as test_volume_build_entry_points_write_nothing_outside_their_tensors)
    ops = lgu.ops
    means, covs = dev(case["means"]), dev(case["covs"])
    lb = [banded(ops.tiled_shape(E, H, Wd, H >> l, Wd >> l)) for l in range(4)]
    lp = (ops._vp * 4)(*[b[1].data_ptr() for b in lb])
    cabi(lgu, "lgu_volume_build_pyramid_f32", ops._ptr(f1), ops._ptr(f2), ops._ptr(means), ops._ptr(covs), None, 0, lp, 4, E, C, H, Wd,
         4, ops._stream(f1))
    torch.cuda.synchronize()
    for l, (big, view, g) in enumerate(lb):
        assert same_bits(view, got[l]) and intact(big, g), l
    # a width the matrix-core builder does not serve (W2 = 30): an explicit refusal, not a fallback
    z = torch.zeros(1, C, H, 30, device="cuda")
    with pytest.raises(lgu._lib.UnsupportedShape):
        ops.volume_build_pyramid(z, z, torch.zeros(1, H, 30, 2, device="cuda"), torch.ones(1, H, 30, 2, device="cuda"))


@gpu
@pytest.mark.parametrize("tiled", [True, False])
def test_corrblock_call_on_the_ladder(native, monkeypatch, tiled):
    """Host glue: CorrBlock.__call__ on the ladder coordinates, twice (the NaN mask persists in offset[1]), against the
    restatement's composition on the block's own pyramid and offsets."""
    lgu = native
    monkeypatch.setattr(lgu.CorrBlock, "TILED_PYRAMID", tiled)
    torch.manual_seed(11)
    E, h, w = 3, H1, W1
    ofsMap = torch.nn.Conv2d(256, 98, 3, padding=1).cuda()
    ofsRes = torch.nn.Conv2d(256, 98, 3, padding=1).cuda()
    GA = lgu.GaussianMask(h, w).cuda()
    f1 = torch.randn(1, E, 128, h, w, device="cuda") * 0.5
    f2 = torch.randn(1, E, 128, h, w, device="cuda") * 0.5
    xy = W.apply_ladder(W.grid_xy(np.random.default_rng(12), 3, h, w), W.MAP_EXTENTS, 3)
    with torch.no_grad():
        blk = lgu.CorrBlock(ofsMap, ofsRes, GA, f1, f2)
        pyr = [host(lgu.ops.volume_retile(v.contiguous(), to_tiled=False, hw=blk._level_hw[i]) if tiled else v)
               for i, v in enumerate(blk.corr_pyramid)]
        offs = [host(o.contiguous()).reshape(E, h, w, 7, 7, 2).copy() for o in blk.offset[:2]] + [None, None]
        c = np.ascontiguousarray(xy.transpose(0, 3, 1, 2))
        for it in range(2):
            got, _, _ = blk(dev(xy)[None])
            want = S.defcorr_pyramid(pyr, c, offs, 3, probe=True)
            agree(host(got)[0], want, 2e-5, "CorrBlock tiled=%d call %d" % (tiled, it))
        assert np.isnan(offs[1]).any()


@gpu
def test_altcorrblock_call_on_the_ladder(native):
    """Host glue: AltCorrBlock.__call__ on the ladder coordinates against the restatement's composition (probe at level 1,
    every edge sampling with edge 0's offsets)."""
    lgu = native
    torch.manual_seed(13)
    N, C, h, w = 4, 128, 16, 48          # the block pools its maps four times: 8 x 24 is too small for it
    ofsMap = torch.nn.Conv2d(256, 98, 3, padding=1).cuda()
    ofsRes = torch.nn.Conv2d(256, 98, 3, padding=1).cuda()
    fmaps = torch.randn(1, N, C, h, w, device="cuda") * 0.5
    ii = torch.tensor([0, 1, 3], device="cuda")
    jj = torch.tensor([1, 2, 0], device="cuda")
    xy = W.apply_ladder(W.grid_xy(np.random.default_rng(14), 3, h, w), [(h >> l, w >> l) for l in range(4)], 3)
    with torch.no_grad():
        blk = lgu.AltCorrBlock(ofsMap, ofsRes, None, fmaps)
        got = blk(dev(xy)[None], ii, jj)
        f1 = host(blk.pyramid[0][0, ii].float().contiguous())
        feats = torch.cat(((blk.pyramid[0][0, ii] * 4.0).permute(0, 3, 1, 2), (blk.pyramid[0][0, jj] * 4.0).permute(0, 3, 1, 2)), 1).float()
        offs, _ = lgu.corr.generate_offsets(ofsMap, ofsRes, feats, 4)
        offs = [host(o.contiguous()).reshape(3, h, w, 7, 7, 2).copy() for o in offs[:2]] + [None, None]
        f2s = [host(blk.pyramid[l][0, jj].float().contiguous()) for l in range(4)]
    want = S.lowmem_pyramid(f1, f2s, xy[:, None], offs, 3, probe=True)
    agree(host(got)[0], want[:, 0], 2e-5, "AltCorrBlock")
