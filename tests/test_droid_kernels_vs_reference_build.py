"""droid_backends' geometry and bundle-adjustment kernels against the REFERENCE's own kernels on the same GPU.

oracle/_ref/ref_droid_kernels*.so are the reference's src/droid_kernels.cu without its Eigen part (the host BA code),
compiled for gfx950 by oracle/build_ref.py together with an own binding (oracle/ref_droid_bind.cu): `_nofma` with
-ffp-contract=off, which is how lgu-slam_amd is built, the other with the compiler's default contraction of a*b+c into
FMA, as nvcc builds the reference.  Skipped when the builds are absent.  Only the Schur assembly and the solve of the
end-to-end step are restated (oracle/ba_oracle.py): in the reference they are Eigen host code.

Against the no-FMA build, which evaluates every per-pixel value in the same fp32 operations as this build:
  * bit for bit (NaN positions included): projmap, iproj, the per-pixel BA outputs Eii, Eij, Cii, wi, EvT6x1,
    pose_retr, disp_retr; depth_filter counts exactly;
  * sums taken in another order (Hs, vs, EEt6x6, Ev6x1, accum) within 2 (n + 2) 2^-24 sum|terms|: either order is
    within (n + 2) 2^-24 sum|terms| of the exact sum, n its longest chain of additions, 2 the roundings of a term;
    frame_distance within tests/test_geom.py's 1e-5 relative (see its test).
Against the contracting build every value moves by a small multiple of 2^-24 of the magnitudes that enter it; each
comparison states its bound.  A threshold decision (depth > 0.25 or > 0.01, floor(), |1/d - 1/d'| < thresh) can flip
between the builds only where the float64 value lies within that bound of the threshold: such pixels (pairs, edges) are
counted, printed (-s) and left out of that comparison.

The reference kernels have no index guards and use 32-bit accessors: only in-range indices and non-empty inputs are
passed here.  tests/test_geom.py and tests/test_ba.py keep covering this build's out-of-range and empty behaviour.
"""
import ctypes
import importlib.util
import os

import numpy as np
import pytest

from oracle import ba_oracle as O
from tests import geom_restatement as G

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from tests import test_ba as TB  # noqa: E402  (scene / perturb of the BA tests)
from tests import test_geom as TG  # noqa: E402  (scene / all_pairs / same_bits / _fd_check of the geometry tests)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFDIR = os.path.join(ROOT, "oracle", "_ref")
U = 2.0 ** -24
f32, f64 = np.float32, np.float64
SHAPES = [(48, 64), (60, 80), (7, 13)]     # the BASELINE frame, BASELINE config 5's, an odd small frame
same_bits = TG.same_bits


def _load(name):
    path = os.path.join(REFDIR, name + ".so")
    if not os.path.exists(path):
        pytest.skip("reference build %s not present (run oracle/build_ref.py where /root/reference exists)" % name)
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def refs():
    """(no-FMA build, contracting build) of the reference's kernels."""
    assert torch.cuda.is_available()
    return _load("ref_droid_kernels_nofma"), _load("ref_droid_kernels")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    torch.cuda.synchronize()
    return t.detach().cpu().numpy()


def vp(t):
    return ctypes.c_void_p(t.data_ptr())


def stream():
    return torch.cuda.current_stream().cuda_stream


def report(what, **kw):
    print("[vs reference build] %s: %s" % (what, ", ".join("%s=%s" % kv for kv in kw.items())))


def _rotation(angle, axis):
    axis = np.asarray(axis, f64) / np.linalg.norm(axis)
    return np.concatenate([np.sin(angle / 2) * axis, [np.cos(angle / 2)]]).astype(f32)


# ---- float64 geometry for the bounds against the contracting build --------------------------------------------------
def _act64(q, X):
    uv = 2.0 * np.cross(q[:3], X)
    return X + q[3] * uv + np.cross(q[:3], uv)


def _rel64(poses, i, j, stereo=False):
    """(t_ij, q_ij, m0) in float64: relSE3 (:96-107), or projective_transform_kernel's fixed stereo baseline (:218-229);
    m0 = |t_j| + 4 |t_i| bounds the magnitudes met while t_ij is formed."""
    if stereo:
        return np.array([-0.1, 0.0, 0.0]), np.array([0.0, 0.0, 0.0, 1.0]), 0.1
    p = np.asarray(poses, f64)
    ti, qi, tj, qj = p[i, :3], p[i, 3:], p[j, :3], p[j, 3:]
    qij = np.array([-qj[3] * qi[0] + qj[0] * qi[3] - qj[1] * qi[2] + qj[2] * qi[1],
                    -qj[3] * qi[1] + qj[1] * qi[3] - qj[2] * qi[0] + qj[0] * qi[2],
                    -qj[3] * qi[2] + qj[2] * qi[3] - qj[0] * qi[1] + qj[1] * qi[0],
                    qj[3] * qi[3] + qj[0] * qi[0] + qj[1] * qi[1] + qj[2] * qi[2]])
    return tj - _act64(qij, ti), qij, np.linalg.norm(tj) + 4 * np.linalg.norm(ti)


def _pixels64(H, W, intr):
    """X (HW,3) = ((u - cx) / fx, (v - cy) / fy, 1), u, v in float64, pixels in row-major order."""
    fx, fy, cx, cy = np.asarray(intr, f64)[:4]
    v, u = np.meshgrid(np.arange(H, dtype=f64), np.arange(W, dtype=f64), indexing="ij")
    u, v = u.ravel(), v.ravel()
    return np.stack([(u - cx) / fx, (v - cy) / fy, np.ones_like(u)], -1), u, v


def _transform64(t, q, m0, X, d):
    """Y = act_se3((t, q), (X, d)) in float64, and dY such that the two builds' fp32 values of each component of Y lie
    within dY of each other: each is at most 16 roundings (T_ij, two cross products, the action, + d t) away from Y, each
    rounding at most 2^-24 of an intermediate, and for a unit quaternion no intermediate exceeds M = 4 |X| + |d| m0:
    dY = 2 * 16 * 2^-24 * M."""
    Y = _act64(q, X) + d[:, None] * t[None]
    return Y, 32 * U * (4 * np.linalg.norm(X, axis=1) + np.abs(d) * m0)


def _project_bound(f, c, Y0, Y2, dY):
    """How far apart the two builds' fp32 values of f * (Y0 / Y2) + c can be, given dY on Y0 and on Y2: the quotient moves
    by (1 + |Y0 / Y2|) dY / |Y2|; each build rounds the result three times (quotient, product, sum)."""
    with np.errstate(divide="ignore", invalid="ignore"):
        r = Y0 / Y2
        return np.abs(f) * dY * (1 + np.abs(r)) / np.abs(Y2) + 6 * U * (np.abs(f * r) + abs(c))


# ---- geometry: projmap, iproj, depth_filter, frame_distance ---------------------------------------------------------
def geo_scene(seed, H, W, N=10):
    """tests/test_geom.py's camera path with 10 % zero or negative disparities, frame 2 behind the camera (disparity
    -2 - |d|) and a rotation of 2.6 rad at frame 4 (most of its points land behind the other cameras and vice versa)."""
    poses, disps, intr = TG.scene(seed, N=N, H=H, W=W, step=0.4, angle=0.3, bad=0.1)
    poses[4, 3:] = _rotation(2.6, [0.3, -0.8, 0.5])
    disps[2] = -np.abs(disps[2]) - 2.0
    return poses, disps, intr


@pytest.mark.parametrize("shape", SHAPES)
def test_projmap_and_iproj_vs_reference(lgu, refs, shape):
    """Bit for bit against the no-FMA build.  Against the contracting build: valid equal and coords within
    _project_bound, except pixels whose float64 depth lies within dY of 0, 0.01 or 0.25; iproj (points Y / d) within
    dY / |d| plus the quotient's roundings, except zero disparities (x / 0)."""
    nofma, fma = refs
    H, W = shape
    poses, disps, intr = geo_scene(71 + W, H, W)
    N = len(poses)
    rng = np.random.default_rng(W)
    ii = np.concatenate([rng.integers(0, N, 24), [0, 2, 4, 4, 9]]).astype(np.int64)    # ii == jj among them
    jj = np.concatenate([rng.integers(0, N, 24), [0, 5, 4, 1, 2]]).astype(np.int64)
    P, D, K, I, J = dev(poses), dev(disps), dev(intr), dev(ii), dev(jj)
    gc, gv = [host(t) for t in lgu.geom.projmap(P, D, K, I, J)]
    rc, rv = [host(t) for t in nofma.projmap(P, D, K, I, J)]
    assert same_bits(gc, rc) and same_bits(gv, rv)
    assert 0 < gv.mean() < 1
    inv = lgu.geom.se3_inverse(P).contiguous()
    gp = host(lgu.geom.iproj(inv, D, K))
    assert same_bits(gp, host(nofma.iproj(inv, D, K)))

    fc, fv = [host(t) for t in fma.projmap(P, D, K, I, J)]
    X, _, _ = _pixels64(H, W, intr)
    fx, fy, cx, cy = np.asarray(intr, f64)
    skipped, worst = 0, 0.0
    for k, (i, j) in enumerate(zip(ii, jj)):
        t, q, m0 = _rel64(poses, i, j)
        Y, dY = _transform64(t, q, m0, X, disps[i].ravel().astype(f64))
        z = Y[:, 2]
        ok = ~((np.abs(z) <= 4 * dY) | (np.abs(z - 0.01) <= dY) | (np.abs(z - 0.25) <= dY))
        skipped += int((~ok).sum())
        assert np.array_equal(fv[k].ravel()[ok], gv[k].ravel()[ok]), k
        assert (fc[k, ..., 2] == 0).all()
        for c, (f, cc) in enumerate(((fx, cx), (fy, cy))):
            b = _project_bound(f, cc, Y[:, c], z, dY)[ok]
            diff = np.abs(gc[k, ..., c].ravel()[ok].astype(f64) - fc[k, ..., c].ravel()[ok])
            assert (diff <= b).all(), (k, c, float((diff - b).max()))
            worst = max(worst, float((diff / np.maximum(b, 1e-300)).max()))
    fp = host(fma.iproj(inv, D, K))
    invh = host(inv).astype(f64)
    for n in range(N):
        d = disps[n].ravel().astype(f64)
        Y, dY = _transform64(invh[n, :3], invh[n, 3:], np.linalg.norm(invh[n, :3]), X, d)
        ok = d != 0
        b = dY[ok, None] / np.abs(d[ok, None]) + 4 * U * np.abs(Y[ok] / d[ok, None])
        diff = np.abs(gp[n].reshape(-1, 3)[ok].astype(f64) - fp[n].reshape(-1, 3)[ok])
        assert (diff <= b).all(), (n, float((diff - b).max()))
    report("projmap %dx%d vs contracting build" % shape, pairs=len(ii), pixels_skipped=skipped,
           worst_diff_over_bound="%.3g" % worst)


def _depth_filter_unsure(poses, disps, intr, ix, thresh):
    """(num, ht, wd) bool: pixels of which one neighbour test can decide differently in the two builds: the depth within
    4 dY of 0, floor(uj) or floor(vj) not constant over the projection bound, or, inside the frame, a corner's
    | |1/dj - 1/d| - thresh | within the bound on 1/dj = Y2 / d, (2 dY / |Y2| + 4 * 2^-24) |1/dj|."""
    N, H, W = disps.shape
    X, _, _ = _pixels64(H, W, intr)
    fx, fy, cx, cy = np.asarray(intr, f64)
    out = np.zeros((len(ix), H * W), bool)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for b, i in enumerate(ix):
            d = disps[i].ravel().astype(f64)
            for n in G.NEIGHBOURS:
                j = int(i) + n
                if not 0 <= j < N:
                    continue
                t, q, m0 = _rel64(poses, int(i), j)
                Y, dY = _transform64(t, q, m0, X, d)
                z = Y[:, 2]
                uj, vj = fx * Y[:, 0] / z + cx, fy * Y[:, 1] / z + cy
                bu, bv = _project_bound(fx, cx, Y[:, 0], z, dY), _project_bound(fy, cy, Y[:, 1], z, dY)
                unsure = (np.abs(z) <= 4 * dY) | (np.floor(uj - bu) != np.floor(uj + bu)) | (np.floor(vj - bv) != np.floor(vj + bv))
                u0, v0 = np.floor(uj), np.floor(vj)
                inside = ~unsure & (u0 >= 0) & (v0 >= 0) & (u0 < W - 1) & (v0 < H - 1)
                uc, vc = np.where(inside, u0, 0).astype(np.int64), np.where(inside, v0, 0).astype(np.int64)
                r = z / d                                            # 1 / dj
                br = np.abs(r) * (2 * dY / np.abs(z) + 4 * U)
                for dv_, du_ in ((0, 0), (0, 1), (1, 0), (1, 1)):
                    c = disps[j][vc + dv_, uc + du_].astype(f64)
                    unsure |= inside & (d != 0) & (np.abs(np.abs(r - 1.0 / c) - float(thresh[b])) <= br)
                out[b] |= unsure
    return out.reshape(len(ix), H, W)


@pytest.mark.parametrize("shape", SHAPES)
def test_depth_filter_counts_vs_reference(lgu, refs, shape):
    """Counts equal to the no-FMA build's everywhere, to the contracting build's except on pixels where a neighbour test
    is within the rounding bound of its threshold (_depth_filter_unsure); the neighbour sets are cut off at both ends of
    the buffer."""
    nofma, fma = refs
    H, W = shape
    N = 14
    poses, disps, intr = TG.scene(83 + H, N=N, H=H, W=W, step=0.05, angle=0.02, bad=0.08)
    ix = np.array([0, 1, 2, 6, N - 5, N - 3, N - 1], np.int64)
    thresh = np.random.default_rng(H).uniform(0.005, 0.5, len(ix)).astype(f32)
    args = [dev(poses), dev(disps), dev(intr), dev(ix), dev(thresh)]
    got = host(lgu.geom.depth_filter(*args))
    assert np.array_equal(got, host(nofma.depth_filter(*args)))
    assert got.max() >= 2 and (got == 0).any()
    fc = host(fma.depth_filter(*args))
    unsure = _depth_filter_unsure(poses, disps, intr, ix, thresh)
    differ = got != fc
    assert not (differ & ~unsure).any(), int((differ & ~unsure).sum())
    report("depth_filter %dx%d vs contracting build" % shape, pixels=got.size, unsure=int(unsure.sum()),
           differing=int(differ.sum()))


def _fd_contraction_bound(poses, disps, intr, i, j, beta):
    """For pair (i, j): None when a depth test (> 0.25) can flip between the builds; otherwise how far the contracting
    build's flow terms can move the pair's mean: sum over counted terms of weight * (bound on du + bound on dv + 6 2^-24
    (|flow| + u + v)), over the valid weight."""
    H, W = disps.shape[1:]
    X, u, v = _pixels64(H, W, intr)
    fx, fy, cx, cy = np.asarray(intr, f64)
    d = disps[i].ravel().astype(f64)
    t, q, m0 = _rel64(poses, i, j)
    wb = float(f32(beta))
    err = val = 0.0
    for qq, w in ((q, wb), (np.array([0.0, 0.0, 0.0, 1.0]), float(f32(1) - f32(wb)))):   # full, translation only
        Y, dY = _transform64(t, qq, m0, X, d)
        z = Y[:, 2]
        if ((np.abs(z - 0.25) <= dY) | (np.abs(z) <= 4 * dY)).any():
            return None
        ok = z > 0.25
        with np.errstate(divide="ignore", invalid="ignore"):
            du, dv = fx * Y[:, 0] / z + cx - u, fy * Y[:, 1] / z + cy - v
            e = _project_bound(fx, cx, Y[:, 0], z, dY) + _project_bound(fy, cy, Y[:, 1], z, dY) + 6 * U * (np.hypot(du, dv) + u + v)
        err += w * e[ok].sum()
        val += w * ok.sum()
    return err / val if val else 0.0


@pytest.mark.parametrize("beta", [0.3, 0.7])
@pytest.mark.parametrize("shape", SHAPES)
def test_frame_distance_vs_reference(lgu, refs, shape, beta):
    """All ordered pairs, i.e. both directions.  tests/test_geom.py's bound: this build's three float32 sums are within
    1.8e-6 of their exact values (relative); the reference's, 256 threads of <= 2 ceil(HW / 256) = 38 terms each and an
    8-level tree, within 46 * 2^-24 = 2.7e-6; so the two means differ by < 1e-5 relative, and each is within 1e-5 of the
    float64 restatement.  The 1000 branch agrees except where the ratio is within 1e-5 of 0.75.  Against the contracting
    build the per-pixel flow terms move as well (_fd_contraction_bound); pairs with a depth test within the bound of
    0.25 are left out."""
    nofma, fma = refs
    H, W = shape
    poses, disps, intr = TG.scene(97 + W, N=8, H=H, W=W, step=0.3, angle=0.2, bad=0.1)
    disps[3] = -np.abs(disps[3]) - 20           # some pairs out of frame 3 fall below the 0.75 ratio: 1000
    ii, jj = TG.all_pairs(len(poses))
    args = [dev(poses), dev(disps), dev(intr), dev(ii), dev(jj)]
    got = host(lgu.geom.frame_distance(*args, beta)).astype(f64)
    want, ratio = G.frame_distance(poses, disps, intr, ii, jj, beta)
    sure = np.abs(ratio - 0.75) > 1e-5
    assert (want[sure] == 1000).any() and (want[sure] != 1000).any()
    r0 = host(nofma.frame_distance(*args, beta)).astype(f64)
    TG._fd_check(got, want, ratio)
    TG._fd_check(r0, want, ratio)
    assert ((got[sure] == 1000) == (r0[sure] == 1000)).all()
    far = sure & (r0 != 1000)
    assert (np.abs(got[far] - r0[far]) <= 1e-5 * np.abs(r0[far])).all()
    far &= r0 != 0                                   # (ii == jj can give exactly 0)
    r1 = host(fma.frame_distance(*args, beta)).astype(f64)
    skipped, checked = 0, 0
    for k, (i, j) in enumerate(zip(ii, jj)):
        b = _fd_contraction_bound(poses, disps, intr, int(i), int(j), beta) if sure[k] else None
        if b is None:
            skipped += 1
            continue
        checked += 1
        assert (got[k] == 1000) == (r1[k] == 1000), k
        if got[k] != 1000:
            assert abs(got[k] - r1[k]) <= 1e-5 * abs(r1[k]) + b, (k, got[k], r1[k], b)
    assert checked >= len(ii) // 2
    report("frame_distance %dx%d beta %.1f" % (H, W, beta), pairs=len(ii),
           max_rel_vs_nofma="%.3g" % float(np.max(np.abs(got[far] - r0[far]) / np.abs(r0[far]))), fma_pairs_skipped=skipped)


# ---- bundle adjustment kernels -------------------------------------------------------------------------------------
def ba_scene(seed, H, W, N=8, rotate=True):
    """tests/test_ba.py's synthetic scene, perturbed (poses from frame 1, depths), with 5 % zero or negative disparities,
    noisy targets (non-zero residuals), random weights, two stereo edges (ii == jj) and, with `rotate`, the last frame
    turned by 2.6 rad (its edges see most points behind the camera)."""
    rng, intr, poses, disps, ii, jj, targets = TB.scene(seed, N=N, H=H, W=W, span=2)
    p, d = TB.perturb(rng, poses, disps, 1)
    m = rng.random(d.shape) < 0.05
    d[m] = np.where(rng.random(int(m.sum())) < 0.5, 0.0, -rng.random(int(m.sum()))).astype(f32)
    if rotate:
        p[N - 1, 3:] = _rotation(2.6, [0.6, 0.7, -0.4])
    ii = np.concatenate([ii, [1, 3]]).astype(np.int64)
    jj = np.concatenate([jj, [1, 3]]).astype(np.int64)
    targets = np.concatenate([targets, targets[:2] + 0.3], 0)
    targets = (targets + rng.standard_normal(targets.shape)).astype(f32)
    weights = (0.1 + rng.random(targets.shape)).astype(f32)
    return intr, p, d, ii, jj, targets, weights


def lgu_build(lgu, targets, weights, poses, disps, intr, ii, jj):
    """lgu_ba_build_f32 -> [Hs, vs, Eii, Eij, Cii, wi] on the device."""
    E, (H, W) = len(ii), disps.shape[1:]
    lib = lgu._lib.load()
    outs = [torch.empty(s, device="cuda") for s in ((4, E, 6, 6), (2, E, 6), (E, 6, H * W), (E, 6, H * W), (E, H * W), (E, H * W))]
    scratch = torch.empty(E * lib.lgu_ba_build_slices(E) * 90, device="cuda")
    ins = [dev(a) for a in (targets, weights, poses, disps, intr, ii, jj)]
    assert lib.lgu_ba_build_f32(*[vp(a) for a in ins + outs + [scratch]], E, H, W, stream()) == 0
    torch.cuda.synchronize()
    return outs


def _ba_magnitudes(targets, weights, poses, disps, intr, ii, jj):
    """Per edge, float64, over the pixels with depth >= 0.2 (MIN_DEPTH 0.25 with a margin): sw = sum of the weights
    .001 w, swr2 = sum of .001 w r^2, R = the largest |target| + |f x / z| + |c| (what enters a residual), |t_ij|; and
    `unsure`, whether some pixel's depth lies within dY of MIN_DEPTH (its depth test may flip between the builds)."""
    E, (H, W) = len(ii), disps.shape[1:]
    X, _, _ = _pixels64(H, W, intr)
    fx, fy, cx, cy = np.asarray(intr, f64)
    mag = np.zeros((E, 4))
    unsure = np.zeros(E, bool)
    for e, (i, j) in enumerate(zip(ii, jj)):
        t, q, m0 = _rel64(poses, i, j, stereo=(i == j))
        Y, dY = _transform64(t, q, m0, X, disps[i].ravel().astype(f64))
        z = Y[:, 2]
        unsure[e] = (np.abs(z - 0.25) <= dY).any()
        ok = z >= 0.2
        zz = np.where(ok, z, 1.0)
        pu, pv = fx * Y[:, 0] / zz + cx, fy * Y[:, 1] / zz + cy
        w = 0.001 * weights[e].reshape(2, -1).astype(f64)
        tg = targets[e].reshape(2, -1).astype(f64)
        r2 = w[0] * (tg[0] - pu) ** 2 + w[1] * (tg[1] - pv) ** 2
        R = np.maximum(np.abs(tg[0]) + np.abs(pu - cx) + abs(cx), np.abs(tg[1]) + np.abs(pv - cy) + abs(cy))
        mag[e] = (w.sum(0)[ok].sum(), r2[ok].sum(), R[ok].max() if ok.any() else 0.0, np.linalg.norm(t))
    return mag, unsure


@pytest.mark.parametrize("shape", SHAPES)
def test_ba_build_vs_reference(lgu, refs, shape):
    """projective_transform_kernel (:176-425) against lgu_ba_build_f32, 8 frames with stereo edges, zero / negative
    disparities and points behind the camera.

    No-FMA build: Eii, Eij, Cii, wi bit for bit.  Hs, vs (256 threads x 2 ceil(HW/256) terms + an 8-level tree there;
    <= 8 slices x that + 9 wave / slice steps here; n = 2 ceil(HW/256) + 17) within 2 (n + 2) 2^-24 S, with S bounding
    sum|terms| by Cauchy-Schwarz: sum w |J_n J_m| <= trace of the edge's 12 x 12 Hessian T; sum w |r J_n| <= sqrt(swr2 T).
    Contracting build: each Jacobian entry moves by <= 32 (1 + |t_ij|) 2^-24 |J| (<= 32 operations on magnitudes the
    rotation and |t_ij| scale) and each residual by 32 * 2^-24 R; Hs gains 64 (1 + |t|) 2^-24 T, vs that times sqrt(swr2 T)
    plus 64 * 2^-24 R sqrt(sw T); the per-pixel outputs agree to 2^-12 of the edge's largest entry (<= 40 operations with
    the residual's cancellation R / |r| <= 50 here: 2 * 40 * 50 * 2^-24 < 2^-12).  Edges with a pixel whose depth test can
    flip are left out of the contracting comparison."""
    nofma, fma = refs
    H, W = shape
    intr, p, d, ii, jj, tg, wt = ba_scene(113 + W, H, W)
    E, HW = len(ii), H * W
    got = [host(t) for t in lgu_build(lgu, tg, wt, p, d, intr, ii, jj)]
    args = [dev(a) for a in (tg, wt, p, d, intr, ii, jj)]
    r0 = [host(t) for t in nofma.projective_transform(*args)]
    r1 = [host(t) for t in fma.projective_transform(*args)]
    names = ("Hs", "vs", "Eii", "Eij", "Cii", "wi")
    for k in range(2, 6):
        assert same_bits(got[k], r0[k]), (names[k], int((got[k] != r0[k]).sum()))
    assert (got[4] == 0).any() and (got[4] != 0).any()          # pixels behind the camera and in front of it
    mag, unsure = _ba_magnitudes(tg, wt, p, d, intr, ii, jj)
    n = 2 * -(-HW // 256) + 17
    H0 = r0[0].astype(f64)
    T = (np.einsum("eii->e", H0[0]) + np.einsum("eii->e", H0[3])) * 1.001
    worst = {}
    for e in range(E):
        sw, swr2, R, tn = mag[e]
        sv = np.sqrt(swr2 * T[e])
        bH, bv = 2 * (n + 2) * U * T[e], 2 * (n + 2) * U * sv
        dH, dv = np.abs(got[0][:, e] - r0[0][:, e]).max(), np.abs(got[1][:, e] - r0[1][:, e]).max()
        assert dH <= bH and dv <= bv, (e, dH, bH, dv, bv)
        if ii[e] == jj[e]:                                          # stereo: the pose blocks carry no weight
            assert not got[0][:, e].any() and not got[1][:, e].any() and not r1[0][:, e].any()
        if unsure[e]:
            continue
        bH1 = bH + 64 * (1 + tn) * U * T[e]
        bv1 = bv + 64 * (1 + tn) * U * sv + 64 * U * R * np.sqrt(sw * T[e])
        assert np.abs(got[0][:, e] - r1[0][:, e]).max() <= bH1, e
        assert np.abs(got[1][:, e] - r1[1][:, e]).max() <= bv1, e
        for k in range(2, 6):
            scale = float(np.abs(r1[k][e]).max())
            diff = float(np.abs(got[k][e].astype(f64) - r1[k][e]).max())
            assert diff <= 2.0 ** -12 * scale, (names[k], e, diff, scale)
            worst[names[k]] = max(worst.get(names[k], 0.0), diff / scale if scale else 0.0)
    report("BA build %dx%d" % shape, edges=E, fma_edges_skipped=int(unsure.sum()),
           **{"fma_rel_" + k: "%.2g" % v for k, v in worst.items()})


@pytest.mark.parametrize("shape", SHAPES)
def test_schur_kernels_and_accum_vs_reference(lgu, refs, shape):
    """accum_cuda, EEt6x6, Ev6x1 (sums: within 2 (n + 2) 2^-24 sum|terms| of each other for both builds, n the longer
    chain: the number of summed rows for accum, ceil(HW / 256) + 9 for the block reductions) and EvT6x1 (six products in
    the same order: bit for bit against the no-FMA build, within 12 * 2^-24 sum|E x| of the contracting one), on the
    reference's own operands of a window with t0 = 2, as ba_cuda forms them (:1394-1417)."""
    H, W = shape
    HW = H * W
    intr, p, d, ii, jj, tg, wt = ba_scene(131 + W, H, W)
    E = len(ii)
    t0, t1 = 2, len(p)
    P = t1 - t0
    ts = np.arange(t0, t1)
    ii_exp, jj_exp = np.concatenate([ts, ii]), np.concatenate([ts, jj])
    kx, kk = np.unique(ii_exp, return_inverse=True)
    kk = kk.astype(np.int64)
    lib, st = lgu._lib.load(), stream()
    nofma = refs[0]
    _, _, Eii, Eij, Cii, wi = nofma.projective_transform(*[dev(a) for a in (tg, wt, p, d, intr, ii, jj)])
    Ev = Eii.view(E, 6 * HW)
    for data, ix, jx in ((Cii, ii, kx), (wi, ii, kx), (Ev, ii, ts)):      # :1398, :1399, :1402
        got = host(lgu.ba._Accum(lib, ix, jx, "cuda")(data, st))
        a = np.abs(host(data)).astype(f64)
        bound = np.stack([2 * ((ix == f).sum() + 2) * U * a[ix == f].sum(0) for f in jx])
        for ref in refs:
            assert (np.abs(got - host(ref.accum(data, dev(ix), dev(jx)))) <= bound).all()

    C = host(nofma.accum(Cii, dev(ii), dev(kx)))
    Q = (1.0 / (C + f32(0.05))).astype(f32)
    w = host(nofma.accum(wi, dev(ii), dev(kx)))
    Ei = host(nofma.accum(Ev, dev(ii), dev(ts))).reshape(P, 6, HW)
    Eall = np.ascontiguousarray(np.concatenate([Ei, host(Eij)], 0))
    nE = len(Eall)
    _, _, idx = O.schur_pairs(jj_exp, kk, t0, t1)
    nb = len(idx)
    assert nb > nE
    Ed, Qd, wd, idd, kkd = dev(Eall), dev(Q), dev(w), dev(idx), dev(kk)
    S = torch.empty(nb, 6, 6, device="cuda")
    assert lib.lgu_ba_eet_f32(vp(Ed), vp(Qd), vp(idd), vp(S), nb, HW, st) == 0
    v = torch.empty(nE, 6, device="cuda")
    assert lib.lgu_ba_ev_f32(vp(Ed), vp(Qd), vp(wd), vp(kkd), vp(v), nE, HW, st) == 0
    S, v = host(S), host(v)
    n = -(-HW // 256) + 9
    A = np.abs(Eall).astype(f64)
    bS = 2 * (n + 2) * U * np.einsum("bnk,bk,bmk->bnm", A[idx[:, 0]], Q[idx[:, 2]].astype(f64), A[idx[:, 1]], optimize=True)
    bv = 2 * (n + 2) * U * np.einsum("enk,ek->en", A, np.abs(Q[kk] * w[kk]).astype(f64))
    for ref in refs:
        assert (np.abs(S - host(ref.eet(Ed, Qd, idd))) <= bS).all()
        assert (np.abs(v - host(ref.ev(Ed, Qd, wd, dev(kk[:, None])))) <= bv).all()

    x = np.random.default_rng(W).standard_normal((P, 6)).astype(f32)
    pidx = (jj_exp - t0).astype(np.int64)                 # pose indices <= 0 included: skipped (:1105, sic)
    xd, pd_ = dev(x), dev(pidx)
    dw = torch.empty(nE, HW, device="cuda")
    assert lib.lgu_ba_evt_f32(vp(Ed), vp(xd), vp(pd_), vp(dw), nE, HW, P, st) == 0
    dw = host(dw)
    assert same_bits(dw, host(nofma.evt(Ed, xd, pd_)))
    live = (pidx > 0) & (pidx < P)
    assert live.any() and (~live).any() and not dw[~live].any()
    bw = 12 * U * np.einsum("enk,en->ek", A, np.abs(x[np.clip(pidx, 0, P - 1)]).astype(f64))
    assert (np.abs(dw - host(refs[1].evt(Ed, xd, pd_))) <= bw).all()


def test_pose_and_disparity_retraction_vs_reference(lgu, refs):
    """pose_retr_kernel (:877-931) on updates through every branch of expSE3: zero, theta^2 below 1e-8 and next to that
    switch, theta below 1e-4, a rotation of 2.7 rad, a large translation.  Bit for bit against the no-FMA build; within
    2^-17 (1 + |pose| + |update|) of the contracting one (<= 30 fp32 operations per entry on magnitudes that sum
    bounds: 2 * 30 * 2^-24 < 2^-17).  disp_retr_kernel (:933-946, one addition) bit for bit against both."""
    rng = np.random.default_rng(5)
    N, t0 = 12, 2
    poses = np.zeros((N, 7), f32)
    for k in range(N):
        poses[k, :3] = rng.standard_normal(3)
        poses[k, 3:] = _rotation(rng.uniform(0, 3), rng.standard_normal(3))
    dx = (0.1 * rng.standard_normal((N - t0, 6))).astype(f32)
    dx[0] = 0                                      # no update
    dx[1, 3:] = [1e-4, 2.1306533e-08, 0]           # theta^2 == float(1e-8) < 1e-8: the series (:119, a double literal)
    dx[2, 3:] = [5e-5, 0, 0]                       # theta^2 < 1e-8
    dx[3, 3:] = [3e-5, -2e-5, 6e-5]                # theta < 1e-4: no translation series
    dx[4, 3:] = [2.0, -1.0, 1.5]                   # 2.7 rad
    dx[5, :3] = [5.0, -3.0, 2.0]                   # large translation
    lib, st = lgu._lib.load(), stream()
    dxd = dev(dx)
    pg = dev(poses)
    assert lib.lgu_ba_pose_retr_f32(vp(pg), vp(dxd), t0, N, st) == 0
    pg = host(pg)
    assert same_bits(pg[:t0], poses[:t0])
    pr = [dev(poses) for _ in refs]
    for ref, p_ in zip(refs, pr):
        ref.pose_retr(p_, dxd, t0, N)
    assert same_bits(pg, host(pr[0]))
    m = 1 + np.abs(poses.astype(f64)).sum(1, keepdims=True) + np.abs(np.concatenate([np.zeros((t0, 6)), dx], 0)).sum(1, keepdims=True)
    assert (np.abs(pg - host(pr[1])) <= 2.0 ** -17 * m).all()
    H, W = 7, 13
    disps = rng.standard_normal((N, H, W)).astype(f32)
    inds = np.array([0, 3, 4, 11], np.int64)
    dz = rng.standard_normal((len(inds), H * W)).astype(f32)
    dg, dzd, idd = dev(disps), dev(dz), dev(inds)
    assert lib.lgu_ba_disp_retr_f32(vp(dg), vp(dzd), vp(idd), len(inds), H * W, st) == 0
    for ref in refs:
        dr = dev(disps)
        ref.disp_retr(dr, dzd, idd)
        assert same_bits(host(dg), host(dr))


def ref_ba(ref, poses, disps, intr, sens, targets, weights, eta, ii, jj, t0, t1, iterations, lm, ep, motion_only):
    """ba_cuda (:1314-1434) composed from the reference's kernels through the binding, with its Eigen host part (the
    SparseBlock assembly and SimplicialLLT solve) from oracle/ba_oracle.py (float64, numpy Cholesky).  Device tensors;
    poses and disps are updated in place.  Returns (dx, dz)."""
    ii_h, jj_h = host(ii), host(jj)
    E = len(ii_h)
    H, W = disps.shape[1:]
    HW = H * W
    P = t1 - t0
    ts_h = np.arange(t0, t1)
    ii_exp_h, jj_exp_h = np.concatenate([ts_h, ii_h]), np.concatenate([ts_h, jj_h])
    kx_h, kk_h = np.unique(ii_exp_h, return_inverse=True)                          # :1340-1344
    ts, ii_exp, kx, kk = dev(ts_h), dev(ii_exp_h), dev(kx_h), dev(kk_h.astype(np.int64)[:, None])
    pi, pj, idx = O.schur_pairs(jj_exp_h, kk_h, t0, t1)
    idx, jpose = dev(idx), dev(jj_exp_h - t0)
    dx = dz = None
    for _ in range(iterations):
        Hs, vs, Eii, Eij, Cii, wi = ref.projective_transform(targets, weights, poses, disps, intr, ii, jj)
        A, b = O.pose_system(host(Hs), host(vs), ii_h, jj_h, t0, P)                  # :1375-1383
        if not motion_only:
            m = (sens[kx] > 0).float().view(-1, HW)                                   # :1394-1400
            C = ref.accum(Cii, ii, kx) + m * 0.05 + (1 - m) * eta.view(-1, HW)
            w = ref.accum(wi, ii, kx) - m * 0.05 * (disps[kx] - sens[kx]).view(-1, HW)
            Q = 1.0 / C
            Ei = ref.accum(Eii.view(E, 6 * HW), ii, ts).view(P, 6, HW)
            Eall = torch.cat([Ei, Eij], 0).contiguous()                               # :1401-1405
            As, bs = O.schur_system(host(ref.eet(Eall, Q, idx)), host(ref.ev(Eall, Q, w, kk)), pi, pj, jj_exp_h - t0, P)
            A, b = A - As, b - bs
        dx = dev(O.solve_block(A, b, lm, ep).reshape(P, 6).astype(f32))
        if not motion_only:
            dz = Q * (w - ref.accum(ref.evt(Eall, dx, jpose), ii_exp, kx))           # :1408-1417
        ref.pose_retr(poses, dx, t0, t1)
        if not motion_only:
            ref.disp_retr(disps, dz, kx)
    return dx, dz


@pytest.mark.parametrize("iterations", [1, 3])
@pytest.mark.parametrize("motion_only", [False, True])
def test_ba_step_composed_from_reference_kernels(lgu, refs, motion_only, iterations):
    """lgu_slam_amd.ba.ba against ba_cuda composed from the reference's own kernels (ref_ba): 48x64, 8 frames, window
    t0 = 2, stereo edges, zero / negative disparities, sensor depth on about half of the pixels.  Both sides sum Hs, vs
    and the Schur products in float32, in different orders, and solve in float64: dx, dz and the moves of the poses and
    disparities agree to 2e-4 of the update after one iteration, 1e-3 after three."""
    H, W = 48, 64
    intr, p, d, ii, jj, tg, wt = ba_scene(151, H, W, rotate=False)
    t0, t1 = 2, len(p)
    rng = np.random.default_rng(17)
    sens = (d * (rng.random(d.shape) > 0.5)).astype(f32)
    K = len(np.unique(np.concatenate([np.arange(t0, t1), ii])))
    eta = (1e-3 * (1 + rng.random((K, H, W)))).astype(f32)
    args = [dev(a) for a in (intr, sens, tg, wt, eta, ii, jj)]
    pr, dr = dev(p), dev(d)
    dxr, dzr = ref_ba(refs[0], pr, dr, *args, t0, t1, iterations, 1e-4, 0.1, motion_only)
    pg, dg = dev(p), dev(d)
    dxg, dzg = lgu.ba.ba(pg, dg, *args, t0, t1, iterations, 1e-4, 0.1, motion_only)
    tol = 2e-4 if iterations == 1 else 1e-3
    dxr, dxg, pr, pg, dr, dg = [host(t) for t in (dxr, dxg, pr, pg, dr, dg)]
    rel = {"dx": np.abs(dxg - dxr).max() / np.abs(dxr).max(), "poses": np.abs(pg - pr).max() / np.abs(pr - p).max()}
    assert np.abs(dxr).max() > 1e-4
    assert np.abs(dxg - dxr).max() <= tol * np.abs(dxr).max() + 1e-7
    assert np.abs(pg - pr).max() <= tol * np.abs(pr - p).max() + 1e-6
    assert same_bits(pg[:t0], p[:t0]) and same_bits(pr[:t0], p[:t0])
    if motion_only:
        assert dzg is None and dzr is None and same_bits(dg, d) and same_bits(dr, d)
    else:
        dzr, dzg = host(dzr), host(dzg)
        rel["dz"] = np.abs(dzg - dzr).max() / np.abs(dzr).max()
        rel["disps"] = np.abs(dg - dr).max() / np.abs(dr - d).max()
        assert dzg.shape == dzr.shape and np.abs(dzg - dzr).max() <= tol * np.abs(dzr).max() + 1e-7
        assert np.abs(dg - dr).max() <= tol * np.abs(dr - d).max() + 1e-6
    report("BA step motion_only=%s iterations=%d" % (motion_only, iterations), **{k: "%.2g" % v for k, v in rel.items()})
