"""CPU restatement (numpy, float32) of the reference's geometry kernels frame_distance, projmap, depth_filter and iproj
(src/droid_kernels.cu:427-851).  TEST INFRASTRUCTURE ONLY.

Every per-pixel value is computed in float32 in the reference's operation order (numpy's float32 `/` and sqrt are
correctly rounded, as the kernels' are), so projmap, depth_filter and iproj are held to it bit for bit.
frame_distance's per-pixel terms are exact float32 values too; its sums are taken here in float64 (the kernel and the
reference sum in float32, each in an order of its own).

Rules this restatement encodes on top of the reference's text:
  * a frame index is valid when 0 <= index < min(len(poses), len(disps)) (the reference reads out of bounds
    otherwise): NaN distance, NaN coordinates / channel 2 = 0 / valid 0, a zero depth_filter row, a skipped
    depth_filter neighbour, NaN iproj points for frames without a pose;
  * depth_filter's `static_cast<int>(floor(u))` converts as the hardware does (v_cvt_i32_f32, what the reference gets
    on both vendors): NaN -> 0, values beyond the int range saturate to INT_MIN / INT_MAX (cvt_i32_sat below).
"""
import numpy as np

from oracle.ba_oracle import act_so3, rel_se3

f32 = np.float32
MIN_DEPTH = 0.25                     # droid_kernels.cu:26
NEIGHBOURS = tuple(-n - 1 if n < 3 else n for n in range(6))   # :700 `neigh < 3 ? ix - neigh - 1 : ix + neigh`
INT_MIN, INT_MAX = -2 ** 31, 2 ** 31 - 1


def _intr(intrinsics):
    return [f32(v) for v in np.asarray(intrinsics, dtype=f32)[:4]]


def pixels(ht, wd, intrinsics):
    """u, v, x = (u - cx) / fx, y = (v - cy) / fy for every pixel in row-major order, float32."""
    fx, fy, cx, cy = _intr(intrinsics)
    v, u = np.meshgrid(np.arange(ht, dtype=f32), np.arange(wd, dtype=f32), indexing="ij")
    u, v = u.ravel(), v.ravel()
    return u, v, (u - cx) / fx, (v - cy) / fy


def act_se3(t, q, x, y, d):
    """act_se3(T, (x, y, 1, d))[0:3] (:69-76) for arrays of pixels: act_so3, then + d * t."""
    X = np.stack([x, y, np.ones_like(x)], -1)
    Y = act_so3(np.asarray(q, f32), X)
    return Y + d[:, None] * np.asarray(t, f32)[None]


def _rel(poses, i, j):
    poses = np.asarray(poses, f32)
    return rel_se3(poses[i, :3], poses[i, 3:], poses[j, :3], poses[j, 3:])


def nvalid(poses, disps):
    return min(len(poses), len(disps))


def cvt_i32_sat(a):
    """v_cvt_i32_f32 on float32 values that are integral (floor()ed) or non-finite."""
    a = np.asarray(a, np.float64)
    out = np.zeros(a.shape, np.int64)
    fin = np.isfinite(a)
    out[fin] = np.clip(a[fin], INT_MIN, INT_MAX).astype(np.int64)
    out[np.isposinf(a)] = INT_MAX
    out[np.isneginf(a)] = INT_MIN
    return out                       # NaN stays 0


def frame_distance_terms(poses, disps, intrinsics, i, j):
    """The per-pixel terms of one pair (:594-640): (d_full, ok_full, d_trans, ok_trans), float32 / bool arrays."""
    fx, fy, cx, cy = _intr(intrinsics)
    ht, wd = disps.shape[1:]
    u, v, x, y = pixels(ht, wd, intrinsics)
    tij, qij = _rel(poses, i, j)
    d = np.asarray(disps[i], f32).ravel()
    Y = act_se3(tij, qij, x, y, d)
    du = fx * (Y[:, 0] / Y[:, 2]) + cx - u
    dv = fy * (Y[:, 1] / Y[:, 2]) + cy - v
    d1 = np.sqrt(du * du + dv * dv)
    Z0, Z1, Z2 = x + d * tij[0], y + d * tij[1], f32(1) + d * tij[2]
    du = fx * (Z0 / Z2) + cx - u
    dv = fy * (Z1 / Z2) + cy - v
    d2 = np.sqrt(du * du + dv * dv)
    return d1, Y[:, 2] > MIN_DEPTH, d2, Z2 > MIN_DEPTH


def frame_distance(poses, disps, intrinsics, ii, jj, beta):
    """(dist, ratio) per pair, float64: exact float32 per-pixel terms (w * d products included) summed in float64;
    ratio = valid / (total + 1e-8), dist = 1000 where ratio < 0.75.  NaN for pairs with an invalid index."""
    wb = f32(beta)
    wc = f32(1) - wb
    nv = nvalid(poses, disps)
    npx = disps.shape[1] * disps.shape[2]
    dist = np.full(len(ii), np.nan)
    ratio = np.full(len(ii), np.nan)
    for k, (i, j) in enumerate(zip(ii, jj)):
        if not (0 <= i < nv and 0 <= j < nv):
            continue
        d1, o1, d2, o2 = frame_distance_terms(poses, disps, intrinsics, int(i), int(j))
        total = npx * (float(wb) + float(wc))
        valid = float(wb) * o1.sum() + float(wc) * o2.sum()
        accum = (wb * d1)[o1].astype(np.float64).sum() + (wc * d2)[o2].astype(np.float64).sum()
        ratio[k] = valid / (total + 1e-8)
        dist[k] = 1000.0 if ratio[k] < 0.75 else accum / valid
    return dist, ratio


def projmap(poses, disps, intrinsics, ii, jj):
    fx, fy, cx, cy = _intr(intrinsics)
    num, (ht, wd) = len(ii), disps.shape[1:]
    u, v, x, y = pixels(ht, wd, intrinsics)
    nv = nvalid(poses, disps)
    coords = np.zeros((num, ht * wd, 3), f32)
    valid = np.zeros((num, ht * wd, 1), f32)
    for k, (i, j) in enumerate(zip(ii, jj)):
        if not (0 <= i < nv and 0 <= j < nv):
            coords[k, :, :2] = np.nan
            continue
        tij, qij = _rel(poses, int(i), int(j))
        Y = act_se3(tij, qij, x, y, np.asarray(disps[i], f32).ravel())
        near = Y[:, 2].astype(np.float64) > 0.01            # :507, a double literal
        with np.errstate(divide="ignore", invalid="ignore"):
            pu = fx * (Y[:, 0] / Y[:, 2]) + cx
            pv = fy * (Y[:, 1] / Y[:, 2]) + cy
        coords[k, :, 0] = np.where(near, pu, u)
        coords[k, :, 1] = np.where(near, pv, v)
        valid[k, :, 0] = (Y[:, 2] > MIN_DEPTH).astype(f32)
    return coords.reshape(num, ht, wd, 3), valid.reshape(num, ht, wd, 1)


def depth_filter_hits(poses, disps, intrinsics, i, j, thresh):
    """For every pixel of frame i: does neighbour j count (:725-772)?  Bool array (ht*wd,)."""
    fx, fy, cx, cy = _intr(intrinsics)
    ht, wd = disps.shape[1:]
    u, v, x, y = pixels(ht, wd, intrinsics)
    tij, qij = _rel(poses, i, j)
    di = np.asarray(disps[i], f32).ravel()
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        Y = act_se3(tij, qij, x, y, di)
        uj = fx * (Y[:, 0] / Y[:, 2]) + cx
        vj = fy * (Y[:, 1] / Y[:, 2]) + cy
        dj = di / Y[:, 2]
        u0, v0 = cvt_i32_sat(np.floor(uj)), cvt_i32_sat(np.floor(vj))
        inside = (u0 >= 0) & (v0 >= 0) & (u0 < wd - 1) & (v0 < ht - 1)
        D = np.asarray(disps[j], f32)
        uc, vc = np.where(inside, u0, 0), np.where(inside, v0, 0)     # corners read only where inside (clipped below)
        r = 1.0 / dj.astype(np.float64)
        t = np.float64(f32(thresh))
        hit = np.zeros(ht * wd, bool)
        for dv_, du_ in ((0, 0), (0, 1), (1, 0), (1, 1)):
            c = D[np.minimum(vc + dv_, ht - 1), np.minimum(uc + du_, wd - 1)]
            hit |= np.abs(r - 1.0 / c.astype(np.float64)) < t
    return inside & hit


def depth_filter(poses, disps, intrinsics, ix, thresh):
    num, (nd, ht, wd) = len(ix), disps.shape
    nv = nvalid(poses, disps)
    counter = np.zeros((num, ht * wd), f32)
    for b, i in enumerate(ix):
        if not (0 <= i < nv):
            continue
        for n in NEIGHBOURS:
            j = int(i) + n
            if 0 <= j < nv:
                counter[b] += depth_filter_hits(poses, disps, intrinsics, int(i), j, thresh[b])
    return counter.reshape(num, ht, wd)


def iproj(poses, disps, intrinsics):
    nd, ht, wd = disps.shape
    u, v, x, y = pixels(ht, wd, intrinsics)
    poses = np.asarray(poses, f32)
    out = np.full((nd, ht * wd, 3), np.nan, f32)
    with np.errstate(divide="ignore", invalid="ignore"):
        for n in range(min(nd, len(poses))):
            d = np.asarray(disps[n], f32).ravel()
            out[n] = act_se3(poses[n, :3], poses[n, 3:], x, y, d) / d[:, None]
    return out.reshape(nd, ht, wd, 3)
