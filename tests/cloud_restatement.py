"""A float64 numpy restatement of the map export (lgu_slam_amd.cloud.point_cloud, csrc/cloud.hip): the count of
depth_filter, the mask, the inverse pose, the back-projection, the colour and the order of the rows, written from the
formulas (reference src/droid_kernels.cu:661-851, droid_slam/visualization.py:92-129) and independent of the library.

poses (Np,7) = t, q(xyzw) world-to-camera; disps (Nd,ht,wd); intrinsics fx, fy, cx, cy; ix (num,); thresh (num,).
"""
import numpy as np

NEIGHBOURS = (-1, -2, -3, 3, 4, 5)


def rotate(q, X):
    """R(q) X for a unit quaternion q = (x, y, z, w); X (...,3)."""
    v, w = np.asarray(q[:3], np.float64), float(q[3])
    uv = 2.0 * np.cross(v, X)
    return X + w * uv + np.cross(v, uv)


def qmul(a, b):
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx,
                     aw * bz + ax * by - ay * bx + az * bw, aw * bw - ax * bx - ay * by - az * bz])


def inverse(pose):
    """(t, q)^-1 = (-R(q)^-1 t, conj(q))."""
    t, q = np.asarray(pose[:3], np.float64), np.asarray(pose[3:], np.float64)
    qi = np.array([-q[0], -q[1], -q[2], q[3]])
    return np.concatenate([-rotate(qi, t), qi])


def relative(pi, pj):
    """T_j T_i^-1 as (t, q)."""
    ii = inverse(pi)
    q = qmul(np.asarray(pj[3:], np.float64), ii[3:])
    return np.concatenate([rotate(pj[3:], ii[:3]) + np.asarray(pj[:3], np.float64), q])


def rays(ht, wd, intrinsics):
    fx, fy, cx, cy = [float(v) for v in intrinsics[:4]]
    v, u = np.meshgrid(np.arange(ht, dtype=np.float64), np.arange(wd, dtype=np.float64), indexing="ij")
    return np.stack([(u - cx) / fx, (v - cy) / fy, np.ones_like(u)], -1)


def counts(poses, disps, intrinsics, ix, thresh):
    """(num,ht,wd) int: for every pixel of frame ix[b], the neighbours ix-1, ix-2, ix-3, ix+3, ix+4, ix+5 inside the buffer in
    which it projects with floor(u) in [0, wd-1), floor(v) in [0, ht-1) and |1/d_proj - 1/d_corner| < thresh[b] for one of the
    four corners.  An ix[b] outside [0, min(Np, Nd)) counts 0."""
    poses, disps = np.asarray(poses, np.float64), np.asarray(disps, np.float64)
    fx, fy, cx, cy = [float(v) for v in intrinsics[:4]]
    Nd, ht, wd = disps.shape
    nvalid = min(len(poses), Nd)
    X = rays(ht, wd, intrinsics)
    out = np.zeros((len(ix), ht, wd), np.int64)
    for b, a in enumerate(int(v) for v in ix):
        if not 0 <= a < nvalid:
            continue
        d = disps[a]
        for n in NEIGHBOURS:
            j = a + n
            if not 0 <= j < nvalid:
                continue
            T = relative(poses[a], poses[j])
            with np.errstate(all="ignore"):
                Y = rotate(T[3:], X) + d[..., None] * T[:3]
                uj, vj, dj = fx * (Y[..., 0] / Y[..., 2]) + cx, fy * (Y[..., 1] / Y[..., 2]) + cy, d / Y[..., 2]
                u0 = np.nan_to_num(np.floor(uj), nan=0.0, posinf=2.0 ** 31, neginf=-2.0 ** 31)
                v0 = np.nan_to_num(np.floor(vj), nan=0.0, posinf=2.0 ** 31, neginf=-2.0 ** 31)
                inside = (u0 >= 0) & (v0 >= 0) & (u0 < wd - 1) & (v0 < ht - 1)
                uc, vc = np.where(inside, u0, 0).astype(np.int64), np.where(inside, v0, 0).astype(np.int64)
                hit = np.zeros_like(inside)
                for dv, du in ((0, 0), (0, 1), (1, 0), (1, 1)):
                    corner = disps[j][np.minimum(vc + dv, ht - 1), np.minimum(uc + du, wd - 1)]
                    hit |= np.abs(1.0 / dj - 1.0 / corner) < float(thresh[b])
            out[b] += inside & hit
    return out


def point_cloud(poses, disps, intrinsics, ix, thresh, images=None, min_count=2, disp_ratio=0.5, disp_floor=None, stride=8, phase=3):
    """(points (total,3), colors (total,3) in [0,1] or None, offsets (num+1,) int64), all float64: the kept pixels of the
    entries in ix order, pixels row-major inside an entry."""
    poses, disps = np.asarray(poses, np.float64), np.asarray(disps, np.float64)
    Nd, ht, wd = disps.shape
    cnt = counts(poses, disps, intrinsics, ix, thresh)
    X = rays(ht, wd, intrinsics)
    pts, cols, offsets = [], [], [0]
    for b, a in enumerate(int(v) for v in ix):
        if not 0 <= a < min(len(poses), Nd):
            offsets.append(offsets[-1])
            continue
        d = disps[a]
        floor = float(disp_floor[b]) if disp_floor is not None else disp_ratio * d.mean()
        keep = (cnt[b] >= min_count) & (d > floor)
        T = inverse(poses[a])
        with np.errstate(all="ignore"):
            P = (rotate(T[3:], X) + d[..., None] * T[:3]) / d[..., None]
        pts.append(P[keep])
        if images is not None:
            rgb = np.asarray(images)[a][::-1, phase::stride, phase::stride].transpose(1, 2, 0).astype(np.float64) / 255.0
            cols.append(rgb[keep])
        offsets.append(offsets[-1] + int(keep.sum()))
    points = np.concatenate(pts) if pts else np.zeros((0, 3))
    colors = None if images is None else (np.concatenate(cols) if cols else np.zeros((0, 3)))
    return points, colors, np.asarray(offsets, np.int64)
