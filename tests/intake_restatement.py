"""The frame intake restated in numpy: what lgu_slam_amd.intake (csrc/intake.hip) is held to.

Float64 coordinates with every operation rounded on its own (numpy evaluates one ufunc at a time, nothing is fused), integer
pixel arithmetic.  It follows OpenCV's published fixed-point scheme for 8-bit images (initUndistortRectifyMap + remap with
INTER_LINEAR: coordinates quantised to 1/32 pixel, 5-bit weights per axis, a rounding shift by 10; resize with INTER_LINEAR:
half-pixel centres, 11-bit weights per axis, a rounding shift by 22) as far as it is known here; OpenCV itself cannot be run
here, so this file, not OpenCV, is the definition.

    camera(K, dist, R, Kn)            the 22 doubles of one camera: fx fy cx cy | fx' fy' cx' cy' | R^-1 row-major | k1 k2 p1 p2 k3
    rectify_coords(cam, h, w)         stage 1's map: (mx, my) float64
    rectify(raw, cam)                 stage 1: (image, fragile)
    resize(img, h1, w1)               stage 2
    frame(raw, cams, resize, crop)    all stages: image (N,3,H,W) uint8 BGR planar, fragile (N,H,W)
    normalize(image, mean, std)       motion_filter.py:56-57 as the device evaluates it: (1,N,3,H,W) float32 RGB
    sensor_disparity(raw, scale, size, crop)    depth_video.py:64-66 behind F.interpolate and the crop

`fragile` marks the pixels a comparison may leave out: one of the stage-1 coordinates that contribute to it has 32 m + 0.5
within 1e-6 of an integer, so a last-bit difference in the map could move the 1/32-pixel cell.
"""
import numpy as np

Q_LIMIT = float(1 << 30)
FRAGILE_WINDOW = 1e-6


def camera(K, dist=None, R=None, Kn=None):
    """K, Kn: (fx, fy, cx, cy); dist: 4 or 5 coefficients k1 k2 p1 p2 [k3]; R: 3x3.  cv2.undistort is R = I, Kn = K."""
    K = np.asarray(K, dtype=np.float64).reshape(4)
    Kn = K if Kn is None else np.asarray(Kn, dtype=np.float64).reshape(4)
    d = np.zeros(5)
    if dist is not None:
        dist = np.asarray(dist, dtype=np.float64).reshape(-1)
        assert dist.size in (4, 5)
        d[:dist.size] = dist
    iR = np.eye(3) if R is None else np.linalg.inv(np.asarray(R, dtype=np.float64).reshape(3, 3))
    return np.concatenate([K, Kn, iR.reshape(9), d])


def rectify_coords(cam, h, w):
    k, kn, ir, d = cam[0:4], cam[4:8], cam[8:17], cam[17:22]
    u = np.arange(w, dtype=np.float64)[None, :].repeat(h, 0)
    v = np.arange(h, dtype=np.float64)[:, None].repeat(w, 1)
    with np.errstate(all="ignore"):
        x = (u - kn[2]) / kn[0]
        y = (v - kn[3]) / kn[1]
        X = (ir[0] * x + ir[1] * y) + ir[2]
        Y = (ir[3] * x + ir[4] * y) + ir[5]
        W = (ir[6] * x + ir[7] * y) + ir[8]
        x = X / W
        y = Y / W
        x2 = x * x
        y2 = y * y
        r2 = x2 + y2
        rad = 1.0 + r2 * (d[0] + r2 * (d[1] + r2 * d[4]))
        t = 2.0 * (x * y)
        xd = (x * rad + d[2] * t) + d[3] * (r2 + 2.0 * x2)
        yd = (y * rad + d[2] * (r2 + 2.0 * y2)) + d[3] * t
        mx = xd * k[0] + k[2]
        my = yd * k[1] + k[3]
    return mx, my


def quantise(m):
    """floor(32 m + 0.5), clamped to [-2^30, 2^30]; a NaN becomes -2^30."""
    with np.errstate(all="ignore"):
        t = np.floor(32.0 * m + 0.5)
        t = np.where(t >= -Q_LIMIT, t, -Q_LIMIT)
        t = np.where(t <= Q_LIMIT, t, Q_LIMIT)
    return t.astype(np.int64)


def _near_cell_edge(m, n):
    """32 m + 0.5 lies within the window of an integer, for a coordinate whose taps can touch the frame [0, n)."""
    with np.errstate(all="ignore"):
        t = 32.0 * m + 0.5
        near = np.abs(t - np.round(t)) < FRAGILE_WINDOW
        return near & (m > -2.0) & (m < n + 1.0)


def _taps(raw, iy, ix):
    """raw (h,w,3) at integer positions, 0 outside the frame, as int64."""
    h, w = raw.shape[:2]
    ok = (iy >= 0) & (iy < h) & (ix >= 0) & (ix < w)
    out = raw[np.clip(iy, 0, h - 1), np.clip(ix, 0, w - 1)].astype(np.int64)
    return out * ok[..., None]


def rectify(raw, cam):
    """Stage 1 of one frame raw (h,w,3) uint8: (image (h,w,3) uint8, fragile (h,w) bool)."""
    h, w = raw.shape[:2]
    mx, my = rectify_coords(cam, h, w)
    qx, qy = quantise(mx), quantise(my)
    ix, iy = qx >> 5, qy >> 5
    ax, ay = (qx & 31)[..., None], (qy & 31)[..., None]
    acc = (_taps(raw, iy, ix) * (32 - ax) * (32 - ay) + _taps(raw, iy, ix + 1) * ax * (32 - ay)
           + _taps(raw, iy + 1, ix) * (32 - ax) * ay + _taps(raw, iy + 1, ix + 1) * ax * ay)
    inside = (mx > -2.0) & (mx < w + 1.0) & (my > -2.0) & (my < h + 1.0)
    fragile = (_near_cell_edge(mx, w) | _near_cell_edge(my, h)) & inside
    return ((acc + 512) >> 10).astype(np.uint8), fragile


def resize_taps(n_out, n_in):
    """i0, i1 (int64) and the 11-bit weight k of i1 for every output index of one axis."""
    o = np.arange(n_out, dtype=np.float64)
    f = (o + 0.5) * (n_in / n_out) - 0.5
    fl = np.floor(f)
    i0 = fl.astype(np.int64)
    a = f - fl
    low, high = i0 < 0, i0 >= n_in - 1
    i0 = np.where(low, 0, i0)
    a = np.where(low, 0.0, a)
    i0 = np.where(high, n_in - 1, i0)
    a = np.where(high, 0.0, a)
    i1 = np.minimum(i0 + 1, n_in - 1)
    k = np.floor(2048.0 * a + 0.5).astype(np.int64)
    return i0, i1, k


def resize(img, h1, w1, fragile=None):
    """Stage 2 of one frame img (h,w,3) uint8; with fragile (h,w) also the output pixels a fragile input contributes to."""
    h, w = img.shape[:2]
    y0, y1, ky = resize_taps(h1, h)
    x0, x1, kx = resize_taps(w1, w)
    p = img.astype(np.int64)
    wy0, wy1 = (2048 - ky)[:, None, None], ky[:, None, None]
    wx0, wx1 = (2048 - kx)[None, :, None], kx[None, :, None]
    acc = (p[y0][:, x0] * wy0 * wx0 + p[y0][:, x1] * wy0 * wx1 + p[y1][:, x0] * wy1 * wx0 + p[y1][:, x1] * wy1 * wx1)
    out = ((acc + (1 << 21)) >> 22).astype(np.uint8)
    if fragile is None:
        return out
    g = fragile
    fr = ((g[y0][:, x0] & (wy0 * wx0 > 0)[..., 0]) | (g[y0][:, x1] & (wy0 * wx1 > 0)[..., 0])
          | (g[y1][:, x0] & (wy1 * wx0 > 0)[..., 0]) | (g[y1][:, x1] & (wy1 * wx1 > 0)[..., 0]))
    return out, fr


def frame(raw, cams=None, size=None, crop=None):
    """raw (N,h0,w0,3) or (N,h0,w0) uint8; cams None (no stage 1), (22,) shared or (N,22); size (h1,w1) or None (no stage 2);
    crop (top, left, H, W) or None.  Returns image (N,3,H,W) uint8 and fragile (N,H,W) bool."""
    raw = np.asarray(raw)
    if raw.ndim == 3:
        raw = np.repeat(raw[..., None], 3, axis=3)
    N, h0, w0, _ = raw.shape
    h1, w1 = (h0, w0) if size is None else size
    top, left, H, W = (0, 0, h1, w1) if crop is None else crop
    images = np.zeros((N, 3, H, W), dtype=np.uint8)
    fragile = np.zeros((N, H, W), dtype=bool)
    cams = None if cams is None else np.asarray(cams, dtype=np.float64)
    for n in range(N):
        img, fr = raw[n], np.zeros((h0, w0), dtype=bool)
        if cams is not None:
            img, fr = rectify(img, cams if cams.ndim == 1 else cams[n])
        if (h1, w1) != (h0, w0):
            img, fr = resize(img, h1, w1, fr)
        images[n] = img[top:top + H, left:left + W].transpose(2, 0, 1)
        fragile[n] = fr[top:top + H, left:left + W]
    return images, fragile


def outside_share(cam, h, w):
    """The share of stage-1 pixels all of whose taps lie outside the raw frame."""
    mx, my = rectify_coords(cam, h, w)
    ix, iy = quantise(mx) >> 5, quantise(my) >> 5
    out = (ix < -1) | (ix >= w) | (iy < -1) | (iy >= h)
    return float(out.mean())


def normalize(image, mean, std):
    """(1,N,3,H,W) float32 RGB of image (N,3,H,W) uint8 BGR: ((float(px) * float32(1/255)) - mean) / std, each fp32 op rounded
    on its own (features.normalize_images, include/lgu_corr.h)."""
    r255 = np.float32(1.0 / 255.0)
    rgb = image[:, ::-1].astype(np.float32)
    m = np.asarray(mean, dtype=np.float32)[None, :, None, None]
    s = np.asarray(std, dtype=np.float32)[None, :, None, None]
    return (((rgb * r255).astype(np.float32) - m).astype(np.float32) / s).astype(np.float32)[None]


def interp_taps(n_out, n_in):
    """F.interpolate(mode='bilinear', align_corners=False) on one axis: i0, i1, the weight of i1 (float64)."""
    o = np.arange(n_out, dtype=np.float64)
    f = np.maximum((o + 0.5) * (n_in / n_out) - 0.5, 0.0)
    i0 = np.minimum(f.astype(np.int64), n_in - 1)
    i1 = i0 + (i0 < n_in - 1)
    return i0, i1, f - i0


def sensor_disparity(raw, scale, size=None, crop=None):
    """raw (h0,w0) uint16 or float32 depth; the depth d = raw * scale (float64) resized to `size`, cropped, sampled at
    [3::8, 3::8], where(d > 0, 1/d, d), rounded to float32 once."""
    d = np.asarray(raw).astype(np.float64) * np.float64(scale)
    h0, w0 = d.shape
    h1, w1 = (h0, w0) if size is None else size
    top, left, H, W = (0, 0, h1, w1) if crop is None else crop
    y0, y1, ly1 = interp_taps(h1, h0)
    x0, x1, lx1 = interp_taps(w1, w0)
    rows = np.arange(top + 3, top + H, 8)
    cols = np.arange(left + 3, left + W, 8)
    y0, y1, ly1 = y0[rows][:, None], y1[rows][:, None], ly1[rows][:, None]
    x0, x1, lx1 = x0[cols][None, :], x1[cols][None, :], lx1[cols][None, :]
    ly0, lx0 = 1.0 - ly1, 1.0 - lx1
    v = ly0 * (lx0 * d[y0, x0] + lx1 * d[y0, x1]) + ly1 * (lx0 * d[y1, x0] + lx1 * d[y1, x1])
    with np.errstate(divide="ignore"):
        return np.where(v > 0, 1.0 / np.where(v > 0, v, 1.0), v).astype(np.float32)
