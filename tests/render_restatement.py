"""The numpy restatement of the offscreen view (lgu_slam_amd.render.render_view, csrc/render.hip): normative.

Every float32 operation is rounded on its own (numpy float32 arrays and scalars, never a Python float in an expression), in
the order the kernels evaluate them; everything else is integer.  Independent of the library.

Frame buffer: one unsigned 64-bit key per pixel, all ones = empty; a primitive offers (bits(z) << 32) | (r << 16) | (g << 8)
| b; a pixel keeps the minimum.  `stats` (when a dict is passed) receives counts the tests use to show that a scene exercises
what it is meant to.
"""
import numpy as np

f32 = np.float32
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)
MAX_SAMPLES = f32(2.0 ** 20)

# The camera actor: the apex, a 2 x 2 base at depth 1.5 (upper left corner first, clockwise in the image, y down), and an
# up-marker hanging from the middle half of the base's lower edge.
FRUSTUM_VERTS = np.array([[0, 0, 0], [-1, -1, 1.5], [1, -1, 1.5], [1, 1, 1.5], [-1, 1, 1.5], [-0.5, 1, 1.5], [0.5, 1, 1.5],
                          [0, 1.2, 1.5]], f32)
# A -> B: the base's four edges, the four apex edges, the marker's two strokes
FRUSTUM_SEGS = ((1, 2), (2, 3), (3, 4), (4, 1), (0, 1), (0, 2), (0, 3), (0, 4), (5, 7), (7, 6))


def cross3(a, b):
    """csrc/se3.hpp cross3 on (...,3) float32 arrays: each product and difference rounded."""
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def act_so3(q, X):
    """csrc/se3.hpp act_so3: uv = 2 (q x X), t = q x uv, Y = (X + q.w uv) + t."""
    q = np.asarray(q, f32)
    X = np.asarray(X, f32)
    qv = np.broadcast_to(q[:3], X.shape)
    uv = cross3(qv, X)
    uv = uv * f32(2.0)
    t = cross3(qv, uv)
    return (X + q[3] * uv) + t


def rel_se3(pi, pj):
    """csrc/se3.hpp rel_se3: the transform from frame i to frame j, (t, q), sums left to right."""
    ti, qi, tj, qj = (np.asarray(v, f32) for v in (pi[:3], pi[3:], pj[:3], pj[3:]))
    q = np.array([((-qj[3] * qi[0] + qj[0] * qi[3]) - qj[1] * qi[2]) + qj[2] * qi[1],
                  ((-qj[3] * qi[1] + qj[1] * qi[3]) - qj[2] * qi[0]) + qj[0] * qi[2],
                  ((-qj[3] * qi[2] + qj[2] * qi[3]) - qj[0] * qi[1]) + qj[1] * qi[0],
                  ((qj[3] * qi[3] + qj[0] * qi[0]) + qj[1] * qi[1]) + qj[2] * qi[2]], f32)
    return tj - act_so3(q, ti), q


def cvt_i32_sat(f):
    """geom_pixel.hpp cvt_i32_sat on a float32 array, as int64: NaN -> 0, saturating."""
    f = np.asarray(f, f32)
    out = np.zeros(f.shape, np.int64)
    ok = np.isfinite(f) & (f < f32(2147483648.0)) & (f >= f32(-2147483648.0))
    out[ok] = f[ok].astype(np.int64)
    out[f >= f32(2147483648.0)] = 2 ** 31 - 1
    out[f < f32(-2147483648.0)] = -2 ** 31
    return out


def colour_bytes(c):
    """(...,3) colours as bytes: uint8 as they are; float32: clamp(floor(c 255 + 0.5), 0, 255), a NaN gives 0."""
    c = np.asarray(c)
    if c.dtype == np.uint8:
        return c.astype(np.uint64)
    with np.errstate(all="ignore"):
        f = np.floor(c.astype(f32) * f32(255.0) + f32(0.5))
        f = np.where(f >= f32(0.0), np.minimum(f, f32(255.0)), f32(0.0))    # a NaN fails f >= 0
    return f.astype(np.uint64)


def pack(rgb):
    rgb = np.asarray(rgb, np.uint64)
    return (rgb[..., 0] << np.uint64(16)) | (rgb[..., 1] << np.uint64(8)) | rgb[..., 2]


def bits(z):
    return np.asarray(z, f32).view(np.uint32).astype(np.uint64)


def project(Y, K):
    fx, fy, cx, cy = (f32(v) for v in K[:4])
    with np.errstate(all="ignore"):
        return fx * (Y[..., 0] / Y[..., 2]) + cx, fy * (Y[..., 1] / Y[..., 2]) + cy


def draw_points(keys, points, colors, view, K, point_size, near, stats=None):
    H, W = keys.shape
    view = np.asarray(view, f32)
    points = np.asarray(points, f32).reshape(-1, 3)
    s = int(point_size)
    if stats is not None:
        stats.update(points_passed=0, offers_inside=0, offers_outside=0, points_rejected=0)
    if len(points) == 0:
        return
    with np.errstate(all="ignore"):
        Y = act_so3(view[3:], points) + view[:3]
        keep = np.isfinite(Y).all(-1) & (Y[:, 2] > f32(near))
        u, v = project(Y, K)
        shift = f32(1.0) - f32(0.5) * f32(s)
        x0, y0 = cvt_i32_sat(np.floor(u + shift)), cvt_i32_sat(np.floor(v + shift))
    key = (bits(Y[:, 2]) << np.uint64(32)) | pack(colour_bytes(colors).reshape(-1, 3))
    if stats is not None:
        stats["points_passed"], stats["points_rejected"] = int(keep.sum()), int((~keep).sum())
    for dy in range(s):
        for dx in range(s):
            x, y = x0 + dx, y0 + dy              # int64: no overflow at the saturated ends
            inside = keep & (x >= 0) & (x < W) & (y >= 0) & (y < H)
            np.minimum.at(keys, (y[inside], x[inside]), key[inside])
            if stats is not None:
                stats["offers_inside"] += int(inside.sum())
                stats["offers_outside"] += int((keep & ~inside).sum())


def draw_frustums(keys, cameras, view, K, near, scale, color, stats=None):
    H, W = keys.shape
    view = np.asarray(view, f32)
    near, scale = f32(near), f32(scale)
    rgb = pack(np.asarray(color, np.uint64))
    if stats is not None:
        stats.update(segments_drawn=0, segments_clipped=0, segments_skipped=0, segments_crossing_edge=0, samples_inside=0)
    for cam in np.asarray(cameras, f32).reshape(-1, 7):
        with np.errstate(all="ignore"):
            tr, qr = rel_se3(cam, view)
            V = act_so3(qr, scale * FRUSTUM_VERTS) + tr
        for ia, ib in FRUSTUM_SEGS:
            A, B = V[ia].copy(), V[ib].copy()
            with np.errstate(all="ignore"):
                in_a, in_b = bool(A[2] >= near), bool(B[2] >= near)
                if not (np.isfinite(A).all() and np.isfinite(B).all()) or not (in_a or in_b):
                    if stats is not None:
                        stats["segments_skipped"] += 1
                    continue
                if not (in_a and in_b):
                    tc = (near - A[2]) / (B[2] - A[2])
                    M = np.array([A[0] + tc * (B[0] - A[0]), A[1] + tc * (B[1] - A[1]), near], f32)
                    if in_a:
                        B = M
                    else:
                        A = M
                    if stats is not None:
                        stats["segments_clipped"] += 1
                ua, va = project(A, K)
                ub, vb = project(B, K)
                wa, wb = f32(1.0) / A[2], f32(1.0) / B[2]
                du, dv, dw = ub - ua, vb - va, wb - wa
                au, av = np.abs(du), np.abs(dv)
                if not (np.isfinite(au) and np.isfinite(av)):
                    if stats is not None:
                        stats["segments_skipped"] += 1
                    continue
                n = np.ceil(np.maximum(au, av))
                if n == f32(0.0):
                    n = f32(1.0)
                if n > MAX_SAMPLES:
                    if stats is not None:
                        stats["segments_skipped"] += 1
                    continue
                tk = np.arange(int(n) + 1).astype(f32) / n
                u, v, w = ua + tk * du, va + tk * dv, wa + tk * dw
                z = f32(1.0) / w
                px, py = np.floor(u + f32(0.5)), np.floor(v + f32(0.5))
                inside = (px >= f32(0.0)) & (px < f32(W)) & (py >= f32(0.0)) & (py < f32(H))
            key = (bits(z[inside]) << np.uint64(32)) | rgb
            np.minimum.at(keys, (py[inside].astype(np.int64), px[inside].astype(np.int64)), key)
            if stats is not None:
                stats["segments_drawn"] += 1
                stats["samples_inside"] += int(inside.sum())
                stats["segments_crossing_edge"] += int(inside.any() and not inside.all())


def render_view(points, colors, view, K, size, point_size=2, background=(255, 255, 255), near=0.01, cameras=None,
                camera_scale=0.05, camera_color=(255, 0, 0), stats=None):
    """(image (H,W,3) uint8, depth (H,W) float32, keys (H,W) uint64)."""
    H, W = size
    keys = np.full((H, W), EMPTY, np.uint64)
    draw_points(keys, points, colors, view, K, point_size, near, stats)
    if cameras is not None and len(cameras):
        draw_frustums(keys, cameras, view, K, near, camera_scale, camera_color, stats)
    empty = keys == EMPTY
    image = np.stack([(keys >> np.uint64(16)) & np.uint64(255), (keys >> np.uint64(8)) & np.uint64(255), keys & np.uint64(255)],
                     -1).astype(np.uint8)
    image[empty] = np.asarray(background, np.uint8)
    depth = (keys >> np.uint64(32)).astype(np.uint32).view(f32).copy()
    depth[empty] = np.inf
    if stats is not None:
        stats["covered"] = int((~empty).sum())
    return image, depth, keys
