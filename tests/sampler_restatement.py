"""CPU restatement (numpy) of the reference's correlation samplers with the DEVICE's float -> int conversion, so that it
speaks for coordinates where C does not: NaN, +-inf and everything beyond the int32 rails.  TEST INFRASTRUCTURE ONLY.

Written from offersample_LGS/defCorrSample_kernel.cu:25-91, corrSample_kernel.cu:24-82, lowMem_defSample.cu:27-134,
gaussianAttn.cu:19-131, src/altcorr_kernel.cu:27-286 and droid_slam/modules/corr.py:88-109.

Rules this restatement encodes on top of the reference's text:
  * `static_cast<int>(floor(c))` converts as the hardware does (tests/geom_restatement.cvt_i32_sat: NaN -> 0, saturation at
    the int32 rails); every later index operation (`- r + i`, `+ 1`) is done in int64 and wrapped to int32, as the
    hardware's adds wrap;
  * the volume samplers use the whole-tap rule (`within_bounds(y1, x1)` around the whole tap, defCorrSample_kernel.cu:67,
    corrSample_kernel.cu:60): a tap that fails it is never written and keeps the 0 of torch::zeros.  Inside it a corner
    past the far edge is a literal 0 (:75-80); its weight is finite whenever the tap is in range and the coordinate is not
    NaN, and with a NaN coordinate the first corner, which is always in range there, makes the tap NaN anyway;
  * the low-memory sampler and altcorr have NO whole-tap rule: every corner is tested alone (lowMem_defSample.cu:102-112,
    altcorr_kernel.cu:89-93) and a corner that fails contributes `0 * weight`.  For a finite coordinate that is 0.  For a
    NaN or infinite one (`inf - floor(inf)` is NaN, :87-88) the weight is NaN and the reference's product is NaN: these
    operators return NaN for EVERY tap of such a pixel, in range or not.  The restatement keeps the IEEE product, because
    that is what the reference's kernels compute (tests/test_vs_reference_build.py holds it to them);
  * volume samplers: float32 throughout in the reference's order (:83-86); `dx = ofs - int(floor(ofs))` subtracts the
    CONVERTED integer (:58-61) in defCorr_index_forward and `x0 - floor(x0)` in corr_index_forward (:52-53);
  * low-memory sampler, altcorr, gaussian mask: weights in float32 as the reference forms them, sums in float64.
"""
import numpy as np

from tests.geom_restatement import cvt_i32_sat

f32 = np.float32


def wrap_i32(a):
    """int64 values -> what an int32 register holds after the same adds."""
    return ((np.asarray(a, np.int64) + 2 ** 31) % 2 ** 32) - 2 ** 31


def floor_i32(a):
    """static_cast<int>(floor(a)) on the device."""
    return cvt_i32_sat(np.floor(np.asarray(a, f32)))


def _gather(V, y, x, ok):
    """V (..., H2, W2) at integer (y, x) (..., T) where ok, a literal 0 elsewhere."""
    H2, W2 = V.shape[-2:]
    flat = V.reshape(V.shape[:-2] + (H2 * W2,))
    idx = np.clip(y, 0, H2 - 1) * W2 + np.clip(x, 0, W2 - 1)
    return np.where(ok, np.take_along_axis(flat, idx, -1), V.dtype.type(0))


def _blend_f32(V, x1, y1, dx, dy):
    """The whole-tap rule and the four-term float32 blend of the volume samplers (defCorrSample_kernel.cu:63-88).
    V (E,H1,W1,H2,W2); x1, y1, dx, dy (E,H1,W1,T)."""
    H2, W2 = V.shape[-2:]
    x2, y2 = wrap_i32(x1 + 1), wrap_i32(y1 + 1)                                   # :64, :66
    okx1, okx2 = (x1 >= 0) & (x1 < W2), (x2 >= 0) & (x2 < W2)
    oky1, oky2 = (y1 >= 0) & (y1 < H2), (y2 >= 0) & (y2 < H2)
    tap = okx1 & oky1                                                            # :67
    Q11 = _gather(V, y1, x1, tap)                                                # :74
    Q21 = _gather(V, y1, x2, tap & okx2)                                         # :75-76
    Q12 = _gather(V, y2, x1, tap & oky2)                                         # :77-78
    Q22 = _gather(V, y2, x2, tap & oky2 & okx2)                                  # :79-80
    one = f32(1)
    with np.errstate(invalid="ignore", over="ignore"):
        out = Q11 * ((one - dy) * (one - dx)) + Q21 * ((one - dy) * dx) + Q12 * (dy * (one - dx)) + Q22 * (dy * dx)  # :83-86
    assert out.dtype == np.float32
    return np.where(tap, out, f32(0))                                            # untouched taps keep torch::zeros


def defCorr_index_forward(volume, coords, offset, r):
    """defCorrSample_kernel.cu:25-91.  volume (E,H1,W1,H2,W2), coords (E,2,H1,W1), offset (E,H1,W1,rd,rd,2) IN/OUT (centre
    tap zeroed, :51-52).  Returns [corr (E,rd,rd,H1,W1)]."""
    E, H1, W1 = volume.shape[:3]
    rd = 2 * r + 1
    offset[:, :, :, r, r, :] = 0
    with np.errstate(invalid="ignore", over="ignore"):
        ofsX = (offset[..., 0] + coords[:, 0][..., None, None]).astype(f32)      # :56   [i][j]
        ofsY = (offset[..., 1] + coords[:, 1][..., None, None]).astype(f32)      # :57
        fx, fy = floor_i32(ofsX), floor_i32(ofsY)                                # :58-59
        dx, dy = ofsX - fx.astype(f32), ofsY - fy.astype(f32)                    # :60-61
    i = np.arange(rd).reshape(rd, 1)
    j = np.arange(rd).reshape(1, rd)
    x1 = wrap_i32(fx - r + i).reshape(E, H1, W1, rd * rd)                        # :63
    y1 = wrap_i32(fy - r + j).reshape(E, H1, W1, rd * rd)                        # :65
    out = _blend_f32(volume, x1, y1, dx.reshape(x1.shape), dy.reshape(x1.shape))
    return [np.ascontiguousarray(out.reshape(E, H1, W1, rd, rd).transpose(0, 3, 4, 1, 2))]


def corr_index_forward(volume, coords, r):
    """corrSample_kernel.cu:24-82."""
    E, H1, W1 = volume.shape[:3]
    rd = 2 * r + 1
    x0 = coords[:, 0].astype(f32)[..., None, None]
    y0 = coords[:, 1].astype(f32)[..., None, None]
    with np.errstate(invalid="ignore"):
        dx, dy = x0 - np.floor(x0), y0 - np.floor(y0)                            # :52-53
    i = np.arange(rd).reshape(rd, 1)
    j = np.arange(rd).reshape(1, rd)
    x1 = wrap_i32(floor_i32(x0) - r + i + 0 * j).reshape(E, H1, W1, rd * rd)     # :55
    y1 = wrap_i32(floor_i32(y0) - r + j + 0 * i).reshape(E, H1, W1, rd * rd)     # :58
    bc = lambda a: np.broadcast_to(a, (E, H1, W1, rd, rd)).reshape(x1.shape)
    out = _blend_f32(volume, x1, y1, bc(dx), bc(dy))
    return [np.ascontiguousarray(out.reshape(E, H1, W1, rd, rd).transpose(0, 3, 4, 1, 2))]


def probe_mask(volume1, coords, offset1):
    """corr.py:94-99: offset[1] *= sigmoid(var(CorrSampler(pyramid[1], coords / 2, 1))), unbiased variance over the nine
    taps.  In place and persistent: a NaN probe leaves that pixel's level-1 offsets NaN for every later call."""
    E, H1, W1 = volume1.shape[:3]
    pr, = corr_index_forward(volume1, (coords / f32(2)).astype(f32), 1)
    with np.errstate(invalid="ignore"):
        var = np.var(pr.reshape(E, 9, H1, W1).astype(np.float64), axis=1, ddof=1)
        mask = (1.0 / (1.0 + np.exp(-var))).astype(f32)
        offset1 *= mask.reshape(E, H1, W1, 1, 1, 1)
    return mask


def defcorr_pyramid(volumes, coords, offsets, r, probe=False):
    """CorrBlock.__call__ (corr.py:88-109): optional probe, then level l sampled at coords / 2^l with offsets[l] (None =
    zeros), concatenated to (E, L*rd*rd, H1, W1).  offsets are modified in place."""
    E, H1, W1 = volumes[0].shape[:3]
    rd = 2 * r + 1
    if probe:
        probe_mask(volumes[1], coords, offsets[1])
    out = []
    for l, v in enumerate(volumes):
        off = offsets[l] if offsets[l] is not None else np.zeros((E, H1, W1, rd, rd, 2), f32)
        c, = defCorr_index_forward(v, (coords / f32(2 ** l)).astype(f32), off, r)            # :102
        out.append(c.reshape(E, rd * rd, H1, W1))
    return np.concatenate(out, 1)


def _pairs(fmap1, fmap2):
    """All dot products <fmap1[b,h1,w1,:], fmap2[b,h2,w2,:]> in float64: (B, H1, W1, H2, W2)."""
    return np.einsum("bhwc,byxc->bhwyx", fmap1.astype(np.float64), fmap2.astype(np.float64))


def lowMem_defSample(fmap1, fmap2, coords, offset, r):
    """lowMem_defSample.cu:27-134.  fmap1 (B,H1,W1,C), fmap2 (B,H2,W2,C), coords (B,S,H1,W1,2), offset (NO,H1,W1,rd,rd,2)
    IN/OUT, row b*n (:80-83), tap [ix][iy].  Returns [corr (B,S,rd,rd,H1,W1)] float64."""
    B, S, H1, W1, _ = coords.shape
    H2, W2 = fmap2.shape[1:3]
    rd = 2 * r + 1
    G = _pairs(fmap1, fmap2)
    out = np.zeros((B, S, rd, rd, H1, W1))
    one = f32(1)
    for b in range(B):
        for n in range(S):
            off = offset[b * n]
            off[:, :, r, r, :] = 0                                               # :80-81
            with np.errstate(invalid="ignore", over="ignore"):
                xs = (coords[b, n, :, :, 0][..., None, None] + off[..., 0]).astype(f32)      # :82   [ix][iy]
                ys = (coords[b, n, :, :, 1][..., None, None] + off[..., 1]).astype(f32)      # :83
                dx, dy = xs - np.floor(xs), ys - np.floor(ys)                    # :87-88
                w11, w21 = (one - dy) * (one - dx), (one - dy) * dx              # :114-117
                w12, w22 = dy * (one - dx), dy * dx
            ix = np.arange(rd).reshape(rd, 1)
            iy = np.arange(rd).reshape(1, rd)
            w2 = wrap_i32(floor_i32(xs) - r + ix).reshape(H1, W1, rd * rd)       # :93
            h2 = wrap_i32(floor_i32(ys) - r + iy).reshape(H1, W1, rd * rd)       # :91
            w2h, h2h = wrap_i32(w2 + 1), wrap_i32(h2 + 1)
            okw, okwh = (w2 >= 0) & (w2 < W2), (w2h >= 0) & (w2h < W2)
            okh, okhh = (h2 >= 0) & (h2 < H2), (h2h >= 0) & (h2h < H2)
            g = G[b]
            fl = lambda a: a.reshape(H1, W1, rd * rd).astype(np.float64)
            with np.errstate(invalid="ignore"):
                q = (_gather(g, h2, w2, okh & okw) * fl(w11) + _gather(g, h2, w2h, okh & okwh) * fl(w21)
                     + _gather(g, h2h, w2, okhh & okw) * fl(w12) + _gather(g, h2h, w2h, okhh & okwh) * fl(w22))
            out[b, n] = q.reshape(H1, W1, rd, rd).transpose(2, 3, 0, 1)          # :128  corr[b][n][ix][iy][h1][w1]
    return [out]


def lowmem_pyramid(fmap1, fmap2s, coords, offsets, r, lbase=0, probe=False):
    """AltCorrBlock.corr_fn's level loop (corr.py:192-213): (B, S, L*rd*rd, H1, W1) float64.  probe: at level 1,
    offset[1] *= sigmoid(var(altcorr_forward(.., coords / 2, 1))) first (:201-206, S = 1), in place."""
    B, S, H1, W1, _ = coords.shape
    rd = 2 * r + 1
    out = []
    for l, f2 in enumerate(fmap2s):
        if probe and l == 1:
            pr, = altcorr_forward(fmap1, f2, (coords / f32(2)).astype(f32), 1)
            with np.errstate(invalid="ignore"):
                var = np.var(pr.reshape(B, 9, H1, W1), axis=1, ddof=1)
                offsets[1] *= (1.0 / (1.0 + np.exp(-var))).astype(f32).reshape(B, H1, W1, 1, 1, 1)
        off = offsets[l] if offsets[l] is not None else np.zeros((B, H1, W1, rd, rd, 2), f32)
        c, = lowMem_defSample(fmap1, f2, (coords / f32(2 ** (lbase + l))).astype(f32), off, r)
        out.append(c.reshape(B, S, rd * rd, H1, W1))
    return np.concatenate(out, 2)


def _alt_geometry(coords, r, H2, W2):
    """The (rd+1)^2 integer taps of altcorr (altcorr_kernel.cu:77-86) and the four blend weights, float32."""
    rd = 2 * r + 1
    xs, ys = coords[..., 0].astype(f32), coords[..., 1].astype(f32)
    with np.errstate(invalid="ignore"):
        dx, dy = xs - np.floor(xs), ys - np.floor(ys)                            # :77-78
    t = np.arange(rd + 1)
    w2 = wrap_i32(floor_i32(xs)[..., None] - r + t)                              # :86  (..., rd+1)
    h2 = wrap_i32(floor_i32(ys)[..., None] - r + t)                              # :85
    ok = ((h2 >= 0) & (h2 < H2))[..., :, None] & ((w2 >= 0) & (w2 < W2))[..., None, :]     # [iy][ix]
    return dx, dy, h2, w2, ok


def altcorr_forward(fmap1, fmap2, coords, r):
    """altcorr_kernel.cu:27-149.  Returns [corr (B,S,rd*rd,H1,W1)] float64; channel = iy + rd * ix (:102-105)."""
    B, S, H1, W1, _ = coords.shape
    H2, W2 = fmap2.shape[1:3]
    rd = 2 * r + 1
    G = _pairs(fmap1, fmap2)
    dx, dy, h2, w2, ok = _alt_geometry(coords, r, H2, W2)
    out = np.zeros((B, S, rd * rd, H1, W1))
    one = f32(1)
    with np.errstate(invalid="ignore"):
        wnw, wne = (dy * dx).astype(np.float64), (dy * (one - dx)).astype(np.float64)        # :112-115
        wsw, wse = ((one - dy) * dx).astype(np.float64), ((one - dy) * (one - dx)).astype(np.float64)
        for n in range(S):
            for iy in range(rd + 1):
                for ix in range(rd + 1):
                    y, x = h2[:, n, :, :, iy, None], w2[:, n, :, :, ix, None]
                    s = _gather(G, y, x, ok[:, n, :, :, iy, ix, None])[..., 0]   # :89-100
                    if iy > 0 and ix > 0:
                        out[:, n, (iy - 1) + rd * (ix - 1)] += s * wnw[:, n]     # :132-133
                    if iy > 0 and ix < rd:
                        out[:, n, (iy - 1) + rd * ix] += s * wne[:, n]
                    if iy < rd and ix > 0:
                        out[:, n, iy + rd * (ix - 1)] += s * wsw[:, n]
                    if iy < rd and ix < rd:
                        out[:, n, iy + rd * ix] += s * wse[:, n]                 # :141-142
    return [out]


def altcorr_backward(fmap1, fmap2, coords, corr_grad, r):
    """altcorr_kernel.cu:152-286 in float64.  Returns [fmap1_grad, fmap2_grad, coords_grad (never written, :336)]."""
    B, S, H1, W1, _ = coords.shape
    H2, W2, C = fmap2.shape[1:]
    rd = 2 * r + 1
    dx, dy, h2, w2, ok = _alt_geometry(coords, r, H2, W2)
    f1, f2 = fmap1.astype(np.float64), fmap2.astype(np.float64)
    g1, g2 = np.zeros_like(f1), np.zeros_like(f2)
    cg = corr_grad.astype(np.float64)
    dx, dy = dx.astype(np.float64), dy.astype(np.float64)
    bi = np.arange(B).reshape(B, 1, 1)
    with np.errstate(invalid="ignore"):
        for n in range(S):
            for iy in range(rd + 1):
                for ix in range(rd + 1):
                    g = np.zeros((B, H1, W1))
                    if iy > 0 and ix > 0:
                        g = g + cg[:, n, (iy - 1) + rd * (ix - 1)] * dy[:, n] * dx[:, n]              # :242-243
                    if iy > 0 and ix < rd:
                        g = g + cg[:, n, (iy - 1) + rd * ix] * dy[:, n] * (1 - dx[:, n])
                    if iy < rd and ix > 0:
                        g = g + cg[:, n, iy + rd * (ix - 1)] * (1 - dy[:, n]) * dx[:, n]
                    if iy < rd and ix < rd:
                        g = g + cg[:, n, iy + rd * ix] * (1 - dy[:, n]) * (1 - dx[:, n])            # :251-252
                    o = ok[:, n, :, :, iy, ix]
                    y = np.clip(h2[:, n, :, :, iy], 0, H2 - 1)
                    x = np.clip(w2[:, n, :, :, ix], 0, W2 - 1)
                    f2v = np.where(o[..., None], f2[bi, y, x], 0.0)              # :224-227
                    g1 += g[..., None] * f2v                                     # :255
                    contrib = np.where(o[..., None], g[..., None] * f1, 0.0)     # :256, :266-267
                    np.add.at(g2, (np.broadcast_to(bi, y.shape), y, x), contrib)
    return [g1, g2, np.zeros(coords.shape)]


def gaussianMask(means, covs, volume, r):
    """gaussianAttn.cu:19-68 in float64.  means / covs (E,H1,W1,2), volume (E,H1,W1,H2,W2).  Returns [volume1]."""
    E, H1, W1, H2, W2 = volume.shape
    rd = 2 * r + 1
    v = volume.astype(np.float64)
    out = np.zeros_like(v)
    mx, my = means[..., 0].astype(f32), means[..., 1].astype(f32)
    cx, cy = floor_i32(mx), floor_i32(my)                                        # :51-52
    c1, c2 = covs[..., 0].astype(np.float64), covs[..., 1].astype(np.float64)
    e_, y_, x_ = np.meshgrid(np.arange(E), np.arange(H1), np.arange(W1), indexing="ij")
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(rd):
            for j in range(rd):
                x1, y1 = wrap_i32(cx - r + i), wrap_i32(cy - r + j)              # :54-56
                ok = (x1 >= 0) & (x1 < W2) & (y1 >= 0) & (y1 < H2)               # :57
                ddx, ddy = x1.astype(f32).astype(np.float64) - mx, y1.astype(f32).astype(np.float64) - my
                ex = np.exp(-0.5 * (ddx / c1 * ddx + ddy / c2 * ddy))            # :58-61
                xc, yc = np.clip(x1, 0, W2 - 1), np.clip(y1, 0, H2 - 1)
                val = v[e_, y_, x_, yc, xc] * 3 * ex                             # :64
                out[e_[ok], y_[ok], x_[ok], yc[ok], xc[ok]] = val[ok]
    return [out]


def gaussianMask_backward(means, covs, volume, volume1_grad, r):
    """gaussianAttn.cu:72-131 in float64.  Returns [means_grad, covs_grad] (E,H1,W1,2)."""
    E, H1, W1, H2, W2 = volume.shape
    rd = 2 * r + 1
    v, gr = volume.astype(np.float64), volume1_grad.astype(np.float64)
    mg, cg = np.zeros(means.shape), np.zeros(covs.shape)
    mx, my = means[..., 0].astype(f32), means[..., 1].astype(f32)
    cx, cy = floor_i32(mx), floor_i32(my)
    c1, c2 = covs[..., 0].astype(np.float64), covs[..., 1].astype(np.float64)
    e_, y_, x_ = np.meshgrid(np.arange(E), np.arange(H1), np.arange(W1), indexing="ij")
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(rd):
            for j in range(rd):
                x1, y1 = wrap_i32(cx - r + i), wrap_i32(cy - r + j)
                ok = (x1 >= 0) & (x1 < W2) & (y1 >= 0) & (y1 < H2)               # :111
                ddx, ddy = x1.astype(f32).astype(np.float64) - mx, y1.astype(f32).astype(np.float64) - my
                ex = np.exp(-0.5 * (ddx / c1 * ddx + ddy / c2 * ddy))            # :112-115
                xc, yc = np.clip(x1, 0, W2 - 1), np.clip(y1, 0, H2 - 1)
                vv, gg = v[e_, y_, x_, yc, xc], gr[e_, y_, x_, yc, xc]
                z = lambda a: np.where(ok, a, 0.0)
                mg[..., 0] += z(3 * vv * (ex * ddx / c1) * gg)                   # :117
                mg[..., 1] += z(3 * vv * (ex * ddy / c2) * gg)                   # :118
                cg[..., 0] += z(3 * vv * (ex * 0.5 * ddx * ddx / (c1 * c1)) * gg)            # :120, :125
                cg[..., 1] += z(3 * vv * (ex * 0.5 * ddy * ddy / (c2 * c2)) * gg)            # :122, :126
    return [mg, cg]


def volume_pyramid(means, covs, volume, num_levels, r=4):
    """CorrBlock.__init__'s post-processing (gaussianMask_cuda.py:79-86 + corr.py:79-86) in float64: level 0 =
    gaussianMask / (6.28 sqrt(cov0 cov1)) + volume, level l = 2 x 2 average pooling of level l-1."""
    E, H1, W1, H2, W2 = volume.shape
    m, = gaussianMask(means, covs, volume, r)
    c = covs.astype(np.float64)
    lvl = m / (6.28 * np.sqrt(c[..., 0] * c[..., 1]))[..., None, None] + volume.astype(np.float64)
    out = [lvl]
    for _ in range(1, num_levels):
        h, w = lvl.shape[3] // 2, lvl.shape[4] // 2
        lvl = lvl[:, :, :, :2 * h, :2 * w].reshape(E, H1, W1, h, 2, w, 2).mean(axis=(4, 6))
        out.append(lvl)
    return out
