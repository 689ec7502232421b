"""Float64 restatements of the four backward operators (defCorr_index_backward, corr_index_backward,
gaussianMask_backward, altcorr_backward), written from the maths in vectorised torch, with gradients from
torch.autograd; the per-element error bounds the tests hold the fp32 implementations to; and the seeded inputs
that tests/test_backward.py and tests/test_vs_reference_build.py share.  Nothing here calls the C oracle or a kernel.

Sampler (with offsets, or plain with X = x0, Y = y0), per source pixel and tap (i, j), r = radius, rd = 2r + 1:

    X = fl32(offset_x + x0), Y = fl32(offset_y + y0)      centre offset zeroed first; one fp32 rounding, as the
                                                          reference forms the position; float64 from here on
    x1 = floor(X) - r + i,  y1 = floor(Y) - r + j         the tap counts iff (y1, x1) is inside the slice
    dx = X - floor(X),      dy = Y - floor(Y)
    out[e, i, j, y, x] = Q11 (1-dy)(1-dx) + Q21 (1-dy) dx + Q12 dy (1-dx) + Q22 dy dx
                                                          Q = volume at (y1|y1+1, x1|x1+1), 0 beyond the slice

X and Y are the autograd leaves: d out / dX is offset_grad[..., 0], d out / dY is offset_grad[..., 1], the centre tap
included (the reference differentiates there, at the zeroed offset).  dx and dy enter as the fp32 numbers the
reference holds: X - floor(X) is exact in fp32 except for -1 < X < 0, where 1 - |X| rounds (absolute error 2^-25);
the restatement takes that fp32 value, so dx and dy are exact inputs of both sides and every bound below is a
relative one.

Gaussian mask:  out = volume * 3 * exp(-(ddx^2 / c1 + ddy^2 / c2) / 2) on the window floor(mean) +- radius, 0
elsewhere; ddx = x - mean_x, ddy = y - mean_y.  Gradients with respect to means and covs.

altcorr:  s[iy, ix] = <fmap1[pixel], fmap2[floor(ys) - r + iy, floor(xs) - r + ix]> on the (rd+1)^2 lattice, 0 where
the lattice point is outside fmap2; out[ox * rd + oy] = s[oy, ox] (1-dy)(1-dx) + s[oy, ox+1] (1-dy) dx
+ s[oy+1, ox] dy (1-dx) + s[oy+1, ox+1] dy dx.  Gradients with respect to both feature maps.


Bounds
------
u = 2^-24 is the unit roundoff of fp32: every fp32 operation returns its exact result times (1 + d), |d| <= u.  A
product of k such factors deviates by at most k u (to first order; one spare unit in every K below pays for the
second-order terms, K u < 1e-4).  A sum of n terms, in ANY order (atomics give none), passes every term through at
most n - 1 additions.  So an output element that the reference's fp32 formula builds as a sum of n terms, each the
result of p roundings, lies within

    |got - ref64| <= K u A,        K = p + (n - 1) + 1,        A = sum of the |terms|

of the exact value.  A comes from the magnitude functions: the weights are non-negative, so A of a scatter output is
the same backward run on |g| (and |volume|, |fmap1|, |fmap2|).  Where A == 0 the reference is exactly 0 and the
implementation must return exactly 0.  Fused multiply-adds only remove roundings.

volume_grad (defCorr / corr_index backward), reference term ((1-dy) * (1-dx)) * g:
    1-dy, 1-dx: one rounding each (exact when the fraction is >= 1/2); their product: 1; times g: 1      p = 4
    at most 4 rd^2 terms land on one element                                                             n <= 4 rd^2
    K_vol = 4 rd^2 + 4
offset_grad, reference (-Q11 (1-dx) - Q21 dx + Q12 (1-dx) + Q22 dx) * g:
    1-dx: 1, product with Q: 1, the common factor g: 1                                                   p = 3
    four terms                                                                                           n = 4
    K_off = 3 + 3 + 1 = 7,   A = (|Q11| (1-dx) + |Q21| dx + |Q12| (1-dx) + |Q22| dx) |g|
forward sampler (only for the adjoint identity), Q11 * ((1-dy) * (1-dx)) + ...:
    p = 4, n = 4, K_fwd = 8
altcorr lattice gradient gl = sum of up to 4 terms gp * dy * dx (or with 1-dy, 1-dx):
    1-dy, 1-dx: 2, two products: 2, three additions: 3                                                   7 roundings
fmap1_grad[c] = sum over (n, lattice point) of gl * fmap2[c]:
    p = 7 + 1, n = S (rd+1)^2                                         K_f1 = S (rd+1)^2 + 8
fmap2_grad[b, h2, w2, c] = sum of gl * fmap1[c] over the N (pixel, n, lattice point) contributions that land
    on (b, h2, w2); N is counted per element                          K_f2 = N + 8
altcorr forward (adjoint identity): C products summed (C), one product with a weight built by 3 roundings (4),
    four terms (3)                                                    K_afwd = C + 9
gaussianMask_backward, reference term 3 * v * (e * ddx / c1) * g with e = expf(f), f = -0.5 (ddx/c1 ddx + ddy/c2 ddy):
    ddx = (float)x1 - mean: 1 rounding, so f carries 2 (ddx twice) + 1 (quotient) + 1 (product) + 1 (sum; both
    summands have one sign, so no cancellation) = 5 roundings, which exp turns into a relative error 5 |f| u;
    the device expf is trusted to 2 ulp = 4 u (the figure test_gaussian_mask_forward_backward already assumes);
    the rest of the term: ddx 1, e*ddx 1, /c1 1, 3*v 1, two products 2 = 6.   Per term (5 |f| + 10) u.
    covs: dE = (float)(e * 0.5 * ddx * ddx / (double)(c1 * c1)): c1*c1 1, ddx twice 2, narrowing 1, 3*v 1, two
    products 2 = 7.  Per term (5 |f| + 11) u.  Both are held to (5 |f| + 12) u.
    nt = rd^2 terms:  |got - ref64| <= u ((12 + nt) A + 5 A_f),   A_f = sum of |term| |f|
    exp(f) underflows in fp32 long before it does in float64 (windows that straddle a border keep only their far
    taps).  An fp32 result that is subnormal or flushed is off by at most t = 2^-126 absolute, and what follows
    multiplies that by the remaining factors; the product of (1 + |factor|) over all factors of a term dominates every
    partial product, so each term adds t (1 + |g|)(1 + 3|v|)(1 + 1/c)(1 + |ddx|) (covs: (1 + ddx^2 / c^2) for the last
    two) to the bound.  At these inputs that is below 1e-33.

Largest err / (u A) observed, against the K the test allows (oracle = the C restatement of the reference, sequential
fp32 on the CPU; HIP = this project's kernels on an MI355X; all cases of tests/test_backward.py):

    output                        K allowed                       oracle      HIP
    volume_grad                   4 rd^2 + 4  (40 .. 904)           2.91     3.07
    volume_grad, plain sampler    4 rd^2 + 4                        3.03     3.09
    offset_grad                   7                                 2.96     2.96
    fmap1_grad                    S (rd+1)^2 + 8  (24 .. 136)       4.37     4.37
    fmap2_grad                    N + 8                             3.96     3.44
    means_grad                    12 + rd^2 + 5 |f|  (|f| to ~80)   56.2     57.3
    covs_grad                     12 + rd^2 + 5 |f|                 58.2     58.2
    sampler forward               8                                 2.92     (adjoint identity only)
    altcorr forward               C + 9                             2.98     (adjoint identity only)

The two Gaussian rows are large because of the 5 |f| u that exp makes of the roundings in its argument, on pixels whose
window keeps only taps far from the mean; elements with A < 2^-100, where the underflow term governs, are left out of
the ratio.
"""
import functools

import numpy as np
import torch

from tests import inputs

U = 2.0 ** -24
TINY = 2.0 ** -126
BW_BOX_FLOATS = 1024     # csrc/defcorr_bwd.hip: a pass whose tap box is larger goes through global atomics
WAVE = 64


def k_vol(radius):
    return 4 * (2 * radius + 1) ** 2 + 4


K_OFF = 7
K_FWD = 8


def k_f1(S, radius):
    return S * (2 * radius + 2) ** 2 + 8


def k_afwd(C):
    return C + 9


def _t64(a):
    return torch.from_numpy(np.array(a, order="C")).double()


def _frac32(x64):
    x = x64.float()
    return (x - torch.floor(x)).double()


# ---------------------------------------------------------------------------------------------------------------------
# sampler
# ---------------------------------------------------------------------------------------------------------------------
def sampler_positions(coords, offset, radius):
    """fp32 numpy coords (E,2,H1,W1) and offset (E,H1,W1,rd,rd,2) or None (plain sampler) -> float64 X, Y (E,H1,W1,rd,rd):
    the fp32 sum the reference forms, centre offset zeroed."""
    c = np.asarray(coords, np.float32)
    E, _, H1, W1 = c.shape
    rd = 2 * radius + 1
    if offset is None:
        o = np.zeros((E, H1, W1, rd, rd, 2), np.float32)
    else:
        o = np.array(offset, np.float32).reshape(E, H1, W1, rd, rd, 2)
        o[:, :, :, radius, radius, :] = 0.0
    X = (o[..., 0] + c[:, 0][..., None, None]).astype(np.float32)
    Y = (o[..., 1] + c[:, 1][..., None, None]).astype(np.float32)
    return _t64(X), _t64(Y)


def _sampler_parts(volume, X, Y, radius):
    E, H1, W1, H2, W2 = volume.shape
    r, rd = radius, 2 * radius + 1
    ar = torch.arange(rd)
    Xd, Yd = X.detach(), Y.detach()
    x1 = torch.floor(Xd).clamp(-2.0 ** 40, 2.0 ** 40).long() - r + ar.view(rd, 1)
    y1 = torch.floor(Yd).clamp(-2.0 ** 40, 2.0 ** 40).long() - r + ar.view(1, rd)
    dx = (X - Xd) + _frac32(Xd)     # value: the fp32 fraction; derivative: 1
    dy = (Y - Yd) + _frac32(Yd)
    valid = (x1 >= 0) & (x1 < W2) & (y1 >= 0) & (y1 < H2)
    xin, yin = x1 + 1 < W2, y1 + 1 < H2
    flat = volume.reshape(E, H1, W1, H2 * W2)

    def corner(yy, xx, m):
        idx = (yy.clamp(0, H2 - 1) * W2 + xx.clamp(0, W2 - 1)).reshape(E, H1, W1, rd * rd)
        q = torch.gather(flat, -1, idx).reshape(E, H1, W1, rd, rd)
        return torch.where(m, q, torch.zeros_like(q))

    Q = (corner(y1, x1, valid), corner(y1, x1 + 1, valid & xin), corner(y1 + 1, x1, valid & yin),
         corner(y1 + 1, x1 + 1, valid & xin & yin))
    return Q, dx, dy, valid


def defcorr_forward64(volume, X, Y, radius):
    """volume (E,H1,W1,H2,W2), X, Y (E,H1,W1,rd,rd), all float64 -> (E,rd,rd,H1,W1)."""
    (Q11, Q21, Q12, Q22), dx, dy, _ = _sampler_parts(volume, X, Y, radius)
    out = Q11 * ((1 - dy) * (1 - dx)) + Q21 * ((1 - dy) * dx) + Q12 * (dy * (1 - dx)) + Q22 * (dy * dx)
    return out.permute(0, 3, 4, 1, 2)


def sampler_backward64(volume, coords, offset, corr_grad, radius):
    """Float64 gradients and magnitudes of the sampler on fp32 numpy inputs; offset None = plain sampler.
    Returns a dict of float64 numpy arrays: fwd, A_fwd, volume_grad, A_vol and (with offsets) offset_grad, A_off
    in the operator's layouts."""
    v = _t64(volume).requires_grad_(True)
    g = _t64(corr_grad)
    X, Y = sampler_positions(coords, offset, radius)
    X.requires_grad_(True)
    Y.requires_grad_(True)
    fwd = defcorr_forward64(v, X, Y, radius)
    vg, xg, yg = torch.autograd.grad(fwd, (v, X, Y), g, allow_unused=True)
    with torch.no_grad():
        va = v.detach().abs().requires_grad_(True)
    a_fwd = defcorr_forward64(va, X.detach(), Y.detach(), radius)
    a_vol, = torch.autograd.grad(a_fwd, va, g.abs())
    out = dict(fwd=fwd.detach().numpy(), A_fwd=a_fwd.detach().numpy(), volume_grad=vg.numpy(), A_vol=a_vol.numpy())
    if offset is not None:
        with torch.no_grad():
            (Q11, Q21, Q12, Q22), dx, dy, _ = _sampler_parts(va.detach(), X.detach(), Y.detach(), radius)
            ga = g.abs().permute(0, 3, 4, 1, 2)
            ax = (Q11 * (1 - dy) + Q21 * (1 - dy) + Q12 * dy + Q22 * dy) * ga
            ay = (Q11 * (1 - dx) + Q21 * dx + Q12 * (1 - dx) + Q22 * dx) * ga
        out["offset_grad"] = torch.stack([xg, yg], -1).numpy()
        out["A_off"] = torch.stack([ax, ay], -1).numpy()
    return out


def tap_paths(coords, offset, radius, H2, W2):
    """What csrc/defcorr_bwd.hip does with these inputs, counted on the CPU in the kernel's own fp32 index arithmetic:
    per (pixel, pass of 64 taps) the number of valid taps and the size of the tap bounding box, plus the border counts
    of the whole input.  Returns dict(nvalid (P, passes), box (P, passes), last_col, last_row, rej_left, rej_right,
    rej_top, rej_bottom)."""
    X, Y = sampler_positions(coords, offset, radius)
    X, Y = X.numpy(), Y.numpy()
    r, rd = radius, 2 * radius + 1
    ar = np.arange(rd)
    x1 = np.floor(X).astype(np.int64) - r + ar.reshape(rd, 1)
    y1 = np.floor(Y).astype(np.int64) - r + ar.reshape(1, rd)
    valid = (x1 >= 0) & (x1 < W2) & (y1 >= 0) & (y1 < H2)
    xh = np.where(x1 + 1 < W2, x1 + 1, x1)
    yh = np.where(y1 + 1 < H2, y1 + 1, y1)
    P, nt = valid.size // (rd * rd), rd * rd
    passes = (nt + WAVE - 1) // WAVE
    pad = passes * WAVE - nt
    f = lambda a, fill: np.pad(a.reshape(P, nt), ((0, 0), (0, pad)), constant_values=fill).reshape(P, passes, WAVE)
    v = f(valid, False)
    big = np.iinfo(np.int64).max
    xlo = np.where(v, f(x1, 0), big).min(-1)
    ylo = np.where(v, f(y1, 0), big).min(-1)
    xhi = np.where(v, f(xh, 0), -big).max(-1)
    yhi = np.where(v, f(yh, 0), -big).max(-1)
    nvalid = v.sum(-1)
    box = np.where(nvalid > 0, (xhi - xlo + 1) * (yhi - ylo + 1), 0)
    return dict(nvalid=nvalid, box=box,
                last_col=int((valid & (x1 + 1 == W2)).sum()), last_row=int((valid & (y1 + 1 == H2)).sum()),
                rej_left=int((x1 < 0).sum()), rej_right=int((x1 >= W2).sum()),
                rej_top=int((y1 < 0).sum()), rej_bottom=int((y1 >= H2).sum()))


# name: (seed, E, H1, W1, H2, W2, radius, coords sigma, offset scale, coords factor, coords shift)
SAMPLER_CASES = {
    "level1": (101, 2, 12, 16, 6, 8, 3, 3.0, 4.0, 0.5, 0.0),
    "odd_target": (102, 1, 5, 7, 9, 11, 3, 2.0, 3.0, 1.0, 0.0),
    "one_by_one": (103, 2, 3, 5, 1, 1, 1, 1.0, 1.0, 1.0, 0.0),
    "large_box": (104, 1, 5, 7, 40, 48, 3, 3.0, 20.0, 1.0, 16.0),     # the source grid sits mid-slice
    "radius4": (105, 1, 5, 7, 9, 11, 4, 2.0, 3.0, 1.0, 0.0),
    "radius7": (106, 1, 4, 4, 12, 16, 7, 2.0, 2.0, 1.0, 0.0),
    "radius5_large_box": (107, 1, 3, 4, 40, 48, 5, 3.0, 20.0, 1.0, 8.0),     # boxes around 1024: passes of both kinds
    "far_outside": (108, 1, 4, 6, 8, 8, 3, 0.0, 4.0, 1.0, 100.0),
}
LARGE_BOX_CASES = ("large_box", "radius5_large_box")
BORDER_CASES = ("level1", "odd_target", "one_by_one", "radius4")


def make_sampler_inputs(rng, E, H1, W1, H2, W2, radius, sigma, off_scale, factor=1.0, shift=0.0):
    rd = 2 * radius + 1
    v = rng.standard_normal((E, H1, W1, H2, W2)).astype(np.float32)
    c = (inputs.grid_coords(rng, E, H1, W1, sigma) * np.float32(factor) + np.float32(shift)).astype(np.float32)
    off = (off_scale * np.tanh(rng.standard_normal((E, H1, W1, rd, rd, 2)))).astype(np.float32)
    g = rng.standard_normal((E, rd, rd, H1, W1)).astype(np.float32)
    return dict(volume=v, coords=c, offset=off, corr_grad=g, radius=radius)


@functools.lru_cache(maxsize=None)
def sampler_case(name):
    seed, E, H1, W1, H2, W2, radius, sigma, osc, factor, shift = SAMPLER_CASES[name]
    case = make_sampler_inputs(np.random.default_rng(seed), E, H1, W1, H2, W2, radius, sigma, osc, factor, shift)
    for a in case.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return case


def sampler_refs(case):
    """(with offsets, plain) float64 references of one input set."""
    a = sampler_backward64(case["volume"], case["coords"], case["offset"], case["corr_grad"], case["radius"])
    b = sampler_backward64(case["volume"], case["coords"], None, case["corr_grad"], case["radius"])
    return a, b


@functools.lru_cache(maxsize=None)
def sampler_case_refs(name):
    return sampler_refs(sampler_case(name))


# ---------------------------------------------------------------------------------------------------------------------
# Gaussian mask
# ---------------------------------------------------------------------------------------------------------------------
def _gauss_parts(means, covs, H2, W2, radius):
    mx, my = means[..., 0:1], means[..., 1:2]
    c1, c2 = covs[..., 0:1], covs[..., 1:2]
    cx = torch.floor(mx.detach()).clamp(-2.0 ** 40, 2.0 ** 40).long()
    cy = torch.floor(my.detach()).clamp(-2.0 ** 40, 2.0 ** 40).long()
    xs, ys = torch.arange(W2), torch.arange(H2)
    inx = (xs >= cx - radius) & (xs <= cx + radius)                  # (E,H1,W1,W2)
    iny = (ys >= cy - radius) & (ys <= cy + radius)                  # (E,H1,W1,H2)
    mask = iny[..., :, None] & inx[..., None, :]
    ddx = (xs.double() - mx)[..., None, :]                           # (E,H1,W1,1,W2)
    ddy = (ys.double() - my)[..., :, None]                           # (E,H1,W1,H2,1)
    f = -0.5 * (ddx * ddx / c1[..., None] + ddy * ddy / c2[..., None])
    return mask, ddx, ddy, f


def gaussmask_forward64(means, covs, volume, radius):
    """means, covs (E,H1,W1,2), volume (E,H1,W1,H2,W2), float64 -> (E,H1,W1,H2,W2)."""
    mask, _, _, f = _gauss_parts(means, covs, volume.shape[3], volume.shape[4], radius)
    out = volume * 3.0 * torch.exp(f)
    return torch.where(mask, out, torch.zeros_like(out))


def gaussmask_backward64(means, covs, volume, volume1_grad, radius):
    """Float64 gradients of the Gaussian mask on fp32 numpy inputs and their per-element bounds (module docstring).
    Returns dict(means_grad, covs_grad, A_means, A_covs, bound_means, bound_covs), each (E,H1,W1,2)."""
    m = _t64(means).requires_grad_(True)
    c = _t64(covs).requires_grad_(True)
    v, g = _t64(volume), _t64(volume1_grad)
    mg, cg = torch.autograd.grad(gaussmask_forward64(m, c, v, radius), (m, c), g)
    nt = (2 * radius + 1) ** 2
    with torch.no_grad():
        mask, ddx, ddy, f = _gauss_parts(m.detach(), c.detach(), v.shape[3], v.shape[4], radius)
        c1, c2 = c.detach()[..., 0, None, None], c.detach()[..., 1, None, None]
        k = mask * (3.0 * v.abs() * g.abs() * torch.exp(f))
        af = f.abs()
        under = mask * (TINY * (1 + g.abs()) * (1 + 3 * v.abs()))
        A_m, A_c, b_m, b_c = [], [], [], []
        for dd, cc in ((ddx, c1), (ddy, c2)):
            tm = k * dd.abs() / cc
            tc = k * 0.5 * dd * dd / (cc * cc)
            A_m.append(tm.sum((-1, -2)))
            A_c.append(tc.sum((-1, -2)))
            b_m.append(U * ((12 + nt) * tm.sum((-1, -2)) + 5 * (tm * af).sum((-1, -2)))
                       + (under * (1 + 1 / cc) * (1 + dd.abs())).sum((-1, -2)))
            b_c.append(U * ((12 + nt) * tc.sum((-1, -2)) + 5 * (tc * af).sum((-1, -2)))
                       + (under * (1 + dd * dd / (cc * cc))).sum((-1, -2)))
    st = lambda l: torch.stack(l, -1).numpy()
    return dict(means_grad=mg.numpy(), covs_grad=cg.numpy(), A_means=st(A_m), A_covs=st(A_c),
                bound_means=st(b_m), bound_covs=st(b_c))


GAUSS_SHAPES = ((2, 6, 8, 6, 8), (1, 5, 7, 9, 10))
GAUSS_RADII = (1, 2, 4, 5)


def make_gauss_inputs(rng, shape, spread, outside=False):
    E, H1, W1, H2, W2 = shape
    v = rng.standard_normal(shape).astype(np.float32)
    g = rng.standard_normal(shape).astype(np.float32)
    if outside:     # no window reaches the slice: half the pixels far to the left / above, half far to the right / below
        means = np.where(rng.random((E, H1, W1, 1)) < 0.5, -20.0, np.array([W2 + 20.0, H2 + 20.0])).astype(np.float32)
        means = (means + rng.random((E, H1, W1, 2)).astype(np.float32)).astype(np.float32)
    else:           # uniform over the slice and a margin of `spread` around it: windows straddle every border
        means = np.stack([rng.uniform(-spread, W2 + spread, (E, H1, W1)), rng.uniform(-spread, H2 + spread, (E, H1, W1))],
                         -1).astype(np.float32)
    covs = rng.uniform(0.05, 5.05, (E, H1, W1, 2)).astype(np.float32)
    return dict(means=means, covs=covs, volume=v, grad=g)


@functools.lru_cache(maxsize=None)
def gauss_case(shape, radius, outside=False):
    rng = np.random.default_rng(200 + 10 * shape[3] + radius + (1000 if outside else 0))
    case = make_gauss_inputs(rng, shape, radius + 1.0, outside)
    case["radius"] = radius
    return case


@functools.lru_cache(maxsize=None)
def gauss_case_refs(shape, radius, outside=False):
    c = gauss_case(shape, radius, outside)
    return gaussmask_backward64(c["means"], c["covs"], c["volume"], c["grad"], radius)


# ---------------------------------------------------------------------------------------------------------------------
# altcorr
# ---------------------------------------------------------------------------------------------------------------------
def _altcorr_lattice(coords, H2, W2, radius):
    r, rl = radius, 2 * radius + 2
    xs, ys = coords[..., 0], coords[..., 1]                                      # (B,S,H1,W1)
    ar = torch.arange(rl)
    w2 = (torch.floor(xs).clamp(-2.0 ** 40, 2.0 ** 40).long() - r)[..., None, None] + ar.view(1, rl)
    h2 = (torch.floor(ys).clamp(-2.0 ** 40, 2.0 ** 40).long() - r)[..., None, None] + ar.view(rl, 1)
    inb = (h2 >= 0) & (h2 < H2) & (w2 >= 0) & (w2 < W2)                          # (B,S,H1,W1,iy,ix)
    idx = h2.clamp(0, H2 - 1) * W2 + w2.clamp(0, W2 - 1)
    return inb, idx, _frac32(xs)[..., None, None], _frac32(ys)[..., None, None]


def altcorr_forward64(fmap1, fmap2, coords, radius):
    """fmap1 (B,H1,W1,C), fmap2 (B,H2,W2,C), coords (B,S,H1,W1,2), float64 -> (B,S,rd*rd,H1,W1), channel ix*rd + iy."""
    B, H1, W1, C = fmap1.shape
    _, H2, W2, _ = fmap2.shape
    S = coords.shape[1]
    rd, rl = 2 * radius + 1, 2 * radius + 2
    inb, idx, dx, dy = _altcorr_lattice(coords, H2, W2, radius)
    full = torch.einsum("bhwc,bkc->bhwk", fmap1, fmap2.reshape(B, H2 * W2, C))   # (B,H1,W1,H2*W2)
    full = full[:, None].expand(B, S, H1, W1, H2 * W2)
    s = torch.gather(full, -1, idx.reshape(B, S, H1, W1, rl * rl)).reshape(B, S, H1, W1, rl, rl)
    s = torch.where(inb, s, torch.zeros_like(s))
    o = (s[..., :-1, :-1] * ((1 - dy) * (1 - dx)) + s[..., :-1, 1:] * ((1 - dy) * dx)
         + s[..., 1:, :-1] * (dy * (1 - dx)) + s[..., 1:, 1:] * (dy * dx))        # (B,S,H1,W1,oy,ox)
    return o.permute(0, 1, 5, 4, 2, 3).reshape(B, S, rd * rd, H1, W1)


def altcorr_backward64(fmap1, fmap2, coords, corr_grad, radius):
    """Float64 gradients, magnitudes and bounds of altcorr on fp32 numpy inputs.  Returns dict(fwd, A_fwd, fmap1_grad,
    fmap2_grad, A_f1, A_f2, N (B,H2,W2) contributions per fmap2 position, bound_f1, bound_f2, bound_fwd)."""
    f1 = _t64(fmap1).requires_grad_(True)
    f2 = _t64(fmap2).requires_grad_(True)
    c, g = _t64(coords), _t64(corr_grad)
    fwd = altcorr_forward64(f1, f2, c, radius)
    g1, g2 = torch.autograd.grad(fwd, (f1, f2), g)
    a1 = f1.detach().abs().requires_grad_(True)
    a2 = f2.detach().abs().requires_grad_(True)
    a_fwd = altcorr_forward64(a1, a2, c, radius)
    A1, A2 = torch.autograd.grad(a_fwd, (a1, a2), g.abs())
    B, H2, W2, C = f2.shape
    S = c.shape[1]
    inb, idx, _, _ = _altcorr_lattice(c, H2, W2, radius)
    N = torch.zeros(B, H2 * W2, dtype=torch.float64)
    N.scatter_add_(1, idx.reshape(B, -1), inb.reshape(B, -1).double())
    N = N.reshape(B, H2, W2)
    return dict(fwd=fwd.detach().numpy(), A_fwd=a_fwd.detach().numpy(), fmap1_grad=g1.numpy(), fmap2_grad=g2.numpy(),
                A_f1=A1.numpy(), A_f2=A2.numpy(), N=N.numpy(),
                bound_f1=(k_f1(S, radius) * U * A1).numpy(), bound_f2=((N[..., None] + 8) * U * A2).numpy(),
                bound_fwd=(k_afwd(C) * U * a_fwd.detach()).numpy())


# name: (seed, B, S, H1, W1, H2, W2, C, radius, coords sigma, coords factor, coords shift)
ALTCORR_CASES = {}
for _C in (32, 96, 160, 256, 512):
    for _r in (3, 1):
        ALTCORR_CASES["c%d_r%d" % (_C, _r)] = (300 + _C + _r, 2, 2, 6, 8, 6, 8, _C, _r, 3.0, 1.0, 0.0)
ALTCORR_CASES["half_scale"] = (391, 2, 1, 3, 5, 2, 3, 64, 3, 2.0, 0.5, 0.0)
ALTCORR_CASES["far_outside"] = (392, 2, 2, 6, 8, 6, 8, 64, 3, 3.0, 1.0, 100.0)


def make_altcorr_inputs(rng, B, S, H1, W1, H2, W2, C, radius, sigma, factor=1.0, shift=0.0):
    rd = 2 * radius + 1
    f1 = (rng.standard_normal((B, H1, W1, C)) * 0.125).astype(np.float32)
    f2 = (rng.standard_normal((B, H2, W2, C)) * 0.125).astype(np.float32)
    ys, xs = np.meshgrid(np.arange(H1, dtype=np.float32), np.arange(W1, dtype=np.float32), indexing="ij")
    c = np.stack([xs, ys], -1)[None, None].repeat(B, 0).repeat(S, 1)
    c = ((c + rng.standard_normal(c.shape) * sigma) * factor + shift).astype(np.float32)
    g = rng.standard_normal((B, S, rd * rd, H1, W1)).astype(np.float32)
    return dict(fmap1=f1, fmap2=f2, coords=c, corr_grad=g, radius=radius)


@functools.lru_cache(maxsize=None)
def altcorr_case(name):
    seed, B, S, H1, W1, H2, W2, C, radius, sigma, factor, shift = ALTCORR_CASES[name]
    return make_altcorr_inputs(np.random.default_rng(seed), B, S, H1, W1, H2, W2, C, radius, sigma, factor, shift)


def altcorr_refs(case):
    return altcorr_backward64(case["fmap1"], case["fmap2"], case["coords"], case["corr_grad"], case["radius"])


@functools.lru_cache(maxsize=None)
def altcorr_case_refs(name):
    return altcorr_refs(altcorr_case(name))


# ---------------------------------------------------------------------------------------------------------------------
# randomized differential inputs
# ---------------------------------------------------------------------------------------------------------------------
def random_sampler_case(seed):
    rng = np.random.default_rng(7000 + seed)
    E, H1, W1 = int(rng.integers(1, 4)), int(rng.integers(1, 11)), int(rng.integers(1, 11))
    H2, W2 = int(rng.integers(1, 25)), int(rng.integers(1, 25))
    radius = int(rng.integers(1, 6))
    osc = float(rng.choice([2.0, 4.0, 20.0]))
    sigma = float(rng.choice([1.0, 5.0, 30.0]))
    desc = dict(E=E, H1=H1, W1=W1, H2=H2, W2=W2, radius=radius, off_scale=osc, sigma=sigma)
    return desc, make_sampler_inputs(rng, E, H1, W1, H2, W2, radius, sigma, osc)


def random_altcorr_case(seed):
    rng = np.random.default_rng(8000 + seed)
    B, H1, W1 = int(rng.integers(1, 4)), int(rng.integers(1, 11)), int(rng.integers(1, 11))
    H2, W2 = int(rng.integers(1, 25)), int(rng.integers(1, 25))
    radius = int(rng.integers(1, 4))          # the operator serves radius <= 3: its lattice must fit one wave
    C = int(rng.choice([32, 64, 96, 128]))
    S = int(rng.choice([1, 2]))
    sigma = float(rng.choice([1.0, 5.0, 30.0]))
    desc = dict(B=B, S=S, H1=H1, W1=W1, H2=H2, W2=W2, C=C, radius=radius, sigma=sigma)
    return desc, make_altcorr_inputs(rng, B, S, H1, W1, H2, W2, C, radius, sigma)


def ratio(got, ref, A):
    """Largest |got - ref| / (u A) over the elements with A > 2^-100 (0 if there are none); below that the underflow
    term of the bound governs, not K."""
    got, ref, A = (np.asarray(a, np.float64) for a in (got, ref, A))
    m = A > 2.0 ** -100
    return float((np.abs(got - ref)[m] / (U * A[m])).max()) if m.any() else 0.0
