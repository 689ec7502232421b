"""Float64 restatement of the Gaussian mask's parameter head (csrc/gausshead.hip, include/lgu_corr.h lgu_gaussian_head;
reference droid_slam/gaussianMask_cuda.py:69-73) and the per-element bound on what the kernel may return.

    s1 = b1 + W1 . x          tt = tanh(s1)          s2 = [bm; bc] + [Wm; Wc] . tt

The chain runs on the operands as the kernel sees them (half mode: rounded to half once; fp32 mode: the fp32 values) with NO
rounding in between; the roundings are what the bound allows for.  Everything is CPU float64 and follows from the
arithmetic, nothing here is measured:

half mode
    a1   = allowance(s1, S1, 256 + 2)                         fp32 accumulation of 256 exact products and the bias in any
                                                              order, one rounding to half, the half subnormal floor
    a2   = a1 + 2^-11 (|tanh s1| + a1) + 4 2^-24 + 2^-25      tanh has largest slope 1, is evaluated in fp32 (4 units at
                                                              |tanh| <= 1) and rounded to half once
    out  = a2 pushed through |W2_h|, plus allowance(s2, S2 + pushed, 16 + 2) + 2^-11 pushed: the pushed amount is counted into
           the layer's S and into the value that is rounded, as conv3_restatement.stack does for a convolution
fp32 mode: no half roundings; products are no longer exact (one rounding per term of the fused multiply-add chain)
    a1   = (2 256 + 2) 2^-24 S1          a2 = a1 + 4 2^-24          out = pushed + (2 16 + 2) 2^-24 (S2 + pushed)
"""
import torch

from tests.conv3_restatement import U24, allowance, h64

CIN, HID = 256, 16
TERMS1, TERMS2 = CIN + 2, HID + 2


def f64(t):
    """The fp32 value of t, as float64."""
    return t.detach().cpu().float().double()


def weights(map, meanMap, covMap):
    """(W1 (16,256), b1 (16), W2 (4,16), b2 (4)) float32 of the three Linear modules: W2 = [meanMap; covMap]."""
    W2 = torch.cat((meanMap.weight.detach().cpu().float(), covMap.weight.detach().cpu().float()))
    b2 = torch.cat((meanMap.bias.detach().cpu().float(), covMap.bias.detach().cpu().float()))
    return map.weight.detach().cpu().float(), map.bias.detach().cpu().float(), W2, b2


def make_weights(seed):
    """Seeded (W1, b1, W2, b2) float32 of the reference's scale (normal, std sqrt(2/16) and sqrt(2/2)) with a NON-ZERO mean
    head and non-zero biases (the reference's initialisation zeroes them)."""
    g = torch.Generator().manual_seed(seed)
    W1 = torch.randn((HID, CIN), generator=g) * (2.0 / HID) ** 0.5
    b1 = torch.randn((HID,), generator=g) * 0.5
    W2 = torch.randn((4, HID), generator=g)
    b2 = torch.randn((4,), generator=g) * 0.5
    return W1, b1, W2, b2


def load(ga, W1, b1, W2, b2):
    """Put (W1, b1, W2, b2) into the GaussianMask `ga` (map is shared with mapA[0])."""
    with torch.no_grad():
        ga.map.weight.copy_(W1), ga.map.bias.copy_(b1)
        ga.meanMap.weight.copy_(W2[:2]), ga.meanMap.bias.copy_(b2[:2])
        ga.covMap.weight.copy_(W2[2:]), ga.covMap.bias.copy_(b2[2:])
    return ga


def make_input(seed, E, h, w):
    """Seeded (E,h,w,256) float32 of the scale of the concatenated feature pair (the fixture's maps have std about 0.3)."""
    g = torch.Generator().manual_seed(seed)
    return torch.randn((E, h, w, CIN), generator=g) * 0.3


def chain(x, W1, b1, W2, b2, half):
    """The float64 chain on the kernel's operands: a dict of s1, S1, tt, s2, S2, W2 (the rounded |W2| is what allowances are
    pushed through), each (E,h,w,.) float64."""
    r = h64 if half else f64
    xr, W1r, b1r, W2r, b2r = r(x), r(W1), r(b1), r(W2), r(b2)
    s1 = xr @ W1r.T + b1r
    S1 = xr.abs() @ W1r.abs().T + b1r.abs()
    tt = torch.tanh(s1)
    s2 = tt @ W2r.T + b2r
    S2 = tt.abs() @ W2r.abs().T + b2r.abs()
    return dict(s1=s1, S1=S1, tt=tt, s2=s2, S2=S2, W2=W2r)


def bounds(c, half):
    """(a1, a2, a_out): allowed |u - s1|, |tt - tanh s1| and |out - s2| per element of the chain `c`."""
    if half:
        a1 = allowance(c["s1"], c["S1"], TERMS1)
        a2 = a1 + 2.0 ** -11 * (c["tt"].abs() + a1) + 4 * U24 + 2.0 ** -25
        moved = a2 @ c["W2"].abs().T
        return a1, a2, moved + allowance(c["s2"], c["S2"] + moved, TERMS2) + 2.0 ** -11 * moved
    a1 = (2 * CIN + 2) * U24 * c["S1"]
    a2 = a1 + 4 * U24
    moved = a2 @ c["W2"].abs().T
    return a1, a2, moved + (2 * HID + 2) * U24 * (c["S2"] + moved)


def split(s2):
    """(mean_ofs (E,h,w,2), cov_raw (E,h*w,2)) of the chain's (E,h,w,4)."""
    E, h, w, _ = s2.shape
    return s2[..., :2], s2[..., 2:].reshape(E, h * w, 2)
