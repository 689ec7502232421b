"""Float64 restatement of the rounding model of csrc/upmask.hip (include/lgu_corr.h, lgu_upmask1x1_c128_h16 and
lgu_upmask_upsample_f32): GraphAgg's upmask = Sequential(Conv2d(128, 576, 1)) under float16 autocast, alone and followed
by DepthVideo.upsample (reference droid_slam/droid_net.py:50-51,67, depth_video.py:124-128).

    x_h = half(x), w_h = half(weight), b_h = half(bias)
    s   = b_h + sum_c x_h[c] * w_h[co, c]
    h   = half(s)
    up  = tests/aggregate_restatement.cvx_upsample64(disps, h, half_weights)      on a GIVEN mask h

The sum is an einsum over the channels, without a convolution call; the test file compares it with
torch.nn.functional.conv2d.  The allowance is tests/conv3_restatement.allowance with TERMS = 128 * 1 * 1 + 2 (the rule of
conv3_restatement.stack).  Everything is CPU float64.
"""
import numpy as np
import torch

from tests import aggregate_restatement as RA
from tests import conv3_restatement as R

CIN, COUT = 128, 576
TERMS = CIN * 1 * 1 + 2       # 130
UPS_TOL = 4e-6                # |up - ref| <= UPS_TOL * max_k |d_k| with float weights
HALF_FLIP = 2.0 ** -11 + UPS_TOL     # half weights: an output may instead be off by one half ulp of a weight ...
HALF_FLIP_FRACTION = 2e-3            # ... for at most this fraction of the outputs


def make_upmask(seed, gain=1.0, sequential=True):
    """The reference's GraphAgg.upmask with seeded default initialisation (CPU, float32); gain scales the weight (gain 3
    with conv3_restatement.make_input gives mask values of the spread tests/test_aggregate.py draws, about 3)."""
    torch.manual_seed(seed)
    conv = torch.nn.Conv2d(CIN, COUT, 1, padding=0)
    with torch.no_grad():
        conv.weight.mul_(gain)
    return torch.nn.Sequential(conv) if sequential else conv


def conv_of(m):
    return m[0] if isinstance(m, torch.nn.Sequential) else m


def layer(x, weight, bias):
    """(s64, S): s = b_h + sum_c x_h * w_h and S = |b_h| + sum_c |x_h * w_h|, float64."""
    xh, wh, bh = R.h64(x), R.h64(weight).reshape(COUT, CIN), R.h64(bias)
    s = torch.einsum("nchw,oc->nohw", xh, wh) + bh.view(1, -1, 1, 1)
    S = torch.einsum("nchw,oc->nohw", xh.abs(), wh.abs()) + bh.abs().view(1, -1, 1, 1)
    return s, S


def single(bias, product):
    """half(b_h + p) for a sum of ONE product p = x_h * w_h (given as float32, where it is exact): the kernel's model is one
    fp32 addition and one rounding to half."""
    return (bias.to(torch.float16).float() + product.float()).to(torch.float16)


def disparities(seed, N, ht, wd):
    """tests/test_aggregate.py's disparity recipe: 0.05 + 1.5 * uniform."""
    g = torch.Generator().manual_seed(seed)
    return (0.05 + 1.5 * torch.rand(N, ht, wd, generator=g)).float()


def upsample(disps, ix, mask_h, half_weights):
    """(rows, want64, bound): the float64 convex upsampling of disps[ix[u]] with the GIVEN half mask mask_h[u], for the u
    with 0 <= ix[u] < N; rows are those ix[u], bound is max_k |d_k| per output."""
    disps = np.asarray(disps, dtype=np.float32)
    ix = np.asarray(ix, dtype=np.int64)
    keep = [u for u in range(len(ix)) if 0 <= ix[u] < disps.shape[0]]
    rows = ix[keep]
    d = disps[rows]
    m = np.asarray(mask_h)[keep].astype(np.float32)
    return rows, RA.cvx_upsample64(d, m, half_weights), RA.upsample_bound(d)


def upsample_ratio(got, want64, bound):
    return np.abs(np.asarray(got, dtype=np.float64) - want64) / bound


def within(r, half_weights):
    """The tolerance the project holds upsample_disps_ to on the ratios r = |up - ref| / max_k |d_k|."""
    if not half_weights:
        return bool(r.max() <= UPS_TOL)
    return bool(r.max() <= HALF_FLIP) and bool((r > UPS_TOL).mean() <= HALF_FLIP_FRACTION)
