"""Float64 restatement of the rounding model of csrc/heads.hip (include/lgu_corr.h, lgu_head3x3_c128_h16) and of the tails
of the update operator that end in such a head, under float16 autocast (reference droid_slam/droid_net.py: delta[2],
weight[2] + Sigmoid, GraphAgg.eta + GradientClip + Softplus).

    x_h = half(x), w_h = half(weight), b_h = half(bias)
    s   = b_h + sum_{c,ky,kx} x_h[c, y + ky - 1, x + kx - 1] * w_h[co, c, ky, kx]        (zero padding)
    h   = half(s)
    y   = h | half(sigmoid(h)) | softplus(h) as float32

The sums are tests/conv3_restatement.py's shifted slices (the layer has the same 1152 products and bias, so the same
allowance with TERMS = 1154); what is new here are the activations' allowances.  Everything is CPU float64.
"""
import torch

from tests import conv3_restatement as R

U24 = R.U24
TERMS = R.TERMS
# softplus_f32's own error in units of 2^-24 * y.  It is not derivable from the format alone, so it follows a measurement:
# torch's own HIP softplus against float64 on the half values of the bound test was at most 1.72 units on an MI355X
# (printed by test_heads.py::test_every_element_is_within_the_derived_bound), and k = max(4, 2 x that).
K_SOFTPLUS = 4.0
ACTS = ("none", "sigmoid", "softplus")


def make_head(seed, cout):
    """Conv2d(128, cout, 3, padding=1) with seeded default initialisation (CPU, float32)."""
    return R.make_conv(seed, cout)


def make_tail(seed, cout, act):
    """[conv, Identity (GradientClip's forward), activation]: the reference's GraphAgg.eta for (1, "softplus")."""
    nn = torch.nn
    torch.manual_seed(seed)
    last = {"none": [], "sigmoid": [nn.Sigmoid()], "softplus": [nn.Softplus()]}[act]
    return nn.Sequential(nn.Conv2d(128, cout, 3, padding=1), R.Identity(), *last)


def make_update(seed):
    """conv3_restatement's Update with the `eta` tail of the reference's GraphAgg added to its `agg`."""
    u = R.make_update(seed)
    u.agg.eta = make_tail(seed + 1000, 1, "softplus")
    return u


def softplus64(s):
    """log(1 + exp(s)) without overflow, float64."""
    return torch.clamp(s, min=0.0) + torch.log1p(torch.exp(-s.abs()))


def act64(s, act):
    if act == "sigmoid":
        return torch.sigmoid(s)
    if act == "softplus":
        return softplus64(s)
    return s


def act_allowance(y, allow, act):
    """The allowance on act(h) given the float64 value y = act(s64) and the allowance `allow` on h:
    sigmoid (conv3_restatement.stack's model): largest slope 1/4, one half rounding, 4 fp32 units;
    softplus: slope <= 1, K_SOFTPLUS fp32 units of the float32 result, no further rounding."""
    if act == "sigmoid":
        a = 0.25 * allow
        return a + 2.0 ** -11 * (y + a) + 4 * U24 * y + 2.0 ** -25
    if act == "softplus":
        return allow + K_SOFTPLUS * U24 * y
    return allow


def head(x, weight, bias):
    """(s64, S) of one head."""
    return R.window_sums(R.h64(x), R.h64(weight), R.h64(bias), 1)


def tail(x, seq):
    """(ref, bound) of a Sequential that conv3_restatement.stack understands, optionally ending in a Softplus."""
    members = list(seq)
    if members and isinstance(members[-1], torch.nn.Softplus):
        y, allow = R.stack(x, members[:-1])
        ref = softplus64(y)
        return ref, act_allowance(ref, allow, "softplus")
    return R.stack(x, members)
