"""Float64 restatement of the rounding model of csrc/conv1.hip (include/lgu_corr.h, lgu_conv1x1_o128_h16): a
Conv2d(Cin, 128, 1) with its bias and an optional ReLU under float16 autocast (reference droid_slam/droid_net.py:
corr_encoder[0] = Conv2d(196, 128, 1) + ReLU).

    x_h = half(x), w_h = half(weight), b_h = half(bias)
    s   = b_h + sum_{c < Cin} x_h[c] * w_h[co, c]
    y   = act(half(s)),  act = relu or the identity

The sum is an einsum over the channels, without a convolution call; the test file compares it with
torch.nn.functional.conv2d.  The allowance is tests/conv3_restatement.allowance with terms = Cin + 2 (the rule of
conv3_restatement.stack: Cin * 1 * 1 products, the bias and slack).  Everything is CPU float64.
"""
import torch

from tests import conv3_restatement as R

COUT = 128


def terms(cin):
    return cin * 1 * 1 + 2


def make_conv(seed, cin):
    """Conv2d(cin, 128, 1) with seeded default initialisation (CPU, float32)."""
    torch.manual_seed(seed)
    return torch.nn.Conv2d(cin, COUT, 1, padding=0)


def layer(x, weight, bias):
    """(s64, S): s = b_h + sum_c x_h * w_h and S = |b_h| + sum_c |x_h * w_h|, float64."""
    cin = weight.shape[1]
    xh, wh, bh = R.h64(x), R.h64(weight).reshape(COUT, cin), R.h64(bias)
    s = torch.einsum("nchw,oc->nohw", xh, wh) + bh.view(1, -1, 1, 1)
    S = torch.einsum("nchw,oc->nohw", xh.abs(), wh.abs()) + bh.abs().view(1, -1, 1, 1)
    return s, S


def act(h, relu):
    """The kernel's activation on a half tensor: h < 0 ? 0 : h (a NaN is kept)."""
    return torch.where(h < 0, torch.zeros_like(h), h) if relu else h


def single(bias, product, relu=False):
    """act(half(b_h + p)) for a sum of ONE product p = x_h * w_h (given as float32, where it is exact): the kernel's model is
    one fp32 addition and one rounding to half."""
    return act((bias.to(torch.float16).float() + product.float()).to(torch.float16), relu)
