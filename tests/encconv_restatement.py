"""Float64 restatement of the rounding model of csrc/encconv.hip (include/lgu_corr.h, lgu_encconv3x3_h16): the residual
stages' convolutions of the reference's BasicEncoder (droid_slam/modules/extractor.py) under float16 autocast.

    w_h = half(weight), b_h = half(bias), x half
    s   = b_h + sum_{c,ky,kx} x[c, st y + ky - 1, st x + kx - 1] * w_h[co, c, ky, kx]     (zero padding, Ho = ceil(H / st))
    y0  = half(s);   y = y0 | relu(y0) | relu(half(res + relu(y0)))
    r   = half(b'_h + sum_c x[c, 2 y, 2 x] * w'_h[co, c])                                  (the 1x1 stride-2 branch)

The sums are written as shifted, strided slices, one window position at a time, without a convolution call; the test
file compares them with torch.nn.functional.conv2d.  Everything is CPU float64.
"""
import torch

from tests.conv3_restatement import allowance, h64, make_input  # noqa: F401  (the layer allowance, unchanged)

SHAPES = ((32, 32, 1), (32, 64, 2), (64, 64, 1), (64, 128, 2), (128, 128, 1))
# (N, H, W) of the input: the project's edge shapes with their even partners for stride 2
EDGE_SIZES = [(1, 1, 1), (1, 2, 2), (1, 2, 3), (2, 9, 33), (2, 10, 34), (1, 5, 65), (3, 16, 40), (1, 17, 130)]
# one production plane per input width: the stem's output of a 384x512 frame, layer1's and layer2's
PRODUCTION = {32: (1, 192, 256), 64: (1, 96, 128), 128: (1, 48, 64)}
EPILOGUES = ("identity", "relu", "residual")


def sizes(cin):
    return EDGE_SIZES + [PRODUCTION[cin]]


def terms3(cin):
    """The additions of the 3x3 sum (9 Cin products and the bias) and their slack."""
    return 9 * cin + 2


def terms1(cin):
    return cin + 2


def out_size(H, W, stride):
    return (H + stride - 1) // stride, (W + stride - 1) // stride


def make_layer(seed, cin, cout, stride):
    """(conv3, conv1): Conv2d(cin, cout, 3, stride, padding=1) and the block's Conv2d(cin, cout, 1, stride=2) (None with
    stride 1), seeded default initialisation (CPU, float32)."""
    torch.manual_seed(seed)
    c3 = torch.nn.Conv2d(cin, cout, 3, stride=stride, padding=1)
    c1 = torch.nn.Conv2d(cin, cout, 1, stride=2) if stride == 2 else None
    return c3, c1


def make_residual(seed, shape):
    """A half residual of scale 2 with exact zeros and negative values: what a block's input (or its branch) looks like."""
    g = torch.Generator().manual_seed(seed)
    r = torch.randn(shape, generator=g) * 2.0
    r[torch.rand(shape, generator=g) < 0.2] = 0.0
    return r.half()


def window_sums(xh, wh, bh, stride):
    """(s64, S): s = b + sum x * w and S = |b| + sum |x * w| over the 3x3 window with padding 1, float64."""
    N, C, H, W = xh.shape
    Ho, Wo = out_size(H, W, stride)
    xp = torch.nn.functional.pad(xh, (1, 1, 1, 1))        # input row stride * y + ky - 1 is row stride * y + ky here
    co = wh.shape[0]
    s = bh.view(1, -1, 1, 1).expand(N, co, Ho, Wo).clone()
    S = bh.abs().view(1, -1, 1, 1).expand(N, co, Ho, Wo).clone()
    for ky in range(3):
        for kx in range(3):
            sl = xp[:, :, ky:ky + stride * (Ho - 1) + 1:stride, kx:kx + stride * (Wo - 1) + 1:stride]
            s += torch.einsum("nchw,oc->nohw", sl, wh[:, :, ky, kx])
            S += torch.einsum("nchw,oc->nohw", sl.abs(), wh[:, :, ky, kx].abs())
    return s, S


def branch_sums(xh, wh, bh):
    """(s64, S) of the 1x1 stride-2 branch: pixel (2y, 2x)."""
    sl = xh[:, :, ::2, ::2]
    w = wh[:, :, 0, 0]
    s = bh.view(1, -1, 1, 1) + torch.einsum("nchw,oc->nohw", sl, w)
    S = bh.abs().view(1, -1, 1, 1) + torch.einsum("nchw,oc->nohw", sl.abs(), w.abs())
    return s, S


def epilogue(s64, kind, res=None):
    """The float64 value of an epilogue on the unrounded sum; res: float64."""
    if kind == "identity":
        return s64
    if kind == "relu":
        return torch.relu(s64)
    assert kind == "residual"
    return torch.relu(res + torch.relu(s64))


def allowed(s64, S, terms, kind, res=None):
    """|y - epilogue(s64)| allowed per element: the layer's allowance (relu and the identity do not widen it), and for the
    residual epilogue the one further half rounding of the sum."""
    a = allowance(s64, S, terms)
    if kind != "residual":
        return a
    return a + 2.0 ** -11 * ((res + torch.relu(s64)).abs() + a) + 2.0 ** -25


def conv(x, c3, c1=None):
    """(s64, S) of the layer and (r64, Sr) of its branch (None, None without one) for the half input x."""
    xh, st = h64(x), c3.stride[0]
    s, S = window_sums(xh, h64(c3.weight), h64(c3.bias), st)
    if c1 is None:
        return s, S, None, None
    r, Sr = branch_sums(xh, h64(c1.weight), h64(c1.bias))
    return s, S, r, Sr
