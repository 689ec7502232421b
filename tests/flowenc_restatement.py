"""Float64 restatement of the rounding model of csrc/flowenc.hip (include/lgu_corr.h, lgu_flow_conv7_relu_h16) and of the
two-layer motion encoder under float16 autocast (reference droid_slam/droid_net.py:82-86).

    x_h = half(x), w_h = half(weight), b_h = half(bias)
    s   = b_h + sum_{c,ky,kx} x_h[c, y + ky - 3, x + kx - 3] * w_h[co, c, ky, kx]        (zero padding)
    y   = relu(half(s))

The sums here are written as shifted slices, one window position at a time, without a convolution call; the test file
compares them with torch.nn.functional.conv2d.  Everything is CPU float64.
"""
import torch

U24 = 2.0 ** -24
TERMS1 = 4 * 7 * 7 + 2        # 198: the additions of the first layer's sum (196 products and the bias) and their slack
TERMS2 = 128 * 3 * 3 + 2      # 1154: the same for the second layer


def make_module(seed):
    """The reference's flow_encoder with seeded default initialisation (CPU, float32)."""
    torch.manual_seed(seed)
    nn = torch.nn
    return nn.Sequential(nn.Conv2d(4, 128, 7, padding=3), nn.ReLU(inplace=True), nn.Conv2d(128, 64, 3, padding=1),
                         nn.ReLU(inplace=True))


def make_input(seed, N, H, W):
    """Clamped normals scaled to reach +-64, with exact +-64 entries (what lgu_motion_features_f32 can write)."""
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn((N, 4, H, W), generator=g) * 40.0).clamp_(-64.0, 64.0)
    flat = x.view(-1)
    if flat.numel():
        flat[0] = 64.0
        flat[-1] = -64.0
        flat[flat.numel() // 2] = 64.0
    return x


def h64(t):
    """The half rounding of t, as float64."""
    return t.detach().cpu().to(torch.float16).double()


def window_sums(xh, wh, bh, pad):
    """(s64, S): s = b + sum x * w and S = |b| + sum |x * w| over the window, float64, by shifted slices."""
    N, C, H, W = xh.shape
    K = wh.shape[2]
    xp = torch.nn.functional.pad(xh, (pad, pad, pad, pad))
    s = bh.view(1, -1, 1, 1).expand(N, wh.shape[0], H, W).clone()
    S = bh.abs().view(1, -1, 1, 1).expand(N, wh.shape[0], H, W).clone()
    for ky in range(K):
        for kx in range(K):
            sl = xp[:, :, ky:ky + H, kx:kx + W]
            s += torch.einsum("nchw,oc->nohw", sl, wh[:, :, ky, kx])
            S += torch.einsum("nchw,oc->nohw", sl.abs(), wh[:, :, ky, kx].abs())
    return s, S


def conv7_relu(x, weight, bias):
    """(s64, S, want) of the first layer: want = relu(half(s64)) as a half tensor."""
    s, S = window_sums(h64(x), h64(weight), h64(bias), 3)
    return s, S, torch.relu(s.to(torch.float16))


def allowance(s64, S, terms):
    """|y - relu(s64)| allowed per element: fp32 accumulation of `terms` additions in any order, one half rounding of the
    accumulated value, and the half subnormal floor."""
    acc = terms * U24 * S
    return acc + 2.0 ** -11 * (s64.abs() + acc) + 2.0 ** -25


def encoder(x, module):
    """(s2, bound) of the whole encoder: the float64 chain s2 = conv2(relu(s1)) on half-rounded inputs and parameters
    (no rounding in between: the roundings are what the bound allows for), and the bound on |out - relu(s2)|: the first
    layer's allowance pushed through |w2_h| plus the second layer's own."""
    F = torch.nn.functional
    c1, c2 = module[0], module[2]
    s1, S1, _ = conv7_relu(x, c1.weight, c1.bias)
    y1 = torch.relu(s1)
    w2, b2 = h64(c2.weight), h64(c2.bias)
    s2 = F.conv2d(y1, w2, b2, padding=1)
    S2 = F.conv2d(y1.abs(), w2.abs(), b2.abs(), padding=1)
    through = F.conv2d(allowance(s1, S1, TERMS1), w2.abs(), None, padding=1)
    return s2, through + allowance(s2, S2, TERMS2)
