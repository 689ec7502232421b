"""Float64 restatement of the rounding models of csrc/encends.hip (include/lgu_corr.h, lgu_encstem7x7_h16 and
lgu_encout1x1_c128_h16): the two ends of the reference's BasicEncoder (droid_slam/modules/extractor.py: conv1, conv2) under
float16 autocast, and the slot formulas of their weight packs.

    stem    x_h = half(x), w_h = half(weight), b_h = half(bias)
            s   = b_h + sum_{c,ky,kx} x_h[c, 2 y + ky - 3, 2 x + kx - 3] * w_h[co, c, ky, kx]   (zero padding, Ho = ceil(H / 2))
            y   = half(s) | relu(half(s))
    output  p   = sum_c x[c] * w_h[co, c];  h = half(b_h + p)
            net = half(tanh(h[:128])), inp = relu(h[128:])                                      (SPLIT, Cout 256)

The sums are written as shifted, strided slices, one window position at a time, without a convolution call; the test
file compares them with torch.nn.functional.conv2d.  Everything is CPU float64.
"""
import torch

from tests.conv3_restatement import allowance, h64  # noqa: F401  (the layer allowance, unchanged)

STEM_TERMS = 7 * 7 * 3 + 2      # 149: the additions of the stem's sum (147 products and the bias) and their slack
OUT_TERMS = 128 + 2             # 130: the rule of encconv_restatement.terms1
COUTS = (128, 256)
# (N, H, W): odd and even sizes, Wo across 16, 32, 64 and 128, several tile rows
STEM_SIZES = [(1, 1, 1), (1, 2, 2), (1, 2, 3), (2, 9, 33), (2, 10, 34), (1, 5, 65), (3, 16, 40), (1, 17, 130), (1, 34, 258)]
# pixel counts off every multiple of 4, 8, 16 and 32
OUT_SIZES = [(1, 1, 1), (1, 2, 3), (2, 9, 33), (1, 5, 65), (3, 16, 40), (1, 17, 130)]


def out_size(H, W):
    return (H + 1) // 2, (W + 1) // 2


def make_stem(seed):
    """Conv2d(3, 32, 7, stride=2, padding=3), seeded default initialisation (CPU, float32)."""
    torch.manual_seed(seed)
    return torch.nn.Conv2d(3, 32, 7, stride=2, padding=3)


def make_out(seed, cout):
    """Conv2d(128, cout, 1), seeded default initialisation (CPU, float32)."""
    torch.manual_seed(seed)
    return torch.nn.Conv2d(128, cout, 1)


def make_image(seed, N, H, W):
    """Seeded normals of scale 1.2: the range of a normalised image (float32)."""
    g = torch.Generator().manual_seed(seed)
    return torch.randn((N, 3, H, W), generator=g) * 1.2


def make_features(seed, N, H, W):
    """Seeded normals of scale 2 with a fifth exact zeros: what layer3's last ReLU hands the output layer (float32)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((N, 128, H, W), generator=g) * 2.0
    x[torch.rand((N, 128, H, W), generator=g) < 0.2] = 0.0
    return x


def stem_sums(xh, wh, bh):
    """(s64, S): s = b + sum x * w and S = |b| + sum |x * w| over the 7x7 window, stride 2, padding 3, float64."""
    N, C, H, W = xh.shape
    Ho, Wo = out_size(H, W)
    xp = torch.nn.functional.pad(xh, (3, 3, 3, 3))        # input row 2 y + ky - 3 is row 2 y + ky here
    co = wh.shape[0]
    s = bh.view(1, -1, 1, 1).expand(N, co, Ho, Wo).clone()
    S = bh.abs().view(1, -1, 1, 1).expand(N, co, Ho, Wo).clone()
    for ky in range(7):
        for kx in range(7):
            sl = xp[:, :, ky:ky + 2 * (Ho - 1) + 1:2, kx:kx + 2 * (Wo - 1) + 1:2]
            s += torch.einsum("nchw,oc->nohw", sl, wh[:, :, ky, kx])
            S += torch.einsum("nchw,oc->nohw", sl.abs(), wh[:, :, ky, kx].abs())
    return s, S


def out_sums(xh, wh, bh):
    """(s64, S) of the 1x1 layer, float64."""
    w = wh[:, :, 0, 0]
    s = bh.view(1, -1, 1, 1) + torch.einsum("nchw,oc->nohw", xh, w)
    S = bh.abs().view(1, -1, 1, 1) + torch.einsum("nchw,oc->nohw", xh.abs(), w.abs())
    return s, S


def stem(x, conv):
    return stem_sums(h64(x), h64(conv.weight), h64(conv.bias))


def out(x, conv):
    return out_sums(h64(x), h64(conv.weight), h64(conv.bias))


def stem_slots():
    """(co, c, ky, kx, holds) of every slot [ky][ct][lane][j] of the stem's pack, index tensors of shape (7,2,64,8): the
    slot holds w_h[co, c, ky, kx] where `holds`, zero elsewhere (c and kx are clamped into range there)."""
    ky, ct, lane, j = torch.meshgrid(torch.arange(7), torch.arange(2), torch.arange(64), torch.arange(8), indexing="ij")
    co, c, kx = 16 * ct + (lane & 15), j & 3, 2 * (lane >> 4) + (j >> 2)
    holds = (c < 3) & (kx < 7)
    return co, c.clamp(max=2), ky, kx.clamp(max=6), holds


def out_slots(cout):
    """(co, c) of every slot [kc][ct][lane][j] of the output layer's pack, shape (4,cout/16,64,8): every slot holds
    w_h[co, c]."""
    kc, ct, lane, j = torch.meshgrid(torch.arange(4), torch.arange(cout // 16), torch.arange(64), torch.arange(8), indexing="ij")
    return 16 * ct + (lane & 15), 32 * kc + 8 * (lane >> 4) + j


def tanh_bound(h):
    """(t, bound): t = tanh of the float64 h and |net - t| allowed: one half rounding of a float tanh within the 5 ulp the
    device library's float tanh is specified to, 2^-11 (|t| + e) + e + 2^-25 with e = 5 * 2^-23 |t|."""
    t = torch.tanh(h)
    e = 5 * 2.0 ** -23 * t.abs()
    return t, 2.0 ** -11 * (t.abs() + e) + e + 2.0 ** -25
