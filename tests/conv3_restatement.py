"""Float64 restatement of the rounding model of csrc/conv3.hip (include/lgu_corr.h, lgu_conv3x3_c128_h16) and of the
Sequentials of the update operator that hold such a layer, under float16 autocast (reference droid_slam/droid_net.py:
corr_encoder, delta, weight, flow_encoder[2], GraphAgg.conv1 / conv2).

    x_h = half(x), w_h = half(weight), b_h = half(bias)
    s   = b_h + sum_{c,ky,kx} x_h[c, y + ky - 1, x + kx - 1] * w_h[co, c, ky, kx]        (zero padding)
    y   = act(half(s)),  act = relu or the identity

The sums here are written as shifted slices, one window position at a time, without a convolution call; the test file
compares them with torch.nn.functional.conv2d.  Everything is CPU float64.
"""
import torch

U24 = 2.0 ** -24
TERMS = 128 * 3 * 3 + 2       # 1154: the additions of the layer's sum (1152 products and the bias) and their slack
COR_PLANES = 196              # 4 levels x 7 x 7: the width of corr_encoder's input


class Identity(torch.nn.Module):
    """Stand-in for the reference's GradientClip, whose forward is the identity."""

    def forward(self, x):
        return x


def make_conv(seed, cout):
    """Conv2d(128, cout, 3, padding=1) with seeded default initialisation (CPU, float32)."""
    torch.manual_seed(seed)
    return torch.nn.Conv2d(128, cout, 3, padding=1)


def _stack(kind):
    nn = torch.nn
    if kind == "corr_encoder":
        return nn.Sequential(nn.Conv2d(COR_PLANES, 128, 1, padding=0), nn.ReLU(inplace=True), nn.Conv2d(128, 128, 3, padding=1),
                             nn.ReLU(inplace=True))
    head = [nn.Conv2d(128, 128, 3, padding=1), nn.ReLU(inplace=True), nn.Conv2d(128, 2, 3, padding=1), Identity()]
    if kind == "delta":
        return nn.Sequential(*head)
    assert kind == "weight"
    return nn.Sequential(*head, nn.Sigmoid())


def make_stack(seed, kind):
    """The reference's corr_encoder, delta or weight with seeded default initialisation (CPU, float32)."""
    torch.manual_seed(seed)
    return _stack(kind)


class Agg(torch.nn.Module):
    """The convolutional part of the reference's GraphAgg: relu(conv1), a mean over the edges of a frame (here: over all
    of them), relu(conv2)."""

    def __init__(self):
        super().__init__()
        self.conv1 = torch.nn.Conv2d(128, 128, 3, padding=1)
        self.conv2 = torch.nn.Conv2d(128, 128, 3, padding=1)
        self.relu = torch.nn.ReLU(inplace=True)

    def forward(self, net):
        net = self.relu(self.conv1(net))
        net = net.mean(dim=0, keepdim=True)
        return self.relu(self.conv2(net))


class Update(torch.nn.Module):
    """Local stand-in shaped like the reference's UpdateModule: the attributes conv3.install_update names."""

    def __init__(self):
        super().__init__()
        nn = torch.nn
        self.corr_encoder = _stack("corr_encoder")
        self.flow_encoder = nn.Sequential(nn.Conv2d(4, 128, 7, padding=3), nn.ReLU(inplace=True), nn.Conv2d(128, 64, 3, padding=1),
                                          nn.ReLU(inplace=True))
        self.weight = _stack("weight")
        self.delta = _stack("delta")
        self.agg = Agg()


def make_update(seed):
    """An Update with seeded default initialisation (CPU, float32)."""
    torch.manual_seed(seed)
    return Update()


def make_input(seed, N, H, W, C=128):
    """Seeded normals of scale 2 with exact zeros sprinkled in (about a third): what layers behind a ReLU see."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((N, C, H, W), generator=g) * 2.0
    x[torch.rand((N, C, H, W), generator=g) < 0.3] = 0.0
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


def through(allow, wh, pad):
    """An allowance on a layer's input pushed through |w_h|: what it can move the layer's sum by."""
    N, C, H, W = allow.shape
    K = wh.shape[2]
    ap = torch.nn.functional.pad(allow, (pad, pad, pad, pad))
    t = torch.zeros((N, wh.shape[0], H, W), dtype=torch.float64)
    for ky in range(K):
        for kx in range(K):
            t += torch.einsum("nchw,oc->nohw", ap[:, :, ky:ky + H, kx:kx + W], wh[:, :, ky, kx].abs())
    return t


def act(s, relu):
    return torch.relu(s) if relu else s


def conv3(x, weight, bias, relu):
    """(s64, S, want) of one layer: want = act(half(s64)) as a half tensor."""
    s, S = window_sums(h64(x), h64(weight), h64(bias), 1)
    return s, S, act(s.to(torch.float16), relu)


def allowance(s64, S, terms):
    """|y - act(s64)| allowed per element: fp32 accumulation of `terms` additions in any order, one half rounding of the
    accumulated value, and the half subnormal floor.  (relu and the identity do not widen it.)"""
    acc = terms * U24 * S
    return acc + 2.0 ** -11 * (s64.abs() + acc) + 2.0 ** -25


def stack(x, seq):
    """(ref, bound) of a whole Sequential under float16 autocast: the float64 chain on the half-rounded input and
    parameters with no rounding in between (the roundings are what the bound allows for), and the bound on
    |out - ref|.  Through a convolution the allowance so far is pushed through |w_h| and the layer adds its own, with
    the pushed amount counted into its S and into the value that is rounded (its operands may be that much larger than
    the chain's); ReLU and the identity
    keep an allowance; a sigmoid, evaluated in fp32 and rounded to half once, scales it by its largest slope 1/4 and adds
    a half rounding and 4 fp32 units of its own."""
    nn = torch.nn
    y = h64(x)
    allow = torch.zeros_like(y)
    for m in seq:
        if isinstance(m, nn.Conv2d):
            wh, bh, pad = h64(m.weight), h64(m.bias), m.padding[0]
            s, S = window_sums(y, wh, bh, pad)
            moved = through(allow, wh, pad)
            terms = m.in_channels * m.kernel_size[0] * m.kernel_size[1] + 2
            y, allow = s, moved + allowance(s, S + moved, terms) + 2.0 ** -11 * moved
        elif isinstance(m, nn.ReLU):
            y = torch.relu(y)
        elif isinstance(m, nn.Sigmoid):
            y = torch.sigmoid(y)
            allow = 0.25 * allow
            allow = allow + 2.0 ** -11 * (y + allow) + 4 * U24 * y + 2.0 ** -25
        else:
            assert isinstance(m, Identity), type(m)
    return y, allow
