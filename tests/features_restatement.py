"""Float64 restatement of the fused instance-norm modes of csrc/instnorm.hip with their error allowance, a stand-in for
the reference's feature encoder (droid_slam/modules/extractor.py: BasicEncoder(128, 'instance')) written from its
architecture, and the seeded weights and inputs that tools/gen_features_golden.py and the tests share.

    IN(x) = (x - mean) / sqrt(var + eps) per (n, c) plane, biased variance, no affine terms
    mode 0  relu(IN(a))      mode 1  relu(b + relu(IN(a)))      mode 2  relu(IN(b) + relu(IN(a)))      mode 3  IN(a)

Allowance per element, with u = 2^-24, L = log2(hw) + 4 and k(x) = mean|x| / sqrt(var + eps) of the plane: a tree sum of
hw fp32 terms moves the mean by at most L u mean|x|, which IN divides by sqrt(var + eps); subtraction, centred sum,
square root, division and product add a handful of roundings relative to |y| + 1.
    E = u (L k(a) + 8 (|y_a| + 1))    mode 1: + 8 u |b|    mode 2: + u (L k(b) + 8 |y_b|)
fp32: |got - ref| <= E.  half: |got - ref| <= ulp_half(|ref| + E) / 2 + E, one rounding.

Encoder: conv1 7x7 stride 2 (3 -> 32), norm1, relu; layer1 (32), layer2 (64, stride 2), layer3 (128, stride 2) of two
residual blocks each; conv2 1x1 (128 -> output_dim).  A block is relu(norm1(conv1 x)), relu(norm2(conv2 .)), plus x (or
norm3(1x1 strided conv x) on the first block of a strided layer), relu.
"""
import hashlib
import math

import numpy as np
import torch
import torch.nn as nn

U = 2.0 ** -24
DIM = 32

# family -> (mu, sigma, dtypes)
FAMILIES = {
    "unit": (0.0, 1.0, ("f32", "h16")),
    "shift": (3.0, 0.5, ("f32", "h16")),
    "ill": (8.0, 0.05, ("f32", "h16")),
    "ill32": (1000.0, 0.01, ("f32",)),
    "tinyvar": (0.0, 0.003, ("f32", "h16")),
    "big": (0.0, 300.0, ("f32",)),
    "const": (0.1, 0.0, ("f32", "h16")),
}
DTYPES = {"f32": torch.float32, "h16": torch.float16}


def family_inputs(family, dtype, planes, hw, seed=0):
    """a, b (planes, hw) of `dtype` on the CPU: randn * sigma + mu, independent draws (numpy RandomState, so the same
    values everywhere), rounded to the dtype: the statistics are those of the stored values."""
    mu, sigma, _ = FAMILIES[family]
    rs = np.random.RandomState(1000 * seed + 7 * planes + hw % 9973)
    out = []
    for _ in range(2):
        x = rs.standard_normal((planes, hw)) * sigma + mu
        out.append(torch.from_numpy(x.astype(np.float32)).to(dtype))
    return out


def _plane_stats(x, eps):
    mean = x.mean(-1, keepdim=True)
    var = ((x - mean) ** 2).mean(-1, keepdim=True)
    sd = torch.sqrt(var + eps)
    return (x - mean) / sd, x.abs().mean(-1, keepdim=True) / sd


def reference(mode, a, b=None, eps=1e-5):
    """(value, E): the float64 result of `mode` on a, b (planes, hw) as stored, and the allowance per element."""
    a = a.double()
    hw = a.shape[-1]
    L = math.log2(hw) + 4
    ya, ka = _plane_stats(a, eps)
    E = U * (L * ka + 8 * (ya.abs() + 1))
    if mode == 0:
        return ya.clamp_min(0), E
    if mode == 3:
        return ya, E
    b = b.double()
    if mode == 1:
        return (b + ya.clamp_min(0)).clamp_min(0), E + U * 8 * b.abs()
    if mode == 2:
        yb, kb = _plane_stats(b, eps)
        return (yb + ya.clamp_min(0)).clamp_min(0), E + U * (L * kb + 8 * yb.abs())
    raise ValueError(mode)


def half_ulp(x):
    """ulp of IEEE half at |x| (float64 tensor): 2^(e - 10) for normal values, 2^-24 below 2^-14."""
    e = torch.floor(torch.log2(x.abs().clamp_min(2.0 ** -14)))
    return torch.pow(torch.tensor(2.0, dtype=torch.float64), e - 10)


def bound(ref, E, dtype):
    return E if dtype == torch.float32 else half_ulp(ref.abs() + E) / 2 + E


def torch_composition(mode, a, b=None, eps=1e-5):
    """The ops the kernel replaces, on a, b (planes, hw) viewed as (1, planes, hw, 1), in their dtype."""
    F = torch.nn.functional
    p, hw = a.shape

    def inorm(x):
        return F.instance_norm(x.view(1, p, hw, 1), eps=eps).view(p, hw)
    if mode == 0:
        return F.relu(inorm(a))
    if mode == 1:
        return F.relu(b + F.relu(inorm(a)))
    if mode == 2:
        return F.relu(inorm(b) + F.relu(inorm(a)))
    return inorm(a)


# ---- the encoder ---------------------------------------------------------------------------------------------------
class RefBlock(nn.Module):
    def __init__(self, cin, cout, stride):
        super().__init__()
        self.conv1 = nn.Conv2d(cin, cout, 3, stride=stride, padding=1)
        self.conv2 = nn.Conv2d(cout, cout, 3, padding=1)
        self.relu = nn.ReLU(inplace=True)
        self.norm1 = nn.InstanceNorm2d(cout)
        self.norm2 = nn.InstanceNorm2d(cout)
        self.downsample = None
        if stride != 1:
            self.norm3 = nn.InstanceNorm2d(cout)
            self.downsample = nn.Sequential(nn.Conv2d(cin, cout, 1, stride=stride), self.norm3)

    def forward(self, x):
        y = self.relu(self.norm1(self.conv1(x)))
        y = self.relu(self.norm2(self.conv2(y)))
        if self.downsample is not None:
            x = self.downsample(x)
        return self.relu(x + y)


class RefEncoder(nn.Module):
    """BasicEncoder(output_dim, norm_fn): the reference's attribute names and state_dict keys.  norm_fn 'instance' is the
    feature encoder; 'none' (empty Sequentials at the norm sites) is the context encoder's shape."""

    def __init__(self, output_dim=128, norm_fn="instance"):
        super().__init__()
        self.norm_fn = norm_fn
        self.conv1 = nn.Conv2d(3, DIM, 7, stride=2, padding=3)
        self.norm1 = nn.InstanceNorm2d(DIM)
        self.relu1 = nn.ReLU(inplace=True)
        self.layer1 = nn.Sequential(RefBlock(DIM, DIM, 1), RefBlock(DIM, DIM, 1))
        self.layer2 = nn.Sequential(RefBlock(DIM, 2 * DIM, 2), RefBlock(2 * DIM, 2 * DIM, 1))
        self.layer3 = nn.Sequential(RefBlock(2 * DIM, 4 * DIM, 2), RefBlock(4 * DIM, 4 * DIM, 1))
        self.conv2 = nn.Conv2d(4 * DIM, output_dim, 1)
        self.dropout = None
        if norm_fn == "none":
            for m in [self] + [b for name in ("layer1", "layer2", "layer3") for b in getattr(self, name)]:
                for attr in ("norm1", "norm2", "norm3"):
                    if hasattr(m, attr):
                        setattr(m, attr, nn.Sequential())
                if getattr(m, "downsample", None) is not None:
                    m.downsample = nn.Sequential(m.downsample[0], m.norm3)
        elif norm_fn != "instance":
            raise ValueError(norm_fn)

    def stages(self, x):
        """The outputs after the stem, layer1, layer2, layer3 and conv2 for x (B, N, 3, H, W)."""
        b, n, c, h, w = x.shape
        out = {}
        y = out["stem"] = self.relu1(self.norm1(self.conv1(x.view(b * n, c, h, w)))).clone()
        for name in ("layer1", "layer2", "layer3"):
            y = out[name] = getattr(self, name)(y).clone()
        y = self.conv2(y)
        out["conv2"] = y.view(b, n, *y.shape[1:])
        return out

    def forward(self, x):
        return self.stages(x)["conv2"]


STAGES = ("stem", "layer1", "layer2", "layer3", "conv2")


# ---- seeded data: numpy's RandomState and exact operations only, the same bits on every machine ----------------------
def _normal(rs, shape, std):
    return torch.from_numpy((std * rs.standard_normal(shape)).astype(np.float32))


def set_weights(m, seed):
    """Every convolution: weight ~ N(0, 2 / fan_out) (the scale of the reference's kaiming init), bias ~ N(0, 0.1^2), in
    state_dict order."""
    rs = np.random.RandomState(seed)
    with torch.no_grad():
        for _, mod in sorted(m.named_modules()):
            if isinstance(mod, nn.Conv2d):
                fan_out = mod.out_channels * mod.kernel_size[0] * mod.kernel_size[1]
                mod.weight.copy_(_normal(rs, tuple(mod.weight.shape), (2.0 / fan_out) ** 0.5))
                mod.bias.copy_(_normal(rs, tuple(mod.bias.shape), 0.1))
    return m


CASES = {"features_fnet_2x40x56": dict(seed=51, N=2, H=40, W=56),
         "features_fnet_1x64x48": dict(seed=52, N=1, H=64, W=48)}


def make_images(seed, N, H, W):
    """(1, N, 3, H, W) float32: smooth gradients plus noise at the scale of a normalised image."""
    rs = np.random.RandomState(seed)
    yy = torch.from_numpy((2.0 * np.arange(H) / (H - 1) - 1.0).astype(np.float32)).view(1, 1, H, 1)
    xx = torch.from_numpy((2.0 * np.arange(W) / (W - 1) - 1.0).astype(np.float32)).view(1, 1, 1, W)
    base = _normal(rs, (N, 3, 1, 1), 1.0) * yy + _normal(rs, (N, 3, 1, 1), 1.0) * xx
    return (base + _normal(rs, (N, 3, H, W), 0.7)).unsqueeze(0).contiguous()


def make_case(name, seed_offset=0):
    """(module, images) of a fixture case, float32 on the CPU; seed_offset != 0 gives further cases of the same shape."""
    cfg = CASES[name]
    m = set_weights(RefEncoder(), cfg["seed"] + 1000 + seed_offset).eval()
    return m, make_images(cfg["seed"] + seed_offset, cfg["N"], cfg["H"], cfg["W"])


def case_sha256(m, images):
    """Pins the images and every parameter (state_dict order)."""
    hsh = hashlib.sha256()
    for t in [images] + [v for _, v in sorted(m.state_dict().items())]:
        hsh.update(np.ascontiguousarray(t.detach().cpu().numpy()).tobytes())
    return hsh.hexdigest()
