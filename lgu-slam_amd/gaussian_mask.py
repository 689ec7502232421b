"""Learnable per-pixel 2-D Gaussian mask on the correlation volume: this build's
counterpart of the reference's droid_slam/gaussianMask_cuda.py (same class names,
constructor and forward signatures, same parameter names so state dicts load)."""
import math

import torch
import torch.nn as nn

from . import _lib, ops
from ._host import (PackCache, bind, check_contiguous, check_device, check_dtype, check_no_grad, check_shape, fused_dtype, launch,
                    unbind)
from ._host import stream as _stream

CIN, HIDDEN = 256, 16         # include/lgu_corr.h LGU_GAUSSHEAD_CIN, LGU_GAUSSHEAD_HIDDEN
WPACK_ELEMS = 4352            # include/lgu_corr.h LGU_GAUSSHEAD_WPACK_ELEMS = 256 * 16 + 64 * 4
BIAS_ELEMS = 20               # include/lgu_corr.h LGU_GAUSSHEAD_BIAS_ELEMS
X_HALF, FP32 = 1, 2           # include/lgu_corr.h LGU_GAUSSHEAD_X_HALF, LGU_GAUSSHEAD_FP32

# The number of pixels E * h * w below which the measured fused parameter head does not beat the module's own three
# linear layers beyond the two spreads (tools/prof_gausshead.py, profiles/gausshead_prof.json):
# an installed GaussianHead sends such calls to the module.  0: every measured shape class kept the fused route.
MIN_FUSED_PIXELS = 0


class GaussianMaskCuda(torch.autograd.Function):
    """reference gaussianMask_cuda.py:7-23: grads for mean and cov only."""

    @staticmethod
    def forward(ctx, mean, cov, corr, radius):
        mean = mean.float()
        cov = cov.float()
        ctx.save_for_backward(mean, cov, corr)
        ctx.radius = radius
        corr1, = ops.gaussianMask(mean, cov, corr, radius)
        return corr1

    @staticmethod
    def backward(ctx, grad_output):
        mean, cov, corr = ctx.saved_tensors
        means_grad, covs_grad = ops.gaussianMask_backward(mean, cov, corr, grad_output.contiguous(), ctx.radius)
        return means_grad, covs_grad, None, None


def per_Corr_Normalization(x, normalIndex, eps=1e-5):
    """(b, h*w, 2) standardised over `normalIndex` per sample, biased variance
    (reference gaussianMask_cuda.py:26-33)."""
    mean = x.mean(dim=normalIndex, keepdim=True)
    std = torch.sqrt(x.var(dim=normalIndex, unbiased=False, keepdim=True) + eps)
    return (x - mean) / std


FUSED_PARAMS = True   # False: the torch composition of gaussian_parameters also in inference (A/B and tests)


class GaussianMask(nn.Module):
    """Predicts a mean (grid + learned shift) and a diagonal covariance per source pixel
    from the concatenated feature pair and re-weights the volume with it
    (reference gaussianMask_cuda.py:35-88)."""

    RADIUS = 4  # window radius hard-wired at the reference call site (:84)

    def __init__(self, h, w):
        super().__init__()
        self.meanMap = nn.Linear(16, 2)
        self.covMap = nn.Linear(16, 2)
        self.map = nn.Linear(256, 16)
        self.cov = torch.eye(2)
        # reference initialisation (:43-56): zero mean head, He-style normal elsewhere
        nn.init.zeros_(self.meanMap.weight); nn.init.zeros_(self.meanMap.bias)
        nn.init.normal_(self.covMap.weight, 0, math.sqrt(2.0 / self.covMap.out_features)); nn.init.zeros_(self.covMap.bias)
        nn.init.normal_(self.map.weight, 0, math.sqrt(2.0 / self.map.out_features)); nn.init.zeros_(self.map.bias)
        self.mapA = nn.Sequential(self.map, nn.Tanh())
        ys, xs = torch.meshgrid(torch.arange(h).float(), torch.arange(w).float(), indexing="ij")
        self.coord = torch.stack([xs, ys], dim=-1).view(h, w, 2)  # (x, y) of every source pixel

    def gaussian_parameters(self, x):
        """mean (b,h,w,2), cov (b,h,w,2) float32 contiguous, det (b,h*w) from the feature pair
        x (b,h,w,256) — everything in forward() up to the kernel call (:66-83)."""
        b, h, w, _ = x.shape
        tt = self.mapA(x)
        mean_ofs = self.meanMap(tt).view(b, h, w, 2)
        cov_raw = self.covMap(tt).view(b, h * w, 2)
        if (FUSED_PARAMS and cov_raw.is_cuda and cov_raw.dtype in (torch.float32, torch.float16)
                and mean_ofs.dtype == cov_raw.dtype and not (torch.is_grad_enabled() and cov_raw.requires_grad)
                and self.coord.shape[:2] == (h, w)):
            # inference: everything below in one launch, with torch's arithmetic (incl. the half roundings under autocast)
            return ops.gaussian_params(mean_ofs.contiguous(), cov_raw.contiguous(), h, w)
        cov = per_Corr_Normalization(cov_raw, [1, 2])
        cov = torch.sigmoid(cov) * 5 + 0.05
        det = cov[:, :, 0] * cov[:, :, 1]
        cov = cov.view(b, h, w, 2).float()
        mean = self.coord.to(device=cov.device, dtype=cov.dtype).expand(b, h, w, 2) + mean_ofs
        return mean.contiguous(), cov.contiguous(), det

    def forward(self, x, corr):
        b, h, w, _ = x.shape
        mean, cov, det = self.gaussian_parameters(x)
        corr1 = GaussianMaskCuda.apply(mean, cov, corr, self.RADIUS)
        corr1 = corr1 / (6.28 * torch.sqrt(det).view(b, h, w, 1, 1)) + corr
        return corr1, mean, det


# ---- the fused parameter head (csrc/gausshead.hip) --------------------------------------------------------------------
def _is_linear(m, cin, cout):
    return isinstance(m, nn.Linear) and m.in_features == cin and m.out_features == cout and m.bias is not None


def pack_gaussian_head(map, meanMap, covMap, half):
    """(wpack (4352), bias (20)) of map = Linear(256, 16), meanMap and covMap = Linear(16, 2), on the parameters' device:
    half tensors rounded once when `half` is set (what float16 autocast evaluates), float32 otherwise.  With
    W1 = map.weight, W2 = [meanMap.weight; covMap.weight] (4,16), lane l, r = l & 15, g = l >> 4:

        half:  wpack[(kc * 64 + l) * 8 + j] = W1[r, 32 kc + 8 g + j]            kc < 8, j < 8
               wpack[4096 + 4 l + j]        = W2[r, 4 g + j] if r < 4 else 0    j < 4
        fp32:  wpack[s * 64 + l]            = W1[r, 16 (s >> 2) + 4 g + (s & 3)]   s < 64
               wpack[4096 + 64 i + l]       = W2[r, 4 g + i] if r < 4 else 0    i < 4
        bias = [map.bias (16); meanMap.bias (2); covMap.bias (2)]

    the A operands of v_mfma_f32_16x16x32_f16 / v_mfma_f32_16x16x16_f16 (half) and of v_mfma_f32_16x16x4_f32 (fp32) as each
    lane loads them (include/lgu_corr.h, lgu_gaussian_head)."""
    if not (_is_linear(map, CIN, HIDDEN) and _is_linear(meanMap, HIDDEN, 2) and _is_linear(covMap, HIDDEN, 2)):
        raise RuntimeError("pack_gaussian_head: map must be Linear(256, 16), meanMap and covMap Linear(16, 2), each with a bias")
    dt = torch.float16 if half else torch.float32
    with torch.no_grad():
        dev = map.weight.device
        w1 = map.weight.detach().to(dt)
        w2 = torch.zeros((16, HIDDEN), dtype=dt, device=dev)
        w2[0:2] = meanMap.weight.detach().to(device=dev, dtype=dt)
        w2[2:4] = covMap.weight.detach().to(device=dev, dtype=dt)
        if half:
            # [r][kc][g][j] -> [kc][g][r][j]; [r][g][j] -> [g][r][j]: lane l = 16 g + r
            p1 = w1.reshape(16, 8, 4, 8).permute(1, 2, 0, 3)
            p2 = w2.reshape(16, 4, 4).permute(1, 0, 2)
        else:
            # [r][m][g][i] -> [m][i][g][r] (s = 4 m + i); [r][g][i] -> [i][g][r]
            p1 = w1.reshape(16, 16, 4, 4).permute(1, 3, 2, 0)
            p2 = w2.reshape(16, 4, 4).permute(2, 1, 0)
        wpack = torch.cat((p1.reshape(-1), p2.reshape(-1))).contiguous()
        bias = torch.cat([b.detach().to(device=dev, dtype=dt) for b in (map.bias, meanMap.bias, covMap.bias)]).contiguous()
    return wpack, bias


def gaussian_head(x, wpack, bias, half=None, hidden=False):
    """(mean_ofs (E,h,w,2), cov_raw (E,h*w,2)[, tt (E,h,w,16)]) of x (E,h,w,256): meanMap(tt), covMap(tt) and, with `hidden`,
    tt = tanh(map(x)) itself, in one launch (csrc/gausshead.hip), with `wpack`, `bias` from pack_gaussian_head(.., half).

    half=True: float16 autocast's arithmetic.  x float32 (rounded to half once) or half, parameters and outputs half; exact
    products, fp32 accumulation, one rounding to half after each bias, one after tanhf.  half=False: everything float32.
    half=None: True when CUDA float16 autocast is on.  Contiguous HIP tensors only (no CPU fallback), every argument error
    raised before anything is launched, no host synchronisation, forward only.  An x that is not 16-byte aligned raises
    UnsupportedShape.  NaN is kept and reaches its own pixel only."""
    if half is None:
        half = torch.is_autocast_enabled("cuda") and torch.get_autocast_dtype("cuda") == torch.float16
    if x.dim() != 4 or x.shape[3] != CIN:
        raise RuntimeError("x must be (E,h,w,%d), got %s" % (CIN, tuple(x.shape)))
    if wpack.numel() != WPACK_ELEMS:
        raise RuntimeError("wpack must hold %d elements (pack_gaussian_head), got %s" % (WPACK_ELEMS, tuple(wpack.shape)))
    named = [(x, "x"), (wpack, "wpack"), (bias, "bias")]
    check_shape(named[2:], (BIAS_ELEMS,))
    check_contiguous(named)
    pdt = torch.float16 if half else torch.float32
    check_dtype(named[:1], (torch.float32, torch.float16) if half else torch.float32)
    check_dtype(named[1:], pdt)
    check_no_grad("gaussian_head", named)
    check_device(named)
    E, h, w, _ = x.shape
    mean_ofs = torch.empty((E, h, w, 2), dtype=pdt, device=x.device)
    cov_raw = torch.empty((E, h * w, 2), dtype=pdt, device=x.device)
    tt = torch.empty((E, h, w, HIDDEN), dtype=pdt, device=x.device) if hidden else None
    if E:
        if h * w == 0:
            raise RuntimeError("gaussian_head: empty sample (h*w = 0)")
        if x.data_ptr() % 16 or wpack.data_ptr() % 16:
            raise _lib.UnsupportedShape("gaussian_head: x and wpack must be 16-byte aligned")
        flags = (0 if half else FP32) | (X_HALF if x.dtype == torch.float16 else 0)
        args = _lib.GaussHeadArgs(x.data_ptr(), wpack.data_ptr(), bias.data_ptr(), mean_ofs.data_ptr(), cov_raw.data_ptr(),
                                  tt.data_ptr() if hidden else None, E, h, w, flags)
        launch("lgu_gaussian_head", "gaussian_head", x.device, args, _stream(x))
    return (mean_ofs, cov_raw, tt) if hidden else (mean_ofs, cov_raw)


class GaussianHead:
    """Callable stand-in for `ga.gaussian_parameters` of one GaussianMask:

        fused = GaussianHead(ga)
        mean, cov, det = fused(x)        # = ga.gaussian_parameters(x), two launches

    Fused route: gaussian_head (csrc/gausshead.hip) followed by ops.gaussian_params, for a HIP tensor x (E,h,w,256) with
    E*h*w >= MIN_FUSED_PIXELS (and > 0), float32 parameters on x's device, `coord` of (h, w), nothing requiring grad while
    grad mode is on, and one of: half x under CUDA float16 autocast, float32 x under CUDA float16 autocast, float32 x with
    autocast off.  Everything else is the class's own gaussian_parameters unchanged: CPU tensors, a bfloat16 autocast,
    half x outside autocast, training, FUSED_PARAMS = False, and an x the kernel refuses (UnsupportedShape).  The packs
    (one per arithmetic mode) are cached under the six parameters.  `fused_calls` counts the fused calls.  The route's
    bits are those of include/lgu_corr.h, not the library GEMM's: it is opt-in."""

    def __init__(self, ga):
        if not isinstance(ga, GaussianMask):
            raise RuntimeError("GaussianHead: the module must be a lgu_slam_amd GaussianMask")
        if not (_is_linear(ga.map, CIN, HIDDEN) and _is_linear(ga.meanMap, HIDDEN, 2) and _is_linear(ga.covMap, HIDDEN, 2)):
            raise RuntimeError("GaussianHead: map must be Linear(256, 16), meanMap and covMap Linear(16, 2), each with a bias")
        self.module = ga
        self._packs = PackCache()
        self.fused_calls = 0

    def params(self):
        ga = self.module
        return (ga.map.weight, ga.map.bias, ga.meanMap.weight, ga.meanMap.bias, ga.covMap.weight, ga.covMap.bias)

    def packed(self, half):
        """(wpack, bias) of the arithmetic mode `half`, cached."""
        ga = self.module
        return self._packs.get(bool(half), self.params(), lambda: pack_gaussian_head(ga.map, ga.meanMap, ga.covMap, bool(half)))

    def _mode(self, x):
        """True / False: the fused route serves this call in half / fp32 mode; None: the module's own path."""
        if not FUSED_PARAMS or not isinstance(x, torch.Tensor) or not x.is_cuda or x.dim() != 4 or x.shape[3] != CIN:
            return None
        E, h, w, _ = x.shape
        if E * h * w == 0 or E * h * w < MIN_FUSED_PIXELS or tuple(self.module.coord.shape[:2]) != (h, w):
            return None
        params = self.params()
        if any(p.dtype != torch.float32 or p.device != x.device for p in params):
            return None
        dt = fused_dtype([x, *params])
        if dt == torch.float16 and x.dtype in (torch.float32, torch.float16):
            return True
        if dt == torch.float32 and x.dtype == torch.float32:
            return False
        return None

    def __call__(self, x):
        ga = self.module
        half = self._mode(x)
        if half is not None:
            E, h, w, _ = x.shape
            try:
                mean_ofs, cov_raw = gaussian_head(x.contiguous(), *self.packed(half), half=half)
            except _lib.UnsupportedShape:
                half = None
        if half is None:
            return type(ga).gaussian_parameters(ga, x)
        out = ops.gaussian_params(mean_ofs, cov_raw, h, w)
        self.fused_calls += 1
        return out


def install(ga):
    """Bind a GaussianHead as `ga.gaussian_parameters`, an instance attribute: forward(), CorrBlock and everything else
    that asks `ga` for its parameters then takes the fused route; the module's parameters and state_dict keys are
    unchanged.  Returns the wrapper; a second call returns the first wrapper.  A module that is not this build's
    GaussianMask raises RuntimeError and binds nothing."""
    if not isinstance(ga, GaussianMask):
        raise RuntimeError("gaussian_mask.install: the module must be a lgu_slam_amd GaussianMask")
    return bind(ga, "gaussian_parameters", GaussianHead, lambda _: GaussianHead(ga))


def uninstall(ga):
    """Undo `install`: the class's gaussian_parameters is used again."""
    unbind(ga, "gaussian_parameters", GaussianHead)
