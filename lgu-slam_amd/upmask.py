"""GraphAgg's upsampling mask (reference droid_slam/droid_net.py:50-51,67):

    agg.upmask = Sequential(Conv2d(128, 576, 1))

the widest output of the update operator: 576 half planes per keyframe, which DepthVideo.upsample (depth_video.py:124-128)
then reduces to 64 floats per coarse pixel.  csrc/upmask.hip evaluates the layer as float16 autocast does (cast, 1x1
convolution, bias, one rounding to half), NCHW in and NCHW out, in one launch (`upmask_conv1x1`), and the same layer fused
with the 9-way softmax, the convex combination of the disparity and the indexed write, so that the 576 planes never reach
memory (`upsample_from_net_`).  Both run one GEMM main loop: the fused form sees the bits the plain one stores.

    upmask.install(update_module.agg.upmask)                    # the module's contract: forward returns upmask
    upmask.upsample_from_net_(video.disps_up, video.disps, ix, net, *wrapper.packed())     # mask-free upsample

Contiguous HIP device tensors only (no CPU fallback), every argument error raised before anything is launched, no host
synchronisation (graph-capturable), forward only: an input that requires grad is refused while grad mode is on.  There is
no fp32 kernel: fp32 evaluation is the module's own forward.
"""
import torch

from . import _lib
from ._host import (FLOAT_OR_HALF, LayerWrapper, bind, check_contiguous, check_device, check_dtype, check_layer_operands,
                    check_no_grad, check_shape, installed, is_conv, launch, serves_half, unbind)
from ._host import stream as _stream

CIN = 128
COUT = 576                    # include/lgu_corr.h LGU_UPMASK_COUT: 9 taps x 8 x 8 sub-pixels
WPACK_HALVES = 73728          # include/lgu_corr.h LGU_UPMASK_WPACK_HALVES = 576 * 128
X_HALF = 1                    # include/lgu_corr.h LGU_UPMASK_X_HALF
UPS_HALF_WEIGHTS = 2          # include/lgu_corr.h LGU_UPS_HALF_WEIGHTS

# The number of pixels N * H * W below which the measured fused layer does not beat the module's own autocast forward
# beyond the two spreads (tools/prof_upmask.py): Upmask sends such calls to the module.
MIN_FUSED_PIXELS = 0


def pack_upmask(weight, bias):
    """(wpack (36,4,64,8) half, bias_h (576) half) of a Conv2d(128, 576, 1) weight (576,128,1,1) and bias (576), on the
    weight's device: wpack[mt, kc, l, j] = half(weight)[16 mt + (l & 15), 32 kc + 8 (l >> 4) + j, 0, 0], the A operand of
    v_mfma_f32_16x16x32_f16 for the row tile mt of 16 output channels and the block kc of 32 input channels as lane l
    loads it.  Every slot holds a weight."""
    check_shape([(weight, "weight")], (COUT, CIN, 1, 1))
    check_shape([(bias, "bias")], (COUT,))
    with torch.no_grad():
        wh = weight.detach().to(torch.float16).reshape(COUT, CIN)
        # [mt][r][kc][g][j] -> [mt][kc][g][r][j]: lane l = 16 g + r
        wpack = wh.reshape(36, 16, 4, 4, 8).permute(0, 2, 3, 1, 4).reshape(36, 4, 64, 8).contiguous()
        bias_h = bias.detach().to(device=wh.device, dtype=torch.float16).contiguous()
    return wpack, bias_h


def _check_net(x, wpack, bias_h):
    if x.dim() != 4 or x.shape[1] != CIN:
        raise RuntimeError("x must be (N,%d,H,W), got %s" % (CIN, tuple(x.shape)))
    if wpack.numel() != WPACK_HALVES:
        raise RuntimeError("wpack must hold %d halves (pack_upmask), got %s" % (WPACK_HALVES, tuple(wpack.shape)))
    check_shape([(bias_h, "bias_h")], (COUT,))


def upmask_conv1x1(x, wpack, bias_h):
    """half(conv2d(half(x), w_h, b_h)) as a new (N,576,H,W) half tensor: x (N,128,H,W) float32 or half (a half x is used as
    it is), wpack and bias_h from `pack_upmask`.  Exact products, fp32 accumulation in a fixed order, one rounding to half;
    NaN is kept.  x and bias_h are served at element alignment; a wpack that is not 16-byte aligned (never the case for
    what pack_upmask returns) raises UnsupportedShape."""
    _check_net(x, wpack, bias_h)
    named = [(x, "x"), (wpack, "wpack"), (bias_h, "bias_h")]
    check_layer_operands("upmask_conv1x1", named)
    N, _, H, W = x.shape
    out = torch.empty((N, COUT, H, W), dtype=torch.float16, device=x.device)
    if out.numel() == 0:
        return out
    flags = X_HALF if x.dtype == torch.float16 else 0
    args = _lib.UpmaskArgs(x.data_ptr(), wpack.data_ptr(), bias_h.data_ptr(), out.data_ptr(), N, H, W, flags)
    launch("lgu_upmask1x1_c128_h16", "upmask_conv1x1", x.device, args, _stream(x))
    return out


def upsample_from_net_(disps_up, disps, ix, x, wpack, bias_h, half_weights=None):
    """GraphAgg.upmask followed by DepthVideo.upsample in one launch, in place: disps_up[ix[u]] = cvx_upsample of
    disps[ix[u]] with the mask upmask_conv1x1(x[u]), for every u, without that mask existing.  disps_up (N,8ht,8wd) and
    disps (N,ht,wd) float32, ix (U,) int64, x (U,128,ht,wd) float32 or half (the `net` behind GraphAgg's conv2 and relu),
    wpack and bias_h from `pack_upmask`.  half_weights: the softmax weights are rounded to half, as torch.softmax of the
    half mask returns them with autocast off; None resolves to `not torch.is_autocast_enabled()`, what
    aggregate.upsample_disps_ does for a half mask.  Rows of disps_up not in ix are untouched; an ix[u] outside [0, N)
    writes nothing; ix must not hold duplicates (it comes from torch.unique).  Equal to aggregate.upsample_disps_ on
    upmask_conv1x1's result, bit for bit.  A disps_up that is not 16-byte aligned raises UnsupportedShape.  Returns
    disps_up."""
    if disps.dim() != 3:
        raise RuntimeError("disps must be (N,ht,wd), got %s" % (tuple(disps.shape),))
    N, ht, wd = disps.shape
    if tuple(disps_up.shape) != (N, 8 * ht, 8 * wd):
        raise RuntimeError("disps_up must be (N,8ht,8wd) = %s, got %s" % ((N, 8 * ht, 8 * wd), tuple(disps_up.shape)))
    if ix.dim() != 1:
        raise RuntimeError("ix must be 1-D, got %s" % (tuple(ix.shape),))
    U = ix.shape[0]
    _check_net(x, wpack, bias_h)
    if tuple(x.shape) != (U, CIN, ht, wd):
        raise RuntimeError("x must be (%d,%d,%d,%d), got %s" % (U, CIN, ht, wd, tuple(x.shape)))
    named = [(disps_up, "disps_up"), (disps, "disps"), (ix, "ix"), (x, "x"), (wpack, "wpack"), (bias_h, "bias_h")]
    check_contiguous(named)
    check_dtype(named[:2], torch.float32)
    check_dtype(named[2:3], torch.int64)
    check_dtype(named[3:4], FLOAT_OR_HALF)
    check_dtype(named[4:], torch.float16)
    if half_weights is None:
        half_weights = not torch.is_autocast_enabled()
    check_no_grad("upsample_from_net_", named)
    check_device(named)
    if U * N * ht * wd == 0:
        return disps_up
    flags = (X_HALF if x.dtype == torch.float16 else 0) | (UPS_HALF_WEIGHTS if half_weights else 0)
    args = _lib.UpmaskUpsArgs(x.data_ptr(), wpack.data_ptr(), bias_h.data_ptr(), disps.data_ptr(), ix.data_ptr(),
                              disps_up.data_ptr(), U, N, ht, wd, flags)
    launch("lgu_upmask_upsample_f32", "upsample_from_net_", disps.device, args, _stream(disps))
    return disps_up


def eligible(m):
    """m is Conv2d(128, 576, 1) with a bias, stride 1, no padding, dilation, groups or padding mode."""
    return is_conv(m, CIN, COUT, 1, pad=0, bias=True)


def parse(module):
    """The convolution of an eligible Conv2d or of a Sequential holding exactly one; None for anything else."""
    if eligible(module):
        return module
    if isinstance(module, torch.nn.Sequential) and len(module) == 1 and eligible(module[0]):
        return module[0]
    return None


class Upmask(LayerWrapper):
    """Callable stand-in for the forward of a Conv2d(128, 576, 1) with a bias, or of an nn.Sequential holding exactly that
    (the reference's GraphAgg.upmask):

        fused = Upmask(update_module.agg.upmask)
        mask = fused(net)                      # = update_module.agg.upmask(net)

    Fused path (csrc/upmask.hip, one launch) for a HIP tensor (N,128,H,W), float32 or half, under CUDA autocast with
    float16, with float32 parameters on the input's device, when nothing requires grad and N*H*W >= MIN_FUSED_PIXELS
    (_host.serves_half).  Everything else goes to the module's own forward unchanged: CPU tensors, other dtypes, a
    bfloat16 autocast, autocast off, and grad.  Unlike the other single-layer wrappers, Upmask also sends a batch of 0
    (N == 0) to the module: a rule of its own, stated in `_serves`, where the others hand it to their operator.  The
    packed weights are cached under the layer's weight and bias (data pointer, version, device); `packed()` returns them
    for `upsample_from_net_`.  `fused_calls` counts the fused launches."""

    def __init__(self, module):
        conv = parse(module)
        if conv is None:
            raise RuntimeError("Upmask: the module must be Conv2d(128, 576, 1) with a bias, or an nn.Sequential holding "
                               "exactly that")
        super().__init__(module, conv, pack_upmask)

    def _serves(self, x):
        if isinstance(x, torch.Tensor) and x.numel() == 0:      # N == 0 included: the module's
            return False
        c = self.conv
        return serves_half(x, CIN, (c.weight, c.bias), MIN_FUSED_PIXELS)

    def _operator(self, x, wpack, bias_h):
        return upmask_conv1x1(x, wpack, bias_h)


def install(module):
    """Bind an Upmask as `module.forward`, an instance attribute: parameters and state_dict keys are unchanged.  Returns
    the wrapper; a second call returns the first wrapper.  A module Upmask does not take raises RuntimeError and binds
    nothing, and so does a module whose forward already carries another wrapper."""
    return installed(module, Upmask, "upmask.install") or bind(module, "forward", Upmask, lambda _: Upmask(module))


def uninstall(module):
    """Undo `install`: the class's forward is used again."""
    unbind(module, "forward", Upmask)
