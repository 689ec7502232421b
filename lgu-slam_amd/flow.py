"""The motion (flow) encoder of LGU-SLAM's update operator (reference droid_slam/droid_net.py:82-86):

    flow_encoder = Sequential(Conv2d(4, 128, 7, padding=3), ReLU, Conv2d(128, 64, 3, padding=1), ReLU)

Under float16 autocast its first layer is a cast launch, a 4-channel 7x7 convolution and an in-place ReLU launch on the
fp32 motion features.  `flow_conv7_relu` (csrc/flowenc.hip) evaluates those three in one launch on the matrix cores, with
the autocast rounding points (include/lgu_corr.h); the second convolution stays the module's own call.

    flow.install(update_module.flow_encoder)   # UpdateModule.forward now reaches the fused path, state_dict keys unchanged

`flow_conv7_relu`: contiguous HIP device tensors only (no CPU fallback), every argument error raised before anything is
launched, no host synchronisation (graph-capturable), forward only: an input that requires grad is refused while grad
mode is on.  There is no fp32 kernel: fp32 evaluation is the module's own forward.
"""
import torch

from . import _lib
from ._host import LayerWrapper, bind, check_layer_operands, check_shape, is_conv, launch, serves_half, unbind
from ._host import stream as _stream

CIN, COUT, KW, PAD, C2 = 4, 128, 7, 3, 64
WPACK_HALVES = 28672             # include/lgu_corr.h LGU_FLOW_CONV7_WPACK_HALVES = 7 * 8 * 64 * 8

# Shape classes (by H * W * N output pixels) at which the measured fused first layer does not beat the module's own
# cast + convolution + ReLU beyond the two spreads (tools/prof_flowenc.py): FlowEncoder sends
# calls with fewer output pixels than this to the module's forward.  0: every shape class kept the fused path.
MIN_FUSED_PIXELS = 0


def pack_conv7(weight, bias):
    """(wpack (7,8,64,8) half, bias_h (128) half) of a Conv2d(4, 128, 7) weight (128,4,7,7) and bias (128), on the weight's
    device.  wpack[ky, ct, l, j] = half(weight)[16 ct + (l & 15), k % 4, ky, k // 4] with k = 8 (l >> 4) + j, and 0 where
    k // 4 == 7: the B operand of v_mfma_f32_16x16x32_f16, one window row per K step."""
    check_shape([(weight, "weight")], (COUT, CIN, KW, KW))
    check_shape([(bias, "bias")], (COUT,))
    with torch.no_grad():
        wh = weight.detach().to(torch.float16)
        slots = torch.zeros((COUT, KW, KW + 1, CIN), dtype=torch.float16, device=wh.device)   # [co][ky][x-slot][c]
        slots[:, :, :KW, :] = wh.permute(0, 2, 3, 1)
        # [ct][cl][ky][g][j] -> [ky][ct][g][cl][j]: lane l = 16 g + cl
        wpack = slots.reshape(COUT // 16, 16, KW, 4, 8).permute(2, 0, 3, 1, 4).reshape(KW, COUT // 16, 64, 8).contiguous()
        bias_h = bias.detach().to(device=wh.device, dtype=torch.float16).contiguous()
    return wpack, bias_h


def flow_conv7_relu(x, wpack, bias_h):
    """relu(conv2d(half(x), w_h, b_h, padding=3)) as a new (N,128,H,W) half tensor: x (N,4,H,W) float32 (a half x is
    widened first, which is exact), wpack and bias_h from `pack_conv7`.  Exact products, fp32 accumulation, one rounding
    to half; NaN is kept.  x and bias_h are served at element alignment; a wpack that is not 16-byte aligned (never the
    case for what pack_conv7 returns) raises UnsupportedShape."""
    if x.dim() != 4 or x.shape[1] != CIN:
        raise RuntimeError("x must be (N,%d,H,W), got %s" % (CIN, tuple(x.shape)))
    if wpack.numel() != WPACK_HALVES:
        raise RuntimeError("wpack must hold %d halves (pack_conv7), got %s" % (WPACK_HALVES, tuple(wpack.shape)))
    named = [(x, "x"), (wpack, "wpack"), (bias_h, "bias_h")]
    check_shape(named[2:], (COUT,))
    check_layer_operands("flow_conv7_relu", named)
    N, _, H, W = x.shape
    out = torch.empty((N, COUT, H, W), dtype=torch.float16, device=x.device)
    if N == 0:
        return out
    if H * W == 0:
        raise RuntimeError("flow_conv7_relu: empty frame (H*W = 0)")
    if x.dtype == torch.float16:
        x = x.float()
    args = _lib.FlowConv7Args(x.data_ptr(), wpack.data_ptr(), bias_h.data_ptr(), out.data_ptr(), N, H, W)
    launch("lgu_flow_conv7_relu_h16", "flow_conv7_relu", x.device, args, _stream(x))
    return out


class FlowEncoder(LayerWrapper):
    """Callable stand-in for the forward of the reference's `flow_encoder`:

        fused = FlowEncoder(update_module.flow_encoder)
        flow = fused(motn)                     # = update_module.flow_encoder(motn)

    Fused path (csrc/flowenc.hip + the module's second convolution) for a HIP tensor (N,4,H,W), float32 or half, under
    CUDA autocast with float16, with float32 parameters (both convolutions') on the input's device and at least
    MIN_FUSED_PIXELS pixels N*H*W (_host.serves_half).  Everything else goes to the module's own forward unchanged: CPU
    tensors, other dtypes, a bfloat16 autocast, autocast off, and grad mode with parameters or an input that require grad.
    The packed weights are cached; the key covers the first layer's weight and bias (data pointer, version, device), so
    load_state_dict and in-place updates are picked up.  `fused_calls` counts the fused launches."""

    def __init__(self, module):
        ok = isinstance(module, torch.nn.Sequential) and len(module) == 4
        ok = ok and is_conv(module[0], CIN, COUT, KW, pad=PAD, bias=True) and isinstance(module[1], torch.nn.ReLU)
        ok = ok and is_conv(module[2], COUT, C2, 3, pad=1, bias=True) and isinstance(module[3], torch.nn.ReLU)
        if not ok:
            raise RuntimeError("FlowEncoder: the module must be Sequential(Conv2d(4, 128, 7, padding=3), ReLU, "
                               "Conv2d(128, 64, 3, padding=1), ReLU) with biases")
        super().__init__(module, module[0], pack_conv7)

    def _serves(self, x):
        c1, c2 = self.conv, self.module[2]
        return serves_half(x, CIN, (c1.weight, c1.bias, c2.weight, c2.bias), MIN_FUSED_PIXELS)

    def _operator(self, x, wpack, bias_h):
        return flow_conv7_relu(x, wpack, bias_h)

    def _finish(self, y):
        return torch.relu_(self.module[2](y))


def install(module):
    """Bind a FlowEncoder as `module.forward` (an instance attribute: parameters and state_dict keys are unchanged), so
    the reference's UpdateModule.forward reaches the fused path.  Returns the wrapper."""
    return bind(module, "forward", FlowEncoder, lambda _: FlowEncoder(module))


def uninstall(module):
    """Undo `install`: the class's forward is used again."""
    unbind(module, "forward", FlowEncoder)
