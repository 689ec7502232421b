"""The update operator's 1x1 convolution behind the correlation lookup (reference droid_slam/droid_net.py):

    corr_encoder[0] = Conv2d(196, 128, 1), followed by ReLU

Under float16 autocast, on the planar fp32 tensor the default lookup writes, the layer is a cast pass over the 784-byte
pixel rows, the library's convolution with its layout passes, a bias launch and a ReLU launch.  `conv1x1`
(csrc/conv1.hip) evaluates cast + convolution + bias (+ ReLU) in one launch on the matrix cores, NCHW in and NCHW out,
with the autocast rounding points (include/lgu_corr.h), for any Conv2d(Cin, 128, 1) with 1 <= Cin <= 224.

    conv1.install(update_module.corr_encoder[0])   # the Conv2d: the Sequential's ReLU stays a launch
    y = conv1.conv1x1(corr, *wrapper.packed(), relu=True)       # the layer with its ReLU, one launch

`conv1x1`: contiguous HIP device tensors only (no CPU fallback), every argument error raised before anything is launched,
no host synchronisation (graph-capturable), forward only: an input that requires grad is refused while grad mode is on.
There is no fp32 kernel: fp32 evaluation is the module's own forward.
"""
import torch

from . import _lib
from ._host import LayerWrapper, bind, check_layer_operands, check_shape, installed, is_conv, launch, serves_half, unbind
from ._host import stream as _stream

COUT = 128                    # include/lgu_corr.h LGU_CONV1_COUT
MAX_CIN = 224                 # include/lgu_corr.h LGU_CONV1_MAX_CIN
WPACK_HALVES = 28672          # include/lgu_corr.h LGU_CONV1_WPACK_HALVES = 7 * 8 * 64 * 8
X_HALF, RELU = 1, 2           # include/lgu_corr.h LGU_CONV1_X_HALF, LGU_CONV1_RELU

# The number of pixels N * H * W below which the measured fused layer does not beat the module's own autocast forward
# beyond the two spreads (tools/prof_update.py): Conv1 sends such calls to the module.
# 0: every measured shape class kept the fused path.
MIN_FUSED_PIXELS = 0


def pack_conv1(weight, bias):
    """(wpack (7,8,64,8) half, bias_h (128) half) of a Conv2d(Cin, 128, 1) weight (128,Cin,1,1) and bias (128), 1 <= Cin <=
    224, on the weight's device.  With c = 32 kc + 8 (l >> 4) + j: wpack[kc, ct, l, j] = half(weight)[16 ct + (l & 15), c, 0, 0]
    where c < Cin and zero where c >= Cin: the B operand of v_mfma_f32_16x16x32_f16, one block kc of 32 input channels per
    K step."""
    cin = weight.shape[1] if weight.dim() == 4 and 1 <= weight.shape[1] <= MAX_CIN else MAX_CIN
    check_shape([(weight, "weight")], (COUT, cin, 1, 1))
    check_shape([(bias, "bias")], (COUT,))
    with torch.no_grad():
        wh = torch.zeros((COUT, MAX_CIN), dtype=torch.float16, device=weight.device)
        wh[:, :cin] = weight.detach().to(torch.float16).reshape(COUT, cin)
        # [ct][cl][kc][g][j] -> [kc][ct][g][cl][j]: lane l = 16 g + cl
        wpack = wh.reshape(COUT // 16, 16, MAX_CIN // 32, 4, 8).permute(2, 0, 3, 1, 4).reshape(MAX_CIN // 32, COUT // 16, 64, 8)
        wpack = wpack.contiguous()
        bias_h = bias.detach().to(device=wh.device, dtype=torch.float16).contiguous()
    return wpack, bias_h


def conv1x1(x, wpack, bias_h, cin=None, relu=False):
    """act(half(conv2d(half(x), w_h, b_h))) as a new (N,128,H,W) half tensor: x (N,Cin,H,W) float32 or half (a half x is used
    as it is), wpack and bias_h from `pack_conv1`, act = relu if `relu` else the identity.  `cin` is the layer's number of
    input channels, which x must have (None: x.shape[1]; the pack's slots for channels >= cin hold zero whatever it was
    made of).  Exact products, fp32 accumulation in a fixed order, one rounding to half; NaN is kept.  x and bias_h are
    served at element alignment; a wpack that is not 16-byte aligned (never the case for what pack_conv1 returns) raises
    UnsupportedShape."""
    if x.dim() != 4:
        raise RuntimeError("x must be (N,Cin,H,W), got %s" % (tuple(x.shape),))
    cin = x.shape[1] if cin is None else int(cin)
    if not 1 <= cin <= MAX_CIN:
        raise RuntimeError("conv1x1: Cin must be in 1..%d, got %d" % (MAX_CIN, cin))
    if x.shape[1] != cin:
        raise RuntimeError("x must be (N,%d,H,W), got %s" % (cin, tuple(x.shape)))
    if wpack.numel() != WPACK_HALVES:
        raise RuntimeError("wpack must hold %d halves (pack_conv1), got %s" % (WPACK_HALVES, tuple(wpack.shape)))
    named = [(x, "x"), (wpack, "wpack"), (bias_h, "bias_h")]
    check_shape(named[2:], (COUT,))
    check_layer_operands("conv1x1", named)
    N, _, H, W = x.shape
    out = torch.empty((N, COUT, H, W), dtype=torch.float16, device=x.device)
    if N == 0:
        return out
    if H * W == 0:
        raise RuntimeError("conv1x1: empty frame (H*W = 0)")
    flags = (X_HALF if x.dtype == torch.float16 else 0) | (RELU if relu else 0)
    args = _lib.Conv1Args(x.data_ptr(), wpack.data_ptr(), bias_h.data_ptr(), out.data_ptr(), N, cin, H, W, flags)
    launch("lgu_conv1x1_o128_h16", "conv1x1", x.device, args, _stream(x))
    return out


def eligible(m):
    """m is Conv2d(1..224, 128, 1) with a bias, stride 1, no padding, dilation, groups or padding mode."""
    return isinstance(m, torch.nn.Conv2d) and 1 <= m.in_channels <= MAX_CIN and is_conv(m, m.in_channels, COUT, 1, pad=0, bias=True)


class Conv1(LayerWrapper):
    """Callable stand-in for the forward of one Conv2d(1..224, 128, 1) with a bias:

        fused = Conv1(update_module.corr_encoder[0])
        y = fused(corr)                        # = update_module.corr_encoder[0](corr); relu=True: = relu(conv(corr))

    Fused path (csrc/conv1.hip, one launch) for a HIP tensor (N,Cin,H,W), float32 or half, under CUDA autocast with
    float16, with float32 parameters on the input's device, when nothing requires grad and N*H*W >= MIN_FUSED_PIXELS
    (_host.serves_half).  Everything else goes to the module's own forward unchanged (followed by relu if relu=True): CPU
    tensors, other dtypes, a bfloat16 autocast, autocast off, and grad.  The packed weights are cached under the layer's
    weight and bias (data pointer, version, device).  `fused_calls` counts the fused launches."""

    def __init__(self, conv, relu=False):
        if not eligible(conv):
            raise RuntimeError("Conv1: the module must be Conv2d(1..%d, 128, 1) with a bias" % MAX_CIN)
        super().__init__(conv, conv, pack_conv1)
        self.relu = bool(relu)

    def _serves(self, x):
        c = self.conv
        return serves_half(x, c.in_channels, (c.weight, c.bias), MIN_FUSED_PIXELS)

    def _operator(self, x, wpack, bias_h):
        return conv1x1(x, wpack, bias_h, cin=self.conv.in_channels, relu=self.relu)


def install(conv, relu=False):
    """Bind a Conv1 (`relu` as in Conv1) as `conv.forward`, an instance attribute: parameters and state_dict keys are
    unchanged.  Returns the wrapper; a second call returns the first wrapper.  A module Conv1 does not take raises
    RuntimeError and binds nothing, and so does a module whose forward already carries another wrapper.

    `install` goes on the Conv2d, corr_encoder[0]: a conv3.Conv3Stack on corr_encoder then reaches it "as itself", in
    either install order, and the Sequential's ReLU stays a launch of its own (update.UpdateOperator fuses it)."""
    return installed(conv, Conv1, "conv1.install") or bind(conv, "forward", Conv1, lambda _: Conv1(conv, relu=relu))


def uninstall(conv):
    """Undo `install`: the class's forward is used again."""
    unbind(conv, "forward", Conv1)
