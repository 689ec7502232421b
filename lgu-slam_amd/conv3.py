"""The update operator's 3x3 convolutions with 128 input channels (reference droid_slam/droid_net.py):

    corr_encoder[2], delta[0], weight[0], agg.conv1, agg.conv2 = Conv2d(128, 128, 3, padding=1)
    flow_encoder[2]                                            = Conv2d(128, 64, 3, padding=1)

Under float16 autocast each of them is a cast, layout passes around the library's convolution, a bias launch and, for four
of the six, a ReLU launch.  `conv3x3` (csrc/conv3.hip) evaluates cast + convolution + bias (+ ReLU) in one launch on the
matrix cores, NCHW in and NCHW out, with the autocast rounding points (include/lgu_corr.h).

    conv3.install(update_module.corr_encoder)      # a Sequential: conv + ReLU pairs become one launch each
    conv3.install(update_module.agg.conv1)         # a Conv2d: its caller applies the ReLU
    conv3.install_update(update_module)            # the six sites at once; state_dict keys unchanged

`conv3x3`: contiguous HIP device tensors only (no CPU fallback), every argument error raised before anything is launched,
no host synchronisation (graph-capturable), forward only: an input that requires grad is refused while grad mode is on.
There is no fp32 kernel: fp32 evaluation is the module's own forward.
"""
import torch

from . import _lib
from ._host import (FLOAT_OR_HALF, LayerWrapper, PackCache, bind, check_layer_operands, check_shape, fused_dtype, installed,
                    is_conv, launch, serves_half, unbind)
from ._host import stream as _stream

CIN = 128
COUTS = (64, 128)
# include/lgu_corr.h LGU_CONV3_WPACK_HALVES_<Cout> = 9 * 4 * (Cout / 16) * 64 * 8
WPACK_HALVES = {64: 73728, 128: 147456}
_COUT_OF_HALVES = {v: k for k, v in WPACK_HALVES.items()}
X_HALF, RELU = 1, 2              # include/lgu_corr.h LGU_CONV3_X_HALF, LGU_CONV3_RELU

# Per Cout, the number of output pixels N * H * W below which the measured fused layer does not beat the module's own
# forward beyond the two spreads (tools/prof_conv3.py): Conv3 and Conv3Stack send such calls to the
# module.  0: every measured shape class kept the fused path.
MIN_FUSED_PIXELS = {64: 0, 128: 0}
# The number of pixels N * H * W below which `conv3x3_fanout` does not beat the separate `conv3x3` launches beyond the two
# spreads (tools/prof_outstage.py): UpdateOperator takes the separate launches below it.
# 80 x 60x80 keeps the fan-out (G = 3: 458 against 539 us); 48 x 48x64 does not at G = 3 (169 +- 10 against 181 +- 10 us:
# inside the spreads), and one threshold cannot keep 1 x 48x64 (37 against 49 us) without it.
MIN_FANOUT_PIXELS = 384000


def pack_conv3(weight, bias):
    """(wpack (9,4,Cout/16,64,8) half, bias_h (Cout) half) of a Conv2d(128, Cout, 3) weight (Cout,128,3,3) and bias (Cout),
    Cout 64 or 128, on the weight's device.  wpack[t, kc, ct, l, j] = half(weight)[16 ct + (l & 15), 32 kc + 8 (l >> 4) + j,
    t // 3, t % 3]: the B operand of v_mfma_f32_16x16x32_f16, one tap t = 3 ky + kx and one block kc of 32 input channels
    per K step.  Every slot holds a weight."""
    cout = weight.shape[0] if weight.dim() == 4 and weight.shape[0] in COUTS else COUTS[1]
    check_shape([(weight, "weight")], (cout, CIN, 3, 3))
    check_shape([(bias, "bias")], (cout,))
    with torch.no_grad():
        wh = weight.detach().to(torch.float16)
        # [ct][cl][kc][g][j][t] -> [t][kc][ct][g][cl][j]: lane l = 16 g + cl
        wpack = wh.reshape(cout // 16, 16, 4, 4, 8, 9).permute(5, 2, 0, 3, 1, 4).reshape(9, 4, cout // 16, 64, 8).contiguous()
        bias_h = bias.detach().to(device=wh.device, dtype=torch.float16).contiguous()
    return wpack, bias_h


def conv3x3(x, wpack, bias_h, relu=False):
    """act(conv2d(half(x), w_h, b_h, padding=1)) as a new (N,Cout,H,W) half tensor: x (N,128,H,W) float32 or half (a half x
    is used as it is), wpack and bias_h from `pack_conv3` (their size gives Cout), act = relu if `relu` else the identity.
    Exact products, fp32 accumulation from the bias in a fixed order, one rounding to half; NaN is kept.  x and bias_h are
    served at element alignment; a wpack that is not 16-byte aligned (never the case for what pack_conv3 returns) raises
    UnsupportedShape."""
    if x.dim() != 4 or x.shape[1] != CIN:
        raise RuntimeError("x must be (N,%d,H,W), got %s" % (CIN, tuple(x.shape)))
    cout = _COUT_OF_HALVES.get(wpack.numel())
    if cout is None:
        raise RuntimeError("wpack must hold %d or %d halves (pack_conv3), got %s"
                           % (WPACK_HALVES[64], WPACK_HALVES[128], tuple(wpack.shape)))
    named = [(x, "x"), (wpack, "wpack"), (bias_h, "bias_h")]
    check_shape(named[2:], (cout,))
    check_layer_operands("conv3x3", named)
    N, _, H, W = x.shape
    out = torch.empty((N, cout, H, W), dtype=torch.float16, device=x.device)
    if N == 0:
        return out
    if H * W == 0:
        raise RuntimeError("conv3x3: empty frame (H*W = 0)")
    flags = (X_HALF if x.dtype == torch.float16 else 0) | (RELU if relu else 0)
    args = _lib.Conv3Args(x.data_ptr(), wpack.data_ptr(), bias_h.data_ptr(), out.data_ptr(), N, H, W, cout, flags)
    launch("lgu_conv3x3_c128_h16", "conv3x3", x.device, args, _stream(x))
    return out


def conv3x3_fanout(x, packs, relu=False):
    """Two or three Conv2d(128, 128, 3, padding=1) of ONE input in one launch: a tuple of len(packs) new (N,128,H,W) half
    tensors, output g with the bits of conv3x3(x, *packs[g], relu=relu).  x (N,128,H,W) float32 or half; packs a sequence of
    two or three (wpack, bias_h) of `pack_conv3` with Cout 128.  The tile of x is staged once for all of them.  x and the
    biases are served at element alignment; a wpack that is not 16-byte aligned raises UnsupportedShape."""
    if x.dim() != 4 or x.shape[1] != CIN:
        raise RuntimeError("x must be (N,%d,H,W), got %s" % (CIN, tuple(x.shape)))
    packs = [tuple(p) for p in packs]
    if len(packs) not in (2, 3) or any(len(p) != 2 for p in packs):
        raise RuntimeError("packs must be two or three (wpack, bias_h) pairs (pack_conv3), got %d" % len(packs))
    named = [(x, "x")]
    for g, (wpack, bias_h) in enumerate(packs):
        if wpack.numel() != WPACK_HALVES[128]:
            raise RuntimeError("packs[%d]: wpack must hold %d halves (pack_conv3, Cout 128), got %s"
                               % (g, WPACK_HALVES[128], tuple(wpack.shape)))
        check_shape([(bias_h, "packs[%d]: bias_h" % g)], (128,))
        named += [(wpack, "packs[%d]: wpack" % g), (bias_h, "packs[%d]: bias_h" % g)]
    check_layer_operands("conv3x3_fanout", named)
    N, _, H, W = x.shape
    outs = tuple(torch.empty((N, 128, H, W), dtype=torch.float16, device=x.device) for _ in packs)
    if N == 0:
        return outs
    if H * W == 0:
        raise RuntimeError("conv3x3_fanout: empty frame (H*W = 0)")
    G = len(packs)
    three = _lib._vp * 3
    flags = (X_HALF if x.dtype == torch.float16 else 0) | (RELU if relu else 0)
    args = _lib.Conv3FanoutArgs(x.data_ptr(), three(*[p[0].data_ptr() for p in packs]), three(*[p[1].data_ptr() for p in packs]),
                                three(*[o.data_ptr() for o in outs]), N, H, W, G, flags)
    launch("lgu_conv3x3_fanout_c128_h16", "conv3x3_fanout", x.device, args, _stream(x))
    return outs


def eligible(m):
    """m is Conv2d(128, 64 or 128, 3, padding=1) with a bias, stride 1, no dilation, groups or padding mode."""
    return any(is_conv(m, CIN, cout, 3, pad=1, bias=True) for cout in COUTS)


def _serves(conv, x):
    """The fused path applies to this call of an eligible `conv` on x."""
    return serves_half(x, CIN, (conv.weight, conv.bias), MIN_FUSED_PIXELS[conv.out_channels])


class Conv3(LayerWrapper):
    """Callable stand-in for the forward of one Conv2d(128, 64 or 128, 3, padding=1) with a bias:

        fused = Conv3(update_module.agg.conv1)
        y = fused(net)                         # = update_module.agg.conv1(net); relu=True: = relu(conv(net))

    Fused path (csrc/conv3.hip) for a HIP tensor (N,128,H,W), float32 or half, under CUDA autocast with float16, with
    float32 parameters on the input's device, when nothing requires grad and N*H*W >= MIN_FUSED_PIXELS[Cout]
    (_host.serves_half).  Everything else goes to the module's own forward unchanged (followed by relu if relu=True): CPU
    tensors, other dtypes, a bfloat16 autocast, autocast off, and grad.  The packed weights are cached under the layer's
    weight and bias (data pointer, version, device).  `fused_calls` counts the fused launches."""

    def __init__(self, conv, relu=False):
        if not eligible(conv):
            raise RuntimeError("Conv3: the module must be Conv2d(128, 64 or 128, 3, padding=1) with a bias")
        super().__init__(conv, conv, pack_conv3)
        self.relu = bool(relu)

    def _serves(self, x):
        return _serves(self.conv, x)

    def _operator(self, x, wpack, bias_h):
        return conv3x3(x, wpack, bias_h, relu=self.relu)


class Conv3Stack:
    """Callable stand-in for the forward of an nn.Sequential that holds at least one eligible convolution (the
    reference's corr_encoder, delta and weight):

        fused = Conv3Stack(update_module.delta)
        d = fused(net)                         # = update_module.delta(net)

    An eligible convolution followed by nn.ReLU is one launch with the ReLU in it (the ReLU member is skipped), one not
    followed by nn.ReLU is one launch without; every other member is called as itself.  The fused path is taken for a HIP
    float32 or half 4-D input under CUDA float16 autocast when nothing (the input, any parameter of the Sequential)
    requires grad; otherwise the whole call goes to the module's own forward.  Inside the fused path a convolution whose
    input does not qualify (shape, MIN_FUSED_PIXELS, parameters) is called as itself, like any other member.
    `fused_calls` counts the fused launches."""

    def __init__(self, module):
        if not isinstance(module, torch.nn.Sequential) or not any(eligible(m) for m in module):
            raise RuntimeError("Conv3Stack: the module must be an nn.Sequential that holds a Conv2d(128, 64 or 128, 3, "
                               "padding=1) with a bias")
        self.module = module
        self._packs = PackCache()
        self.fused_calls = 0

    def _fused(self, x):
        if not isinstance(x, torch.Tensor) or not x.is_cuda or x.dim() != 4 or x.dtype not in FLOAT_OR_HALF:
            return False
        return fused_dtype([x] + list(self.module.parameters())) == torch.float16

    def __call__(self, x):
        seq = self.module
        if not self._fused(x):
            return type(seq).forward(seq, x)
        members = list(seq)
        i = 0
        while i < len(members):
            m = members[i]
            if eligible(m) and _serves(m, x):
                relu = i + 1 < len(members) and isinstance(members[i + 1], torch.nn.ReLU)
                wpack, bias_h = self._packs.of(m, pack_conv3)
                x = conv3x3(x.contiguous(), wpack, bias_h, relu=relu)
                self.fused_calls += 1
                i += 2 if relu else 1
            else:
                x = m(x)
                i += 1
        return x


_WRAPPERS = (Conv3, Conv3Stack)


def install(module, relu=False):
    """Bind a Conv3 (module a Conv2d; `relu` as in Conv3) or a Conv3Stack (module an nn.Sequential) as `module.forward`,
    an instance attribute: parameters and state_dict keys are unchanged.  Returns the wrapper; a second call returns the
    first wrapper.  Anything else raises RuntimeError and binds nothing, and so does a Sequential whose forward already
    carries another wrapper (install on its eligible member instead)."""
    cur = installed(module, _WRAPPERS, "conv3.install", "; install on the eligible Conv2d inside it")
    if cur is not None:
        return cur
    if isinstance(module, torch.nn.Conv2d):
        return bind(module, "forward", Conv3, lambda _: Conv3(module, relu=relu))
    if isinstance(module, torch.nn.Sequential):
        return bind(module, "forward", Conv3Stack, lambda _: Conv3Stack(module))
    raise RuntimeError("conv3.install: the module must be a Conv2d or an nn.Sequential, got %s" % type(module).__name__)


def uninstall(module):
    """Undo `install`: the class's forward is used again."""
    for cls in _WRAPPERS:
        unbind(module, "forward", cls)


def _sites(update):
    return (("corr_encoder", update.corr_encoder), ("flow_encoder[2]", update.flow_encoder[2]), ("delta", update.delta),
            ("weight", update.weight), ("agg.conv1", update.agg.conv1), ("agg.conv2", update.agg.conv2))


def install_update(update):
    """`install` on the six sites of an object shaped like the reference's UpdateModule: corr_encoder, delta and weight as
    stacks, flow_encoder[2], agg.conv1 and agg.conv2 as convolutions without ReLU (their callers apply it).  Works with
    or without flow.install / gru.install on the same module.  Returns {site name: wrapper}."""
    sites = _sites(update)
    for name, m in sites:       # refuse before anything is bound
        ok = any(eligible(c) for c in m) if isinstance(m, torch.nn.Sequential) else eligible(m)
        if not ok:
            raise RuntimeError("conv3.install_update: %s holds no Conv2d(128, 64 or 128, 3, padding=1) with a bias" % name)
    return {name: install(m) for name, m in sites}


def uninstall_update(update):
    """Undo `install_update`."""
    for _, m in _sites(update):
        uninstall(m)
