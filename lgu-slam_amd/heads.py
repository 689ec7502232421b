"""The update operator's narrow 3x3 output heads with 128 input channels (reference droid_slam/droid_net.py):

    delta[2]   = Conv2d(128, 2, 3, padding=1)
    weight[2]  = Conv2d(128, 2, 3, padding=1), followed by GradientClip and Sigmoid
    agg.eta    = Sequential(Conv2d(128, 1, 3, padding=1), GradientClip, Softplus)

Under float16 autocast each of them is a cast, layout passes around a library convolution sized for wide outputs, a bias
launch and, for two of the three, an activation launch, all for one or two channels.  `head_conv3x3` (csrc/heads.hip)
evaluates cast + convolution + bias (+ sigmoid or softplus) in one launch, NCHW in and NCHW out, with the autocast
rounding points (include/lgu_corr.h).

    heads.install(update_module.delta[2])          # a Conv2d: one launch
    heads.install(update_module.agg.eta)           # a tail Sequential: conv + GradientClip + Softplus in one launch
    heads.install_update(update_module)            # the three sites at once; state_dict keys unchanged

`head_conv3x3`: contiguous HIP device tensors only (no CPU fallback), every argument error raised before anything is
launched, no host synchronisation (graph-capturable), forward only: an input that requires grad is refused while grad mode
is on.  There is no fp32 kernel: fp32 evaluation is the module's own forward.
"""
import torch

from . import _lib
from ._host import (FLOAT_OR_HALF, LayerWrapper, bind, check_contiguous, check_device, check_dtype, check_layer_operands,
                    check_no_grad, check_shape, installed, is_conv, launch, serves_half, unbind)
from ._host import stream as _stream

CIN = 128
COUTS = (1, 2)
# include/lgu_corr.h LGU_HEAD_WPACK_HALVES_<Cout> = 4 * ceil(9 * Cout / 16) * 64 * 8
WPACK_HALVES = {1: 2048, 2: 4096}
_COUT_OF_HALVES = {v: k for k, v in WPACK_HALVES.items()}
X_HALF, SIGMOID, SOFTPLUS = 1, 2, 4      # include/lgu_corr.h LGU_HEAD_X_HALF, LGU_HEAD_SIGMOID, LGU_HEAD_SOFTPLUS
ACTS = {"none": 0, "sigmoid": SIGMOID, "softplus": SOFTPLUS}
# type names of the members a tail may hold between its convolution and its activation: their forward is the identity
PASSTHROUGH = ("GradientClip", "Identity")

# Per Cout, the number of output pixels N * H * W below which the measured fused layer does not beat the module's own
# forward beyond the two spreads (tools/prof_heads.py): Head sends such calls to the module.
# 0: every measured shape class kept the fused path.
MIN_FUSED_PIXELS = {1: 0, 2: 0}
PAIR_F32 = 8                             # include/lgu_corr.h LGU_HEAD_PAIR_F32
# The number of pixels N * H * W below which `head_pair` does not beat the two `head_conv3x3` launches and their edge-major
# copies beyond the two spreads (tools/prof_outstage.py): UpdateOperator takes those below it.
# 0: every measured shape class kept the pair, in both output modes.
MIN_PAIR_PIXELS = 0


def pack_head(weight, bias):
    """(wpack (4,NT,64,8) half, bias_h (Cout) half) of a Conv2d(128, Cout, 3) weight (Cout,128,3,3) and bias (Cout), Cout 1
    or 2, on the weight's device; NT = 1 for Cout 1 and 2 for Cout 2.  With the column q = 16 nt + (l & 15):
    wpack[kc, nt, l, j] = half(weight)[q % Cout, 32 kc + 8 (l >> 4) + j, t // 3, t % 3] for the tap t = q // Cout where
    q < 9 Cout, and zero where q >= 9 Cout: the B operand of v_mfma_f32_16x16x32_f16 whose columns are the per-tap partial
    sums, one block kc of 32 input channels per K step."""
    cout = weight.shape[0] if weight.dim() == 4 and weight.shape[0] in COUTS else COUTS[1]
    check_shape([(weight, "weight")], (cout, CIN, 3, 3))
    check_shape([(bias, "bias")], (cout,))
    nt = (9 * cout + 15) // 16
    with torch.no_grad():
        wh = weight.detach().to(torch.float16)
        cols = torch.zeros((16 * nt, CIN), dtype=torch.float16, device=wh.device)
        cols[:9 * cout] = wh.permute(2, 3, 0, 1).reshape(9 * cout, CIN)          # q = t * Cout + co
        # [nt][cl][kc][g][j] -> [kc][nt][g][cl][j]: lane l = 16 g + cl
        wpack = cols.reshape(nt, 16, 4, 4, 8).permute(2, 0, 3, 1, 4).reshape(4, nt, 64, 8).contiguous()
        bias_h = bias.detach().to(device=wh.device, dtype=torch.float16).contiguous()
    return wpack, bias_h


def head_conv3x3(x, wpack, bias_h, act="none"):
    """act(half(conv2d(half(x), w_h, b_h, padding=1))) as a new (N,Cout,H,W) tensor: x (N,128,H,W) float32 or half (a half x
    is used as it is), wpack and bias_h from `pack_head` (their size gives Cout), act "none" (half out), "sigmoid"
    (evaluated in fp32 on the half value, half out) or "softplus" (beta 1, threshold 20, evaluated in fp32 on the half
    value, float32 out: the dtype torch's autocast gives softplus).  Exact products, fp32 accumulation in a fixed order,
    one rounding to half; NaN is kept.  x and bias_h are served at element alignment; a wpack that is not 16-byte aligned
    (never the case for what pack_head returns) raises UnsupportedShape."""
    if act not in ACTS:
        raise RuntimeError("act must be one of 'none', 'sigmoid', 'softplus', got %r" % (act,))
    if x.dim() != 4 or x.shape[1] != CIN:
        raise RuntimeError("x must be (N,%d,H,W), got %s" % (CIN, tuple(x.shape)))
    cout = _COUT_OF_HALVES.get(wpack.numel())
    if cout is None:
        raise RuntimeError("wpack must hold %d or %d halves (pack_head), got %s"
                           % (WPACK_HALVES[1], WPACK_HALVES[2], tuple(wpack.shape)))
    named = [(x, "x"), (wpack, "wpack"), (bias_h, "bias_h")]
    check_shape(named[2:], (cout,))
    check_layer_operands("head_conv3x3", named)
    N, _, H, W = x.shape
    out = torch.empty((N, cout, H, W), dtype=torch.float32 if act == "softplus" else torch.float16, device=x.device)
    if out.numel() == 0:
        return out
    flags = (X_HALF if x.dtype == torch.float16 else 0) | ACTS[act]
    args = _lib.HeadArgs(x.data_ptr(), wpack.data_ptr(), bias_h.data_ptr(), out.data_ptr(), N, H, W, cout, flags)
    launch("lgu_head3x3_c128_h16", "head_conv3x3", x.device, args, _stream(x))
    return out


def head_pair(d, w, pack_delta, pack_weight, coords=None):
    """The reference's delta[2] and weight[2] + Sigmoid in one launch, edge-major: d and w (N,128,H,W), the same shape and
    dtype (float32 or half), pack_delta and pack_weight (wpack, bias_h) of `pack_head` with Cout 2.

    Without `coords`: (delta, weight), each a new (1,N,H,W,2) half tensor with the bits of
    head_conv3x3(d, *pack_delta, act="none") and head_conv3x3(w, *pack_weight, act="sigmoid") behind the reference's
    view / permute / [..., :2] / contiguous.
    With `coords` (1,N,H,W,2) float32: (target, weight), each a new (1,N,H,W,2) float32 tensor, target = coords +
    delta.float() (one fp32 add, coords read at that element only) and weight = weight.float(): what the factor graph
    keeps."""
    for t, name in ((d, "d"), (w, "w")):
        if t.dim() != 4 or t.shape[1] != CIN:
            raise RuntimeError("%s must be (N,%d,H,W), got %s" % (name, CIN, tuple(t.shape)))
    check_shape([(w, "w")], d.shape)
    named = [(d, "d"), (w, "w")]
    for (wpack, bias_h), name in ((pack_delta, "pack_delta"), (pack_weight, "pack_weight")):
        if wpack.numel() != WPACK_HALVES[2]:
            raise RuntimeError("%s: wpack must hold %d halves (pack_head, Cout 2), got %s" % (name, WPACK_HALVES[2], tuple(wpack.shape)))
        check_shape([(bias_h, name + ": bias_h")], (2,))
        named += [(wpack, name + ": wpack"), (bias_h, name + ": bias_h")]
    N, _, H, W = d.shape
    if coords is not None:
        check_shape([(coords, "coords")], (1, N, H, W, 2))
        named.append((coords, "coords"))
    check_contiguous(named)
    check_dtype(named[:1], FLOAT_OR_HALF)
    check_dtype(named[1:2], d.dtype)
    check_dtype(named[2:6], torch.float16)
    check_dtype(named[6:], torch.float32)
    check_no_grad("head_pair", named)
    check_device(named)
    odt = torch.float16 if coords is None else torch.float32
    outs = tuple(torch.empty((1, N, H, W, 2), dtype=odt, device=d.device) for _ in range(2))
    if outs[0].numel() == 0:
        return outs
    two = _lib._vp * 2
    flags = (X_HALF if d.dtype == torch.float16 else 0) | (0 if coords is None else PAIR_F32)
    args = _lib.HeadPairArgs(two(d.data_ptr(), w.data_ptr()), two(pack_delta[0].data_ptr(), pack_weight[0].data_ptr()),
                             two(pack_delta[1].data_ptr(), pack_weight[1].data_ptr()), two(outs[0].data_ptr(), outs[1].data_ptr()),
                             None if coords is None else coords.data_ptr(), N, H, W, flags)
    launch("lgu_head3x3_pair_c128_h16", "head_pair", d.device, args, _stream(d))
    return outs


def eligible(m):
    """m is Conv2d(128, 1 or 2, 3, padding=1) with a bias, stride 1, no dilation, groups or padding mode."""
    return any(is_conv(m, CIN, cout, 3, pad=1, bias=True) for cout in COUTS)


def parse(module):
    """(conv, act) of an eligible Conv2d or of a tail Sequential [eligible conv, PASSTHROUGH members..., at most one final
    Sigmoid or Softplus(beta=1, threshold=20)]; None for anything else."""
    nn = torch.nn
    if eligible(module):
        return module, "none"
    if not isinstance(module, nn.Sequential) or len(module) == 0 or not eligible(module[0]):
        return None
    rest, act = list(module)[1:], "none"
    if rest and isinstance(rest[-1], nn.Sigmoid):
        rest, act = rest[:-1], "sigmoid"
    elif rest and isinstance(rest[-1], nn.Softplus):
        if rest[-1].beta != 1 or rest[-1].threshold != 20:
            return None
        rest, act = rest[:-1], "softplus"
    if any(type(m).__name__ not in PASSTHROUGH for m in rest):
        return None
    return module[0], act


class Head(LayerWrapper):
    """Callable stand-in for the forward of one Conv2d(128, 1 or 2, 3, padding=1) with a bias, or of a "tail"
    nn.Sequential that is exactly [such a convolution, zero or more members whose type name is in PASSTHROUGH, at most
    one final nn.Sigmoid or nn.Softplus(beta=1, threshold=20)] (the reference's GraphAgg.eta):

        fused = Head(update_module.agg.eta)
        eta = fused(net)                       # = update_module.agg.eta(net)

    Fused path (csrc/heads.hip, one launch with the activation in it) for a HIP tensor (N,128,H,W), float32 or half,
    under CUDA autocast with float16, with float32 parameters on the input's device, when nothing requires grad and
    N*H*W >= MIN_FUSED_PIXELS[Cout] (_host.serves_half; the convolution's weight and bias are all the parameters a tail
    has).  The result has the module's own dtype there: half, or float32 behind a Softplus (which autocast evaluates in
    float32).  Everything else goes to the module's own forward unchanged: CPU tensors, other dtypes, a bfloat16 autocast,
    autocast off, and grad.  The packed weights are cached under the layer's weight and bias (data pointer, version,
    device).  `fused_calls` counts the fused launches."""

    def __init__(self, module):
        parsed = parse(module)
        if parsed is None:
            raise RuntimeError("Head: the module must be Conv2d(128, 1 or 2, 3, padding=1) with a bias, or an nn.Sequential of "
                               "such a convolution, members named %s and at most one final Sigmoid or Softplus(beta=1, "
                               "threshold=20)" % " or ".join(PASSTHROUGH))
        super().__init__(module, parsed[0], pack_head)
        self.act = parsed[1]

    def _serves(self, x):
        c = self.conv
        return serves_half(x, CIN, (c.weight, c.bias), MIN_FUSED_PIXELS[c.out_channels])

    def _operator(self, x, wpack, bias_h):
        return head_conv3x3(x, wpack, bias_h, act=self.act)


def install(module):
    """Bind a Head as `module.forward`, an instance attribute: parameters and state_dict keys are unchanged.  Returns the
    wrapper; a second call returns the first wrapper.  A module Head does not take raises RuntimeError and binds nothing,
    and so does a module whose forward already carries another wrapper.

    Through `install` the Sigmoid of the reference's `weight` stays a launch of its own: `install` goes on weight[2], the
    Conv2d, because a wrapper that owned the whole `weight` Sequential would collide with conv3's Conv3Stack on it.  Only
    a tail that is a Sequential of its own (agg.eta) gets its activation fused."""
    return installed(module, Head, "heads.install") or bind(module, "forward", Head, lambda _: Head(module))


def uninstall(module):
    """Undo `install`: the class's forward is used again."""
    unbind(module, "forward", Head)


def _sites(update):
    return (("delta[2]", update.delta[2]), ("weight[2]", update.weight[2]), ("agg.eta", update.agg.eta))


def install_update(update):
    """`install` on the three sites of an object shaped like the reference's UpdateModule: delta[2] and weight[2] as
    convolutions (weight's Sigmoid stays its own launch, see `install`), agg.eta as a tail with the softplus fused.  Works
    with or without conv3.install_update on the same module, in either order: a Conv3Stack calls delta[2] and weight[2]
    as themselves.  Refuses before anything is bound if a site does not match.  Returns {site name: wrapper}."""
    sites = _sites(update)
    for name, m in sites:       # refuse before anything is bound
        parsed = parse(m)
        want_tail = name == "agg.eta"
        ok = parsed is not None and isinstance(m, torch.nn.Sequential) == want_tail and (not want_tail or parsed[1] == "softplus")
        if not ok:
            raise RuntimeError("heads.install_update: %s is not %s" % (name, "a Sequential of Conv2d(128, 1 or 2, 3, padding=1), "
                               "pass-through members and Softplus" if want_tail else "a Conv2d(128, 1 or 2, 3, padding=1) with a bias"))
        cur = m.__dict__.get("forward")
        if cur is not None and not isinstance(cur, Head):
            raise RuntimeError("heads.install_update: the forward of %s already carries a %s" % (name, type(cur).__name__))
    return {name: install(m) for name, m in sites}


def uninstall_update(update):
    """Undo `install_update`."""
    for _, m in _sites(update):
        uninstall(m)
