"""The 3x3 convolutions of the encoders' residual stages (reference droid_slam/modules/extractor.py: layer1..3 of
BasicEncoder, two ResidualBlocks each, DIM = 32):

    layer1  Conv2d(32, 32, 3, padding=1) x 4
    layer2  Conv2d(32, 64, 3, stride=2, padding=1) + Conv2d(32, 64, 1, stride=2),  Conv2d(64, 64, 3, padding=1) x 3
    layer3  Conv2d(64, 128, 3, stride=2, padding=1) + Conv2d(64, 128, 1, stride=2), Conv2d(128, 128, 3, padding=1) x 3

Under float16 autocast each of them is the library's convolution with its layout passes and a bias launch, and in the
norm-free context encoder a ReLU, an add and another ReLU behind it.  `enc_conv3x3` (csrc/encconv.hip) evaluates the
convolution, the bias and that tail in one launch on the matrix cores, NCHW half in and NCHW half out, and on the strided
shapes gives the block's 1x1 stride-2 downsample branch from the same launch (include/lgu_corr.h states the rounding
points).  `context.ContextEncoder` and `features.FeatureEncoder(convs=True)` are its callers.

The two ends of the same encoder, conv1 = Conv2d(3, 32, 7, stride=2, padding=3) and conv2 = Conv2d(128, Cout, 1), are
`enc_stem7x7` and `enc_out1x1` (csrc/encends.hip), one launch each: the stem with the norm-free encoder's ReLU as its
epilogue, the output layer with the context encoder's `net.tanh()` / `inp.relu()` split.  `ContextEncoder(ends=True)`
and `FeatureEncoder(ends=True)` are their callers.

The feature encoder's instance norms fold into the same launches (`enc_conv3x3_norm`): the producer convolution adds exact
integer sums of its stored outputs to per-plane accumulators (`new_stats`), the consumer normalises while it stages its
input and writes the staged tensor out where it is a residual later; `stats_mean_rstd` is the (mean, rstd) the consumer
forms.  `features.FeatureEncoder(convs=True, norms=True)` is the caller.

`enc_conv3x3`, `enc_conv3x3_norm`, `enc_stem7x7`, `enc_out1x1`: contiguous HIP device tensors only (no CPU fallback), every argument error
raised before anything is launched, no host synchronisation (graph-capturable), forward only: an input that requires grad
is refused while grad mode is on.  There is no fp32 kernel: fp32 evaluation is the module's own forward.
"""
import torch

from . import _lib
from ._host import check_contiguous, check_device, check_dtype, check_layer_operands, check_no_grad, check_shape, is_conv, launch
from ._host import stream as _stream

# (Cin, Cout, stride) of Conv2d(Cin, Cout, 3, stride, padding=1) the kernel serves
SHAPES = ((32, 32, 1), (32, 64, 2), (64, 64, 1), (64, 128, 2), (128, 128, 1))
_CHANNELS = tuple(sorted({(cin, cout) for cin, cout, _ in SHAPES}))
_STRIDE_OF = {(cin, cout): s for cin, cout, s in SHAPES}
RELU, RESIDUAL = 1, 2            # include/lgu_corr.h LGU_ENCCONV_RELU, LGU_ENCCONV_RESIDUAL

# Per (Cin, Cout, stride), the number of output pixels N * Ho * Wo below which the measured fused layer does not beat the
# module's own call with the tail it replaces beyond the two spreads (tools/prof_encconv.py):
# ContextEncoder and FeatureEncoder(convs=True) send such calls to the module's convolution.  0: every measured class (1
# and 16 frames of 384x512) kept the fused path.
MIN_FUSED_PIXELS = {shape: 0 for shape in SHAPES}

# FeatureEncoder(norms=True): the pixels N * H * W of the images below which the folded route (the instance norms inside
# the twelve convolutions) is not taken and the per-site route runs.  Set from the measurement of tools/prof_encconv.py
# --norms: 0 only for classes where the folded forward beat the per-site one beyond both spreads.
# 1 << 62: neither measured class (1 and 16 frames of 384x512) did, the folded forward is the slower one at both, so
# norms=True keeps today's route until a caller lowers this.
MIN_NORMS_PIXELS = 1 << 62
MAX_STATS_PLANE = 1 << 22        # pixels per plane the exact sums are proved for (include/lgu_corr.h)
NORM, RES, RES_NORM = 1, 2, 3    # LGU_ENCNORM_NORM, LGU_ENCNORM_RES, LGU_ENCNORM_RES_NORM
EMIT = 1                         # LGU_ENCNORM_EMIT
_PRE = {"norm": (NORM, 2), "res": (RES, 3), "res_norm": (RES_NORM, 4)}

STEM = (3, 32)                   # (Cin, Cout) of the 7x7 stride-2 stem
OUT_CIN, OUT_COUTS = 128, (128, 256)
X_HALF, STEM_RELU = 1, 2         # include/lgu_corr.h LGU_ENCSTEM_X_HALF, LGU_ENCSTEM_RELU
SPLIT = 1                        # LGU_ENCOUT_SPLIT
# The same rule for the two ends (tools/prof_encconv.py): output pixels N * Ho * Wo of the stem, and
# N * H * W of the output layer per Cout, below which the module's own call is taken.  0: every measured class (1 and 16
# frames of 384x512) kept the fused path.
MIN_STEM_PIXELS = 0
MIN_OUT_PIXELS = {128: 0, 256: 0}


def _check_channels(weight, k, who):
    ok = weight.dim() == 4 and (weight.shape[1], weight.shape[0]) in _CHANNELS and (k == 3 or weight.shape[0] != weight.shape[1])
    cin, cout = (weight.shape[1], weight.shape[0]) if ok else (64, 128)
    if not ok or tuple(weight.shape[2:]) != (k, k):
        raise RuntimeError("%s: weight must be (Cout,Cin,%d,%d) with (Cin, Cout) in %s, got %s"
                           % (who, k, k, [c for c in _CHANNELS if k == 3 or c[0] != c[1]], tuple(weight.shape)))
    return cin, cout


def pack_enc3(weight, bias):
    """(wpack (9,Cin/32,Cout/16,64,8) half, bias_h (Cout) half) of a Conv2d(Cin, Cout, 3) weight (Cout,Cin,3,3) and bias
    (Cout), (Cin, Cout) one of (32,32), (32,64), (64,64), (64,128), (128,128), on the weight's device.
    wpack[t, kc, ct, l, j] = half(weight)[16 ct + (l & 15), 32 kc + 8 (l >> 4) + j, t // 3, t % 3]: the B operand of
    v_mfma_f32_16x16x32_f16, one tap t = 3 ky + kx and one block kc of 32 input channels per K step, channel tile ct of 16
    output channels, lane l, element j.  Every slot holds a weight."""
    cin, cout = _check_channels(weight, 3, "pack_enc3")
    check_shape([(bias, "bias")], (cout,))
    with torch.no_grad():
        wh = weight.detach().to(torch.float16)
        # [ct][cl][kc][g][j][t] -> [t][kc][ct][g][cl][j]: lane l = 16 g + cl
        wpack = wh.reshape(cout // 16, 16, cin // 32, 4, 8, 9).permute(5, 2, 0, 3, 1, 4).reshape(9, cin // 32, cout // 16, 64, 8)
        bias_h = bias.detach().to(device=wh.device, dtype=torch.float16).contiguous()
    return wpack.contiguous(), bias_h


def pack_enc1(weight, bias):
    """(dpack (Cin/32,Cout/16,64,8) half, bias_h (Cout) half) of a downsample branch's Conv2d(Cin, Cout, 1, stride=2)
    weight (Cout,Cin,1,1) and bias (Cout), (Cin, Cout) (32,64) or (64,128), on the weight's device.
    dpack[kc, ct, l, j] = half(weight)[16 ct + (l & 15), 32 kc + 8 (l >> 4) + j, 0, 0]: block kc of 32 input channels,
    channel tile ct of 16 output channels, lane l, element j.  Every slot holds a weight."""
    cin, cout = _check_channels(weight, 1, "pack_enc1")
    check_shape([(bias, "bias")], (cout,))
    with torch.no_grad():
        wh = weight.detach().to(torch.float16)
        # [ct][cl][kc][g][j] -> [kc][ct][g][cl][j]
        dpack = wh.reshape(cout // 16, 16, cin // 32, 4, 8).permute(2, 0, 3, 1, 4).reshape(cin // 32, cout // 16, 64, 8)
        bias_h = bias.detach().to(device=wh.device, dtype=torch.float16).contiguous()
    return dpack.contiguous(), bias_h


def out_size(H, W, stride):
    """(Ho, Wo) = (ceil(H / stride), ceil(W / stride)): torch's rule for kernel 3, padding 1."""
    return (H + stride - 1) // stride, (W + stride - 1) // stride


def enc_conv3x3(x, pack, stride=1, relu=False, residual=None, down=None):
    """The convolution Conv2d(Cin, Cout, 3, stride, padding=1) of half x (N,Cin,H,W) with `pack` = (wpack, bias_h) of
    `pack_enc3` (the bias gives Cout), as a new (N,Cout,Ho,Wo) half tensor y, (Ho, Wo) = out_size(H, W, stride):

        y0 = half(b_h + sum x * w_h)      exact products, fp32 accumulation from the bias in a fixed order, one rounding
        y  = y0                           relu=False, residual=None
           = relu(y0)                     relu=True
           = relu(residual + relu(y0))    residual (N,Cout,Ho,Wo) half: the tail of a norm-free ResidualBlock, the add
                                          rounded to half once; relu=True says nothing more with it

    down = (dpack, dbias_h) of `pack_enc1` (stride 2 only): returns (y, r) with r = half(b'_h + sum_c x[c, 2y, 2x] w'_h),
    the block's 1x1 stride-2 downsample branch, from the same launch; y has the bits of the call without it.  NaN is kept.

    Refusals, in this order, all before anything is launched: x not 4-D, stride not 1 or 2, pack not a pair, bias_h not 1-D,
    (Cin, Cout, stride) not a served shape (UnsupportedShape), the size of wpack, x not half, the shape then the dtype of
    residual, down with stride 1, down not a pair, the sizes of dpack and dbias_h, then contiguity, dtypes (half), grad
    and device of x, wpack, bias_h, residual, dpack, dbias_h in that order (_host.check_layer_operands); then N == 0
    returns the empty result and H*W == 0 raises.  x, residual and the biases are served at element alignment; a pack that
    is not 16-byte aligned (never the case for what the pack functions return) raises UnsupportedShape."""
    if x.dim() != 4:
        raise RuntimeError("x must be (N,Cin,H,W), got %s" % (tuple(x.shape),))
    if stride not in (1, 2):
        raise RuntimeError("stride must be 1 or 2, got %r" % (stride,))
    if not isinstance(pack, (tuple, list)) or len(pack) != 2:
        raise RuntimeError("pack must be (wpack, bias_h) of pack_enc3")
    wpack, bias_h = pack
    if bias_h.dim() != 1:
        raise RuntimeError("bias_h must be (Cout,), got %s" % (tuple(bias_h.shape),))
    N, cin, H, W = x.shape
    cout = bias_h.shape[0]
    if (cin, cout, stride) not in SHAPES:
        raise _lib.UnsupportedShape("enc_conv3x3 serves (Cin, Cout, stride) in %s, got (%d, %d, %d)" % (list(SHAPES), cin, cout, stride))
    if wpack.numel() != 9 * cin * cout:
        raise RuntimeError("wpack must hold %d halves (pack_enc3, %d -> %d), got %s" % (9 * cin * cout, cin, cout, tuple(wpack.shape)))
    check_dtype([(x, "x")], torch.float16)
    Ho, Wo = out_size(H, W, stride)
    named = [(x, "x"), (wpack, "wpack"), (bias_h, "bias_h")]
    if residual is not None:
        check_shape([(residual, "residual")], (N, cout, Ho, Wo))
        check_dtype([(residual, "residual")], torch.float16)
        named.append((residual, "residual"))
    if down is not None:
        if stride != 2:
            raise RuntimeError("down (the 1x1 stride-2 branch) needs stride=2")
        if not isinstance(down, (tuple, list)) or len(down) != 2:
            raise RuntimeError("down must be (dpack, dbias_h) of pack_enc1")
        dpack, dbias_h = down
        if dpack.numel() != cin * cout:
            raise RuntimeError("dpack must hold %d halves (pack_enc1, %d -> %d), got %s" % (cin * cout, cin, cout, tuple(dpack.shape)))
        check_shape([(dbias_h, "dbias_h")], (cout,))
        named += [(dpack, "dpack"), (dbias_h, "dbias_h")]
    check_layer_operands("enc_conv3x3", named)
    out = torch.empty((N, cout, Ho, Wo), dtype=torch.float16, device=x.device)
    r = torch.empty_like(out) if down is not None else None
    if N > 0:
        if H * W == 0:
            raise RuntimeError("enc_conv3x3: empty frame (H*W = 0)")
        flags = RESIDUAL if residual is not None else (RELU if relu else 0)
        args = _lib.EncConvArgs(x.data_ptr(), wpack.data_ptr(), bias_h.data_ptr(), residual.data_ptr() if residual is not None else None,
                                out.data_ptr(), down[0].data_ptr() if down is not None else None,
                                down[1].data_ptr() if down is not None else None, r.data_ptr() if down is not None else None,
                                N, H, W, cin, cout, stride, flags)
        launch("lgu_encconv3x3_h16", "enc_conv3x3", x.device, args, _stream(x))
    return out if down is None else (out, r)


def stats_replicas():
    """R, the slots per plane of an accumulator tensor (lgu_encstats_replicas)."""
    return int(_lib.load().lgu_encstats_replicas())


def new_stats(N, C, device):
    """Zeroed accumulators (N,C,R,4) int64 for the exact sums of N x C half planes: per plane R = stats_replicas() slots of
    S1 = sum x 2^24, LO = sum (x 2^24)^2 mod 2^40, HI = sum (x 2^24)^2 >> 40 and BAD = the number of non-finite values
    (include/lgu_corr.h).  One fill launch."""
    return torch.zeros((N, C, stats_replicas(), 4), dtype=torch.int64, device=device)


def stats_mean_rstd(acc, cnt, eps=1e-5):
    """(N,C,2) float32 {mean, rstd} of the planes of cnt pixels whose accumulators (N,C,R,4) int64 `acc` holds: the device
    function the consumer's prologue uses (lgu_encstats_finalize), double arithmetic in the order of include/lgu_corr.h; a
    plane with BAD != 0 gives NaN for both.  Refusals in this order: acc not (N,C,R,4), not int64, cnt outside
    [1, 2^22] (above: UnsupportedShape), eps < 0, then contiguity and device."""
    if acc.dim() != 4 or tuple(acc.shape[2:]) != (stats_replicas(), 4):
        raise RuntimeError("acc must be (N,C,%d,4), got %s" % (stats_replicas(), tuple(acc.shape)))
    check_dtype([(acc, "acc")], torch.int64)
    if cnt < 1:
        raise RuntimeError("cnt must be >= 1, got %r" % (cnt,))
    if cnt > MAX_STATS_PLANE:
        raise _lib.UnsupportedShape("stats_mean_rstd serves planes of at most 2^22 pixels, got %d" % cnt)
    if not eps >= 0:
        raise ValueError("eps must be >= 0, got %r" % (eps,))
    check_contiguous([(acc, "acc")])
    check_device([(acc, "acc")])
    out = torch.empty((acc.shape[0], acc.shape[1], 2), dtype=torch.float32, device=acc.device)
    if out.numel():
        args = _lib.EncStatsArgs(acc.data_ptr(), out.data_ptr(), acc.shape[0] * acc.shape[1], int(cnt), float(eps))
        launch("lgu_encstats_finalize", "stats_mean_rstd", acc.device, args, _stream(acc))
    return out


def enc_conv3x3_norm(x, pack, stride=1, down=None, pre=None, keep=False, emit=False, eps=1e-5, stats_out=None):
    """`enc_conv3x3(h, pack, stride, down=down)` (identity epilogue) of a tensor h that is formed while x is staged, with the
    exact sums of the outputs on request: one launch, (out, r, kept, out_stats, r_stats) with None where not asked for.

        pre None                   h = x
        ("norm", sx)               h = half(relu(IN(x; sx)))                         extractor.py:49-50
        ("res", sx, y)             h = half(relu(float(y) + relu(IN(x; sx))))        :50, :55, no downsample
        ("res_norm", sx, y, sy)    h = half(relu(IN(y; sy) + relu(IN(x; sx))))       :50-55, with downsample.1

    IN(v; s) = (float(v) - mean) * rstd per plane with (mean, rstd) = stats_mean_rstd(s, H * W, eps) as the launch forms
    them itself; sx, sy: accumulators (N,Cin,R,4) int64 of x's and y's planes, y (N,Cin,H,W) half.  One rounding to half; the
    padding is zeros of h.  keep=True (with a prologue): kept = h as a new (N,Cin,H,W) half tensor.  emit=True: the sums of
    out's planes are added to out_stats (N,Cout,R,4), those of r's to r_stats; stats_out gives the accumulators to add to
    (a tensor, or with `down` a pair; zero them first with `new_stats`), otherwise new zeroed ones are made.  out and r are
    bit for bit enc_conv3x3's on h.  pre None without emit is enc_conv3x3 itself.

    Refusals, in this order, all before anything is launched: x not 4-D, stride not 1 or 2, pack not a pair, bias_h not 1-D,
    (Cin, Cout, stride) not a served shape (UnsupportedShape), the size of wpack, x not half, down with stride 1, down not a
    pair, the sizes of dpack and dbias_h, the form of pre, keep without pre, eps < 0, the shape then the dtype of sx, y, sy,
    stats_out without emit, the form of stats_out, the shape then the dtype of its tensors, H * W > 2^22
    (UnsupportedShape), then contiguity of every operand, the packs' dtype (half), grad and device, in the order x, wpack,
    bias_h, dpack, dbias_h, sx, y, sy, out_stats, r_stats; then N == 0 returns the empty result and H*W == 0 raises."""
    if x.dim() != 4:
        raise RuntimeError("x must be (N,Cin,H,W), got %s" % (tuple(x.shape),))
    if stride not in (1, 2):
        raise RuntimeError("stride must be 1 or 2, got %r" % (stride,))
    if not isinstance(pack, (tuple, list)) or len(pack) != 2:
        raise RuntimeError("pack must be (wpack, bias_h) of pack_enc3")
    wpack, bias_h = pack
    if bias_h.dim() != 1:
        raise RuntimeError("bias_h must be (Cout,), got %s" % (tuple(bias_h.shape),))
    N, cin, H, W = x.shape
    cout = bias_h.shape[0]
    if (cin, cout, stride) not in SHAPES:
        raise _lib.UnsupportedShape("enc_conv3x3_norm serves (Cin, Cout, stride) in %s, got (%d, %d, %d)" % (list(SHAPES), cin, cout, stride))
    if wpack.numel() != 9 * cin * cout:
        raise RuntimeError("wpack must hold %d halves (pack_enc3, %d -> %d), got %s" % (9 * cin * cout, cin, cout, tuple(wpack.shape)))
    check_dtype([(x, "x")], torch.float16)
    packs = [(wpack, "wpack"), (bias_h, "bias_h")]
    if down is not None:
        if stride != 2:
            raise RuntimeError("down (the 1x1 stride-2 branch) needs stride=2")
        if not isinstance(down, (tuple, list)) or len(down) != 2:
            raise RuntimeError("down must be (dpack, dbias_h) of pack_enc1")
        dpack, dbias_h = down
        if dpack.numel() != cin * cout:
            raise RuntimeError("dpack must hold %d halves (pack_enc1, %d -> %d), got %s" % (cin * cout, cin, cout, tuple(dpack.shape)))
        check_shape([(dbias_h, "dbias_h")], (cout,))
        packs += [(dpack, "dpack"), (dbias_h, "dbias_h")]
    mode, sx, y, sy = 0, None, None, None
    if pre is not None:
        if not isinstance(pre, (tuple, list)) or not pre or pre[0] not in _PRE or len(pre) != _PRE[pre[0]][1]:
            raise RuntimeError('pre must be None, ("norm", sx), ("res", sx, y) or ("res_norm", sx, y, sy)')
        mode = _PRE[pre[0]][0]
        sx, y, sy = (tuple(pre[1:]) + (None, None))[:3]
    elif keep:
        raise RuntimeError("keep=True needs a prologue (pre): without one the staged tensor is x")
    if not eps >= 0:
        raise ValueError("eps must be >= 0, got %r" % (eps,))
    R = stats_replicas()
    rest = []
    for t, name, shape, dt in ((sx, "sx", (N, cin, R, 4), torch.int64), (y, "y", (N, cin, H, W), torch.float16), (sy, "sy", (N, cin, R, 4), torch.int64)):
        if t is not None:
            check_shape([(t, name)], shape)
            check_dtype([(t, name)], dt)
            rest.append((t, name))
    so, sr = None, None
    if stats_out is not None:
        if not emit:
            raise RuntimeError("stats_out needs emit=True")
        if down is None:
            if not isinstance(stats_out, torch.Tensor):
                raise RuntimeError("stats_out must be one accumulator tensor (N,Cout,R,4) without down")
            so = stats_out
        else:
            if not isinstance(stats_out, (tuple, list)) or len(stats_out) != 2:
                raise RuntimeError("stats_out must be (out_stats, r_stats) with down")
            so, sr = stats_out
        for t, name in ((so, "out_stats"), (sr, "r_stats")):
            if t is not None:
                check_shape([(t, name)], (N, cout, R, 4))
                check_dtype([(t, name)], torch.int64)
                rest.append((t, name))
    if H * W > MAX_STATS_PLANE:
        raise _lib.UnsupportedShape("enc_conv3x3_norm serves planes of at most 2^22 pixels, got %d x %d" % (H, W))
    named = [(x, "x")] + packs + rest
    check_contiguous(named)
    check_dtype(packs, torch.float16)
    check_no_grad("enc_conv3x3_norm", named)
    check_device(named)
    if mode == 0 and not emit:
        got = enc_conv3x3(x, pack, stride=stride, down=down)
        return (got if down is None else got[0]), (None if down is None else got[1]), None, None, None
    Ho, Wo = out_size(H, W, stride)
    out = torch.empty((N, cout, Ho, Wo), dtype=torch.float16, device=x.device)
    r = torch.empty_like(out) if down is not None else None
    kept = torch.empty_like(x) if keep else None
    if emit and so is None:
        so = new_stats(N, cout, x.device)
        sr = new_stats(N, cout, x.device) if down is not None else None
    if N > 0:
        if H * W == 0:
            raise RuntimeError("enc_conv3x3_norm: empty frame (H*W = 0)")

        def p(t):
            return t.data_ptr() if t is not None else None
        args = _lib.EncConvNormArgs(x.data_ptr(), wpack.data_ptr(), bias_h.data_ptr(), out.data_ptr(), p(down[0]) if down is not None else None,
                                    p(down[1]) if down is not None else None, p(r), p(y), p(sx), p(sy), p(kept), p(so), p(sr), float(eps),
                                    N, H, W, cin, cout, stride, mode, EMIT if emit else 0)
        launch("lgu_encconv3x3_norm_h16", "enc_conv3x3_norm", x.device, args, _stream(x))
    return out, r, kept, so, sr


def shape_of(conv):
    """(Cin, Cout, stride) if `conv` is a Conv2d(Cin, Cout, 3, stride, padding=1) with a bias the kernel serves, else None."""
    for shape in SHAPES:
        if is_conv(conv, shape[0], shape[1], 3, stride=shape[2], pad=1, bias=True):
            return shape
    return None


def serves(conv, x):
    """A call of the eligible `conv` on the half NCHW tensor x is large enough for the fused path (MIN_FUSED_PIXELS, read
    at the call)."""
    shape = shape_of(conv)
    if shape is None or x.dim() != 4 or x.shape[1] != shape[0] or x.shape[2] * x.shape[3] == 0:
        return False
    Ho, Wo = out_size(x.shape[2], x.shape[3], shape[2])
    return x.shape[0] * Ho * Wo >= MIN_FUSED_PIXELS[shape]


def pack_stem(weight, bias):
    """(wpack (7,2,64,8) half, bias_h (32) half) of the stem's Conv2d(3, 32, 7) weight (32,3,7,7) and bias (32), on the
    weight's device.  A K step of v_mfma_f32_16x16x32_f16 is one window row ky of 8 x-slots x 4 channels:
    wpack[ky, ct, l, j] = half(weight)[16 ct + (l & 15), j & 3, ky, 2 (l >> 4) + (j >> 2)] where the channel j & 3 < 3 and
    the x-slot 2 (l >> 4) + (j >> 2) < 7, and 0 in every other slot (the 4th channel and the 8th x-slot pad the K step)."""
    if weight.dim() != 4 or tuple(weight.shape) != (32, 3, 7, 7):
        raise RuntimeError("pack_stem: weight must be (32,3,7,7), got %s" % (tuple(weight.shape),))
    check_shape([(bias, "bias")], (32,))
    with torch.no_grad():
        wp = torch.zeros((32, 4, 7, 8), dtype=torch.float16, device=weight.device)
        wp[:, :3, :, :7] = weight.detach().to(torch.float16)
        # [ct][cl][ch][ky][g][s] -> [ky][ct][g][cl][s][ch]: lane l = 16 g + cl, element j = 4 s + ch, x-slot 2 g + s
        wpack = wp.reshape(2, 16, 4, 7, 4, 2).permute(3, 0, 4, 1, 5, 2).reshape(7, 2, 64, 8)
        bias_h = bias.detach().to(device=wp.device, dtype=torch.float16).contiguous()
    return wpack.contiguous(), bias_h


def pack_out1(weight, bias):
    """(wpack (4,Cout/16,64,8) half, bias_h (Cout) half) of the output layer's Conv2d(128, Cout, 1) weight (Cout,128,1,1)
    and bias (Cout), Cout 128 or 256, on the weight's device.
    wpack[kc, ct, l, j] = half(weight)[16 ct + (l & 15), 32 kc + 8 (l >> 4) + j, 0, 0]: block kc of 32 input channels,
    channel tile ct of 16 output channels, lane l, element j.  Every slot holds a weight."""
    if weight.dim() != 4 or weight.shape[0] not in OUT_COUTS or tuple(weight.shape[1:]) != (OUT_CIN, 1, 1):
        raise RuntimeError("pack_out1: weight must be (Cout,128,1,1) with Cout in %s, got %s" % (list(OUT_COUTS), tuple(weight.shape)))
    cout = weight.shape[0]
    check_shape([(bias, "bias")], (cout,))
    with torch.no_grad():
        wh = weight.detach().to(torch.float16)
        # [ct][cl][kc][g][j] -> [kc][ct][g][cl][j]
        wpack = wh.reshape(cout // 16, 16, 4, 4, 8).permute(2, 0, 3, 1, 4).reshape(4, cout // 16, 64, 8)
        bias_h = bias.detach().to(device=wh.device, dtype=torch.float16).contiguous()
    return wpack.contiguous(), bias_h


def enc_stem7x7(x, pack, relu=False):
    """The stem Conv2d(3, 32, 7, stride=2, padding=3) of x (N,3,H,W), float32 or half, with `pack` = (wpack, bias_h) of
    `pack_stem`, as a new (N,32,Ho,Wo) half tensor, (Ho, Wo) = out_size(H, W, 2):

        y0 = half(b_h + sum half(x) * w_h)    exact products, fp32 accumulation from the bias, window rows ascending, one
                                              rounding; padding, the row or column past an odd size included, is exact zeros
        y  = y0 | relu(y0)                    relu=False (what an instance norm reads) | relu=True.  NaN is kept.

    A half x gives the bits of the float32 x it is the rounding of.  Refusals, in this order, all before anything is
    launched: x not 4-D, pack not a pair, bias_h not 1-D, (Cin, Cout) not (3, 32) (UnsupportedShape), the size of wpack, then
    contiguity, dtypes (x float32 or half, the pack half), grad and device of x, wpack, bias_h in that order
    (_host.check_layer_operands); then N == 0 returns the empty result and H*W == 0 raises.  x and bias_h are served at
    element alignment; a pack that is not 16-byte aligned (never the case for what pack_stem returns) raises
    UnsupportedShape."""
    if x.dim() != 4:
        raise RuntimeError("x must be (N,3,H,W), got %s" % (tuple(x.shape),))
    if not isinstance(pack, (tuple, list)) or len(pack) != 2:
        raise RuntimeError("pack must be (wpack, bias_h) of pack_stem")
    wpack, bias_h = pack
    if bias_h.dim() != 1:
        raise RuntimeError("bias_h must be (Cout,), got %s" % (tuple(bias_h.shape),))
    N, cin, H, W = x.shape
    cout = bias_h.shape[0]
    if (cin, cout) != STEM:
        raise _lib.UnsupportedShape("enc_stem7x7 serves (Cin, Cout) = (3, 32), got (%d, %d)" % (cin, cout))
    if wpack.numel() != 7 * 2 * 64 * 8:
        raise RuntimeError("wpack must hold %d halves (pack_stem), got %s" % (7 * 2 * 64 * 8, tuple(wpack.shape)))
    check_layer_operands("enc_stem7x7", [(x, "x"), (wpack, "wpack"), (bias_h, "bias_h")])
    Ho, Wo = out_size(H, W, 2)
    out = torch.empty((N, cout, Ho, Wo), dtype=torch.float16, device=x.device)
    if N > 0:
        if H * W == 0:
            raise RuntimeError("enc_stem7x7: empty frame (H*W = 0)")
        flags = (X_HALF if x.dtype == torch.float16 else 0) | (STEM_RELU if relu else 0)
        args = _lib.EncStemArgs(x.data_ptr(), wpack.data_ptr(), bias_h.data_ptr(), out.data_ptr(), N, H, W, cin, cout, flags)
        launch("lgu_encstem7x7_h16", "enc_stem7x7", x.device, args, _stream(x))
    return out


def enc_out1x1(x, pack, split=False):
    """The output layer Conv2d(128, Cout, 1) of half x (N,128,H,W) with `pack` = (wpack, bias_h) of `pack_out1` (the bias
    gives Cout, 128 or 256):

        h = half(b_h + sum_c x[c] * w_h[co, c])    exact products, fp32 accumulation from zero in four blocks of 32 channels,
                                                   one addition of the bias, one rounding.  NaN is kept.

    split=False returns h as a new (N,Cout,H,W) half tensor.  split=True (Cout 256) returns (net, inp), two new (N,128,H,W)
    half tensors: net = half(tanh(float(h[:, :128]))) (tanh(+-inf) = +-1), inp = relu(h[:, 128:]).

    Refusals, in this order, all before anything is launched: x not 4-D, pack not a pair, bias_h not 1-D, Cin not 128 or
    Cout not 128 or 256 (UnsupportedShape), split with Cout 128, the size of wpack, x not half, then contiguity, dtypes
    (half), grad and device of x, wpack, bias_h in that order (_host.check_layer_operands); then N == 0 returns the empty
    result and H*W == 0 raises.  x and bias_h are served at element alignment; a pack that is not 16-byte aligned raises
    UnsupportedShape."""
    if x.dim() != 4:
        raise RuntimeError("x must be (N,128,H,W), got %s" % (tuple(x.shape),))
    if not isinstance(pack, (tuple, list)) or len(pack) != 2:
        raise RuntimeError("pack must be (wpack, bias_h) of pack_out1")
    wpack, bias_h = pack
    if bias_h.dim() != 1:
        raise RuntimeError("bias_h must be (Cout,), got %s" % (tuple(bias_h.shape),))
    N, cin, H, W = x.shape
    cout = bias_h.shape[0]
    if cin != OUT_CIN or cout not in OUT_COUTS:
        raise _lib.UnsupportedShape("enc_out1x1 serves Cin = 128 and Cout in %s, got (%d, %d)" % (list(OUT_COUTS), cin, cout))
    if split and cout != 256:
        raise RuntimeError("split=True (net, inp of 128 planes each) needs Cout = 256, got %d" % cout)
    if wpack.numel() != cin * cout:
        raise RuntimeError("wpack must hold %d halves (pack_out1, 128 -> %d), got %s" % (cin * cout, cout, tuple(wpack.shape)))
    check_dtype([(x, "x")], torch.float16)
    check_layer_operands("enc_out1x1", [(x, "x"), (wpack, "wpack"), (bias_h, "bias_h")])
    out = torch.empty((N, 128 if split else cout, H, W), dtype=torch.float16, device=x.device)
    inp = torch.empty_like(out) if split else None
    if N > 0:
        if H * W == 0:
            raise RuntimeError("enc_out1x1: empty frame (H*W = 0)")
        args = _lib.EncOutArgs(x.data_ptr(), wpack.data_ptr(), bias_h.data_ptr(), out.data_ptr(), inp.data_ptr() if split else None,
                               N, H, W, cin, cout, SPLIT if split else 0)
        launch("lgu_encout1x1_c128_h16", "enc_out1x1", x.device, args, _stream(x))
    return (out, inp) if split else out


def serves_stem(conv, x):
    """A call of `conv` on the NCHW tensor x takes the fused stem: conv is Conv2d(3, 32, 7, stride=2, padding=3) with a bias
    and the call has at least MIN_STEM_PIXELS output pixels (read at the call)."""
    if not is_conv(conv, STEM[0], STEM[1], 7, stride=2, pad=3, bias=True):
        return False
    if x.dim() != 4 or x.shape[1] != STEM[0] or x.shape[2] * x.shape[3] == 0:
        return False
    Ho, Wo = out_size(x.shape[2], x.shape[3], 2)
    return x.shape[0] * Ho * Wo >= MIN_STEM_PIXELS


def serves_out(conv, x):
    """A call of `conv` on the half NCHW tensor x takes the fused output layer: conv is Conv2d(128, Cout, 1) with a bias,
    Cout 128 or 256, and the call has at least MIN_OUT_PIXELS[Cout] pixels (read at the call)."""
    cout = getattr(conv, "out_channels", None)
    if cout not in OUT_COUTS or not is_conv(conv, OUT_CIN, cout, 1, bias=True):
        return False
    if x.dim() != 4 or x.shape[1] != OUT_CIN or x.shape[2] * x.shape[3] == 0:
        return False
    return x.shape[0] * x.shape[2] * x.shape[3] >= MIN_OUT_PIXELS[cout]
