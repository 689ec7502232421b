"""LGU-SLAM's feature encoder (reference droid_slam/modules/extractor.py: BasicEncoder(output_dim=128,
norm_fn='instance'), run on every incoming frame by MotionFilter.track and PoseTrajectoryFiller) on the HIP kernels of
csrc/instnorm.hip.

By default the 13 convolutions stay the module's own calls (MIOpen); with `convs=True` the twelve 3x3 convolutions of
layer1..3 go through csrc/encconv.hip under float16 autocast (`encconv.enc_conv3x3`, identity epilogue, the 1x1 downsample
branch of a strided block from its first launch), opt-in because the library's summation order differs and
`features.install(m)` keeps its bits; with `ends=True` the stem and the output 1x1 go through csrc/encends.hip
(`encconv.enc_stem7x7`, `encconv.enc_out1x1`), opt-in for the same reason and independent of `convs`; with `norms=True` (and
`convs`) 11 of the 13 instance-norm launches fold into the twelve convolutions (`encconv.enc_conv3x3_norm`: exact integer
statistics from the producer's write-out, the normalisation in the consumer's staging loop), 17 launches per forward with
`ends`, opt-in because its bits are not `instance_norm_relu`'s.  Everything around them, 15 InstanceNorm2d sites, 13 ReLUs and
6 residual add + ReLU pairs, becomes one call per site group, 13 per forward: each convolution output is read once, the
statistics are taken in fp32 from the stored values, and the block output is rounded to the tensor type once.  A call
is one launch while H*W <= resident_limit(dtype): every site of a 384x512 frame under float16 autocast (13 launches).
In fp32 the five 192x256 sites of such a frame exceed the limit (24576 floats) and take a statistics launch, an apply
launch and a stream-ordered allocation each: 18 launches per forward; those calls capture in a torch.cuda.graph only if
the runtime captures hipMallocAsync / hipFreeAsync, the single-launch calls always do.

    features.install(net.fnet)                        # net.fnet(images) now reaches the fused path, state_dict unchanged
    images = features.normalize_images(frames_u8)     # (N,3,H,W) uint8 BGR -> (1,N,3,H,W) float32, MotionFilter.track's
    fmaps = net.fnet(images)

`instance_norm_relu` and `normalize_images`: contiguous HIP device tensors only (no CPU fallback; normalize_images uploads
a CPU uint8 image as uint8), every argument error raised before anything is launched, no host synchronisation, forward
only: inputs that require grad are refused while grad mode is on.
"""
import ctypes

import torch

from . import _lib, encconv
from ._host import (FLOAT_OR_HALF, PackCache, bind, check_contiguous, check_device, check_dtype, check_no_grad, check_shape, dtype_name,
                    fused_dtype, is_conv, launch, typed, unbind)
from ._host import ptr as _ptr, stream as _stream

IMAGENET_MEAN = (0.485, 0.456, 0.406)     # motion_filter.py:30-31, RGB
IMAGENET_STD = (0.229, 0.224, 0.225)
LAYERS = ("layer1", "layer2", "layer3")


def resident_limit(dtype):
    """Largest H*W the single-launch kernel serves for tensors of `dtype`."""
    return int(_lib.load().lgu_instnorm_resident_limit(torch.empty((), dtype=dtype).element_size()))


def instance_norm_relu(a, residual=None, *, norm_residual=False, relu=True, eps=1e-5, out=None):
    """The element-wise tail of one convolution of the encoder, fused (IN = InstanceNorm2d without affine terms or
    running statistics, biased variance):

        residual None, relu        relu(IN(a))                      extractor.py:49-50, :188-189
        residual, not normalised   relu(residual + relu(IN(a)))     :50, :55 without a downsample branch
        residual, norm_residual    relu(IN(residual) + relu(IN(a))) :50-55 with the 1x1 downsample branch and its norm
        residual None, relu=False  IN(a)

    a, residual, out: (N,C,H,W) float32 or float16, contiguous, same shape and dtype.  out=None allocates; out may be a
    or residual themselves (in place), any other overlap is the caller's error.  Statistics and arithmetic are fp32, a
    half result is rounded once."""
    if a.dim() != 4:
        raise RuntimeError("a must be (N,C,H,W), got %s" % (tuple(a.shape),))
    check_dtype([(a, "a")], FLOAT_OR_HALF)
    if residual is None:
        if norm_residual:
            raise ValueError("norm_residual=True needs a residual")
        mode = 0 if relu else 3
    else:
        if not relu:
            raise ValueError("relu=False is served without a residual only")
        mode = 2 if norm_residual else 1
    named = [(a, "a")] + ([(residual, "residual")] if residual is not None else []) + ([(out, "out")] if out is not None else [])
    for pair in named[1:]:
        check_shape([pair], a.shape)
        check_dtype([pair], a.dtype)
    N, C, H, W = a.shape
    hw = H * W
    if hw == 1:
        raise ValueError("Expected more than 1 spatial element when training, got input size %s" % (a.size(),))
    if not eps >= 0:
        raise ValueError("eps must be >= 0, got %r" % (eps,))
    check_contiguous(named)
    check_no_grad("instance_norm_relu", named)
    check_device(named)
    if out is None:
        out = torch.empty_like(a)
    if N * C == 0:
        return out
    if hw == 0:
        raise RuntimeError("instance_norm_relu: empty planes (H*W = 0), the statistics are undefined")
    return _instnorm(a, residual, out, mode, float(eps))


def _instnorm(a, b, out, mode, eps):
    """The call itself, for arguments already checked (instance_norm_relu, FeatureEncoder._fused)."""
    launch(typed("lgu_instnorm_relu", a.dtype), "instance_norm_relu", a.device, a.data_ptr(),
           b.data_ptr() if b is not None else None, out.data_ptr(), a.shape[0] * a.shape[1], a.shape[2] * a.shape[3], eps, mode,
           torch.cuda.current_stream(a.device).cuda_stream)
    return out


def normalize_images(image, mean=IMAGENET_MEAN, std=IMAGENET_STD):
    """(1,N,3,H,W) float32 RGB from (N,3,H,W) uint8 BGR: channel c = (image[:, 2-c] / 255 - mean[c]) / std[c], the bits
    of motion_filter.py:56-57 (`image[None, :, [2,1,0]].to(device) / 255.0`, `sub_(MEAN)`, `div_(STDV)`) on the device
    (where `/ 255.0` is a product with float(1 / 255), include/lgu_corr.h) in one launch.
    A CPU image is uploaded as uint8 to the current HIP device; mean, std: 3 numbers each, used as
    float32."""
    if image.dim() != 4 or image.shape[1] != 3:
        raise RuntimeError("image must be (N,3,H,W), got %s" % (tuple(image.shape),))
    if image.dtype != torch.uint8:
        raise RuntimeError("expected scalar type Byte but found %s (image)" % dtype_name(image.dtype))
    if len(mean) != 3 or len(std) != 3:
        raise RuntimeError("mean and std must have 3 entries")
    if not image.is_cuda:
        image = image.contiguous().to(torch.device("cuda"))
    check_contiguous([(image, "image")])
    N, _, H, W = image.shape
    out = torch.empty((1, N, 3, H, W), dtype=torch.float32, device=image.device)
    if N * H * W == 0:
        return out
    m = (ctypes.c_float * 3)(*[float(v) for v in mean])
    s = (ctypes.c_float * 3)(*[float(v) for v in std])
    launch("lgu_image_normalize_u8", "normalize_images", image.device, _ptr(image), _ptr(out), N, H * W, m, s, _stream(image))
    return out


def _check_norm(m, channels, name):
    if (not isinstance(m, torch.nn.InstanceNorm2d) or m.affine or m.track_running_stats
            or getattr(m, "weight", None) is not None or getattr(m, "bias", None) is not None
            or m.num_features != channels):
        raise RuntimeError("FeatureEncoder: %s must be InstanceNorm2d(%d) with affine=False and track_running_stats=False"
                           % (name, channels))


def _check_conv(m, cin, cout, k, stride, pad, name):
    if not is_conv(m, cin, cout, k, stride, pad):
        raise RuntimeError("FeatureEncoder: %s must be Conv2d(%d, %d, %d, stride=%d, padding=%d)"
                           % (name, cin, cout, k, stride, pad))


class _Like:
    """The shape of a tensor that does not exist yet, for encconv.serves."""
    __slots__ = ("shape",)

    def __init__(self, shape):
        self.shape = tuple(shape)

    def dim(self):
        return len(self.shape)


class FeatureEncoder:
    """Callable stand-in for the forward of the reference's `BasicEncoder(output_dim, norm_fn='instance')`:

        fused = FeatureEncoder(net.fnet)
        fmaps = fused(images)             # = net.fnet(images), images (B,N,3,H,W)

    Fused path (the module's own Conv2d calls + one csrc/instnorm.hip call per site, 13 per forward) for HIP tensors
    when either autocast is off and the images are float32, or CUDA autocast is on with float16 (the half kernels); the
    parameters must be float32 and contiguous NCHW, and nothing may require grad while grad mode is on.  Everything
    else goes to the module's own forward unchanged: CPU tensors, a bfloat16 autocast, channels-last, training with
    gradients, a dropout in training mode.

    convs=True: under float16 autocast the twelve residual-stage convolutions are `encconv.enc_conv3x3` launches (identity
    epilogue; a strided block's 1x1 downsample branch comes from its first launch) where the call has at least
    encconv.MIN_FUSED_PIXELS of its shape and the layer has one of the kernel's shapes; the instance-norm calls are the
    same.  The fp32 path does not change.  The default, False, keeps every convolution the module's own.

    ends=True: under float16 autocast the stem is `encconv.enc_stem7x7` with the identity epilogue (norm1's call reads it)
    where conv1 is Conv2d(3, 32, 7, stride=2, padding=3) with a bias and the call has at least encconv.MIN_STEM_PIXELS output
    pixels, and the output layer `encconv.enc_out1x1` where conv2 has a bias and gives 128 or 256 planes and the call has at
    least encconv.MIN_OUT_PIXELS of them (csrc/encends.hip); the instance-norm calls are the same.  Independent of `convs`;
    the fp32 path does not change.  The default, False, keeps both the module's own.

    norms=True (with convs=True): under float16 autocast, where all twelve residual-stage convolutions are served, every
    plane has at most 2^22 pixels and the call has at least encconv.MIN_NORMS_PIXELS image pixels (N * H * W), the instance
    norms between the convolutions are folded into them (`encconv.enc_conv3x3_norm`): stem, norm1's call, one fill of the
    accumulators of the whole forward, twelve convolutions (each but the last adds the exact sums of its outputs; each but
    the first normalises, adds the residual and applies the ReLUs while it stages its input; the first convolution of a
    block whose input is a residual later writes it out), the last block's norm call, the output layer: 17 launches with
    `ends`, counted in `folded_calls`.  The statistics are exact and the normalised value is rounded to half once, so the
    bits are not those of the per-site route.  Every other call runs the per-site route unchanged.  The default, False,
    keeps the 13 instance-norm calls.  As measured the folded forward is the slower one at 1 and
    16 frames of 384x512, so encconv.MIN_NORMS_PIXELS is 1 << 62 and the flag changes nothing until that is lowered.

    Construction refuses (RuntimeError naming the attribute) anything but conv1 / norm1 / layer1..3 of two residual
    blocks each / conv2 with InstanceNorm2d(affine=False, track_running_stats=False) at every norm site."""

    def __init__(self, module, convs=False, ends=False, norms=False):
        conv1 = getattr(module, "conv1", None)
        if not isinstance(conv1, torch.nn.Conv2d):
            raise RuntimeError("FeatureEncoder: conv1 must be a Conv2d")
        dim = conv1.out_channels
        _check_conv(conv1, conv1.in_channels, dim, 7, 2, 3, "conv1")
        _check_norm(getattr(module, "norm1", None), dim, "norm1")
        cin = dim
        self.blocks = []
        for name in LAYERS:
            layer = getattr(module, name, None)
            if not isinstance(layer, torch.nn.Sequential) or len(layer) != 2:
                raise RuntimeError("FeatureEncoder: %s must be a Sequential of two residual blocks" % name)
            for i, blk in enumerate(layer):
                where = "%s.%d." % (name, i)
                c1 = getattr(blk, "conv1", None)
                if not isinstance(c1, torch.nn.Conv2d):
                    raise RuntimeError("FeatureEncoder: %sconv1 must be a Conv2d" % where)
                cout, stride = c1.out_channels, c1.stride[0]
                _check_conv(c1, cin, cout, 3, stride, 1, where + "conv1")
                _check_conv(getattr(blk, "conv2", None), cout, cout, 3, 1, 1, where + "conv2")
                _check_norm(getattr(blk, "norm1", None), cout, where + "norm1")
                _check_norm(getattr(blk, "norm2", None), cout, where + "norm2")
                down = getattr(blk, "downsample", None)
                if down is None:
                    if stride != 1 or cin != cout:
                        raise RuntimeError("FeatureEncoder: %sdownsample is missing (stride %d, %d -> %d channels)"
                                           % (where, stride, cin, cout))
                else:
                    if not isinstance(down, torch.nn.Sequential) or len(down) != 2:
                        raise RuntimeError("FeatureEncoder: %sdownsample must be Sequential(Conv2d 1x1, InstanceNorm2d)" % where)
                    _check_conv(down[0], cin, cout, 1, stride, 0, where + "downsample.0")
                    _check_norm(down[1], cout, where + "downsample.1")
                    if down[1].eps != blk.norm2.eps:
                        raise RuntimeError("FeatureEncoder: %sdownsample.1 must have norm2's eps" % where)
                self.blocks.append(blk)
                cin = cout
        conv2 = getattr(module, "conv2", None)
        if not isinstance(conv2, torch.nn.Conv2d):
            raise RuntimeError("FeatureEncoder: conv2 must be a Conv2d")
        _check_conv(conv2, cin, conv2.out_channels, 1, 1, 0, "conv2")
        self.module = module
        self.convs = bool(convs)
        self.ends = bool(ends)
        self.norms = bool(norms)
        self._packs = PackCache()
        self.fused_calls = 0
        self.folded_calls = 0        # calls made by folded forwards, 17 each: one launch each with `ends`

    def _convs(self):
        m = self.module
        convs = [m.conv1, m.conv2]
        for blk in self.blocks:
            convs += [blk.conv1, blk.conv2] + ([blk.downsample[0]] if blk.downsample is not None else [])
        return convs

    def _mode(self, x):
        """torch.float16 / torch.float32 for the fused path, None for the module's forward."""
        m = self.module
        if not isinstance(x, torch.Tensor) or not x.is_cuda or x.dim() != 5 or not x.is_contiguous():
            return None
        if m.training and getattr(m, "dropout", None) is not None:
            return None
        params = [p for c in self._convs() for p in (c.weight, c.bias) if p is not None]
        if any(p.dtype != torch.float32 or p.device != x.device or not p.is_contiguous() for p in params):
            return None
        dt = fused_dtype([x] + params)
        if dt == torch.float16:                  # autocast casts float32 images on the way into conv1
            return dt if x.dtype in FLOAT_OR_HALF else None
        return dt if x.dtype == dt else None

    def _fused(self, x, dt):
        """The fused forward, or None if a convolution returned something the kernels do not take (then nothing of the
        caller's has been written)."""
        m = self.module
        b, n, c1, h1, w1 = x.shape

        def ok(t):      # what instance_norm_relu would check; the shapes follow from the architecture
            return t.dtype == dt and t.is_contiguous() and t.shape[2] * t.shape[3] > 1 and not t.requires_grad

        x4 = x.view(b * n, c1, h1, w1)
        ends = self.ends and dt == torch.float16      # the stem and the output layer on csrc/encends.hip
        if ends and encconv.serves_stem(m.conv1, x4):
            y = encconv.enc_stem7x7(x4, self._packs.of(m.conv1, encconv.pack_stem))
        else:
            y = m.conv1(x4)
        if not ok(y):
            return None
        y = _instnorm(y, None, y, 0, m.norm1.eps)
        own = self.convs and dt == torch.float16      # the residual stages on csrc/encconv.hip
        if own and self.norms and self._folds(x4, y):
            out = self._output(self._folded(y), ends, b, n)
            self.folded_calls += 17                   # stem, norm1, the fill, twelve convolutions, the last norm, the output layer
            return out
        for blk in self.blocks:
            r = None
            if own and encconv.serves(blk.conv1, y):
                p1 = self._packs.of(blk.conv1, encconv.pack_enc3)
                if blk.downsample is None:
                    t = encconv.enc_conv3x3(y, p1)
                else:
                    t, r = encconv.enc_conv3x3(y, p1, stride=2, down=self._packs.of(blk.downsample[0], encconv.pack_enc1))
            else:
                t = blk.conv1(y)
            if not ok(t):
                return None
            t = _instnorm(t, None, t, 0, blk.norm1.eps)
            if own and encconv.serves(blk.conv2, t):
                t = encconv.enc_conv3x3(t, self._packs.of(blk.conv2, encconv.pack_enc3))
            else:
                t = blk.conv2(t)
            if not ok(t):
                return None
            if blk.downsample is None:
                y = _instnorm(t, y, t, 1, blk.norm2.eps)
            else:
                if r is None:
                    r = blk.downsample[0](y)
                if not ok(r):
                    return None
                y = _instnorm(t, r, t, 2, blk.norm2.eps)
        return self._output(y, ends, b, n)

    def _output(self, y, ends, b, n):
        m = self.module
        if ends and encconv.serves_out(m.conv2, y):
            y = encconv.enc_out1x1(y, self._packs.of(m.conv2, encconv.pack_out1))
        else:
            y = m.conv2(y)
        return y.view(b, n, y.shape[1], y.shape[2], y.shape[3])

    def _folds(self, x4, y):
        """The folded route serves this call: y (N,32,H,W) is norm1's output for the images x4."""
        if x4.shape[0] * x4.shape[2] * x4.shape[3] < encconv.MIN_NORMS_PIXELS or y.shape[2] * y.shape[3] > encconv.MAX_STATS_PLANE:
            return False
        like = _Like(y.shape)
        for i, blk in enumerate(self.blocks):
            shape = encconv.shape_of(blk.conv1)
            if shape is None or (blk.downsample is not None) != (shape[2] == 2) or not encconv.serves(blk.conv1, like):
                return False
            if blk.downsample is not None and (i % 2 == 1 or blk.downsample[0].bias is None):
                return False
            like = _Like((like.shape[0], shape[1]) + encconv.out_size(like.shape[2], like.shape[3], shape[2]))
            if not encconv.serves(blk.conv2, like):
                return False
        return like.shape[2] * like.shape[3] > 1      # what the last block's norm call needs

    def _folded(self, y):
        """layer1..3 with the instance norms inside the convolutions, from norm1's output to layer3's: 15 launches."""
        N, R = y.shape[0], encconv.stats_replicas()
        packs = self._packs
        flat = encconv.new_stats(N, self._stat_planes(), y.device).view(-1)
        taken = [0]

        def site(c):                                  # the accumulators of one convolution's output planes
            k = N * c * R * 4
            taken[0] += k
            return flat[taken[0] - k:taken[0]].view(N, c, R, 4)

        x, pre, resid, eps = y, None, y, 0.0          # resid: the block's input where it exists as a tensor
        for i, blk in enumerate(self.blocks):
            last = i == len(self.blocks) - 1
            cout = blk.conv1.out_channels
            s1 = site(cout)
            if blk.downsample is None:
                t, _, kept, _, _ = encconv.enc_conv3x3_norm(x, packs.of(blk.conv1, encconv.pack_enc3), pre=pre, keep=pre is not None,
                                                            emit=True, eps=eps, stats_out=s1)
                resid = kept if pre is not None else resid
            else:
                sr = site(cout)
                t, r, _, _, _ = encconv.enc_conv3x3_norm(x, packs.of(blk.conv1, encconv.pack_enc3), stride=2,
                                                         down=packs.of(blk.downsample[0], encconv.pack_enc1), pre=pre, emit=True,
                                                         eps=eps, stats_out=(s1, sr))
            s2 = None if last else site(cout)
            t = encconv.enc_conv3x3_norm(t, packs.of(blk.conv2, encconv.pack_enc3), pre=("norm", s1), emit=not last, eps=blk.norm1.eps,
                                         stats_out=s2)[0]
            if last:
                return _instnorm(t, resid, t, 1, blk.norm2.eps)
            pre = ("res", s2, resid) if blk.downsample is None else ("res_norm", s2, r, sr)
            x, eps = t, blk.norm2.eps

    def _stat_planes(self):
        """Planes per image that a folded forward takes statistics of: every convolution output but the last, and the
        two branches."""
        total = sum(2 * blk.conv1.out_channels + (blk.conv1.out_channels if blk.downsample is not None else 0) for blk in self.blocks)
        return total - self.blocks[-1].conv1.out_channels

    def __call__(self, x):
        m = self.module
        dt = self._mode(x)
        out = None
        if dt is not None and x.shape[0] * x.shape[1] > 0:
            out = self._fused(x, dt)
        if out is None:
            return type(m).forward(m, x)
        self.fused_calls += 1
        return out


def install(module, convs=False, ends=False, norms=False):
    """Bind a FeatureEncoder as `module.forward` (an instance attribute: parameters, buffers and state_dict keys are
    unchanged), so every caller of the encoder reaches the fused path.  `convs`, `ends` and `norms` as in FeatureEncoder.
    Returns the wrapper; a second call returns the one already installed (with the flags it was made with)."""
    return bind(module, "forward", FeatureEncoder, lambda _: FeatureEncoder(module, convs=convs, ends=ends, norms=norms))


def uninstall(module):
    """Undo `install`: the class's forward is used again."""
    unbind(module, "forward", FeatureEncoder)
