"""LGU-SLAM's context encoder (reference droid_slam/droid_net.py: `cnet = BasicEncoder(output_dim=256, norm_fn='none')`,
droid_slam/modules/extractor.py) on the HIP kernels of csrc/encconv.hip.

Without norms every tail of a residual-stage convolution is pointwise: bias, ReLU, residual add, ReLU.  Under float16
autocast the module pays separate launches for each of them around each library convolution; here the twelve 3x3
convolutions of layer1..3 are one `encconv.enc_conv3x3` launch each with the tail as its epilogue, and the two strided
blocks get their 1x1 downsample branch from their first launch.  By default the stem (7x7, stride 2) and the output 1x1
stay the module's own calls; with `ends=True` they are csrc/encends.hip's (`encconv.enc_stem7x7` with the ReLU,
`encconv.enc_out1x1`): 14 launches per forward and no library convolution, opt-in because the bits are not the library's.
`net_inp` gives the pair MotionFilter.track makes of the output, `tanh` of the first 128 planes and `relu` of the others,
with `ends=True` from the output layer's own launch.

    context.install(net.cnet)                 # net.cnet(images) now reaches the fused path, state_dict unchanged
    wr = context.install(net.cnet, ends=True) # the stem and the output layer too
    net_, inp = wr.net_inp(images)            # = cnet(images).split([128,128], dim=2), .tanh(), .relu()

The instance-norm feature encoder is `features.install`'s.
"""
import torch

from . import encconv
from ._host import FLOAT_OR_HALF, PackCache, bind, fused_dtype, is_conv, unbind

LAYERS = ("layer1", "layer2", "layer3")


def _empty(m):
    return isinstance(m, torch.nn.Sequential) and len(m) == 0


def _check_empty(m, name):
    if isinstance(m, torch.nn.InstanceNorm2d):
        raise RuntimeError("ContextEncoder: %s is an InstanceNorm2d: this is the feature encoder's architecture, use "
                           "features.install" % name)
    if not _empty(m):
        raise RuntimeError("ContextEncoder: %s must be an empty nn.Sequential() (norm_fn='none')" % name)


def _check_conv(m, cin, cout, k, stride, pad, name):
    if not is_conv(m, cin, cout, k, stride, pad, bias=True):
        raise RuntimeError("ContextEncoder: %s must be Conv2d(%d, %d, %d, stride=%d, padding=%d) with a bias"
                           % (name, cin, cout, k, stride, pad))


class ContextEncoder:
    """Callable stand-in for the forward of the reference's `BasicEncoder(output_dim, norm_fn='none')`:

        fused = ContextEncoder(net.cnet)
        ctx = fused(images)               # = net.cnet(images), images (B,N,3,H,W)

    Fused path (the module's conv1 and its ReLU, twelve csrc/encconv.hip launches, the module's conv2) under CUDA autocast
    with float16 for a contiguous 5-D HIP tensor, float32 or half, when the parameters are float32 on its device, nothing
    requires grad while grad mode is on and no dropout is active.  Everything else goes to the module's own forward
    unchanged: fp32, a bfloat16 autocast, CPU tensors, channels-last, gradients, a dropout in training mode.  Inside the
    fused path a convolution whose call is below encconv.MIN_FUSED_PIXELS of its shape is the module's convolution with
    its tail in torch.

    ends=True: the stem is `encconv.enc_stem7x7(relu=True)` where conv1 takes 3 channels and the call has at least
    encconv.MIN_STEM_PIXELS output pixels, and the output layer `encconv.enc_out1x1` where conv2 gives 128 or 256 planes and
    the call has at least encconv.MIN_OUT_PIXELS of them: 14 launches and no Conv2d of the module.  The default, False, keeps
    both the module's own calls.

    `net_inp(images)` returns (tanh(ctx[:, :, :128]), relu(ctx[:, :, 128:])) of ctx = the encoder's output as two contiguous
    (B,N,128,h,w) tensors (output_dim 256 only): with ends=True on the fused route the output layer's launch writes both,
    on every other route it is this forward followed by torch's split, tanh and relu.

    The packed weights are cached under each layer's weight and bias (data pointer, version, device):
    load_state_dict after install takes effect.  `fused_calls` counts the fused forwards.

    Construction refuses (RuntimeError naming the attribute) anything but conv1 (7x7, stride 2, to 32 channels) / an empty
    norm1 / layer1..3 of two residual blocks each with the channel counts and strides 32, 64 / 2, 128 / 2 and an empty
    nn.Sequential() at every norm site / the 1x1 conv2; an instance-norm encoder is pointed to features.install."""

    def __init__(self, module, ends=False):
        conv1 = getattr(module, "conv1", None)
        if not isinstance(conv1, torch.nn.Conv2d):
            raise RuntimeError("ContextEncoder: conv1 must be a Conv2d")
        _check_conv(conv1, conv1.in_channels, 32, 7, 2, 3, "conv1")
        _check_empty(getattr(module, "norm1", None), "norm1")
        cin = 32
        self.blocks = []
        for name, cout, stride in zip(LAYERS, (32, 64, 128), (1, 2, 2)):
            layer = getattr(module, name, None)
            if not isinstance(layer, torch.nn.Sequential) or len(layer) != 2:
                raise RuntimeError("ContextEncoder: %s must be a Sequential of two residual blocks" % name)
            for i, blk in enumerate(layer):
                where = "%s.%d." % (name, i)
                s = stride if i == 0 else 1
                _check_conv(getattr(blk, "conv1", None), cin, cout, 3, s, 1, where + "conv1")
                _check_conv(getattr(blk, "conv2", None), cout, cout, 3, 1, 1, where + "conv2")
                _check_empty(getattr(blk, "norm1", None), where + "norm1")
                _check_empty(getattr(blk, "norm2", None), where + "norm2")
                down = getattr(blk, "downsample", None)
                if s == 1:
                    if down is not None:
                        raise RuntimeError("ContextEncoder: %sdownsample must be None (stride 1)" % where)
                else:
                    if not isinstance(down, torch.nn.Sequential) or len(down) != 2:
                        raise RuntimeError("ContextEncoder: %sdownsample must be Sequential(Conv2d 1x1, nn.Sequential())" % where)
                    _check_conv(down[0], cin, cout, 1, s, 0, where + "downsample.0")
                    _check_empty(down[1], where + "downsample.1")
                self.blocks.append(blk)
                cin = cout
        conv2 = getattr(module, "conv2", None)
        if not isinstance(conv2, torch.nn.Conv2d):
            raise RuntimeError("ContextEncoder: conv2 must be a Conv2d")
        _check_conv(conv2, cin, conv2.out_channels, 1, 1, 0, "conv2")
        self.module = module
        self.ends = bool(ends)
        self._packs = PackCache()
        self.fused_calls = 0

    def _convs(self):
        m = self.module
        convs = [m.conv1, m.conv2]
        for blk in self.blocks:
            convs += [blk.conv1, blk.conv2] + ([blk.downsample[0]] if blk.downsample is not None else [])
        return convs

    def _serves(self, x):
        m = self.module
        if not isinstance(x, torch.Tensor) or not x.is_cuda or x.dim() != 5 or not x.is_contiguous():
            return False
        if x.dtype not in FLOAT_OR_HALF or x.shape[0] * x.shape[1] * x.shape[3] * x.shape[4] == 0:
            return False
        if m.training and getattr(m, "dropout", None) is not None:
            return False
        params = [p for c in self._convs() for p in (c.weight, c.bias)]
        if any(p.dtype != torch.float32 or p.device != x.device or not p.is_contiguous() for p in params):
            return False
        return fused_dtype([x] + params) == torch.float16

    def _block(self, blk, y):
        c1, c2 = blk.conv1, blk.conv2
        down = blk.downsample[0] if blk.downsample is not None else None
        r = y
        if encconv.serves(c1, y):
            p1 = self._packs.of(c1, encconv.pack_enc3)
            if down is None:
                t = encconv.enc_conv3x3(y, p1, relu=True)
            else:
                t, r = encconv.enc_conv3x3(y, p1, stride=2, relu=True, down=self._packs.of(down, encconv.pack_enc1))
        else:
            t = torch.relu(c1(y)).contiguous()
            if down is not None:
                r = down(y).contiguous()
        if encconv.serves(c2, t):
            return encconv.enc_conv3x3(t, self._packs.of(c2, encconv.pack_enc3), residual=r)
        return torch.relu(r + torch.relu(c2(t))).contiguous()

    def _fused(self, x, split=False):
        """The fused forward; with `split` the pair (net, inp) when the output layer's launch made it, else the output.  None
        if the stem returned something the kernels do not take."""
        m = self.module
        b, n, c1, h1, w1 = x.shape
        x4 = x.view(b * n, c1, h1, w1)
        if self.ends and encconv.serves_stem(m.conv1, x4):
            y = encconv.enc_stem7x7(x4, self._packs.of(m.conv1, encconv.pack_stem), relu=True)
        else:
            y = torch.relu(m.conv1(x4))
            if y.dtype != torch.float16:
                return None
            y = y.contiguous()
        for blk in self.blocks:
            y = self._block(blk, y)
        if self.ends and encconv.serves_out(m.conv2, y):
            pack = self._packs.of(m.conv2, encconv.pack_out1)
            if split:
                return tuple(t.view(b, n, 128, t.shape[2], t.shape[3]) for t in encconv.enc_out1x1(y, pack, split=True))
            y = encconv.enc_out1x1(y, pack)
        else:
            y = m.conv2(y)
        return y.view(b, n, y.shape[1], y.shape[2], y.shape[3])

    def __call__(self, x):
        m = self.module
        out = self._fused(x) if self._serves(x) else None
        if out is None:
            return type(m).forward(m, x)
        self.fused_calls += 1
        return out

    def net_inp(self, x):
        """(net, inp) = (tanh(ctx[:, :, :128]), relu(ctx[:, :, 128:])) of ctx = self(x), two contiguous (B,N,128,h,w) tensors
        (reference motion_filter.py:36-37)."""
        m = self.module
        if m.conv2.out_channels != 256:
            raise RuntimeError("ContextEncoder.net_inp: output_dim must be 256 (net and inp of 128 planes each), got %d"
                               % m.conv2.out_channels)
        out = self._fused(x, split=True) if self._serves(x) else None
        if out is None:
            out = type(m).forward(m, x)
        else:
            self.fused_calls += 1
        if isinstance(out, tuple):
            return out
        net, inp = out.split([128, 128], dim=2)
        return net.tanh().contiguous(), inp.relu().contiguous()


def install(module, ends=False):
    """Bind a ContextEncoder as `module.forward` (an instance attribute: parameters, buffers and state_dict keys are
    unchanged), so every caller of the encoder reaches the fused path.  `ends` as in ContextEncoder.  Returns the wrapper;
    a second call returns the one already installed (with the `ends` it was made with)."""
    return bind(module, "forward", ContextEncoder, lambda _: ContextEncoder(module, ends=ends))


def uninstall(module):
    """Undo `install`: the class's forward is used again."""
    unbind(module, "forward", ContextEncoder)
