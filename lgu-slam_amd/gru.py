"""LGU-SLAM's KAN-bias GRU (reference droid_slam/modules/gru_kanBias.py, modules/kan.py), the GRU of `UpdateModule`
(droid_net.py:120), on the HIP kernels of csrc/kangru.hip.

Everything around the three 3x3 convolutions is fused: the pooled context vector (1x1 convolution on the matrix cores,
gate, product, spatial mean), the three KANLinear heads in one launch, the z / r gates (r*net written in place over
channels 0..127 of the net_inp buffer, which conv_q then reads as cat(r*net, inp)) and the blend.  By default the
convolutions stay the module's own calls, on the same tensors as in the reference.  With `convs=True`, under float16
autocast, they are csrc/gruconv.hip's: convz and convr as one 256-wide launch with the gates as its epilogue, convq with
the blend as its epilogue, both reading net, inp, corr and flow where they lie (no cat, no layout pass).

    gru.install(update_module.gru)               # UpdateModule.forward now reaches the fused path, state_dict keys unchanged
    gru.install(update_module.gru, convs=True)   # and the three convolutions are fused too: 5 launches per forward

Op-level functions (`kangru_context`, `kan_heads`, `kangru_gates_`, `kangru_blend`, `gru_conv3x3`, `gru_conv_zr`,
`gru_conv_q`): contiguous HIP device tensors only
(no CPU fallback), every argument error raised before anything is launched, no host synchronisation (graph-capturable),
forward only: inputs that require grad are refused while grad mode is on.  float32 tensors select the fp32 kernels,
float16 tensors the half kernels with the reference's autocast rounding points (include/lgu_corr.h).
"""
import torch

from . import _lib
from ._host import (PackCache, bind, check_contiguous, check_device, check_dtype, check_no_grad, check_same_dtype, check_shape,
                    fused_dtype, is_conv, launch, typed, unbind)
from ._host import ptr as _ptr, stream as _stream

C, CIN, NKNOT, NBASIS = 128, 448, 10, 6
K_FEAT = C + C * NBASIS          # 896 features per edge: [silu(x) | B(x)]
CTX_PIXELS = 256                 # include/lgu_corr.h LGU_KANGRU_CTX_PIXELS
HEADS = ("kanz_glo", "kanr_glo", "kanq_glo")
CONVS = ("convz", "convr", "convq")
# include/lgu_corr.h LGU_GRUCONV_*: 126 K steps x Cout/16 channel tiles x 64 lanes x 8 halves
GRUCONV_STEPS, MAX_SEGMENTS = 126, 4
GRUCONV_WPACK_HALVES = {128: 516096, 256: 1032192}
_COUT_OF_HALVES = {v: k for k, v in GRUCONV_WPACK_HALVES.items()}
PLAIN, ZR, Q = 0, 1, 2

# The number of pixels E * H * W below which a `convs=True` call takes the convs=False path: the smallest measured shape
# class from which on the fused convolutions beat it beyond the two spreads added together (tools/prof_gruconv.py,
# DESIGN.md section 3.16).  0: every measured class kept the fused convolutions.
MIN_FUSED_CONV_PIXELS = 0


def _fmap(t, name, channels=C):
    if t.dim() != 4 or t.shape[1] != channels:
        raise RuntimeError("%s must be (E,%d,H,W), got %s" % (name, channels, tuple(t.shape)))


def _checked(named, what):
    """What follows an operator's shape checks when all its operands share one dtype; returns that dtype."""
    check_contiguous(named)
    dt = check_same_dtype(named)
    check_no_grad(what, named)
    check_device(named)
    return dt


def kangru_context(net, weight, bias):
    """glo (E,128) = mean over the pixels of sigmoid(w(net)) * net (gru_kanBias.py:23-24): net (E,128,H,W), weight
    (128,128,1,1) or (128,128) and bias (128) of net's dtype.  Half: the convolution output with its bias (one rounding,
    as the library adds the bias), the sigmoid, the product and the mean are each rounded to half, as under autocast."""
    _fmap(net, "net")
    named = [(net, "net"), (weight, "weight"), (bias, "bias")]
    check_shape(named[1:2], (C, C, 1, 1) if weight.dim() == 4 else (C, C))
    check_shape(named[2:], (C,))
    dt = _checked(named, "kangru_context")
    E, _, H, W = net.shape
    glo = torch.empty((E, C), dtype=dt, device=net.device)
    if E == 0:
        return glo
    if H * W == 0:
        raise RuntimeError("kangru_context: empty frame (H*W = 0), the mean is undefined")
    partial = torch.empty((E, (H * W + CTX_PIXELS - 1) // CTX_PIXELS, C), dtype=torch.float32, device=net.device)
    launch(typed("lgu_kangru_context", dt), "kangru_context", net.device, _ptr(net), _ptr(weight), _ptr(bias), E, H * W,
           _ptr(partial), _ptr(glo), _stream(net))
    return glo


def kan_heads(glo, grid, wpack):
    """(3,E,128): the three KANLinear heads of glo (E,128) (kan.py:147-161).  grid (3,128,10) float32: each head's
    knots; wpack (384,896) of glo's dtype from `pack_heads`."""
    if glo.dim() != 2 or glo.shape[1] != C:
        raise RuntimeError("glo must be (E,%d), got %s" % (C, tuple(glo.shape)))
    named = [(glo, "glo"), (grid, "grid"), (wpack, "wpack")]
    check_shape(named[1:2], (3, C, NKNOT))
    check_shape(named[2:], (3 * C, K_FEAT))
    check_contiguous(named)
    dt = check_same_dtype([named[0], named[2]])
    check_dtype(named[1:2], torch.float32)
    check_no_grad("kan_heads", named)
    check_device(named)
    E = glo.shape[0]
    out = torch.empty((3, E, C), dtype=dt, device=glo.device)
    if E == 0:
        return out
    launch(typed("lgu_kan_heads", dt), "kan_heads", glo.device, _ptr(glo), _ptr(grid), _ptr(wpack), E, _ptr(out), _stream(glo))
    return out


def kangru_gates_(net_inp, cz, cr, kz, kr, net):
    """z = sigmoid(cz + kz) (returned, (E,128,H,W)) and, in place, net_inp[:, :128] = sigmoid(cr + kr) * net
    (gru_kanBias.py:30-32): net_inp (E,448,H,W); cz, cr, net (E,128,H,W); kz, kr (E,128) broadcast over the pixels."""
    _fmap(net_inp, "net_inp", CIN)
    E, _, H, W = net_inp.shape
    check_shape([(cz, "cz"), (cr, "cr"), (net, "net")], (E, C, H, W))
    check_shape([(kz, "kz"), (kr, "kr")], (E, C))
    dt = _checked([(net_inp, "net_inp"), (cz, "cz"), (cr, "cr"), (kz, "kz"), (kr, "kr"), (net, "net")], "kangru_gates_")
    z = torch.empty((E, C, H, W), dtype=dt, device=net.device)
    if E * H * W == 0:
        return z
    launch(typed("lgu_kangru_gates", dt), "kangru_gates_", net.device, _ptr(cz), _ptr(cr), _ptr(kz), _ptr(kr), _ptr(net), E,
           H * W, _ptr(z), _ptr(net_inp), _stream(net))
    return z


def kangru_blend(cq, kq, z, net):
    """(1 - z) * net + z * tanh(cq + kq) (gru_kanBias.py:32-34) as a new (E,128,H,W) tensor: cq, z, net (E,128,H,W),
    kq (E,128)."""
    _fmap(cq, "cq")
    E, _, H, W = cq.shape
    check_shape([(z, "z"), (net, "net")], (E, C, H, W))
    check_shape([(kq, "kq")], (E, C))
    dt = _checked([(cq, "cq"), (kq, "kq"), (z, "z"), (net, "net")], "kangru_blend")
    out = torch.empty((E, C, H, W), dtype=dt, device=net.device)
    if E * H * W == 0:
        return out
    launch(typed("lgu_kangru_blend", dt), "kangru_blend", net.device, _ptr(cq), _ptr(kq), _ptr(z), _ptr(net), E, H * W,
           _ptr(out), _stream(net))
    return out


def pack_gruconv(convs):
    """(wpack (126, Cout/16, 64, 8) half, bias_h (Cout) half) of one Conv2d(448, 128, 3, padding=1) or of the pair
    (convz, convr), whose outputs are stacked (0..127 the first, 128..255 the second), on the weights' device.
    wpack[s, ct, l, j] = half(weight)[16 ct + (l & 15), 64 c64 + 32 kc + 8 (l >> 4) + j, t // 3, t % 3] with
    s = (c64 * 9 + t) * 2 + kc: the B operand of v_mfma_f32_16x16x32_f16 in the kernel's K order (7 chunks of 64 channels,
    9 taps t = 3 ky + kx within a chunk, 2 blocks of 32 channels within a tap).  Every slot holds a weight."""
    convs = [convs] if isinstance(convs, torch.nn.Module) else list(convs)
    if len(convs) not in (1, 2):
        raise RuntimeError("pack_gruconv: one convolution or the pair (convz, convr), got %d" % len(convs))
    for i, m in enumerate(convs):
        _check_conv(m, CIN, C, 3, 1, "convolution %d" % i)
    cout = C * len(convs)
    with torch.no_grad():
        wh = torch.cat([m.weight.detach() for m in convs], 0).to(torch.float16)
        # [ct][cl][c64][kc][g][j][t] -> [c64][t][kc][ct][g][cl][j]: lane l = 16 g + cl
        wpack = wh.reshape(cout // 16, 16, 7, 2, 4, 8, 9).permute(2, 6, 3, 0, 4, 1, 5).reshape(GRUCONV_STEPS, cout // 16, 64, 8)
        wpack = wpack.contiguous()
        bias_h = torch.cat([m.bias.detach() for m in convs], 0).to(device=wh.device, dtype=torch.float16).contiguous()
    return wpack, bias_h


def _gruconv(what, mode, segments, wpack, bias_h, couts, extra, like):
    """The checks of the three fused-convolution operators in their one order (shapes, pack size, contiguity, dtypes,
    no-grad, device) and the launch.  extra: [(tensor, name, shape tail after E)]; like: how many (E,128,H,W) outputs."""
    segments = list(segments)
    if not 1 <= len(segments) <= MAX_SEGMENTS:
        raise RuntimeError("%s: 1 to %d segments, got %d" % (what, MAX_SEGMENTS, len(segments)))
    named = [(t, "segments[%d]" % i) for i, t in enumerate(segments)]
    x0 = segments[0]
    if x0.dim() != 4:
        raise RuntimeError("segments[0] must be (E,ch,H,W), got %s" % (tuple(x0.shape),))
    E, _, H, W = x0.shape
    for t, name in named:
        if t.dim() != 4 or t.shape[0] != E or tuple(t.shape[2:]) != (H, W) or t.shape[1] % 32 != 0 or t.shape[1] == 0:
            raise RuntimeError("%s must be (%d,ch,%d,%d) with ch a multiple of 32, got %s" % (name, E, H, W, tuple(t.shape)))
    if sum(t.shape[1] for t in segments) != CIN:
        raise RuntimeError("%s: the segments' channels must sum to %d, got %s" % (what, CIN, [t.shape[1] for t in segments]))
    for t, name, tail in extra:
        check_shape([(t, name)], (E,) + tuple(H if d == "H" else W if d == "W" else d for d in tail))
    cout = _COUT_OF_HALVES.get(wpack.numel())
    if cout not in couts:
        raise RuntimeError("wpack must hold %s halves (pack_gruconv), got %s"
                           % (" or ".join(str(GRUCONV_WPACK_HALVES[c]) for c in couts), tuple(wpack.shape)))
    check_shape([(bias_h, "bias_h")], (cout,))
    named += [(wpack, "wpack"), (bias_h, "bias_h")] + [(t, name) for t, name, _ in extra]
    check_contiguous(named)
    check_dtype(named, torch.float16)
    check_no_grad(what, named)
    check_device(named)
    outs = [torch.empty((E, cout if mode == PLAIN else C, H, W), dtype=torch.float16, device=x0.device) for _ in range(like)]
    if E == 0:
        return outs
    if H * W == 0:
        raise RuntimeError("%s: empty frame (H*W = 0)" % what)
    a = _lib.GruConvArgs()
    for i, t in enumerate(segments):
        a.seg[i], a.seg_ch[i] = t.data_ptr(), t.shape[1]
    a.nseg, a.wpack, a.bias = len(segments), wpack.data_ptr(), bias_h.data_ptr()
    by_name = {name: t.data_ptr() for t, name, _ in extra}
    a.k0 = by_name.get("kz", by_name.get("kq"))
    a.k1, a.net, a.z = by_name.get("kr"), by_name.get("net"), by_name.get("z")
    a.out0, a.out1 = outs[0].data_ptr(), outs[1].data_ptr() if like > 1 else None
    a.N, a.H, a.W, a.Cout, a.mode, a.flags = E, H, W, cout, mode, 0
    launch("lgu_gruconv3x3_c448_h16", what, x0.device, a, _stream(x0))
    return outs


_FMAP = (C, "H", "W")


def gru_conv3x3(segments, wpack, bias_h):
    """half(conv2d(cat(segments, 1), w_h, b_h, padding=1)) as a new (E,Cout,H,W) half tensor: `segments` 1 to 4 half
    tensors (E,ch_i,H,W), every ch_i a multiple of 32, summing to 448 (the concatenation is never made and the split does
    not change a bit); wpack and bias_h from `pack_gruconv` (their size gives Cout, 128 or 256).  Exact products, fp32
    accumulation from the bias in one fixed order, one rounding to half."""
    return _gruconv("gru_conv3x3", PLAIN, segments, wpack, bias_h, (128, 256), [], 1)[0]


def gru_conv_zr(segments, wpack, bias_h, kz, kr, net):
    """(z, rnet), both new (E,128,H,W): what `kangru_gates_` makes of c = gru_conv3x3(segments, ...) with the 256-wide pack
    of (convz, convr), z = sigmoid(c[:, :128] + kz), rnet = sigmoid(c[:, 128:] + kr) * net with its half roundings, in the
    convolution's own launch.  kz, kr (E,128); net (E,128,H,W)."""
    return tuple(_gruconv("gru_conv_zr", ZR, segments, wpack, bias_h, (256,),
                          [(kz, "kz", (C,)), (kr, "kr", (C,)), (net, "net", _FMAP)], 2))


def gru_conv_q(segments, wpack, bias_h, kq, z, net):
    """The new net (E,128,H,W): what `kangru_blend` makes of c = gru_conv3x3(segments, ...) with convq's 128-wide pack,
    (1 - z) * net + z * tanh(c + kq) with its half roundings, in the convolution's own launch.  segments[0] is r * net.
    kq (E,128); z, net (E,128,H,W)."""
    return _gruconv("gru_conv_q", Q, segments, wpack, bias_h, (128,),
                    [(kq, "kq", (C,)), (z, "z", _FMAP), (net, "net", _FMAP)], 1)[0]


def pack_heads(heads, dtype):
    """(grid (3,128,10) float32, wpack (384,896) dtype) of three KANLinear heads: row h*128 + o of wpack is
    [base_weight[o] | (spline_weight * spline_scaler[..., None])[o].flatten()], the product formed in float32 and then
    cast (what autocast hands the spline GEMM)."""
    with torch.no_grad():
        grid = torch.stack([h.grid.detach().float() for h in heads]).contiguous()
        rows = [torch.cat([h.base_weight.detach().float(), (h.spline_weight * h.spline_scaler.unsqueeze(-1)).reshape(C, -1)], 1)
                .to(dtype) for h in heads]
        return grid, torch.cat(rows, 0).contiguous()


def _check_conv(m, cin, cout, k, pad, name):
    if not is_conv(m, cin, cout, k, pad=pad, bias=True):
        raise RuntimeError("KanBiasGRU: %s must be Conv2d(%d, %d, %d, padding=%d) with bias" % (name, cin, cout, k, pad))


def _check_kan(m, name):
    ok = (getattr(m, "in_features", None) == C and getattr(m, "out_features", None) == C
          and getattr(m, "grid_size", None) == 3 and getattr(m, "spline_order", None) == 3
          and getattr(m, "enable_standalone_scale_spline", False) is True
          and isinstance(getattr(m, "base_activation", None), torch.nn.SiLU))
    if ok:
        for attr, shape in (("grid", (C, NKNOT)), ("base_weight", (C, C)), ("spline_weight", (C, C, NBASIS)),
                            ("spline_scaler", (C, C))):
            t = getattr(m, attr, None)
            ok = ok and isinstance(t, torch.Tensor) and tuple(t.shape) == shape
    if not ok:
        raise RuntimeError("KanBiasGRU: %s must be KANLinear(128, 128, grid_size=3, spline_order=3) with SiLU and a "
                           "standalone spline scaler" % name)


class KanBiasGRU:
    """Callable stand-in for the forward of the reference's `KAN_bias_GRU(128, 320)`:

        fused = KanBiasGRU(update_module.gru)
        net = fused(net, inp, corr, flow)      # = update_module.gru(net, inp, corr, flow)

    Fused path (csrc/kangru.hip + the module's three conv calls) for HIP tensors when either CUDA autocast is on with
    float16 and net / inputs are half, or autocast is off and net / inputs are float32; the module's parameters must
    be float32 (the reference's).  Everything else goes to the module's own forward unchanged: CPU tensors, other
    dtypes, a bfloat16 autocast, and grad mode with parameters or inputs that require grad (training / backward).
    The packed weights are cached; the key covers every parameter and buffer they are made of (data pointer and
    version), so load_state_dict, in-place updates and update_grid are picked up.

    convs=True: in the float16-autocast mode, and from MIN_FUSED_CONV_PIXELS pixels E*H*W on, the three convolutions
    are csrc/gruconv.hip's: context, heads, one launch for convz + convr + gates and one for convq + blend, 5 launches.
    The inputs are read where they lie when there are at most three of them and every channel count is a multiple of
    32; otherwise they are concatenated once into one 320-channel segment.  `fused_conv_calls` counts these calls.  In
    fp32 mode and on every route to the module's own forward `convs` changes nothing."""

    def __init__(self, module, convs=False):
        for name in ("convz", "convr", "convq"):
            _check_conv(getattr(module, name, None), CIN, C, 3, 1, name)
        _check_conv(getattr(module, "w", None), C, C, 1, 0, "w")
        for name in HEADS:
            _check_kan(getattr(module, name, None), name)
        self.module = module
        self._packs = PackCache()
        self.fused_calls = 0
        self.convs = bool(convs)
        self.fused_conv_calls = 0

    def _sources(self):
        m = self.module
        ts = [m.w.weight, m.w.bias]
        for name in HEADS:
            h = getattr(m, name)
            ts += [h.grid, h.base_weight, h.spline_weight, h.spline_scaler]
        return ts

    def packed(self, dtype):
        """(w (128,128), b (128), grid (3,128,10), wpack (384,896)) for the kernels in `dtype`, cached."""
        m = self.module

        def make():
            with torch.no_grad():
                w = m.w.weight.detach().reshape(C, C).to(dtype).contiguous()
                b = m.w.bias.detach().to(dtype).contiguous()
                return (w, b) + pack_heads([getattr(m, n) for n in HEADS], dtype)
        return self._packs.get("heads", self._sources(), make, dtype)

    def conv_packed(self):
        """((wpack_zr, bias_zr), (wpack_q, bias_q)) for gru_conv_zr and gru_conv_q, cached under the three convolutions'
        weights and biases."""
        m = self.module
        return self._packs.get("convs", [p for n in CONVS for p in (getattr(m, n).weight, getattr(m, n).bias)],
                               lambda: (pack_gruconv((m.convz, m.convr)), pack_gruconv(m.convq)))

    def _mode(self, net, inputs):
        """torch.float16 / torch.float32 for the fused path, None for the module's forward."""
        ts = (net,) + tuple(inputs)
        if not inputs or not all(isinstance(t, torch.Tensor) and t.is_cuda for t in ts):
            return None
        params = self._sources() + [getattr(self.module, n).weight for n in ("convz", "convr", "convq")] + \
            [getattr(self.module, n).bias for n in ("convz", "convr", "convq")]
        if any(p.dtype != torch.float32 or p.device != net.device for p in params):
            return None
        if any(t.device != net.device or t.dim() != 4 for t in ts):
            return None
        dt = fused_dtype(list(ts) + params)
        if dt is None or any(t.dtype != dt for t in ts):
            return None
        E, ch, H, W = net.shape
        if ch != C or sum(t.shape[1] for t in inputs) != CIN - C or \
                any(t.shape[0] != E or tuple(t.shape[2:]) != (H, W) for t in inputs):
            return None
        return dt

    def __call__(self, net, *inputs):
        m = self.module
        dt = self._mode(net, inputs)
        if dt is None:
            return type(m).forward(m, net, *inputs)
        E, _, H, W = net.shape
        if E == 0:
            return torch.empty((0, C, H, W), dtype=dt, device=net.device)
        net = net.contiguous()
        w, b, grid, wpack = self.packed(dt)
        if self.convs and dt == torch.float16 and H * W > 0 and E * H * W >= MIN_FUSED_CONV_PIXELS:
            if len(inputs) <= MAX_SEGMENTS - 1 and all(t.shape[1] % 32 == 0 and t.shape[1] > 0 for t in inputs):
                rest = [t.contiguous() for t in inputs]
            else:
                rest = [torch.cat(tuple(inputs), dim=1)]
            (wzr, bzr), (wq, bq) = self.conv_packed()
            k = kan_heads(kangru_context(net, w, b), grid, wpack)
            z, rnet = gru_conv_zr([net] + rest, wzr, bzr, k[0], k[1], net)
            out = gru_conv_q([rnet] + rest, wq, bq, k[2], z, net)
            self.fused_calls += 1
            self.fused_conv_calls += 1
            return out
        net_inp = torch.cat((net,) + tuple(inputs), dim=1)
        glo = kangru_context(net, w, b)
        k = kan_heads(glo, grid, wpack)
        cz = m.convz(net_inp)
        cr = m.convr(net_inp)
        z = kangru_gates_(net_inp, cz.contiguous(), cr.contiguous(), k[0], k[1], net)
        cq = m.convq(net_inp)                               # reads cat(r*net, inp)
        self.fused_calls += 1
        return kangru_blend(cq.contiguous(), k[2], z, net)


def install(module, convs=False):
    """Bind a KanBiasGRU as `module.forward` (an instance attribute: parameters, buffers and state_dict keys are
    unchanged), so the reference's UpdateModule.forward reaches the fused path.  Returns the wrapper; a second call
    returns the first wrapper with `convs` set as given."""
    wrapper = bind(module, "forward", KanBiasGRU, lambda _: KanBiasGRU(module, convs=convs))
    wrapper.convs = bool(convs)
    return wrapper


def uninstall(module):
    """Undo `install`: the class's forward is used again."""
    unbind(module, "forward", KanBiasGRU)
