"""LGU-SLAM's KAN-bias GRU (reference droid_slam/modules/gru_kanBias.py, modules/kan.py), the GRU of `UpdateModule`
(droid_net.py:120), on the HIP kernels of csrc/kangru.hip.

Everything around the three 3x3 convolutions is fused: the pooled context vector (1x1 convolution on the matrix cores,
gate, product, spatial mean), the three KANLinear heads in one launch, the z / r gates (r*net written in place over
channels 0..127 of the net_inp buffer, which conv_q then reads as cat(r*net, inp)) and the blend.  The convolutions
stay the module's own calls, on the same tensors as in the reference.

    gru.install(update_module.gru)   # UpdateModule.forward now reaches the fused path, state_dict keys unchanged

Op-level functions (`kangru_context`, `kan_heads`, `kangru_gates_`, `kangru_blend`): contiguous HIP device tensors only
(no CPU fallback), every argument error raised before anything is launched, no host synchronisation (graph-capturable),
forward only: inputs that require grad are refused while grad mode is on.  float32 tensors select the fp32 kernels,
float16 tensors the half kernels with the reference's autocast rounding points (include/lgu_corr.h).
"""
import torch

from ._host import (bind, check_contiguous, check_device, check_dtype, check_no_grad, check_same_dtype, check_shape, fused_dtype,
                    is_conv, launch, param_key, typed, unbind)
from ._host import ptr as _ptr, stream as _stream

C, CIN, NKNOT, NBASIS = 128, 448, 10, 6
K_FEAT = C + C * NBASIS          # 896 features per edge: [silu(x) | B(x)]
CTX_PIXELS = 256                 # include/lgu_corr.h LGU_KANGRU_CTX_PIXELS
HEADS = ("kanz_glo", "kanr_glo", "kanq_glo")


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
    version), so load_state_dict, in-place updates and update_grid are picked up."""

    def __init__(self, module):
        for name in ("convz", "convr", "convq"):
            _check_conv(getattr(module, name, None), CIN, C, 3, 1, name)
        _check_conv(getattr(module, "w", None), C, C, 1, 0, "w")
        for name in HEADS:
            _check_kan(getattr(module, name, None), name)
        self.module = module
        self._key = None
        self._packed = None
        self.fused_calls = 0

    def _sources(self):
        m = self.module
        ts = [m.w.weight, m.w.bias]
        for name in HEADS:
            h = getattr(m, name)
            ts += [h.grid, h.base_weight, h.spline_weight, h.spline_scaler]
        return ts

    def packed(self, dtype):
        """(w (128,128), b (128), grid (3,128,10), wpack (384,896)) for the kernels in `dtype`, cached."""
        ts = self._sources()
        key = (dtype,) + param_key(ts)
        if key != self._key:
            m = self.module
            with torch.no_grad():
                w = m.w.weight.detach().reshape(C, C).to(dtype).contiguous()
                b = m.w.bias.detach().to(dtype).contiguous()
                grid, wpack = pack_heads([getattr(m, n) for n in HEADS], dtype)
            self._packed, self._key = (w, b, grid, wpack), key
        return self._packed

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
        net_inp = torch.cat((net,) + tuple(inputs), dim=1)
        glo = kangru_context(net, w, b)
        k = kan_heads(glo, grid, wpack)
        cz = m.convz(net_inp)
        cr = m.convr(net_inp)
        z = kangru_gates_(net_inp, cz.contiguous(), cr.contiguous(), k[0], k[1], net)
        cq = m.convq(net_inp)                               # reads cat(r*net, inp)
        self.fused_calls += 1
        return kangru_blend(cq.contiguous(), k[2], z, net)


def install(module):
    """Bind a KanBiasGRU as `module.forward` (an instance attribute: parameters, buffers and state_dict keys are
    unchanged), so the reference's UpdateModule.forward reaches the fused path.  Returns the wrapper."""
    return bind(module, "forward", KanBiasGRU, lambda _: KanBiasGRU(module))


def uninstall(module):
    """Undo `install`: the class's forward is used again."""
    unbind(module, "forward", KanBiasGRU)
