"""The host vocabulary of the operator layer, once: pointer and stream plumbing, the dtype names, the argument refusals,
the launch, and what the module wrappers share: the Conv2d predicate, the packed-weight cache (`PackCache`), the autocast /
grad decision, the routing predicate of the half-only layers (`serves_half`), the route-and-count call of a single-layer
wrapper (`LayerWrapper`: Conv1, Conv3, Head, Upmask, FlowEncoder), and bind / unbind / `installed` of a forward.

Every refusal takes a list of (tensor, "name") pairs and raises the text the reference (or torch) raises for the same
defect.  The ORDER in which an operator calls them is part of its behaviour (an argument with two defects reports the
first): each operator states its own order, nothing here reorders checks across operators.
"""
import ctypes

import torch

from . import _lib

_vp = ctypes.c_void_p


# ---- pointers, streams, the device guard ----------------------------------------------------------------------------
def ptr(t):
    return _vp(t.data_ptr())


def stream(t):
    return _vp(torch.cuda.current_stream(t.device).cuda_stream)


class CurrentDevice:
    """Launch guard: the library launches on the CURRENT device, so a call whose buffers live on another device switches
    for the call — and costs one integer comparison when it already is current (the usual one-process-per-GPU case)."""

    def __init__(self, device):
        self.idx = device.index if device.index is not None else torch.cuda.current_device()
        self.prev = -1

    def __enter__(self):
        cur = torch.cuda.current_device()
        if cur != self.idx:
            self.prev = cur
            torch.cuda.set_device(self.idx)

    def __exit__(self, *exc):
        if self.prev >= 0:
            torch.cuda.set_device(self.prev)
            self.prev = -1
        return False


SUFFIX = {torch.float32: "_f32", torch.float16: "_h16"}     # lgu_<entry>_f32 / _h16 by tensor dtype
FLOAT_OR_HALF = tuple(SUFFIX)


def typed(symbol, dtype):
    return symbol + SUFFIX[dtype]


def launch(symbol, what, device, *args):
    """One library call on `device`: a non-zero return code raises as "`what` failed: ..." (_lib.check)."""
    with CurrentDevice(device):
        rc = getattr(_lib.load(), symbol)(*args)
    if rc:
        _lib.check(rc, what)


# ---- dtype names ----------------------------------------------------------------------------------------------------
_TORCH_NAME = {torch.float32: "Float", torch.float16: "Half", torch.float64: "Double", torch.bfloat16: "BFloat16",
               torch.int64: "Long", torch.int32: "Int"}


def dtype_name(dt):
    """The name torch's own "expected scalar type" errors use; a dtype outside the table as torch prints it."""
    return _TORCH_NAME.get(dt, str(dt))


def bare_name(dt):
    """torch's spelling without the prefix ("float16"): what the correlation operators' refusals print."""
    return str(dt).replace("torch.", "")


# ---- refusals -------------------------------------------------------------------------------------------------------
_CONTIGUOUS = "%s must be contiguous"
_NO_CPU = "%s must be a HIP device tensor: lgu_slam_amd has no CPU fallback"


def check_contiguous(pairs):
    """The reference's CHECK_INPUT: TORCH_CHECK(x.is_contiguous(), #x " must be contiguous") (droid.cpp:48-49)."""
    for t, name in pairs:
        if not t.is_contiguous():
            raise RuntimeError(_CONTIGUOUS % name)


def check_dtype(pairs, want):
    """Every tensor has dtype `want`, or one of them if `want` is a tuple ("Float or Half")."""
    ok = want if isinstance(want, tuple) else (want,)
    for t, name in pairs:
        if t.dtype not in ok:
            raise RuntimeError("expected scalar type %s but found %s (%s)"
                               % (" or ".join(dtype_name(d) for d in ok), dtype_name(t.dtype), name))


def check_same_dtype(pairs, first=FLOAT_OR_HALF):
    """The first tensor's dtype is one of `first` and every other tensor has it; returns it."""
    check_dtype(pairs[:1], first)
    check_dtype(pairs[1:], pairs[0][0].dtype)
    return pairs[0][0].dtype


def check_shape(pairs, shape):
    for t, name in pairs:
        if tuple(t.shape) != tuple(shape):
            raise RuntimeError("%s must be %s, got %s" % (name, tuple(shape), tuple(t.shape)))


def check_hip(pairs):
    for t, name in pairs:
        if not t.is_cuda:
            raise RuntimeError(_NO_CPU % name)


def check_device(pairs):
    """Every tensor on a HIP device, then every tensor on the first one's."""
    check_hip(pairs)
    for t, name in pairs:
        if t.device != pairs[0][0].device:
            raise RuntimeError("%s is on %s, expected %s" % (name, t.device, pairs[0][0].device))


def needs_grad(tensors):
    return torch.is_grad_enabled() and any(t.requires_grad for t in tensors)


def check_no_grad(what, pairs):
    if needs_grad([t for t, _ in pairs]):
        raise RuntimeError("%s has no autograd: its outputs would carry no gradient. Call it under torch.no_grad() or "
                           "pass detached inputs" % what)


def check_operands(pairs, dtype=None):
    """The order of the correlation operators and of ba: CHECK_INPUT on every argument first, then per argument what this
    library additionally requires, HIP device and dtype.  dtype None: float32, named "Float" as the reference's accessors
    name it; a given dtype is printed bare.  (One call frame: the prepared plans call this once per lookup.)"""
    for t, name in pairs:
        if not t.is_contiguous():
            raise RuntimeError(_CONTIGUOUS % name)
    want, spelled = (torch.float32, "Float") if dtype is None else (dtype, bare_name(dtype))
    for t, name in pairs:
        if not t.is_cuda:
            raise RuntimeError(_NO_CPU % name)
        if t.dtype != want:
            raise RuntimeError("expected scalar type %s but found %s (%s)" % (spelled, bare_name(t.dtype), name))


def check_layer_operands(what, named):
    """What follows the shape checks of a half-only layer operator `what`: named[0] is x, float32 or half, the rest are
    the packs, half."""
    check_contiguous(named)
    check_dtype(named[:1], FLOAT_OR_HALF)
    check_dtype(named[1:], torch.float16)
    check_no_grad(what, named)
    check_device(named)


# ---- what the module wrappers share ---------------------------------------------------------------------------------
def is_conv(m, cin, cout, k, stride=1, pad=0, bias=None):
    """m is Conv2d(cin, cout, k, stride, pad) without dilation, groups or a padding mode; bias=True: and has a bias."""
    return (isinstance(m, torch.nn.Conv2d) and m.in_channels == cin and m.out_channels == cout and m.kernel_size == (k, k)
            and m.stride == (stride, stride) and m.padding == (pad, pad) and m.dilation == (1, 1) and m.groups == 1
            and m.padding_mode == "zeros" and (not bias or m.bias is not None))


def param_key(tensors):
    """Identity of the parameters a packed-weight cache was made of: load_state_dict, in-place updates and moves change it."""
    return tuple((t.data_ptr(), t._version, t.device) for t in tensors)


def capturing(device=None):
    """The current stream of `device` (default: the current device) is recording a graph.  What is made then is only
    recorded, not run, and lives in the graph's private memory pool: every cache of the package uses such a value for the
    call and does not keep it; a value kept from before the capture is used as it is."""
    if not torch.cuda.is_available():
        return False
    if device is None or device.index is None or device.index == torch.cuda.current_device():
        return torch.cuda.is_current_stream_capturing()
    with torch.cuda.device(device):
        return torch.cuda.is_current_stream_capturing()


def no_upload_while_capturing(what, device=None):
    """Refusal of a host table that would have to be uploaded while the stream records a graph: the copy waits for the
    host, which a capture does not allow, and its contents are indices.  Callers ask before the launches the table serves."""
    if capturing(device):
        raise RuntimeError("%s: its index table has to be uploaded, which a stream that is capturing a graph cannot do; "
                           "make the same call once before the capture" % what)


class PackCache:
    """Packed weights, one entry per slot, each kept while the parameters it was made of are what they were (`param_key`):
    load_state_dict, in-place updates and moves make a new pack, which replaces the slot's old one.  A pack made while the
    stream is capturing a graph serves that call and is not kept (`capturing`)."""

    def __init__(self):
        self._slots = {}

    def get(self, slot, tensors, make, *extra):
        """`make()`, cached under `slot` while (extra, param_key(tensors)) is unchanged."""
        key = (extra, param_key(tensors))
        hit = self._slots.get(slot)
        if hit is None or hit[0] != key:
            if capturing(tensors[0].device if len(tensors) and tensors[0].is_cuda else None):   # asked on a miss only
                return make()
            hit = (key, make())
            self._slots[slot] = hit
        return hit[1]

    def of(self, conv, pack):
        """pack(conv.weight, conv.bias), cached per layer."""
        return self.get(id(conv), (conv.weight, conv.bias), lambda: pack(conv.weight, conv.bias))


def fused_dtype(tensors):
    """The dtype a fused path computes in now: float16 under CUDA float16 autocast, float32 with autocast off; None (the
    module's own forward) under any other autocast, or when grad mode is on and one of `tensors` requires grad."""
    if needs_grad(tensors):
        return None
    if torch.is_autocast_enabled("cuda"):
        return torch.float16 if torch.get_autocast_dtype("cuda") == torch.float16 else None
    return torch.float32


def serves_half(x, cin, params, min_pixels):
    """The fused path of a layer that has a half kernel only serves this call: x is a HIP tensor (N,cin,H,W), float32 or
    half, with a non-empty frame and at least `min_pixels` pixels N*H*W; `params` are float32 on x's device; CUDA float16
    autocast is on and nothing requires grad.  (A batch of 0 is served: the operators return the empty result.)"""
    if not isinstance(x, torch.Tensor) or not x.is_cuda or x.dim() != 4 or x.shape[1] != cin:
        return False
    if x.dtype not in FLOAT_OR_HALF or x.shape[2] * x.shape[3] == 0:
        return False
    if any(p.dtype != torch.float32 or p.device != x.device for p in params):
        return False
    if fused_dtype([x, *params]) != torch.float16:      # there is no fp32 kernel
        return False
    return x.shape[0] * x.shape[2] * x.shape[3] >= min_pixels


class LayerWrapper:
    """Callable stand-in for the forward of `module`, whose layer `conv` has a fused half kernel.  A call the subclass's
    `_serves(x)` admits is `_operator(x.contiguous(), *packed())`, counted in `fused_calls` once the operator has
    returned, then `_finish`; every other call is the module's own forward, followed by a ReLU where `relu` is set.

    A subclass checks its module, hands `conv` and its pack function to this constructor, and states `_serves` (one
    `serves_half` with its Cin, the parameters it gates on and its module's MIN_FUSED_PIXELS, read at the call) and
    `_operator` (its operator function)."""

    relu = False

    def __init__(self, module, conv, pack):
        self.module = module
        self.conv = conv
        self._pack = pack
        self._packs = PackCache()
        self.fused_calls = 0

    def packed(self):
        """(wpack, bias_h) of `conv`, cached."""
        return self._packs.of(self.conv, self._pack)

    def _finish(self, y):
        return y

    def __call__(self, x):
        m = self.module
        if not self._serves(x):
            y = type(m).forward(m, x)
            return torch.relu(y) if self.relu else y
        y = self._operator(x.contiguous(), *self.packed())
        self.fused_calls += 1
        return self._finish(y)


def installed(module, classes, who, hint=""):
    """The wrapper of `classes` that `module.forward` already carries; None if nothing is bound there (or `module` is no
    nn.Module); a wrapper of any other kind is refused in the name of `who`."""
    cur = module.__dict__.get("forward") if isinstance(module, torch.nn.Module) else None
    if cur is None or isinstance(cur, classes):
        return cur
    raise RuntimeError("%s: forward already carries a %s%s" % (who, type(cur).__name__, hint))


def bind(obj, attr, cls, make):
    """Set `make(previous instance attribute or None)` as the instance attribute obj.attr (the class and a module's
    parameters, buffers and state_dict keys are untouched); a `cls` already bound there is returned instead."""
    cur = obj.__dict__.get(attr)
    if isinstance(cur, cls):
        return cur
    wrapper = make(cur)
    setattr(obj, attr, wrapper)
    return wrapper


def unbind(obj, attr, cls):
    """Undo `bind`: the class's attribute is used again.  Returns the wrapper that was removed, or None."""
    cur = obj.__dict__.get(attr)
    if isinstance(cur, cls):
        delattr(obj, attr)
        return cur
    return None
