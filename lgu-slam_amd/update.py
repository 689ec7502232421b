"""The whole update operator (reference droid_slam/droid_net.py, UpdateModule.forward and GraphAgg.forward) written with
this package's operator functions, so that the fused activations do not stop at the reference's Sequential boundaries:

    wrapper = update.install(net.update, gru_convs=True)
    net, delta, weight, eta, upmask = net.update(net, inp, corr, flow, ii, jj)

The per-site wrappers (flow, conv3, heads, gru, upmask, conv1) each own one layer; UpdateOperator owns the module's
forward.  On its fused route the ReLU behind corr_encoder[0], agg.conv1 and agg.conv2 and the Sigmoid of `weight` are part
of their convolution's launch, scatter_mean gets its dim_size from torch.unique (no second host read), and with
defer_upmask=True the features behind agg.conv2 are handed out in place of the 576-plane mask, for
upmask.upsample_from_net_.  Everything it cannot serve goes to the module's own forward with the arguments untouched.
Forward only; batch 1; not graph-capturable with `ii` given (torch.unique reads the host).
"""
import torch

from . import aggregate, conv1, conv3, flow as _flow, gru as _gru, heads, upmask
from ._host import FLOAT_OR_HALF, PackCache, bind, fused_dtype, installed, unbind


def _refuse(site, want):
    raise RuntimeError("UpdateOperator: %s must be %s" % (site, want))


def _check_stack(m, site, first, first_text):
    """m is Sequential(first-eligible conv, ReLU, Conv2d(128, 128, 3, padding=1), ReLU)."""
    nn = torch.nn
    ok = isinstance(m, nn.Sequential) and len(m) == 4 and first(m[0]) and isinstance(m[1], nn.ReLU) and isinstance(m[3], nn.ReLU)
    if not (ok and conv3.eligible(m[2]) and m[2].out_channels == 128):
        _refuse(site, "Sequential(%s, ReLU, Conv2d(128, 128, 3, padding=1), ReLU) with biases" % first_text)


def _check_head_stack(m, site, act):
    """m is Sequential(Conv2d(128, 128, 3, padding=1), ReLU, <a heads tail with two outputs and the activation `act`>)."""
    nn = torch.nn
    ok = isinstance(m, nn.Sequential) and len(m) >= 3 and conv3.eligible(m[0]) and m[0].out_channels == 128
    ok = ok and isinstance(m[1], nn.ReLU)
    parsed = heads.parse(m[2:]) if ok else None
    if parsed is None or parsed[0].out_channels != 2 or parsed[1] != act:
        _refuse(site, "Sequential(Conv2d(128, 128, 3, padding=1), ReLU, Conv2d(128, 2, 3, padding=1), pass-through members%s)"
                % (", Sigmoid" if act == "sigmoid" else ""))


def _check_agg(agg):
    for name in ("conv1", "conv2"):
        c = getattr(agg, name, None)
        if not (conv3.eligible(c) and c.out_channels == 128):
            _refuse("agg." + name, "Conv2d(128, 128, 3, padding=1) with a bias")
    parsed = heads.parse(getattr(agg, "eta", None))
    if parsed is None or parsed[0].out_channels != 1 or parsed[1] != "softplus" or not isinstance(agg.eta, torch.nn.Sequential):
        _refuse("agg.eta", "Sequential(Conv2d(128, 1, 3, padding=1), pass-through members, Softplus)")
    if upmask.parse(getattr(agg, "upmask", None)) is None:
        _refuse("agg.upmask", "Conv2d(128, 576, 1) with a bias, or a Sequential holding exactly that")


class UpdateOperator:
    """Callable stand-in for `UpdateModule.forward(net, inp, corr, flow=None, ii=None, jj=None)` of a module shaped like the
    reference's (corr_encoder, flow_encoder, gru, delta, weight, agg with conv1, conv2, eta and upmask):

        fused = UpdateOperator(update_module, gru_convs=True)
        net, delta, weight, eta, upmask = fused(net, inp, corr, flow, ii, jj)

    Fused route: CUDA float16 autocast, every tensor on one HIP device, float32 parameters on that device, nothing
    requiring grad, net / inp / corr / flow 5-D float32 or half with batch 1 and equal (num, ht, wd), num > 0 and
    ht * wd > 0.  The forward is then the reference's, written with conv1x1, conv3x3, flow_conv7_relu, a KanBiasGRU
    (which routes itself: float32 net / inp reach the module's GRU), head_conv3x3, scatter_mean and upmask_conv1x1; the
    results have the shapes and dtypes the module returns under autocast.  Anything else goes to the module's own forward
    with the arguments untouched, where per-site installs on the submodules act as before; on the fused route they are
    not called, and nothing is bound on a submodule here.

    gru_convs: the GRU's three convolutions on csrc/gruconv.hip (KanBiasGRU's `convs`).
    defer_upmask: the fifth result is the aggregated features (1,U,128,ht,wd) half that agg.upmask would have consumed, in
    place of the (1,U,576,ht,wd) mask, which is then not written; `upmask_packed()` gives the layer's packed weights for
    upmask.upsample_from_net_.  `fused_calls` counts whole fused forwards, `module_calls` the others.

    Behind the GRU, delta[0], weight[0] and (with ii) agg.conv1 are one conv3x3_fanout launch where num * ht * wd reaches
    conv3.MIN_FANOUT_PIXELS, and delta[2] and weight[2] one head_pair launch that writes (1,num,ht,wd,2) directly where it
    reaches heads.MIN_PAIR_PIXELS; below them the separate launches, with the same bits.  `fanout_calls` and `pair_calls`
    count the two.
    coords1 (keyword of the call): a (1,num,ht,wd,2) float32 tensor, the factor graph's coordinates.  The second and third
    results are then `coords1 + delta.to(dtype=torch.float)` and `weight.to(dtype=torch.float)`, float32, what
    FactorGraph.update and update_lowmem keep: written by head_pair's launch on the fused route, formed with torch from the
    half results on every other route, the module's own included."""

    def __init__(self, update, gru_convs=False, defer_upmask=False):
        _check_stack(getattr(update, "corr_encoder", None), "corr_encoder", conv1.eligible, "Conv2d(1..224, 128, 1)")
        self._flow = _flow.FlowEncoder(getattr(update, "flow_encoder", None))      # raises unless shaped like the reference's
        if not conv3.eligible(update.flow_encoder[2]):
            _refuse("flow_encoder[2]", "Conv2d(128, 64, 3, padding=1) with a bias")
        _check_head_stack(getattr(update, "delta", None), "delta", "none")
        _check_head_stack(getattr(update, "weight", None), "weight", "sigmoid")
        if getattr(update, "agg", None) is None:
            _refuse("agg", "a GraphAgg")
        _check_agg(update.agg)
        self.gru = _gru.KanBiasGRU(getattr(update, "gru", None), convs=gru_convs)   # raises unless KAN_bias_GRU(128, 320)
        self.module = update
        self.defer_upmask = bool(defer_upmask)
        self._packs = PackCache()
        self._upmask_conv = upmask.parse(update.agg.upmask)
        self.fused_calls = 0
        self.fanout_calls = 0
        self.pair_calls = 0
        self.module_calls = 0

    def upmask_packed(self):
        """(wpack, bias_h) of agg.upmask for upmask.upsample_from_net_, cached."""
        return self._packs.of(self._upmask_conv, upmask.pack_upmask)

    def _fused(self, net, inp, corr, flow, ii, coords1=None):
        ts = [net, inp, corr] + ([] if flow is None else [flow])
        if not all(isinstance(t, torch.Tensor) and t.is_cuda and t.dim() == 5 and t.dtype in FLOAT_OR_HALF for t in ts):
            return False
        if ii is not None and not (isinstance(ii, torch.Tensor) and ii.dim() == 1 and ii.shape[0] == net.shape[1]):
            return False
        dev = net.device
        shape = (1,) + tuple(net.shape[1:2]) + tuple(net.shape[3:])
        if any(t.device != dev or (t.shape[0], t.shape[1]) + tuple(t.shape[3:]) != shape for t in ts):
            return False
        if net.shape[1] == 0 or net.shape[3] * net.shape[4] == 0:
            return False
        if coords1 is not None:      # the factor graph's coordinates: (1, num, ht, wd, 2) float32 on the same device
            if not (isinstance(coords1, torch.Tensor) and coords1.dtype == torch.float32 and coords1.device == dev):
                return False
            if tuple(coords1.shape) != (1, net.shape[1], net.shape[3], net.shape[4], 2):
                return False
            ts = ts + [coords1]
        m = self.module
        if net.shape[2] != 128 or corr.shape[2] != m.corr_encoder[0].in_channels or (flow is not None and flow.shape[2] != 4):
            return False
        params = list(m.parameters()) + list(m.buffers())
        if any(p.device != dev or (p.is_floating_point() and p.dtype != torch.float32) for p in params):
            return False
        return fused_dtype(ts + params) == torch.float16

    def __call__(self, net, inp, corr, flow=None, ii=None, jj=None, coords1=None):
        m = self.module
        if not self._fused(net, inp, corr, flow, ii, coords1):
            self.module_calls += 1
            out = type(m).forward(m, net, inp, corr, flow, ii, jj)
            if coords1 is None:
                return out
            return (out[0], coords1 + out[1].to(dtype=torch.float), out[2].to(dtype=torch.float)) + tuple(out[3:])
        _, num, _, ht, wd = net.shape
        packs = self._packs
        c3, hd = conv3.pack_conv3, heads.pack_head
        if flow is None:
            flow = torch.zeros((1, num, 4, ht, wd), device=net.device)
        net, inp, corr, flow = (t.reshape(num, -1, ht, wd).contiguous() for t in (net, inp, corr, flow))

        ce = m.corr_encoder
        corr = conv1.conv1x1(corr, *packs.of(ce[0], conv1.pack_conv1), cin=ce[0].in_channels, relu=True)
        corr = conv3.conv3x3(corr, *packs.of(ce[2], c3), relu=True)
        flow = _flow.flow_conv7_relu(flow, *self._flow.packed())
        flow = conv3.conv3x3(flow, *packs.of(m.flow_encoder[2], c3), relu=True)
        net = self.gru(net, inp, corr, flow)

        # the trunk behind the GRU: delta[0], weight[0] and (with ii) agg.conv1 read the same x, in one launch where that
        # was measured to win, else in one launch each.  Same bits either way.
        x = net.contiguous()
        trunk = [m.delta[0], m.weight[0]] + ([] if ii is None else [m.agg.conv1])
        if num * ht * wd >= conv3.MIN_FANOUT_PIXELS:
            feats = conv3.conv3x3_fanout(x, [packs.of(c, c3) for c in trunk], relu=True)
            self.fanout_calls += 1
        else:
            feats = [conv3.conv3x3(x, *packs.of(c, c3), relu=True) for c in trunk]
        d, w = feats[0], feats[1]
        if num * ht * wd >= heads.MIN_PAIR_PIXELS:
            coords = None if coords1 is None else coords1.contiguous()
            delta, weight = heads.head_pair(d, w, packs.of(m.delta[2], hd), packs.of(m.weight[2], hd), coords=coords)
            self.pair_calls += 1
        else:
            def to_edges(t):       # the reference's view / permute / [..., :2] / contiguous
                return t.view(1, num, -1, ht, wd).permute(0, 1, 3, 4, 2)[..., :2].contiguous()
            delta = to_edges(heads.head_conv3x3(d, *packs.of(m.delta[2], hd), act="none"))
            weight = to_edges(heads.head_conv3x3(w, *packs.of(m.weight[2], hd), act="sigmoid"))
            if coords1 is not None:      # the factor graph's own two expressions
                delta, weight = coords1 + delta.to(dtype=torch.float), weight.to(dtype=torch.float)
        net = net.view(1, num, -1, ht, wd)
        self.fused_calls += 1
        if ii is None:
            return net, delta, weight

        agg = m.agg
        uniq, ix = torch.unique(ii.to(net.device), return_inverse=True)
        U = uniq.shape[0]
        a = aggregate.scatter_mean(feats[2].view(1, num, 128, ht, wd), ix.contiguous(), dim=1, dim_size=U)
        a = conv3.conv3x3(a.view(U, 128, ht, wd), *packs.of(agg.conv2, c3), relu=True)
        eta = heads.head_conv3x3(a, *packs.of(agg.eta[0], hd), act="softplus").view(1, U, ht, wd)
        if self.defer_upmask:
            return net, delta, weight, .01 * eta, a.view(1, U, 128, ht, wd)
        mask = upmask.upmask_conv1x1(a, *self.upmask_packed())
        return net, delta, weight, .01 * eta, mask.view(1, U, 576, ht, wd)


def install(update, gru_convs=False, defer_upmask=False):
    """Bind an UpdateOperator as `update.forward`, an instance attribute: parameters, submodules and state_dict keys are
    unchanged, and nothing is bound on a submodule.  Returns the wrapper; a second call returns the first wrapper with
    the flags set as given.  A module that is not shaped like the reference's raises RuntimeError and binds nothing, and
    so does a module whose forward already carries another wrapper."""
    cur = installed(update, UpdateOperator, "update.install")
    if cur is not None:
        cur.gru.convs = bool(gru_convs)
        cur.defer_upmask = bool(defer_upmask)
        return cur
    return bind(update, "forward", UpdateOperator, lambda _: UpdateOperator(update, gru_convs=gru_convs, defer_upmask=defer_upmask))


def uninstall(update):
    """Undo `install`: the class's forward is used again."""
    unbind(update, "forward", UpdateOperator)
