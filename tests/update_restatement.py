"""A stand-in shaped like the reference's UpdateModule with its GraphAgg (droid_slam/droid_net.py), written for the tests of
lgu_slam_amd.update: the same attribute names, Sequential layouts and state_dict keys, the same data flow in forward.

    corr -> corr_encoder, flow -> flow_encoder (None: zeros), net = gru(net, inp, corr, flow),
    delta = delta(net), weight = weight(net), each viewed per edge, channel-last, [..., :2];
    with ii: eta, upmask = agg(net, ii): relu(conv1), the mean over the edges of each distinct ii, relu(conv2), then
    0.01 * softplus(eta conv) per frame and the 576-plane mask.

The GRU is tests/kangru_restatement.RefGRU, GradientClip's forward is conv3_restatement.Identity, and the mean over the
edges is written with index_add_ (the reference takes it from torch_scatter).  CPU or GPU, any dtype torch serves.

The stand-in is pinned by tests/golden/update_*.npz: the reference's own UpdateModule, loaded with this module's state_dict
and run in float64 on the CPU by tools/gen_update_golden.py on the CASES below, recorded with `record` (the same hooks on
both modules).  tests/test_update.py holds the stand-in in float64 to every recorded stage and result.
"""
import hashlib

import numpy as np
import torch

from tests import conv3_restatement as R
from tests import kangru_restatement as RK


def segment_mean(src, ix, size):
    """The mean over dim 1 of src (b, num, ...) by segment ix (num,), as (b, size, ...) of src's dtype; summed in float32,
    a float64 src in float64 (a float32 sum there put the float64 forward 2^-24 of the summed terms away from the
    reference's, more than the fixture's own rounding behind agg.conv2)."""
    acc = torch.promote_types(src.dtype, torch.float32)
    out = torch.zeros((src.shape[0], size) + tuple(src.shape[2:]), dtype=acc, device=src.device)
    out.index_add_(1, ix, src.to(acc))
    count = torch.bincount(ix, minlength=size).clamp(min=1).to(acc)
    return (out / count.view(1, -1, *([1] * (src.dim() - 2)))).to(src.dtype)


class GraphAgg(torch.nn.Module):
    def __init__(self):
        super().__init__()
        nn = torch.nn
        self.conv1 = nn.Conv2d(128, 128, 3, padding=1)
        self.conv2 = nn.Conv2d(128, 128, 3, padding=1)
        self.relu = nn.ReLU(inplace=True)
        self.eta = nn.Sequential(nn.Conv2d(128, 1, 3, padding=1), R.Identity(), nn.Softplus())
        self.upmask = nn.Sequential(nn.Conv2d(128, 8 * 8 * 9, 1, padding=0))

    def forward(self, net, ii):
        batch, num, ch, ht, wd = net.shape
        net = net.view(batch * num, ch, ht, wd)
        uniq, ix = torch.unique(ii, return_inverse=True)
        net = self.relu(self.conv1(net))
        net = segment_mean(net.view(batch, num, 128, ht, wd), ix, uniq.shape[0])
        net = self.relu(self.conv2(net.view(-1, 128, ht, wd)))
        eta = self.eta(net).view(batch, -1, ht, wd)
        upmask = self.upmask(net).view(batch, -1, 8 * 8 * 9, ht, wd)
        return .01 * eta, upmask


class Update(torch.nn.Module):
    def __init__(self):
        super().__init__()
        nn = torch.nn
        self.corr_encoder = R._stack("corr_encoder")
        self.flow_encoder = nn.Sequential(nn.Conv2d(4, 128, 7, padding=3), nn.ReLU(inplace=True), nn.Conv2d(128, 64, 3, padding=1),
                                          nn.ReLU(inplace=True))
        self.weight = R._stack("weight")
        self.delta = R._stack("delta")
        self.gru = RK.RefGRU()
        self.agg = GraphAgg()

    def forward(self, net, inp, corr, flow=None, ii=None, jj=None):
        batch, num, ch, ht, wd = net.shape
        if flow is None:
            flow = torch.zeros(batch, num, 4, ht, wd, device=net.device)
        out = (batch, num, -1, ht, wd)
        net, inp, corr, flow = (t.view(batch * num, -1, ht, wd) for t in (net, inp, corr, flow))
        corr = self.corr_encoder(corr)
        flow = self.flow_encoder(flow)
        net = self.gru(net, inp, corr, flow)
        delta = self.delta(net).view(*out).permute(0, 1, 3, 4, 2)[..., :2].contiguous()
        weight = self.weight(net).view(*out).permute(0, 1, 3, 4, 2)[..., :2].contiguous()
        net = net.view(*out)
        if ii is None:
            return net, delta, weight
        eta, upmask = self.agg(net, ii.to(net.device))
        return net, delta, weight, eta, upmask


def make_update(seed, portable=False):
    """An Update with seeded default initialisation of the convolutions and kangru_restatement's trained-like GRU weights
    (CPU, float32).  portable: the convolutions outside the GRU are drawn once more with numpy's RandomState at the default
    initialisation's scale (uniform in +-fan_in^-1/2), which gives the same bits on every machine; torch's own CPU
    generator gives other draws where the CPU lacks AVX2, so what a stored hash pins must not come from it."""
    torch.manual_seed(seed)
    u = Update()
    RK.set_weights(u.gru, seed + 1000)
    if portable:
        rs = np.random.RandomState(seed + 2000)
        with torch.no_grad():
            for name, mod in sorted(u.named_modules()):
                if isinstance(mod, torch.nn.Conv2d) and not name.startswith("gru."):
                    k = float(mod.weight[0].numel()) ** -0.5
                    for p in (mod.weight, mod.bias):
                        p.copy_(torch.from_numpy(rs.uniform(-k, k, tuple(p.shape)).astype(np.float32)))
    return u


def make_inputs(seed, num, ht, wd, batch=1, portable=False):
    """net, inp, corr, flow (CPU, float32) as the update operator sees them: kangru_restatement's net and inp, the planar
    correlation features of conv3_restatement.make_input's recipe, and a small flow / residual tensor.  portable: corr
    and flow follow the same recipes with numpy's RandomState (see make_update)."""
    net, inp, _, _ = RK.make_inputs(seed, batch * num, ht, wd)
    if portable:
        rs = np.random.RandomState(seed + 1)
        corr = 2.0 * rs.standard_normal((batch * num, R.COR_PLANES, ht, wd))
        corr[rs.random_sample(corr.shape) < 0.3] = 0.0
        corr = torch.from_numpy(corr.astype(np.float32))
        flow = torch.from_numpy((3.0 * rs.standard_normal((batch * num, 4, ht, wd))).astype(np.float32))
    else:
        corr = R.make_input(seed + 1, batch * num, ht, wd, C=R.COR_PLANES)
        g = torch.Generator().manual_seed(seed + 2)
        flow = torch.randn((batch * num, 4, ht, wd), generator=g) * 3.0

    def edges(t):
        return t.view(batch, num, -1, ht, wd).contiguous()
    return edges(net), edges(inp), edges(corr), edges(flow)


# ---- the fixture cases (tests/golden/update_*.npz, tools/gen_update_golden.py) ----------------------------------------
# update_segments: unequal segments whose first appearances are unsorted (unique = [2, 4, 7], sizes 1, 2, 2).
# update_one_frame: one segment of three; 33 columns cross a 32-column tile and 5 rows a 4-row tile of the 3x3 kernels;
#   flow=None takes the zero-flow branch.
# update_distinct: every edge its own frame, unsorted, one pixel.
CASES = {"update_segments": dict(seed=61, num=5, ht=6, wd=9, ii=[4, 4, 7, 2, 7], flow=True),
         "update_one_frame": dict(seed=62, num=3, ht=5, wd=33, ii=[6, 6, 6], flow=False),
         "update_distinct": dict(seed=63, num=2, ht=1, wd=1, ii=[1, 0], flow=True)}
STAGES = ("corr_feat", "flow_feat", "gru", "agg1", "mean", "agg2")       # in the order the forward reaches them
RESULTS = ("net", "delta", "weight", "eta", "upmask")
AFTER_MEAN = ("mean", "agg2", "eta", "upmask")                           # what lies behind the mean over the edges


def make_case(name):
    """(module, (net, inp, corr, flow or None), ii) of a fixture case, float32 on the CPU: make_update(seed) and
    make_inputs(seed + 1, ...), the pairing of seeds the GPU tests use, both with portable draws (numpy's RandomState and
    exact operations only: the same bits on every machine, so the sha256 in the fixture pins them wherever the tests run)."""
    cfg = CASES[name]
    u = make_update(cfg["seed"], portable=True).eval()
    net, inp, corr, flow = make_inputs(cfg["seed"] + 1, cfg["num"], cfg["ht"], cfg["wd"], portable=True)
    return u, (net, inp, corr, flow if cfg["flow"] else None), torch.tensor(cfg["ii"])


def case_sha256(u, ins, ii):
    """Pins the inputs that are given, ii and every parameter and buffer (state_dict order)."""
    hsh = hashlib.sha256()
    for t in [t for t in ins if t is not None] + [ii] + [v for _, v in sorted(u.state_dict().items())]:
        hsh.update(np.ascontiguousarray(t.detach().cpu().numpy()).tobytes())
    return hsh.hexdigest()


def record(u):
    """Forward hooks on a module with the reference UpdateModule's attribute names (the stand-in or the reference's own):
    returns (rec, handles).  After a forward rec holds STAGES: the outputs of corr_encoder, flow_encoder and gru, what
    agg.relu returned at its first and second call (agg.conv1 and agg.conv2 behind their ReLU) and the input of agg.conv2
    (the per-frame mean)."""
    rec, handles = {"relu": []}, []

    def keep(key):
        def fn(mod, args, res):
            rec[key] = res.detach().clone()
        return fn
    for attr, key in (("corr_encoder", "corr_feat"), ("flow_encoder", "flow_feat"), ("gru", "gru")):
        handles.append(getattr(u, attr).register_forward_hook(keep(key)))
    handles.append(u.agg.relu.register_forward_hook(lambda mod, args, res: rec["relu"].append(res.detach().clone())))
    handles.append(u.agg.conv2.register_forward_pre_hook(lambda mod, args: rec.__setitem__("mean", args[0].detach().clone())))
    return rec, handles


def run_recorded(u, ins, ii):
    """{stage or result: tensor} of one forward of `u` under no_grad, the hooks removed afterwards.  The forward runs with
    net's dtype as torch's default dtype, so that the zeros the forward makes for flow=None are of the module's dtype (in
    float64 the module's own zero-flow branch runs, not a zero tensor handed in)."""
    rec, handles = record(u)
    default = torch.get_default_dtype()
    try:
        torch.set_default_dtype(ins[0].dtype)
        with torch.no_grad():
            out = u(*ins, ii)
    finally:
        torch.set_default_dtype(default)
        for h in handles:
            h.remove()
    relu = rec.pop("relu")
    assert len(relu) == 2 and len(out) == len(RESULTS), (len(relu), len(out))
    rec["agg1"], rec["agg2"] = relu
    rec.update(zip(RESULTS, out))
    assert set(rec) == set(STAGES + RESULTS), sorted(rec)
    return rec
