"""A stand-in shaped like the reference's UpdateModule with its GraphAgg (droid_slam/droid_net.py), written for the tests of
lgu_slam_amd.update: the same attribute names, Sequential layouts and state_dict keys, the same data flow in forward.

    corr -> corr_encoder, flow -> flow_encoder (None: zeros), net = gru(net, inp, corr, flow),
    delta = delta(net), weight = weight(net), each viewed per edge, channel-last, [..., :2];
    with ii: eta, upmask = agg(net, ii): relu(conv1), the mean over the edges of each distinct ii, relu(conv2), then
    0.01 * softplus(eta conv) per frame and the 576-plane mask.

The GRU is tests/kangru_restatement.RefGRU, GradientClip's forward is conv3_restatement.Identity, and the mean over the
edges is written with index_add_ (the reference takes it from torch_scatter).  CPU or GPU, any dtype torch serves.
"""
import torch

from tests import conv3_restatement as R
from tests import kangru_restatement as RK


def segment_mean(src, ix, size):
    """The mean over dim 1 of src (b, num, ...) by segment ix (num,), as (b, size, ...) of src's dtype; summed in float32."""
    out = torch.zeros((src.shape[0], size) + tuple(src.shape[2:]), dtype=torch.float32, device=src.device)
    out.index_add_(1, ix, src.float())
    count = torch.bincount(ix, minlength=size).clamp(min=1).to(torch.float32)
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


def make_update(seed):
    """An Update with seeded default initialisation of the convolutions and kangru_restatement's trained-like GRU weights
    (CPU, float32)."""
    torch.manual_seed(seed)
    u = Update()
    RK.set_weights(u.gru, seed + 1000)
    return u


def make_inputs(seed, num, ht, wd, batch=1):
    """net, inp, corr, flow (CPU, float32) as the update operator sees them: kangru_restatement's net and inp, the planar
    correlation features of conv3_restatement.make_input's recipe, and a small flow / residual tensor."""
    net, inp, _, _ = RK.make_inputs(seed, batch * num, ht, wd)
    corr = R.make_input(seed + 1, batch * num, ht, wd, C=R.COR_PLANES)
    g = torch.Generator().manual_seed(seed + 2)
    flow = torch.randn((batch * num, 4, ht, wd), generator=g) * 3.0

    def edges(t):
        return t.view(batch, num, -1, ht, wd).contiguous()
    return edges(net), edges(inp), edges(corr), edges(flow)
