"""Op-for-op torch restatement of LGU-SLAM's KAN-bias GRU forward (reference droid_slam/modules/gru_kanBias.py with the
KANLinear heads of modules/kan.py), written from the maths, and the seeded inputs and weights that
tools/gen_kangru_golden.py and the tests share.

    inp      = cat(inputs)                       (E, 320, H, W)
    net_inp  = cat(net, inp)                     (E, 448, H, W)
    glo      = mean_p( sigmoid(w(net)) * net )   (E, 128)
    k_h      = KAN_h(glo),  KAN(x) = silu(x) Wbᵀ + B(x) (Ws ⊙ scaler)ᵀ
    z, r     = sigmoid(conv_z(net_inp) + k_z), sigmoid(conv_r(net_inp) + k_r)
    q        = tanh(conv_q(cat(r * net, inp)) + k_q)
    out      = (1 - z) * net + z * q

B(x): per input feature its 10 knots g_0..g_9 (the `grid` buffer row); order 0 is the half-open indicator
[g_j <= x < g_{j+1}] in x's dtype, then for k = 1..3
    B_j^k = (x - g_j) / (g_{j+k} - g_j) * B_j^{k-1} + (g_{j+k+1} - x) / (g_{j+k+1} - g_{j+1}) * B_{j+1}^{k-1}
evaluated as written (left to right), giving 6 bases per feature.  Runs on CPU or GPU, with autocast on or off: the
same torch calls as the reference, so autocast rounds where it rounds there.
"""
import hashlib

import numpy as np
import torch
import torch.nn.functional as F

C, CIN, NKNOT, NB = 128, 448, 10, 6
HEADS = ("kanz_glo", "kanr_glo", "kanq_glo")


def bases(x, grid):
    """(N, 128, 6) cubic B-spline bases of x (N, 128) on grid (128, 10)."""
    xe = x.unsqueeze(-1)
    b = ((xe >= grid[:, :-1]) & (xe < grid[:, 1:])).to(x.dtype)
    for k in range(1, 4):
        lo, hi = grid[:, :-(k + 1)], grid[:, k + 1:]
        left = (xe - lo) / (grid[:, k:-1] - lo) * b[:, :, :-1]
        right = (hi - xe) / (hi - grid[:, 1:-k]) * b[:, :, 1:]
        b = left + right
    return b.contiguous()


def kan(x, head):
    """KANLinear(128, 128, grid_size=3, spline_order=3) of x (N, 128): base GEMM + spline GEMM, added."""
    base = F.linear(F.silu(x), head.base_weight)
    scaled = head.spline_weight * head.spline_scaler.unsqueeze(-1)
    spline = F.linear(bases(x, head.grid).view(x.size(0), -1), scaled.view(head.out_features, -1))
    return base + spline


def forward(m, net, *inputs, parts=False):
    """The GRU forward of module `m` (the reference's attribute names); parts=True also returns the intermediates."""
    inp = torch.cat(inputs, dim=1)
    net_inp = torch.cat([net, inp], dim=1)
    E, c, h, w = net.shape
    gate = torch.sigmoid(m.w(net)) * net
    glo = gate.view(E, c, h * w).mean(-1).view(E, c)
    ks = [kan(glo, getattr(m, n)) for n in HEADS]
    kz, kr, kq = (k.view(E, c, 1, 1) for k in ks)
    cz, cr = m.convz(net_inp), m.convr(net_inp)
    z = torch.sigmoid(cz + kz)
    r = torch.sigmoid(cr + kr)
    cq = m.convq(torch.cat([r * net, inp], dim=1))
    q = torch.tanh(cq + kq)
    out = (1 - z) * net + z * q
    if not parts:
        return out
    return out, dict(gate=gate, glo=glo, kz=ks[0], kr=ks[1], kq=ks[2], cz=cz, cr=cr, cq=cq, z=z, r=r, q=q)


def gates(cz, cr, kz, kr, net):
    """z and r * net as the reference composes them, given the conv outputs and the (E, 128) biases."""
    E = net.shape[0]
    z = torch.sigmoid(cz + kz.view(E, C, 1, 1))
    r = torch.sigmoid(cr + kr.view(E, C, 1, 1))
    return z, r * net


def blend(cq, kq, z, net):
    q = torch.tanh(cq + kq.view(net.shape[0], C, 1, 1))
    return (1 - z) * net + z * q


class KanHead(torch.nn.Module):
    """The reference KANLinear(128, 128, grid_size=3) as far as its forward reads it (same attributes and state_dict
    keys); its parameters are set by `set_weights`, not by the reference's lstsq init."""

    def __init__(self):
        super().__init__()
        self.in_features = self.out_features = C
        self.grid_size, self.spline_order = 3, 3
        self.enable_standalone_scale_spline = True
        self.base_activation = torch.nn.SiLU()
        self.register_buffer("grid", (torch.arange(-3, 7) * (2 / 3) - 1).expand(C, -1).contiguous())
        self.base_weight = torch.nn.Parameter(torch.zeros(C, C))
        self.spline_weight = torch.nn.Parameter(torch.zeros(C, C, NB))
        self.spline_scaler = torch.nn.Parameter(torch.zeros(C, C))

    def forward(self, x):
        return kan(x, self)


class RefGRU(torch.nn.Module):
    """KAN_bias_GRU(128, 320): the reference's modules and state_dict keys, the restatement as forward."""

    def __init__(self):
        super().__init__()
        self.convz = torch.nn.Conv2d(CIN, C, 3, padding=1)
        self.convr = torch.nn.Conv2d(CIN, C, 3, padding=1)
        self.convq = torch.nn.Conv2d(CIN, C, 3, padding=1)
        self.kanz_glo, self.kanr_glo, self.kanq_glo = KanHead(), KanHead(), KanHead()
        self.w = torch.nn.Conv2d(C, C, 1, padding=0)

    def forward(self, net, *inputs):
        return forward(self, net, *inputs)


# ---- seeded data -----------------------------------------------------------------------------------------------------
# numpy's RandomState and exact operations only (no transcendental functions, no reductions): the same bits on every
# machine, so the sha256 in the fixture pins them wherever the tests run.
def _normal(rs, shape, std):
    return torch.from_numpy((std * rs.standard_normal(shape)).astype(np.float32))


def make_inputs(seed, E, H, W):
    """net, inp, corr, flow (float32, CPU) at the scales of the update operator: net in [-0.95, 0.95] with a per-channel
    offset (so the pooled context spreads over the knots), the encoder outputs non-negative."""
    rs = np.random.RandomState(seed)
    net = (_normal(rs, (E, C, 1, 1), 0.8) + _normal(rs, (E, C, H, W), 0.4)).clamp(-0.95, 0.95)
    inp = _normal(rs, (E, 128, H, W), 1.0).clamp_min(0)
    corr = _normal(rs, (E, 128, H, W), 1.0).clamp_min(0)
    flow = _normal(rs, (E, 64, H, W), 1.0).clamp_min(0)
    return net, inp, corr, flow


def set_weights(m, seed):
    """Trained-like scales: convolutions ~ N(0, 1/fan_in), biases ~ N(0, 0.1^2), KAN weights ~ N(0, 0.3^2) and
    N(0, 1/128); the default uniform grid on [-1, 1]."""
    rs = np.random.RandomState(seed)
    with torch.no_grad():
        for name in ("convz", "convr", "convq", "w"):
            conv = getattr(m, name)
            fan = conv.weight[0].numel()
            conv.weight.copy_(_normal(rs, tuple(conv.weight.shape), fan ** -0.5))
            conv.bias.copy_(_normal(rs, tuple(conv.bias.shape), 0.1))
        for name in HEADS:
            h = getattr(m, name)
            h.base_weight.copy_(_normal(rs, tuple(h.base_weight.shape), C ** -0.5))
            h.spline_weight.copy_(_normal(rs, tuple(h.spline_weight.shape), 0.3))
            h.spline_scaler.copy_(_normal(rs, tuple(h.spline_scaler.shape), 0.3))
    return m


def nonuniform_grid(seed, glo):
    """(3, 128, 10) monotone knots, per feature: i % 5 == 0: knot 3 + (i // 5) % 4 placed exactly on glo[i % E, i];
    1: every knot above the data; 2: every knot below it; else random spacing around the data.  Built once by
    tools/gen_kangru_golden.py from the reference's glo and stored in the fixture."""
    rs = np.random.RandomState(seed)
    E = glo.shape[0]
    out = torch.empty(3, C, NKNOT, dtype=torch.float32)
    for h in range(3):
        knots = torch.from_numpy(np.cumsum(0.15 + 0.9 * rs.random_sample((C, NKNOT)), 1))
        knots = knots - knots[:, 4:6].mean(1, keepdim=True) + 0.3 * (torch.from_numpy(rs.random_sample((C, 1))) - 0.5)
        for i in range(C):
            row = knots[i].float()
            if i % 5 == 0:
                j = 3 + (i // 5) % 4
                row = row - row[j] + glo[i % E, i]
                row[j] = glo[i % E, i]
            elif i % 5 == 1:
                row = row - row[0] + 1.5
            elif i % 5 == 2:
                row = row - row[-1] - 1.5
            assert bool((row[1:] > row[:-1]).all())
            out[h, i] = row
    return out


CASES = {"kangru_uniform": dict(seed=41, E=3, H=12, W=16, grid=None),
         "kangru_nonuniform": dict(seed=42, E=3, H=12, W=16, grid=7)}


def make_case(name, grid=None):
    """(module, (net, inp, corr, flow)) of a fixture case, float32 on the CPU.  The non-uniform case takes its knots
    (3, 128, 10) from the fixture (`grid`); without them they are built from this machine's restated glo."""
    cfg = CASES[name]
    m = set_weights(RefGRU(), cfg["seed"] + 1000)
    ins = make_inputs(cfg["seed"], cfg["E"], cfg["H"], cfg["W"])
    if cfg["grid"] is not None:
        if grid is None:
            with torch.no_grad():
                _, p = forward(m, *ins, parts=True)
            grid = nonuniform_grid(cfg["grid"], p["glo"])
        with torch.no_grad():
            for h, n in enumerate(HEADS):
                getattr(m, n).grid.copy_(torch.as_tensor(grid[h]))
    return m, ins


def case_sha256(m, ins):
    """Pins the inputs and every parameter and buffer (state_dict order)."""
    hsh = hashlib.sha256()
    for t in list(ins) + [v for _, v in sorted(m.state_dict().items())]:
        hsh.update(np.ascontiguousarray(t.detach().cpu().numpy()).tobytes())
    return hsh.hexdigest()
