"""Float64 restatement of the rounding model of csrc/gruconv.hip (include/lgu_corr.h, lgu_gruconv3x3_c448_h16) and of the
KAN-bias GRU's forward around it under float16 autocast (reference droid_slam/modules/gru_kanBias.py).

    w_h = half(weight), b_h = half(bias)
    s   = b_h + sum_{c,ky,kx} x[c, y + ky - 1, x + kx - 1] * w_h[co, c, ky, kx]        (x half, zero padding)
    c   = half(s)

The sums are conv3_restatement.window_sums (shifted slices, one window position at a time, no convolution call) over the
448 channels; the allowance of one layer is conv3_restatement.allowance with TERMS = 448 * 9 + 2.  Seeded data and
weights are kangru_restatement's.  Everything is CPU float64.
"""
import torch

from tests import conv3_restatement as R3
from tests import kangru_restatement as RK

U24 = R3.U24
C, CIN = 128, 448
TERMS = CIN * 3 * 3 + 2          # 4034: the additions of the layer's sum (4032 products and the bias) and their slack
STEPS = 126
SPLITS = ([448], [128, 320], [128, 128, 128, 64])
h64 = R3.h64


def make_module(seed):
    """KAN_bias_GRU(128, 320) as kangru_restatement builds it, with its seeded trained-like weights (CPU, float32)."""
    return RK.set_weights(RK.RefGRU(), seed)


def make_inputs(seed, E, H, W):
    """(net, inp, corr, flow) of kangru_restatement.make_inputs, rounded to half."""
    return tuple(t.half() for t in RK.make_inputs(seed, E, H, W))


def split(x, chans):
    """x (E,448,H,W) cut along the channels into contiguous tensors of `chans` channels."""
    assert sum(chans) == x.shape[1]
    return [t.contiguous() for t in torch.split(x, chans, dim=1)]


def stacked(convs):
    """(weight (Cout,448,3,3), bias (Cout)) of one convolution or of several with their outputs stacked."""
    convs = [convs] if isinstance(convs, torch.nn.Module) else list(convs)
    return torch.cat([m.weight.detach() for m in convs], 0), torch.cat([m.bias.detach() for m in convs], 0)


def conv(x, weight, bias):
    """(s64, S) of the layer on a half x (E,448,H,W): s = b_h + sum x * w_h, S = |b_h| + sum |x * w_h|."""
    return R3.window_sums(h64(x), h64(weight), h64(bias), 1)


def allowance(s64, S):
    return R3.allowance(s64, S, TERMS)


def slot_source(cout):
    """For every slot [s, ct, l, j] of the pack, the (co, c, ky, kx) the header's formula puts there."""
    s, ct, lane, j = torch.meshgrid(torch.arange(STEPS), torch.arange(cout // 16), torch.arange(64), torch.arange(8), indexing="ij")
    c64, t, kc = s // 18, (s // 2) % 9, s % 2
    return 16 * ct + (lane & 15), 64 * c64 + 32 * kc + 8 * (lane >> 4) + j, t // 3, t % 3


def _half_round(value, allow):
    """The allowance after one rounding to half of a quantity known to within `allow` of `value`."""
    return allow + 2.0 ** -11 * (value.abs() + allow) + 2.0 ** -25


def forward(m, net, inp, corr, flow, kz, kr, kq):
    """(out64, bound) of the GRU's forward under float16 autocast, taking the heads' outputs kz, kr, kq (E,128) as given:
    the float64 chain on the half inputs and half-rounded weights with no rounding in between, and the bound on
    |out - out64| of an evaluation that rounds where csrc/gruconv.hip and csrc/kangru.hip round.

      c_z, c_r: each within the layer's allowance a of its s.
      v = half(c + k): a_v = round(a).   g = half(sigmoid(v)), sigmoid in fp32 (4 fp32 units), slope at most 1/4:
        a_g = round(a_v / 4) + 4 U24 g.
      rnet = half(r * net), the product of two halves exact in fp32, |net| < 1: a_rn = round(a_r).
      c_q: a_rn on the first 128 channels pushed through |w_h| of convq, counted into S and into the rounded value, plus
        the layer's own allowance (conv3_restatement.stack's rule).
      q = half(tanh(half(c_q + kq))), tanh in fp32 (4 fp32 units), slope at most 1: a_q = round(round(a_cq)) + 4 U24 |q|.
      out = half(half(half(1 - z) * net) + half(z * q)): 1 - z is exact in fp32; a_t0 = round(a_z); times net, exact,
        |net| < 1: a_t1 = round(a_t0); z * q exact, |z|, |q| <= 1: a_t2 = round(a_z + a_q + a_z a_q); the fp32 sum of two
        halves rounds once in fp32 (U24 relative), then to half: a_out = round(a_t1 + a_t2 + U24 (|out| + a_t1 + a_t2)).
    """
    E = net.shape[0]
    x = torch.cat([net, inp, corr, flow], 1)
    assert x.dtype == torch.float16 and float(net.abs().max()) < 1.0
    n64, k = h64(net), [h64(t).view(E, C, 1, 1) for t in (kz, kr, kq)]
    wzr, bzr = stacked((m.convz, m.convr))
    s, S = conv(x, wzr, bzr)
    a = allowance(s, S)
    gate, a_gate = [], []
    for i in range(2):
        v = s[:, C * i:C * (i + 1)] + k[i]
        a_v = _half_round(v, a[:, C * i:C * (i + 1)])
        gv = torch.sigmoid(v)
        gate.append(gv)
        a_gate.append(_half_round(gv, 0.25 * a_v) + 4 * U24 * gv)
    z, r = gate
    a_z, a_r = a_gate
    rnet = r * n64
    a_rn = _half_round(rnet, a_r)
    wq, bq = h64(m.convq.weight), h64(m.convq.bias)
    xq = torch.cat([rnet, h64(x[:, C:])], 1)
    sq, Sq = R3.window_sums(xq, wq, bq, 1)
    moved = R3.through(a_rn, wq[:, :C], 1)
    a_cq = moved + R3.allowance(sq, Sq + moved, TERMS) + 2.0 ** -11 * moved
    v = sq + k[2]
    q = torch.tanh(v)
    a_q = _half_round(q, _half_round(v, a_cq)) + 4 * U24 * q.abs()
    t1, t2 = (1 - z) * n64, z * q
    a_t1 = _half_round(t1, _half_round(1 - z, a_z))
    a_t2 = _half_round(t2, a_z + a_q + a_z * a_q)
    out = t1 + t2
    both = a_t1 + a_t2
    return out, _half_round(out, both + U24 * (out.abs() + both))
