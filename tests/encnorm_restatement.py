"""Restatement of the instance norms folded into the encoders' convolutions (include/lgu_corr.h, lgu_encconv3x3_norm_h16
and lgu_encstats_finalize; csrc/encstats.hpp), in two parts:

1. the exact plane statistics, in numpy with Python integers: xi = h 2^24 of a finite half h is an integer, and per plane
       S1 = sum xi      LO = sum (xi^2 mod 2^40)      HI = sum (xi^2 >> 40)      BAD = number of non-finite values
2. the double lines that turn them into (mean, rstd), in numpy scalars, and the three prologues in float32 torch operations
   applied one at a time (no expression a compiler could contract):
       IN(v; mu, rho) = (float(v) - mu) * rho          relu(v) = v < 0 ? 0 : v (a NaN is kept)
       NORM      h = half(relu(IN(x)))
       RES       h = half(relu(float(y) + relu(IN(x))))
       RES_NORM  h = half(relu(IN(y) + relu(IN(x))))

The convolution that follows is tests/encconv_restatement.py unchanged: `conv_after(h, c3, c1)`.  The allowance of the
prologues against the float64 instance norm is DESIGN.md section 3.13's with L = 2: the statistics carry one fp32 rounding
each and no summation tree.  Everything is on the CPU.
"""
import numpy as np
import torch

from tests import encconv_restatement as EC
from tests import features_restatement as FR

MODES = ("norm", "res", "res_norm")
WORDS = ("S1", "LO", "HI", "BAD")
MAX_PLANE = 1 << 22
U = 2.0 ** -24
L_FOLDED = 2.0


# ---- part 1: the integer sums -----------------------------------------------------------------------------------------
def int_sums(h):
    """{S1, LO, HI, BAD} of every plane of the half tensor h (..., H, W): object arrays of Python ints of shape h.shape[:-2]."""
    a = h.detach().cpu().numpy() if isinstance(h, torch.Tensor) else np.asarray(h)
    assert a.dtype == np.float16
    lead = a.shape[:-2]
    a = a.reshape(-1, a.shape[-2] * a.shape[-1])
    fin = np.isfinite(a)
    scaled = np.where(fin, a.astype(np.float64), 0.0) * 2.0 ** 24
    assert bool(np.all(scaled == np.rint(scaled))) and bool(np.all(np.abs(scaled) < 2.0 ** 40))   # xi is an integer below 2^40
    xi = scaled.astype(np.int64).astype(object)
    sq = xi * xi
    out = {"S1": xi.sum(-1), "LO": (sq % (1 << 40)).sum(-1), "HI": (sq >> 40).sum(-1), "BAD": (~fin).sum(-1).astype(object)}
    return {k: np.asarray(v, dtype=object).reshape(lead) for k, v in out.items()}


def decompose(h):
    """(m, k) with |h| = m 2^(k - 24), 0 <= m < 2048, 0 <= k <= 29, of finite half values (int64 arrays)."""
    bits = np.asarray(h, dtype=np.float16).view(np.uint16).astype(np.int64)
    e, f = (bits >> 10) & 31, bits & 1023
    assert bool(np.all(e < 31))
    return np.where(e > 0, f | 1024, f), np.where(e > 0, e - 1, 0)


def words_of(acc):
    """The four words of every plane of a device accumulator (N,C,R,4) int64, summed over the R slots as Python ints."""
    a = acc.detach().cpu().numpy().astype(object).sum(2)
    return {k: a[..., i] for i, k in enumerate(WORDS)}


def acc_from(sums, R, device="cpu"):
    """An accumulator tensor (N,C,R,4) int64 holding the sums of `int_sums`, spread over the R slots (slot r > 0 takes
    value // (r + 2), slot 0 the rest): the result must not depend on how a plane's sum is split."""
    shape = sums["S1"].shape
    out = np.zeros(shape + (R, 4), dtype=np.int64)
    for i, k in enumerate(WORDS):
        for idx in np.ndindex(*shape):
            rest = int(sums[k][idx])
            for r in range(1, R):
                part = rest // (r + 2)
                out[idx + (r, i)] = part
                rest -= part
            out[idx + (0, i)] = rest
    return torch.from_numpy(out).to(device)


# ---- part 2: (mean, rstd) and the prologues -------------------------------------------------------------------------------
def mean_rstd(S1, LO, HI, BAD, cnt, eps=1e-5):
    """(mean, rstd) as numpy float32 scalars: the lines of include/lgu_corr.h, each step rounded once in double."""
    a = np.float64(int(S1))
    q = np.float64(int(HI)) * np.float64(2.0 ** 40) + np.float64(int(LO))
    n = np.float64(cnt)
    mean = np.float32(a / (n * np.float64(2.0 ** 24)))
    sq = a * a
    d = q - sq / n
    var = d / (n * np.float64(2.0 ** 48))
    var = var if var > 0.0 else np.float64(0.0)
    with np.errstate(divide="ignore"):                   # a constant plane with eps = 0: rstd = inf, as on the device
        rstd = np.float32(np.float64(1.0) / np.sqrt(var + np.float64(np.float32(eps))))
    if int(BAD) != 0:
        return np.float32(np.nan), np.float32(np.nan)
    return mean, rstd


def mean_rstd_table(sums, cnt, eps=1e-5):
    """(..., 2) float32 tensor {mean, rstd} of every plane of `int_sums` / `words_of`."""
    shape = sums["S1"].shape
    out = np.zeros(shape + (2,), dtype=np.float32)
    for idx in np.ndindex(*shape):
        out[idx] = mean_rstd(sums["S1"][idx], sums["LO"][idx], sums["HI"][idx], sums["BAD"][idx], cnt, eps)
    return torch.from_numpy(out)


def _relu(t):
    return torch.where(t < 0, torch.zeros((), dtype=t.dtype), t)       # a NaN compares false and is kept


def _in(v, mr):
    mu, rho = mr[..., 0, None, None], mr[..., 1, None, None]
    d = v.float() - mu
    return d * rho


def prologue(mode, x, mr_x, y=None, mr_y=None):
    """The half tensor h the convolution sees: x, y half (N,C,H,W) on the CPU, mr_x, mr_y (N,C,2) float32 {mean, rstd}."""
    t = _relu(_in(x, mr_x))
    if mode == "res":
        t = y.float() + t
        t = _relu(t)
    elif mode == "res_norm":
        t = _in(y, mr_y) + t
        t = _relu(t)
    else:
        assert mode == "norm"
    return t.to(torch.float16)


def conv_after(h, c3, c1=None):
    """(s64, S, r64, Sr) of the layer on the staged tensor h: tests/encconv_restatement.py, unchanged."""
    return EC.conv(h, c3, c1)


# ---- the allowance of a prologue against the float64 instance norm ----------------------------------------------------
def reference(mode, x, y=None, eps=1e-5):
    """(value, E) per element for planes x, y (planes, hw) as stored: tests/features_restatement.reference with L = 2 in E
    (mode "norm" is its mode 0, "res" 1, "res_norm" 2)."""
    k = {"norm": 0, "res": 1, "res_norm": 2}[mode]
    ref, E = FR.reference(k, x, y, eps)
    L = np.log2(x.shape[-1]) + 4
    _, ka = FR._plane_stats(x.double(), eps)
    E = E - FR.U * (L - L_FOLDED) * ka
    if mode == "res_norm":
        _, kb = FR._plane_stats(y.double(), eps)
        E = E - FR.U * (L - L_FOLDED) * kb
    return ref, E
