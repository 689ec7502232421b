"""numpy restatements of csrc/aggregate.hip in its stated order, float32 (the kernels' arithmetic) and float64.

scatter_mean32(src, index, M): src (outer,n,inner) float32 / float16, the fp32 sum over the j with index[j] == m in
    ascending j, one fp32 division by the count, rounded once to src's dtype; 0 for an empty segment; an index outside
    [0, M) is skipped.  scatter_mean64 does the same sums in float64 (result float64).
cvx_upsample32(data, mask, half_weights): data (B,ht,wd), mask (B,576,ht,wd) values -> (B,8ht,8wd) float32, in the
    order m = max_k x_k, e_k = exp(x_k - m), s = sum e_k, w_k = e_k / s [, w_k rounded to half], out = sum w_k d_k
    (ascending k, every step rounded to float32).  cvx_upsample64 follows the same order in float64 (weights rounded to
    half directly from float64 in the half-weight mode).  neighbour_max_abs(data) is max_k |d_k| per coarse pixel,
    the scale of the stated bound.
"""
import numpy as np


def _segments(index, n, M):
    index = np.asarray(index, dtype=np.int64).reshape(-1)
    assert index.shape[0] == n
    return [(j, int(index[j])) for j in range(n) if 0 <= index[j] < M]


def scatter_mean32(src, index, M):
    src = np.asarray(src)
    outer, n, inner = src.shape
    acc = np.zeros((outer, M, inner), dtype=np.float32)
    cnt = np.zeros(M, dtype=np.int64)
    for j, m in _segments(index, n, M):
        acc[:, m] = acc[:, m] + src[:, j].astype(np.float32)
        cnt[m] += 1
    c = np.maximum(cnt, 1).astype(np.float32)[None, :, None]
    out = np.where(cnt[None, :, None] > 0, acc / c, np.float32(0)).astype(np.float32)
    return out.astype(src.dtype)


def scatter_mean64(src, index, M):
    src = np.asarray(src)
    outer, n, inner = src.shape
    acc = np.zeros((outer, M, inner), dtype=np.float64)
    cnt = np.zeros(M, dtype=np.int64)
    for j, m in _segments(index, n, M):
        acc[:, m] += src[:, j].astype(np.float64)
        cnt[m] += 1
    return np.where(cnt[None, :, None] > 0, acc / np.maximum(cnt, 1)[None, :, None], 0.0)


def _neighbours(data, dt):
    """d_k (B,9,ht,wd): the 3x3 neighbourhood, k = ky*3 + kx, zero outside the frame (F.unfold(padding=1))."""
    B, ht, wd = data.shape
    dp = np.pad(np.asarray(data, dtype=dt), ((0, 0), (1, 1), (1, 1)))
    return np.stack([dp[:, ky:ky + ht, kx:kx + wd] for ky in range(3) for kx in range(3)], 1)


def neighbour_max_abs(data):
    return np.abs(_neighbours(data, np.float64)).max(1)


def _cvx(data, mask, half_weights, dt):
    data = np.asarray(data)
    B, ht, wd = data.shape
    x = np.asarray(mask, dtype=np.float64 if dt == np.float64 else np.float32).astype(dt).reshape(B, 9, 8, 8, ht, wd)
    m = x[:, 0]
    for k in range(1, 9):
        m = np.where(x[:, k] > m, x[:, k], m)
    e = np.exp(x - m[:, None]).astype(dt)
    s = e[:, 0]
    for k in range(1, 9):
        s = s + e[:, k]
    w = (e / s[:, None]).astype(dt)
    if half_weights:
        w = w.astype(np.float16).astype(dt)
    d = _neighbours(data, dt)[:, :, None, None]           # (B,9,1,1,ht,wd)
    acc = w[:, 0] * d[:, 0]
    for k in range(1, 9):
        acc = acc + w[:, k] * d[:, k]
    # (B,a,b,ht,wd) -> (B,ht,a,wd,b) -> output pixel (8y+a, 8x+b)
    return acc.transpose(0, 3, 1, 4, 2).reshape(B, 8 * ht, 8 * wd).astype(dt)


def cvx_upsample32(data, mask, half_weights=False):
    return _cvx(data, mask, half_weights, np.float32)


def cvx_upsample64(data, mask, half_weights=False):
    return _cvx(data, mask, half_weights, np.float64)


def upsample_bound(data):
    """Per output (B,8ht,8wd): max_k |d_k| of its coarse pixel, repeated over the 8x8 sub-pixels."""
    return np.repeat(np.repeat(neighbour_max_abs(data), 8, 1), 8, 2)
