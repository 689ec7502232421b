"""numpy restatement of the proximity-edge selection (include/lgu_corr.h, "proximity edges of the factor graph"), the
authority for ties and for device-computed distances, where no fixture from the reference can exist.  The fixtures
tests/golden/proximity_*.npz (the reference's own method, distinct distances) hold it to the reference.

Window: rows i in [t0, t), columns j in [t1, t), one distance per cell at f = (i - t0) * (t - t1) + (j - t1).
"""
import numpy as np


def check(t, t0, t1, rad, nms):
    """The argument rules; returns n."""
    if not 0 <= t1 <= t0 <= t:
        raise ValueError("need 0 <= t1 <= t0 <= t")
    if rad < 0 or nms < 0:
        raise ValueError("rad and nms must be >= 0")
    if t1 > max(t0 - rad - 1, 0):
        raise ValueError("need t1 <= max(t0 - rad - 1, 0)")
    return (t - t0) * (t - t1)


def radius(i, j, nms):
    return max(min(abs(int(i) - int(j)) - 2, nms), 0)


def prefix_edges(t, t0, rad, stereo):
    es = []
    for i in range(t0, t):
        if stereo:
            es.append((i, i))
        for j in range(max(i - rad - 1, 0), i):
            es += [(i, j), (j, i)]
    return es


def prefix_len(t, t0, rad, stereo):
    return sum((1 if stereo else 0) + 2 * min(rad + 1, i) for i in range(t0, t))


def capacity(t, t0, rad, stereo, max_factors):
    return max(prefix_len(t, t0, rad, stereo), max_factors + 2)


def proximity_edges(d, t, known_ii, known_jj, t0=0, t1=0, rad=2, nms=2, thresh=16.0, max_factors=-1, stereo=False):
    """(ii, jj) int64 arrays.  d: n float32 values (not modified)."""
    n = check(t, t0, t1, rad, nms)
    d = np.asarray(d, np.float32).reshape(-1)
    assert d.shape[0] == n
    R, W = t - t0, t - t1
    dead = np.zeros((R, W), bool)

    def kill_diamond(i, j):
        r = radius(i, j, nms)
        for i1 in range(max(i - r, t0), min(i + r, t - 1) + 1):
            rem = r - abs(i1 - i)
            lo, hi = max(j - rem, t1), min(j + rem, t - 1)
            if lo <= hi:
                dead[i1 - t0, lo - t1:hi - t1 + 1] = True

    if n:
        I = np.arange(t0, t)[:, None]
        J = np.arange(t1, t)[None, :]
        D = d.reshape(R, W)
        dead |= (I - rad < J) | (D > 100) | np.isnan(D)
        dead |= (J >= np.maximum(I - rad - 1, 0)) & (J < I)
        if stereo:
            dead |= I == J
        for i, j in zip(np.asarray(known_ii, np.int64).tolist(), np.asarray(known_jj, np.int64).tolist()):
            if abs(i) < 2 ** 40 and abs(j) < 2 ** 40:       # farther than any diamond reaches (nms < 2^31)
                kill_diamond(i, j)
    es = prefix_edges(t, t0, rad, stereo)
    if n:
        key = np.where(d == 0, np.float32(0), d)            # -0 orders as +0; NaN cells are dead already
        for f in np.argsort(key, kind="stable").tolist():
            if not float(d[f]) <= float(thresh):
                break                                       # ascending: nothing later passes (NaNs sort last)
            if dead.flat[f]:
                continue
            if len(es) > max_factors:
                break
            i, j = t0 + f // W, t1 + f % W
            es += [(i, j), (j, i)]
            kill_diamond(i, j)
    e = np.asarray(es, np.int64).reshape(-1, 2)
    return e[:, 0].copy(), e[:, 1].copy()


def neighborhood_edges(t0, t1, r=3, stereo=False):
    """FactorGraph.add_neighborhood_factors: the pairs of [t0, t1) with c < |i - j| <= r, row-major; c = 1 if stereo."""
    c = 1 if stereo else 0
    es = [(i, j) for i in range(t0, t1) for j in range(t0, t1) if c < abs(i - j) <= r]
    e = np.asarray(es, np.int64).reshape(-1, 2)
    return e[:, 0].copy(), e[:, 1].copy()
