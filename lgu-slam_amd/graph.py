"""Which edges the factor graph gets: `FactorGraph.add_proximity_factors` and `add_neighborhood_factors` of the
reference (droid_slam/factor_graph.py:304-383) without its per-candidate host loop, on the kernels of csrc/graphsel.hip.

    ii, jj = graph.proximity_edges(poses, disps, intrinsics, t, ii_known, jj_known, t0, t1, rad=2, nms=2, ...)
    graph.install(factor_graph)     # factor_graph.add_proximity_factors(...) now selects on the device

The window is rows i in [t0, t), columns j in [t1, t); a cell's flat index is (i - t0) * (t - t1) + (j - t1).  The
semantics are the reference's (include/lgu_corr.h states them), with two deviations: equal distances are visited in
ascending flat index (the reference's argsort leaves their order open) and a NaN distance is never selected (the
reference would accept it).

Two forms: "small" (n = (t - t0)(t - t1) <= 4096: one launch of one workgroup, keys sorted in LDS) and "sorted" (any n
<= 2^24: key build, `torch.sort` of the int64 keys, greedy pass).  Contiguous HIP device tensors only (no CPU fallback),
every argument error is raised before anything is launched, kernels go to the current stream, and one call reads the
device once: the edge count.
"""
import torch

from . import _lib
from ._host import bind, check_contiguous, check_device, check_dtype, launch, unbind
from ._host import ptr as _ptr, stream as _stream
from .geom import check_geometry, frame_distance

SMALL_MAX = 4096          # include/lgu_corr.h LGU_PROXIMITY_SMALL_MAX
MAX_CELLS = 1 << 24
MAX_T = 1 << 30
FORMS = (None, "small", "sorted")


def _int(v, name):
    if isinstance(v, bool) or not isinstance(v, int):
        try:
            iv = int(v)
        except (TypeError, ValueError):
            iv = None
        if iv is None or iv != v:
            raise RuntimeError("proximity_edges: %s must be an integer, got %r" % (name, v))
        v = iv
    return v


def window_cells(t, t0, t1, rad, nms):
    """The argument rules of the window; returns n = (t - t0) * (t - t1)."""
    if not 0 <= t1 <= t0 <= t:
        raise RuntimeError("proximity_edges: need 0 <= t1 <= t0 <= t, got t = %d, t0 = %d, t1 = %d" % (t, t0, t1))
    if rad < 0 or nms < 0:
        raise RuntimeError("proximity_edges: rad and nms must be >= 0, got rad = %d, nms = %d" % (rad, nms))
    if t1 > max(t0 - rad - 1, 0):
        raise RuntimeError("proximity_edges: need t1 <= max(t0 - rad - 1, 0) (the neighbourhood columns of row t0 must lie "
                           "inside the window), got t0 = %d, t1 = %d, rad = %d" % (t0, t1, rad))
    n = (t - t0) * (t - t1)
    if n > MAX_CELLS or t > MAX_T:
        raise _lib.UnsupportedShape("proximity_edges: the window has %d cells (t = %d); served up to 2^24 cells, t <= 2^30"
                                    % (n, t))
    return n


def prefix_len(t, t0, rad, stereo):
    """Length of the fixed prefix: per row i in [t0, t), (i, i) if stereo and two entries per j in [max(i-rad-1, 0), i)."""
    m = min(rad, t) + 1

    def below(x):      # sum over k < x of min(m, k)
        return x * (x - 1) // 2 if x <= m else m * (m - 1) // 2 + (x - m) * m
    return (t - t0 if stereo else 0) + 2 * (below(t) - below(t0))


def capacity(t, t0, t1, rad, stereo, max_factors):
    """Entries the edge buffers need: the final length is <= max(prefix, max_factors + 2) and <= prefix + 2 n."""
    p = prefix_len(t, t0, rad, stereo)
    return min(max(p, max_factors + 2), p + 2 * (t - t0) * (t - t1))


def _pair_list(t, t0, t1, rad, device):
    """(ii, jj, f) of the cells that i - rad < j does not kill (j in [t1, i - rad]), row-major, built on the device from
    sizes the host knows: no synchronisation."""
    total = sum(max(i - rad - t1 + 1, 0) for i in range(t0, t))
    rows = torch.arange(t0, t, device=device)
    cnt = (rows - (rad + t1 - 1)).clamp_(min=0)
    starts = torch.cumsum(cnt, 0) - cnt
    ii = torch.repeat_interleave(rows, cnt, output_size=total)
    pos = torch.arange(total, device=device) - torch.repeat_interleave(starts, cnt, output_size=total)
    return ii, pos + t1, (ii - t0) * (t - t1) + pos


def proximity_edges(poses, disps, intrinsics, t, ii_known, jj_known, t0=0, t1=0, rad=2, nms=2, beta=0.25, thresh=16.0,
                    max_factors=-1, stereo=False, dist=None, form=None):
    """(ii, jj) int64 device tensors: the edge list `add_proximity_factors` hands to `add_factors`, in its order.

    poses (Np,7), disps (Nd,ht,wd), intrinsics (>= 4,) as for `geom.frame_distance`; t the frame count; ii_known,
    jj_known int64 (K,) the graph's edges `ii ++ ii_bad ++ ii_inac` (None = none).  The distance of a cell is
    .5 * (frame_distance(i -> j) + frame_distance(j -> i)) in float32 (DepthVideo.distance, bidirectional), computed only
    for the cells that `i - rad < j` leaves alive; each value equals the all-pairs call bit for bit.  `dist` (n,) float32
    replaces that computation (poses, disps and intrinsics are then ignored and may be None).  `form`: None picks
    "small" for n <= 4096 and "sorted" above; "small" beyond 4096 raises UnsupportedShape."""
    t, t0, t1, rad, nms, max_factors = (_int(v, k) for v, k in ((t, "t"), (t0, "t0"), (t1, "t1"), (rad, "rad"), (nms, "nms"),
                                                                  (max_factors, "max_factors")))
    n = window_cells(t, t0, t1, rad, nms)
    if form not in FORMS:
        raise RuntimeError("proximity_edges: form must be None, 'small' or 'sorted', got %r" % (form,))
    if form == "small" and n > SMALL_MAX:
        raise _lib.UnsupportedShape("proximity_edges: the small form serves n <= %d cells, got %d" % (SMALL_MAX, n))
    if nms >= 1 << 31 or abs(max_factors) >= 1 << 62:
        raise RuntimeError("proximity_edges: nms or max_factors out of range")
    thresh, beta, stereo = float(thresh), float(beta), bool(stereo)
    if (ii_known is None) != (jj_known is None):
        raise RuntimeError("ii_known and jj_known must both be given or both be None")
    named = [(poses, "poses"), (disps, "disps"), (intrinsics, "intrinsics")] if dist is None else [(dist, "dist")]
    known = [] if ii_known is None else [(ii_known, "ii_known"), (jj_known, "jj_known")]
    for pairs, dtype in ((named, torch.float32), (known, torch.int64)):
        for pair in pairs:                        # contiguity and dtype per tensor, in sequence
            check_contiguous([pair])
            check_dtype([pair], dtype)
    named = named + known
    if ii_known is not None:
        if ii_known.dim() != 1 or jj_known.dim() != 1 or ii_known.shape[0] != jj_known.shape[0]:
            raise RuntimeError("ii_known and jj_known must be 1-D and of equal length, got %s and %s"
                               % (tuple(ii_known.shape), tuple(jj_known.shape)))
        if ii_known.shape[0] >= 1 << 31:
            raise RuntimeError("proximity_edges: too many known edges")
    if dist is None:
        check_geometry(poses, disps, intrinsics)
    elif dist.dim() != 1 or dist.shape[0] != n:
        raise RuntimeError("dist must be 1-D with one value per cell (%d), got %s" % (n, tuple(dist.shape)))
    cap = capacity(t, t0, t1, rad, stereo, max_factors)
    if prefix_len(t, t0, rad, stereo) > 1 << 30:
        raise RuntimeError("proximity_edges: the neighbourhood prefix alone exceeds 2^30 entries")
    check_device(named)
    dev = named[0][0].device
    if n == 0:                                    # no rows: the prefix is empty
        return torch.empty((0,), dtype=torch.int64, device=dev), torch.empty((0,), dtype=torch.int64, device=dev)
    if dist is None:
        pi, pj, f = _pair_list(t, t0, t1, rad, dev)
        num = pi.shape[0]
        dist = torch.full((n,), float("inf"), dtype=torch.float32, device=dev)
        if num:
            d = frame_distance(poses, disps, intrinsics, torch.cat([pi, pj]), torch.cat([pj, pi]), beta)
            dist.index_copy_(0, f, .5 * (d[:num] + d[num:]))
    nk = 0 if ii_known is None else ii_known.shape[0]
    kii, kjj = (_ptr(ii_known), _ptr(jj_known)) if nk else (None, None)
    e_ii = torch.empty((cap,), dtype=torch.int64, device=dev)
    e_jj = torch.empty((cap,), dtype=torch.int64, device=dev)
    count = torch.empty((1,), dtype=torch.int32, device=dev)
    st = _stream(dist)
    rad = min(rad, t)                             # selects what any larger rad selects; fits the C int
    if form == "small" or (form is None and n <= SMALL_MAX):
        launch("lgu_proximity_select_small", "proximity_select_small", dev, _ptr(dist), kii, kjj, nk, t, t0, t1, rad, nms, thresh,
               max_factors, int(stereo), _ptr(e_ii), _ptr(e_jj), cap, _ptr(count), st)
    else:
        keys = torch.empty((n,), dtype=torch.int64, device=dev)
        work = torch.empty(((n + 31) // 32,), dtype=torch.int32, device=dev)
        launch("lgu_proximity_keys", "proximity_keys", dev, _ptr(dist), kii, kjj, nk, t, t0, t1, rad, nms, thresh, int(stereo),
               _ptr(keys), _ptr(work), st)
        keys = torch.sort(keys).values.contiguous()
        launch("lgu_proximity_select_sorted", "proximity_select_sorted", dev, _ptr(keys), _ptr(work), t, t0, t1, rad, nms,
               max_factors, int(stereo), _ptr(e_ii), _ptr(e_jj), cap, _ptr(count), st)
    m = int(count.item())                         # the one read of the device
    return e_ii[:m], e_jj[:m]


def neighborhood_edges(t0, t1, r=3, stereo=False, device=None):
    """(ii, jj) int64: the edges of `add_neighborhood_factors(t0, t1, r)` (factor_graph.py:304-316): every ordered pair
    of frames in [t0, t1) with c < |i - j| <= r, row-major, c = 1 with stereo else 0.  Built on the host (no kernel) and
    moved to `device`."""
    ix = torch.arange(t0, t1)
    ii, jj = torch.meshgrid(ix, ix, indexing="ij")
    ii, jj = ii.reshape(-1), jj.reshape(-1)
    gap = (ii - jj).abs()
    keep = (gap > (1 if stereo else 0)) & (gap <= r)
    ii, jj = ii[keep], jj[keep]
    return (ii, jj) if device is None else (ii.to(device), jj.to(device))


class ProximityFactors:
    """Bound stand-in for `FactorGraph.add_proximity_factors` (same signature).  It reads graph.video.{poses, disps,
    intrinsics, counter.value, stereo} and graph.{ii, jj, ii_bad, jj_bad, ii_inac, jj_inac, max_factors}, selects with
    `proximity_edges` and hands the result to graph.add_factors(ii, jj, remove); nothing else on the object changes."""

    def __init__(self, graph, previous=None):
        self.graph = graph
        self.previous = previous          # the instance attribute `install` replaced, if there was one
        self.calls = 0

    def __call__(self, t0=0, t1=0, rad=2, nms=2, beta=0.25, thresh=16.0, remove=False):
        g = self.graph
        v = g.video
        t = int(v.counter.value)
        dev = v.disps.device
        kii = torch.cat([g.ii, g.ii_bad, g.ii_inac], 0).to(device=dev, dtype=torch.int64).contiguous()
        kjj = torch.cat([g.jj, g.jj_bad, g.jj_inac], 0).to(device=dev, dtype=torch.int64).contiguous()
        ii, jj = proximity_edges(v.poses[:t], v.disps, v.intrinsics[0], t, kii, kjj, t0=t0, t1=t1, rad=rad, nms=nms, beta=beta,
                                 thresh=thresh, max_factors=g.max_factors, stereo=bool(v.stereo))
        self.calls += 1
        g.add_factors(ii, jj, remove)


def install(graph):
    """Bind a ProximityFactors as `graph.add_proximity_factors` (an instance attribute); returns it."""
    return bind(graph, "add_proximity_factors", ProximityFactors, lambda previous: ProximityFactors(graph, previous=previous))


def uninstall(graph):
    """Undo `install`: the class's method (or the instance attribute that was there before) is used again."""
    cur = unbind(graph, "add_proximity_factors", ProximityFactors)
    if cur is not None and cur.previous is not None:
        graph.add_proximity_factors = cur.previous
