"""Proximity edges of the factor graph selected on the device (lgu_slam_amd.graph, csrc/graphsel.hip; reference
droid_slam/factor_graph.py:304-383).

The result is integer data and is held exactly, values and order: to the fixtures tests/golden/proximity_*.npz (the
reference's own add_proximity_factors on seeded distinct distances, tools/gen_graph_golden.py) and, for ties, NaNs and
device-computed distances, to the numpy restatement tests/graph_restatement.py, which itself reproduces every fixture.
"""
import ctypes
import glob
import os
import subprocess
import sys
import types
import warnings

import numpy as np
import pytest

from tests import graph_restatement as G

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
REFERENCE = os.environ.get("LGU_REFERENCE", "/root/reference")   # the reference tree, where present (CPU tests only)
ENTRIES = ("lgu_proximity_select_small", "lgu_proximity_keys", "lgu_proximity_select_sorted")
HELPERS = ("lgu_proximity_prefix_len", "lgu_proximity_capacity", "lgu_proximity_work_bytes")
FIXTURES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLD, "proximity_*.npz")))
SMALL_MAX = 4096
f32 = np.float32


def fixture(name):
    with np.load(os.path.join(GOLD, name + ".npz")) as z:
        a = {k: z[k] for k in z.files}
    p = dict(t=int(a["t"]), t0=int(a["t0"]), t1=int(a["t1"]), rad=int(a["rad"]), nms=int(a["nms"]), thresh=float(a["thresh"]),
             max_factors=int(a["max_factors"]), stereo=bool(a["stereo"]))
    return a, p


def seeded_distances(seed, n, thresh, share=0.3):
    """n distinct float32 values in seeded order, about `share` of them under thresh."""
    rs = np.random.RandomState(seed)
    return (thresh / (share * max(n, 1)) * (rs.permutation(n) + 0.5)).astype(f32)


def want(d, kii, kjj, p):
    return G.proximity_edges(d, p["t"], kii, kjj, p["t0"], p["t1"], p["rad"], p["nms"], p["thresh"], p["max_factors"], p["stereo"])


def forms_for(n):
    return ("small", "sorted", None) if n <= SMALL_MAX else ("sorted", None)


# ---------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------

def test_header_declares_and_library_exports_the_proximity_entries(lgu):
    from tests.test_abi import declared_symbols
    syms = declared_symbols()
    lib = ctypes.CDLL(lgu.build())
    for s in ENTRIES + HELPERS:
        assert s in syms, s
        assert hasattr(lib, s), s
    for s in ENTRIES:
        assert s in lgu._lib.SIGNATURES, s
    assert "graph" in vars(lgu)                          # exported from the package
    assert "graphsel.hip" in lgu._build.SOURCES


def test_fixtures_cover_the_cases():
    assert len(FIXTURES) == 7
    ns = {name: (fixture(name)[1]["t"] - fixture(name)[1]["t0"]) * (fixture(name)[1]["t"] - fixture(name)[1]["t1"]) for name in FIXTURES}
    assert max(ns.values()) > SMALL_MAX                  # one beyond the one-launch form
    assert any(fixture(n)[1]["max_factors"] == -1 for n in FIXTURES) and any(fixture(n)[1]["nms"] == 0 for n in FIXTURES)
    assert any(fixture(n)[1]["stereo"] for n in FIXTURES)
    for name in FIXTURES:
        a, p = fixture(name)
        assert np.unique(a["d"]).shape[0] == a["d"].shape[0] == ns[name]     # distinct: the reference's argsort is decided
        if "frontend_t30" in name:                       # some known edges lie outside the window
            assert ((a["known_ii"] < p["t0"]) | (a["known_ii"] >= p["t"]) | (a["known_jj"] < p["t1"])).any()
            assert a["ii"].shape[0] == p["max_factors"] + 2                      # the bound on the length is met


@pytest.mark.parametrize("name", FIXTURES)
def test_restatement_reproduces_the_reference_fixture(name):
    a, p = fixture(name)
    ii, jj = want(a["d"], a["known_ii"], a["known_jj"], p)
    assert ii.tolist() == a["ii"].tolist() and jj.tolist() == a["jj"].tolist()
    assert G.prefix_edges(p["t"], p["t0"], p["rad"], p["stereo"]) == list(zip(ii.tolist(), jj.tolist()))[:G.prefix_len(
        p["t"], p["t0"], p["rad"], p["stereo"])]
    assert ii.shape[0] <= G.capacity(p["t"], p["t0"], p["rad"], p["stereo"], p["max_factors"])


@pytest.mark.skipif(not os.path.isdir(os.path.join(REFERENCE, "droid_slam")), reason="reference tree not present")
def test_fixtures_regenerate_from_the_live_reference():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_graph_golden.py"), "--reference", REFERENCE, "--check"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count("matches") == len(FIXTURES)


def test_prefix_and_capacity_helpers_agree(lgu):
    lib = lgu._lib.load()
    for t, t0, t1, rad, stereo, mf in ((12, 0, 0, 2, 0, 48), (40, 0, 0, 2, 1, 640), (30, 25, 5, 2, 0, 48), (9, 4, 0, 0, 1, -1),
                                       (5, 5, 0, 3, 1, 7), (7, 3, 0, 50, 0, 10 ** 12), (1, 0, 0, 0, 0, 0)):
        pl = G.prefix_len(t, t0, rad, bool(stereo))
        assert pl == len(G.prefix_edges(t, t0, rad, bool(stereo)))
        assert lgu.graph.prefix_len(t, t0, rad, bool(stereo)) == pl == lib.lgu_proximity_prefix_len(t, t0, rad, stereo)
        cap = min(max(pl, mf + 2), pl + 2 * (t - t0) * (t - t1))
        assert lgu.graph.capacity(t, t0, t1, rad, bool(stereo), mf) == cap == lib.lgu_proximity_capacity(t, t0, t1, rad, stereo, mf)
        assert lib.lgu_proximity_work_bytes(t, t0, t1) == 4 * (((t - t0) * (t - t1) + 31) // 32)
    assert lib.lgu_proximity_prefix_len(3, 4, 2, 0) == -1 and lib.lgu_proximity_work_bytes(5000, 0, 0) == -1


def test_c_entries_refuse_bad_windows_before_any_launch(lgu):
    """The rules are checked first: bad arguments come back as codes even with null pointers and no device."""
    lib = lgu._lib.load()
    BAD, UNS = lgu._lib.LGU_E_BADARG, lgu._lib.LGU_E_UNSUPPORTED

    def small(t, t0, t1, rad=2, nms=2, nk=0):
        return lib.lgu_proximity_select_small(None, None, None, nk, t, t0, t1, rad, nms, 16.0, 10, 0, None, None, 0, None, None)

    def keys(t, t0, t1, rad=2, nms=2):
        return lib.lgu_proximity_keys(None, None, None, 0, t, t0, t1, rad, nms, 16.0, 0, None, None, None)

    def srt(t, t0, t1, rad=2, nms=2):
        return lib.lgu_proximity_select_sorted(None, None, t, t0, t1, rad, nms, 10, 0, None, None, 0, None, None)

    for fn in (small, keys, srt):
        assert fn(5, 6, 0) == BAD and fn(5, 2, 3) == BAD and fn(-1, 0, 0) == BAD and fn(5, 0, -1) == BAD
        assert fn(9, 4, 2) == BAD                        # t1 > max(t0 - rad - 1, 0)
        assert fn(9, 4, 0, rad=-1) == BAD and fn(9, 4, 0, nms=-1) == BAD
        assert fn(5000, 0, 0) == UNS                     # 25e6 cells > 2^24
    assert small(70, 0, 0) == UNS                        # 4900 cells: beyond the one-launch form
    assert small(12, 0, 0, nk=-1) == BAD
    assert small(12, 0, 0) == BAD and srt(12, 0, 0) == BAD   # null count
    assert keys(12, 0, 0) == BAD                         # null buffers
    assert keys(12, 12, 0) == 0                          # n == 0: nothing to do


def test_argument_errors_are_raised_without_a_device(lgu, monkeypatch):
    def no_launch():
        raise AssertionError("the library was reached")
    monkeypatch.setattr(lgu._lib, "load", no_launch)
    P = lgu.graph.proximity_edges
    poses = torch.zeros(12, 7)
    poses[:, 6] = 1
    disps, intr = torch.ones(12, 6, 8), torch.tensor([8.0, 8.0, 4.0, 3.0])
    kii, kjj = torch.arange(3), torch.arange(3) + 4
    d = torch.ones(144)

    def call(t=12, dist=d, ki=kii, kj=kjj, p=poses, ds=disps, k=intr, **kw):
        return P(p, ds, k, t, ki, kj, dist=dist, **kw)

    with pytest.raises(RuntimeError, match="need 0 <= t1 <= t0 <= t"):
        call(t0=13)
    with pytest.raises(RuntimeError, match="need 0 <= t1 <= t0 <= t"):
        call(t0=3, t1=4)
    with pytest.raises(RuntimeError, match="rad and nms must be >= 0"):
        call(nms=-1)
    with pytest.raises(RuntimeError, match=r"need t1 <= max\(t0 - rad - 1, 0\)"):
        call(t0=4, t1=2)
    with pytest.raises(lgu._lib.UnsupportedShape, match="2\\^24"):
        call(t=5000)
    with pytest.raises(lgu._lib.UnsupportedShape, match="small form"):
        call(t=70, dist=torch.ones(4900), form="small")
    with pytest.raises(RuntimeError, match="form must be"):
        call(form="large")
    with pytest.raises(RuntimeError, match="t must be an integer"):
        call(t=12.5)
    with pytest.raises(RuntimeError, match="^dist must be contiguous$"):
        call(dist=torch.ones(288)[::2])
    with pytest.raises(RuntimeError, match="expected scalar type Float but found Double \\(dist\\)"):
        call(dist=d.double())
    with pytest.raises(RuntimeError, match="dist must be 1-D with one value per cell \\(144\\)"):
        call(dist=torch.ones(143))
    with pytest.raises(RuntimeError, match="expected scalar type Long but found Int \\(ii_known\\)"):
        call(ki=kii.int())
    with pytest.raises(RuntimeError, match="ii_known and jj_known must be 1-D and of equal length"):
        call(kj=torch.arange(2))
    with pytest.raises(RuntimeError, match="both be given or both be None"):
        call(kj=None)
    with pytest.raises(RuntimeError, match="^disps must be contiguous$"):
        call(dist=None, ds=torch.ones(12, 8, 6).transpose(1, 2))
    with pytest.raises(RuntimeError, match="poses must be \\(N,7\\)"):
        call(dist=None, p=torch.zeros(12, 6))
    with pytest.raises(RuntimeError, match="dist must be a HIP device tensor"):      # all other arguments are valid
        call()
    with pytest.raises(RuntimeError, match="poses must be a HIP device tensor"):
        call(dist=None)


@pytest.mark.parametrize("t0,t1,r,stereo", [(0, 7, 3, False), (2, 12, 3, True), (0, 5, 1, False), (4, 4, 3, False), (0, 3, 9, True)])
def test_neighborhood_edges_equal_the_direct_evaluation(lgu, t0, t1, r, stereo):
    ii, jj = lgu.graph.neighborhood_edges(t0, t1, r=r, stereo=stereo)
    wi, wj = G.neighborhood_edges(t0, t1, r, stereo)
    assert ii.dtype == jj.dtype == torch.int64
    assert ii.tolist() == wi.tolist() and jj.tolist() == wj.tolist()


def row_major_case(nms, t=40):
    """Distances that grow with the flat index: the visiting order is row-major, so the neighbours of a cell along its
    row are its neighbours in the sorted order too."""
    p = dict(t=t, t0=0, t1=0, rad=2, nms=nms, thresh=16.0, max_factors=10 ** 6, stereo=False)
    d = (1.0 + 0.001 * np.arange(t * t)).astype(f32)
    return d, p


def window_events(d, p, ii, jj):
    """(same, cross): among the accepted edges of the result (ii, jj), how often the FIRST live candidate of a 64-wide
    window of the sorted candidates suppressed a later candidate of the same window, and how often one accepted in the
    LAST lane of a window suppressed a candidate of the next window."""
    t, t0, t1, rad, W = p["t"], p["t0"], p["t1"], p["rad"], p["t"] - p["t1"]
    cand = []
    for f in np.argsort(d, kind="stable").tolist():
        i, j = t0 + f // W, t1 + f % W
        if i - rad < j or (max(i - rad - 1, 0) <= j < i) or not d[f] <= p["thresh"]:
            continue
        cand.append((i, j))
    rank = {c: k for k, c in enumerate(cand)}
    npre = G.prefix_len(t, t0, rad, p["stereo"])
    acc = list(zip(ii[npre::2].tolist(), jj[npre::2].tolist()))
    accset, same, cross, first_of = set(), 0, 0, {}
    for a in acc:
        first_of.setdefault(rank[a] // 64, a)
    for (ai, aj) in acc:
        ra, r = rank[(ai, aj)], G.radius(ai, aj, p["nms"])
        hit = [rank[c] for c in cand[ra + 1:ra + 129] if abs(c[0] - ai) + abs(c[1] - aj) <= r]
        if first_of[ra // 64] == (ai, aj) and any(h // 64 == ra // 64 for h in hit):
            same += 1
        if ra % 64 == 63 and any(h // 64 == ra // 64 + 1 for h in hit):
            cross += 1
        accset.add((ai, aj))
    return same, cross


@pytest.mark.parametrize("nms", [1, 3])
def test_row_major_case_has_same_window_and_cross_window_suppression(nms):
    """The inputs of the GPU test below do exercise both events (checked on the restatement's result)."""
    d, p = row_major_case(nms)
    ii, jj = want(d, [], [], p)
    same, cross = window_events(d, p, ii, jj)
    assert same > 0 and cross > 0, (same, cross)


# ---------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------

def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def select(lgu, d, kii, kjj, p, form=None, geometry=(None, None, None)):
    known = (None, None) if kii is None else (dev(np.asarray(kii, np.int64)), dev(np.asarray(kjj, np.int64)))
    ii, jj = lgu.graph.proximity_edges(*geometry, p["t"], known[0], known[1], t0=p["t0"], t1=p["t1"], rad=p["rad"], nms=p["nms"],
                                       thresh=p["thresh"], max_factors=p["max_factors"], stereo=p["stereo"], dist=dev(d), form=form)
    assert ii.dtype == jj.dtype == torch.int64 and ii.is_cuda and jj.is_cuda
    return host(ii).tolist(), host(jj).tolist()


def check_all_forms(lgu, d, kii, kjj, p):
    wi, wj = want(d, [] if kii is None else kii, [] if kjj is None else kjj, p)
    n = (p["t"] - p["t0"]) * (p["t"] - p["t1"])
    for form in forms_for(n):
        gi, gj = select(lgu, d, kii, kjj, p, form)
        assert gi == wi.tolist() and gj == wj.tolist(), form
    return wi, wj


@pytest.mark.gpu
@pytest.mark.parametrize("name", FIXTURES)
def test_fixture_parity_in_every_form(lgu, name):
    a, p = fixture(name)
    n = a["d"].shape[0]
    dummy = (torch.zeros(3), torch.zeros(2, 2), torch.zeros(1, dtype=torch.float64))   # ignored when dist is given
    for form in forms_for(n):
        gi, gj = select(lgu, a["d"], a["known_ii"], a["known_jj"], p, form, geometry=dummy)
        assert gi == a["ii"].tolist() and gj == a["jj"].tolist(), form


def _geometry(lgu, seed, **kw):
    from tests.test_geom import all_pairs, scene
    N = 12
    poses, disps, intr = scene(seed, N=N, H=48, W=64, **kw)
    P, D, K = dev(poses), dev(disps), dev(intr)
    ai, aj = all_pairs(N)
    d1 = lgu.geom.frame_distance(P, D, K, dev(ai), dev(aj), 0.25)
    d2 = lgu.geom.frame_distance(P, D, K, dev(aj), dev(ai), 0.25)
    return (P, D, K), host(.5 * (d1 + d2)).reshape(N, N)


@pytest.mark.gpu
@pytest.mark.parametrize("t0,t1", [(0, 0), (8, 2)])
def test_device_computed_distances_match_the_all_pairs_matrix(lgu, t0, t1):
    """End to end: distances computed on the pruned pair list select what the restatement selects from the all-pairs
    matrix (copied to the host)."""
    geo, dm = _geometry(lgu, 5)
    N = dm.shape[0]
    d = np.ascontiguousarray(dm[t0:, t1:]).reshape(-1)
    I, J = np.meshgrid(np.arange(t0, N), np.arange(t1, N), indexing="ij")
    live = d[(J <= I - 2 - 2).reshape(-1)]
    p = dict(t=N, t0=t0, t1=t1, rad=2, nms=1, thresh=float(np.median(live)), max_factors=200, stereo=False)
    kii, kjj = np.array([9, 3], np.int64), np.array([4, 11], np.int64)
    wi, wj = want(d, kii, kjj, p)
    assert wi.shape[0] > G.prefix_len(N, t0, 2, False)           # some cells are selected
    for form in ("small", "sorted", None):
        ii, jj = lgu.graph.proximity_edges(*geo, N, dev(kii), dev(kjj), t0=t0, t1=t1, rad=2, nms=1, beta=0.25, thresh=p["thresh"],
                                           max_factors=200, form=form)
        assert host(ii).tolist() == wi.tolist() and host(jj).tolist() == wj.tolist(), form


@pytest.mark.gpu
def test_ties_are_visited_in_ascending_flat_index(lgu):
    """All poses identical: many distances are bit-equal; the result is the stable restatement's in both forms."""
    geo, dm = _geometry(lgu, 9, step=0.0, angle=0.0)
    N = dm.shape[0]
    d = dm.reshape(-1)
    I, J = np.meshgrid(np.arange(N), np.arange(N), indexing="ij")
    live = d[(J <= I - 4).reshape(-1)]
    assert np.unique(live).shape[0] < live.shape[0] // 2          # ties among the candidates
    p = dict(t=N, t0=0, t1=0, rad=2, nms=1, thresh=16.0, max_factors=200, stereo=False)
    wi, wj = want(d, [], [], p)
    assert wi.shape[0] > G.prefix_len(N, 0, 2, False)
    for form in ("small", "sorted"):
        ii, jj = lgu.graph.proximity_edges(*geo, N, None, None, rad=2, nms=1, beta=0.25, thresh=16.0, max_factors=200, form=form)
        assert host(ii).tolist() == wi.tolist() and host(jj).tolist() == wj.tolist(), form
    rs = np.random.RandomState(3)                                  # and a synthetic case: 5 distinct values over 900 cells
    d2 = rs.randint(1, 6, size=900).astype(f32)
    check_all_forms(lgu, d2, None, None, dict(t=30, t0=0, t1=0, rad=2, nms=2, thresh=4.0, max_factors=300, stereo=False))


@pytest.mark.gpu
@pytest.mark.parametrize("nms", [1, 3])
def test_suppression_inside_a_wave_window_and_across_windows(lgu, nms):
    d, p = row_major_case(nms)
    check_all_forms(lgu, d, None, None, p)


@pytest.mark.gpu
@pytest.mark.parametrize("t,t0,t1,rad", [(1, 0, 0, 0), (13, 0, 0, 2), (256, 240, 0, 2), (241, 224, 0, 2), (64, 0, 0, 1)],
                         ids=["n1", "n169", "n4096_rows16", "n4097", "n4096_square"])
def test_edge_shapes_across_the_dispatch_boundary(lgu, t, t0, t1, rad):
    n = (t - t0) * (t - t1)
    p = dict(t=t, t0=t0, t1=t1, rad=rad, nms=2, thresh=16.0, max_factors=G.prefix_len(t, t0, rad, False) + 40, stereo=False)
    rs = np.random.RandomState(n)
    nk = 7 if n > 1 else 0
    kii = rs.randint(0, t, size=nk).astype(np.int64)
    kjj = rs.randint(0, t, size=nk).astype(np.int64)
    d = seeded_distances(n, n, 16.0) if n > 1 else np.array([1.0], f32)
    wi, _ = check_all_forms(lgu, d, kii, kjj, p)
    assert wi.shape[0] > G.prefix_len(t, t0, rad, False)
    if n > SMALL_MAX:
        with pytest.raises(lgu._lib.UnsupportedShape):
            select(lgu, d, kii, kjj, p, "small")


@pytest.mark.gpu
def test_bitmap_in_global_memory_beyond_the_lds_limit(lgu):
    """n = 725^2 = 525 625 cells: the greedy pass keeps its bitmap in the workspace, not in LDS."""
    t = 725
    n = t * t
    assert (n + 31) // 32 > 16000
    p = dict(t=t, t0=0, t1=0, rad=2, nms=2, thresh=16.0, max_factors=16 * t, stereo=False)
    rs = np.random.RandomState(77)
    kii = rs.randint(0, t, size=500).astype(np.int64)
    kjj = rs.randint(0, t, size=500).astype(np.int64)
    d = seeded_distances(5, n, 16.0, share=0.01)
    wi, wj = want(d, kii, kjj, p)
    assert G.prefix_len(t, 0, 2, False) + 500 < wi.shape[0]
    gi, gj = select(lgu, d, kii, kjj, p)
    assert gi == wi.tolist() and gj == wj.tolist()


@pytest.mark.gpu
def test_empty_window_thresholds_bounds_and_nan(lgu):
    empty = lgu.graph.proximity_edges(None, None, None, 9, None, None, t0=9, t1=0, dist=torch.empty(0, device="cuda"), max_factors=50)
    assert [tuple(x.shape) for x in empty] == [(0,), (0,)] and empty[0].dtype == torch.int64 and empty[0].is_cuda
    t = 20
    n = t * t
    base = dict(t=t, t0=0, t1=0, rad=2, nms=2, thresh=16.0, max_factors=400, stereo=False)
    d = seeded_distances(41, n, 16.0)
    pre = G.prefix_len(t, 0, 2, False)
    wi, _ = check_all_forms(lgu, d + f32(17.0), None, None, base)           # every cell above thresh: the prefix only
    assert wi.shape[0] == pre
    for mf, length in ((pre - 1, pre), (pre, pre + 2), (pre + 1, pre + 2), (-1, pre), (0, pre)):
        wi, _ = check_all_forms(lgu, d, None, None, dict(base, max_factors=mf))
        assert wi.shape[0] == length, mf
    wi, _ = check_all_forms(lgu, d, None, None, dict(base, stereo=True, rad=0, nms=0))   # the stereo diagonal is dead
    assert wi.shape[0] > G.prefix_len(t, 0, 0, True)
    dn = d.copy()                                                            # a NaN where the smallest distance was
    f = int(np.argmin(np.where(np.arange(n) % t <= np.arange(n) // t - 4, d, np.inf)))
    dn[f] = np.nan
    w0, w1 = check_all_forms(lgu, d, None, None, base)
    n0, n1 = check_all_forms(lgu, dn, None, None, base)
    cell = (f // t, f % t)
    assert cell in list(zip(w0.tolist(), w1.tolist())) and cell not in list(zip(n0.tolist(), n1.tolist()))
    dm = d.copy()                                                            # negative values and -0 order as numbers
    dm[::7] = -dm[::7]
    dm[3::11] = f32(-0.0)
    dm[5::13] = f32(0.0)
    check_all_forms(lgu, dm, None, None, base)


_SENT = -777


def _banded(n, dtype, guard=1024):
    big = torch.full((n + 2 * guard,), _SENT, dtype=dtype, device="cuda")
    return big, big[guard:guard + n], guard


def _bands_intact(big, guard):
    return bool((big[:guard] == _SENT).all()) and bool((big[-guard:] == _SENT).all())


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["proximity_frontend_t30", "proximity_backend_t40_stereo", "proximity_default_max"])
def test_entries_write_nothing_at_or_beyond_count(lgu, name):
    """Through the C ABI into sentinel-filled memory, with and without known edges (null pointers): the first `count`
    entries are the result, everything from `count` on and the bands around every buffer are untouched."""
    from lgu_slam_amd.ops import _ptr, _stream
    lib = lgu._lib.load()
    a, p = fixture(name)
    t, t0, t1, rad, nms, thresh, mf, stereo = (p[k] for k in ("t", "t0", "t1", "rad", "nms", "thresh", "max_factors", "stereo"))
    n = a["d"].shape[0]
    d = dev(a["d"])
    st = _stream(d)
    for known in (True, False):
        kii, kjj = (dev(a["known_ii"]), dev(a["known_jj"])) if known else (None, None)
        nk = a["known_ii"].shape[0] if known else 0
        kp = (_ptr(kii), _ptr(kjj)) if nk else (None, None)
        wi, wj = want(a["d"], a["known_ii"] if known else [], a["known_jj"] if known else [], p)
        cap = lib.lgu_proximity_capacity(t, t0, t1, rad, int(stereo), mf)
        assert cap >= wi.shape[0]
        for form in ("small", "sorted"):
            bi, ei, g = _banded(cap, torch.int64)
            bj, ej, _ = _banded(cap, torch.int64)
            bc, cnt, _ = _banded(1, torch.int32)
            bands = [bi, bj, bc]
            if form == "small":
                assert lib.lgu_proximity_select_small(_ptr(d), kp[0], kp[1], nk, t, t0, t1, rad, nms, thresh, mf, int(stereo),
                                                      _ptr(ei), _ptr(ej), cap, _ptr(cnt), st) == 0
            else:
                words = lib.lgu_proximity_work_bytes(t, t0, t1) // 4
                bk, keys, _ = _banded(n, torch.int64)
                bw, work, _ = _banded(words, torch.int32)
                bands += [bk, bw]
                assert lib.lgu_proximity_keys(_ptr(d), kp[0], kp[1], nk, t, t0, t1, rad, nms, thresh, int(stereo), _ptr(keys),
                                              _ptr(work), st) == 0
                assert bool((keys >= 0).all())                           # fully written, non-negative
                skeys = torch.sort(keys).values.contiguous()
                assert lib.lgu_proximity_select_sorted(_ptr(skeys), _ptr(work), t, t0, t1, rad, nms, mf, int(stereo), _ptr(ei),
                                                       _ptr(ej), cap, _ptr(cnt), st) == 0
            torch.cuda.synchronize()
            m = int(cnt.item())
            assert host(ei[:m]).tolist() == wi.tolist() and host(ej[:m]).tolist() == wj.tolist(), (form, known)
            assert bool((ei[m:] == _SENT).all()) and bool((ej[m:] == _SENT).all())
            assert all(_bands_intact(b, g) for b in bands)
            if form == "small" and cap > 0:                              # a capacity below the bound is refused
                assert lib.lgu_proximity_select_small(_ptr(d), kp[0], kp[1], nk, t, t0, t1, rad, nms, thresh, mf, int(stereo),
                                                      _ptr(ei), _ptr(ej), cap - 1, _ptr(cnt), st) == lgu._lib.LGU_E_BADARG


@pytest.mark.gpu
def test_one_device_read_per_call(lgu):
    """The call synchronises the host once (the edge count), in either form, distances included."""
    geo, dm = _geometry(lgu, 5)
    N = dm.shape[0]
    kii, kjj = dev(np.array([9, 3], np.int64)), dev(np.array([4, 11], np.int64))
    thresh = float(np.median(dm))
    for form in ("small", "sorted"):
        lgu.graph.proximity_edges(*geo, N, kii, kjj, thresh=thresh, max_factors=100, form=form)     # warm every kernel up
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("warn")
        try:
            with warnings.catch_warnings(record=True) as seen:
                warnings.simplefilter("always")
                lgu.graph.proximity_edges(*geo, N, kii, kjj, thresh=thresh, max_factors=100, form=form)
        finally:
            torch.cuda.set_sync_debug_mode("default")
        syncs = [w for w in seen if "synchroniz" in str(w.message)]
        assert len(syncs) == 1, [str(w.message) for w in seen]


class _Graph:
    def add_proximity_factors(self, *a, **k):
        raise AssertionError("the class's method was called")


@pytest.mark.gpu
def test_install_binds_the_method_and_uninstall_restores_it(lgu):
    from tests.test_geom import scene
    N, t = 12, 10
    poses, disps, intr = scene(5, N=N, H=48, W=64)
    P, D = dev(poses), dev(disps)
    K = dev(np.tile(np.append(intr, 0).astype(f32)[:4], (N, 1)))
    calls = []
    video = types.SimpleNamespace(poses=P, disps=D, intrinsics=K, counter=types.SimpleNamespace(value=t), stereo=False)
    edges = dict(ii=dev(np.array([9, 3], np.int64)), jj=dev(np.array([4, 8], np.int64)), ii_bad=dev(np.array([7], np.int64)),
                 jj_bad=dev(np.array([2], np.int64)), ii_inac=dev(np.zeros(0, np.int64)), jj_inac=dev(np.zeros(0, np.int64)))
    for graph in (types.SimpleNamespace(), _Graph()):
        vars(graph).update(video=video, max_factors=60, add_factors=lambda ii, jj, remove=False: calls.append((ii, jj, remove)),
                           **edges)
        before = dict(vars(graph))
        w = lgu.graph.install(graph)
        assert lgu.graph.install(graph) is w and graph.add_proximity_factors is w
        graph.add_proximity_factors(6, 1, rad=2, nms=1, beta=0.3, thresh=30.0, remove=True)
        (ii, jj, remove), = calls
        calls.clear()
        kii, kjj = torch.cat([edges["ii"], edges["ii_bad"]]), torch.cat([edges["jj"], edges["jj_bad"]])
        wi, wj = lgu.graph.proximity_edges(P[:t], D, K[0], t, kii, kjj, t0=6, t1=1, rad=2, nms=1, beta=0.3, thresh=30.0,
                                           max_factors=60)
        assert remove is True and torch.equal(ii, wi) and torch.equal(jj, wj)
        assert ii.shape[0] > G.prefix_len(t, 6, 2, False) and int(ii.max()) < t
        graph.add_proximity_factors()                                       # the reference's defaults
        (ii, jj, remove), = calls
        calls.clear()
        assert remove is False and ii.shape[0] >= G.prefix_len(t, 0, 2, False)
        lgu.graph.uninstall(graph)
        after = vars(graph)                                                 # nothing else on the object changed
        assert sorted(after) == sorted(before) and all(after[k] is before[k] for k in before)
    assert graph.add_proximity_factors.__func__ is _Graph.add_proximity_factors
