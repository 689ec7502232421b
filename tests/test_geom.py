"""The geometry entries of droid_backends (lgu_slam_amd.geom, csrc/geom.hip): frame_distance, projmap, depth_filter,
iproj (reference src/droid_kernels.cu:427-851).

projmap, depth_filter and iproj are held bit for bit (counts exactly) to the float32 restatement
tests/geom_restatement.py.  frame_distance's per-pixel terms are exact float32 values of the restatement summed in
float64; the kernel sums them in float32 in a fixed order: per lane at most 2 * 8 terms in sequence, a 64-lane butterfly
(6 levels) and the wave sums (<= 16) in sequence, i.e. every term passes through at most ~30 roundings of relative
error 2^-24 each.  All terms are non-negative, so each of the three sums is within 30 * 6e-8 = 1.8e-6 of its exact value
(relative), and the ratio accum / valid within ~4e-6: the bound used below is 1e-5.  The 1000 branch (ratio < 0.75) must
agree exactly, except for pairs whose float64 ratio lies within 1e-5 of 0.75.
"""
import ctypes

import numpy as np
import pytest

from tests import geom_restatement as G

torch = pytest.importorskip("torch")

f32 = np.float32
GEOM_ENTRIES = ("lgu_frame_distance_f32", "lgu_projmap_f32", "lgu_depth_filter_f32", "lgu_iproj_f32")


def _quat(rng, angle):
    axis = rng.standard_normal(3)
    axis /= np.linalg.norm(axis)
    a = angle * rng.standard_normal()
    return np.concatenate([np.sin(a / 2) * axis, [np.cos(a / 2)]])


def scene(seed, N=12, H=48, W=64, step=0.1, angle=0.05, bad=0.0):
    """Camera path (N,7) float32 (a random walk of `step`, rotations of ~`angle`), disparities in [0.2, 1.2) with a
    fraction `bad` of them zero or negative, intrinsics of a DROID-like 48x64 frame (fx = fy = 0.8 W)."""
    rng = np.random.default_rng(seed)
    poses = np.zeros((N, 7), f32)
    t = np.zeros(3)
    for k in range(N):
        poses[k, :3] = t
        poses[k, 3:] = _quat(rng, angle)
        t = t + step * rng.standard_normal(3)
    disps = (0.2 + rng.random((N, H, W))).astype(f32)
    if bad:
        m = rng.random((N, H, W)) < bad
        disps[m] = np.where(rng.random(int(m.sum())) < 0.5, 0.0, -rng.random(int(m.sum()))).astype(f32)
    intr = np.array([0.8 * W, 0.8 * W, W / 2, H / 2], f32)
    return poses, disps, intr


def all_pairs(N):
    ii, jj = np.meshgrid(np.arange(N), np.arange(N), indexing="ij")
    return ii.ravel().astype(np.int64), jj.ravel().astype(np.int64)


def same_bits(a, b):
    a, b = np.asarray(a, f32), np.asarray(b, f32)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool((na == nb).all()) and bool((a[~na].view(np.int32) == b[~nb].view(np.int32)).all())


# ---------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------

def test_header_declares_and_library_exports_the_geometry_entries(lgu):
    from tests.test_abi import declared_symbols
    syms = declared_symbols()
    lib = ctypes.CDLL(lgu.build())
    for s in GEOM_ENTRIES:
        assert s in syms, s
        assert hasattr(lib, s), s
        assert s in lgu._lib.SIGNATURES, s


def test_dropin_binds_the_geometry_entries(lgu):
    _, b = lgu.install_dropins()
    for n in ("frame_distance", "projmap", "depth_filter", "iproj"):
        assert getattr(b, n) is getattr(lgu.geom, n), n
    for n in ("ba", "corr_index_forward", "corr_index_backward"):
        with pytest.raises(NotImplementedError):
            getattr(b, n)()
    assert "geom" in vars(lgu)                          # exported from the package


def _cpu_args():
    poses = torch.zeros(4, 7)
    poses[:, 6] = 1
    return poses, torch.ones(4, 6, 8), torch.tensor([8.0, 8.0, 4.0, 3.0]), torch.arange(3), torch.arange(3)


@pytest.mark.parametrize("op", ["frame_distance", "projmap", "depth_filter", "iproj"])
def test_input_checks_raise_before_any_launch(lgu, monkeypatch, op):
    def no_launch():
        raise AssertionError("the library was reached")
    monkeypatch.setattr(lgu._lib, "load", no_launch)
    fn = getattr(lgu.geom, op)
    poses, disps, intr, ii, jj = _cpu_args()
    thresh = torch.full((3,), 0.1)

    def call(p=poses, d=disps, k=intr, i=ii, j=jj):
        if op == "frame_distance":
            return fn(p, d, k, i, j, 0.3)
        if op == "projmap":
            return fn(p, d, k, i, j)
        if op == "depth_filter":
            return fn(p, d, k, i, thresh)
        return fn(p, d, k)

    with pytest.raises(RuntimeError, match="^disps must be contiguous$"):
        call(d=torch.ones(4, 8, 6).transpose(1, 2))
    with pytest.raises(RuntimeError, match="^poses must be contiguous$"):
        call(p=torch.zeros(7, 4).t())
    if op != "iproj":
        with pytest.raises(RuntimeError, match="expected scalar type Long but found Int"):
            call(i=ii.int())
    if op in ("frame_distance", "projmap"):
        with pytest.raises(RuntimeError, match="ii and jj must be 1-D and of equal length"):
            call(j=torch.arange(2))
    with pytest.raises(RuntimeError, match="expected scalar type Float but found Double"):
        call(d=disps.double())
    with pytest.raises(RuntimeError, match="must be a HIP device tensor"):   # all other arguments are valid
        call()


def test_torch_ops_registration(lgu):
    from lgu_slam_amd import torch_ops
    assert sorted(torch_ops.GEOM_REGISTERED) == ["depth_filter", "frame_distance", "iproj", "projmap"]
    assert "float beta" in str(torch.ops.lgu.frame_distance.default._schema)
    assert str(torch.ops.lgu.projmap.default._schema).endswith("-> Tensor[]")
    assert str(torch.ops.lgu.depth_filter.default._schema).endswith("-> Tensor")
    assert "Tensor intrinsics" in str(torch.ops.lgu.iproj.default._schema)


def _compose(a, b):
    """(a * b) of SE3 (...,7) = t, q(xyzw), pure torch float64."""
    ta, qa, tb, qb = a[..., :3], a[..., 3:], b[..., :3], b[..., 3:]
    va, wa, vb, wb = qa[..., :3], qa[..., 3:], qb[..., :3], qb[..., 3:]
    q = torch.cat([wa * vb + wb * va + torch.cross(va, vb, dim=-1), wa * wb - (va * vb).sum(-1, keepdim=True)], -1)
    uv = 2 * torch.cross(va, tb, dim=-1)
    t = ta + tb + wa * uv + torch.cross(va, uv, dim=-1)
    return torch.cat([t, q], -1)


def test_se3_inverse_composes_to_identity(lgu):
    poses, _, _ = scene(3, N=64, step=0.1, angle=1.0)
    p = torch.from_numpy(poses)
    inv = lgu.geom.se3_inverse(p)
    assert inv.dtype == torch.float32 and inv.shape == p.shape
    for c in (_compose(p.double(), inv.double()), _compose(inv.double(), p.double())):
        assert float(c[:, :3].abs().max()) < 1e-6
        assert float((c[:, 3:6]).abs().max()) < 1e-6 and float((c[:, 6] - 1).abs().max()) < 1e-6


def test_restatement_neighbour_set_and_conversion_rule():
    assert G.NEIGHBOURS == (-1, -2, -3, 3, 4, 5)
    assert sorted(G.NEIGHBOURS) != [-3, -2, -1, 1, 2, 3]
    got = G.cvt_i32_sat(np.array([np.nan, np.inf, -np.inf, 3e9, -3e9, -1.0, 0.0, 7.0], f32))
    assert got.tolist() == [0, 2 ** 31 - 1, -2 ** 31, 2 ** 31 - 1, -2 ** 31, -1, 0, 7]
    # frames 0 and N-1 see only the neighbours inside the buffer: a scene where every neighbour agrees everywhere
    N = 10
    poses = np.zeros((N, 7), f32)
    poses[:, 6] = 1
    disps = np.full((N, 6, 8), 0.5, f32)
    intr = np.array([8, 8, 4, 3], f32)
    cnt = G.depth_filter(poses, disps, intr, [0, 1, 2, 3, 5, 6, 9, N, -1], np.full(9, 0.1, f32))
    interior = (slice(0, 5), slice(0, 7))     # the last row / column never have a corner inside
    assert [int(c[interior].min()) for c in cnt] == [3, 4, 5, 6, 5, 4, 3, 0, 0]
    assert int(cnt[:, 5, :].max()) == 0 and int(cnt[:, :, 7].max()) == 0


def test_restatement_threshold_is_double():
    """|1/dj - 1/d| < thresh compared in double: d = float32(4/9) counts against 1/dj = 2 and thresh 0.25 (its double
    difference is just below 0.25, its float32 difference rounds onto 0.25); the next float32 below does not count."""
    intr = np.array([8, 8, 4, 3], f32)
    poses = np.zeros((4, 7), f32)
    poses[:, 6] = 1
    t = f32(0.25)
    d = f32(1 / 2.25)
    below = np.nextafter(d, f32(0))
    assert 1.0 / float(d) - 2.0 < 0.25 and abs(f32(1) / d - f32(2)) >= t       # double counts, float32 would not
    assert 1.0 / float(below) - 2.0 > 0.25
    disps = np.full((4, 4, 4), d, f32)
    disps[0] = 0.5                                     # 1/dj = 2 exactly (identity poses: dj = d_own)
    assert G.depth_filter_hits(poses, disps, intr, 0, 3, t).reshape(4, 4)[:3, :3].all()
    disps[3] = below
    assert not G.depth_filter_hits(poses, disps, intr, 0, 3, t).any()


def test_restatement_frame_distance_invalid_pairs_and_identity():
    poses, disps, intr = scene(5, N=6, H=12, W=16)
    dist, ratio = G.frame_distance(poses[:4], disps, intr, [0, 1, 4, 0, -1], [0, 2, 0, 5, 1], 0.3)
    assert np.isnan(dist[2:]).all() and not np.isnan(dist[:2]).any()
    assert dist[0] < 1e-3 and ratio[0] == pytest.approx(1.0)


# ---------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------

def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def _fd_check(got, want, ratio):
    """got (kernel) against the restatement's (want, ratio): NaN where want is NaN, the 1000 branch exactly (except
    ratios within 1e-5 of 0.75), relative error <= 1e-5 elsewhere."""
    got = np.asarray(got, np.float64)
    assert np.isnan(got).tolist() == np.isnan(want).tolist()
    ok = ~np.isnan(want) & ~(np.abs(ratio - 0.75) <= 1e-5)
    assert ((got[ok] == 1000.0) == (want[ok] == 1000.0)).all()
    m = ok & (want != 1000.0)
    err = np.abs(got[m] - want[m])
    assert (err <= 1e-5 * np.abs(want[m])).all(), float(np.max(err / np.maximum(np.abs(want[m]), 1e-30)))


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["wide", "near_identity", "invalid_terms", "short_poses", "odd_shape"])
def test_frame_distance_matches_restatement(lgu, case):
    kw = dict(wide=dict(step=0.5, angle=0.3), near_identity=dict(step=1e-3, angle=1e-3),
              invalid_terms=dict(step=0.3, angle=0.1, bad=0.3), short_poses=dict(step=0.2, angle=0.1),
              odd_shape=dict(step=0.2, angle=0.1, H=37, W=150))[case]
    poses, disps, intr = scene(11 + len(case), N=kw.pop("N", 12), **kw)
    N = len(poses)
    ii, jj = all_pairs(N)
    if case == "short_poses":      # DepthVideo.distance: poses[:counter] with the whole disparity buffer
        poses = poses[:8]
        sel = (ii < 8) & (jj < 8)
        ii, jj = ii[sel], jj[sel]
    if case == "invalid_terms":    # push a few frames behind the camera: ratios below 0.75 -> 1000
        disps[3] = -np.abs(disps[3]) - 2
    want, ratio = G.frame_distance(poses, disps, intr, ii, jj, 0.3)
    got = host(lgu.geom.frame_distance(dev(poses), dev(disps), dev(intr), dev(ii), dev(jj), 0.3))
    assert got.dtype == np.float32 and got.shape == (len(ii),)
    _fd_check(got, want, ratio)
    if case == "invalid_terms":
        assert (got == 1000.0).any() and (got != 1000.0).any()
    assert np.abs(got[ii == jj]).max() < 1e-2          # ii == jj: T_ij is the identity up to rounding


@pytest.mark.gpu
@pytest.mark.parametrize("N", [20, 101], ids=["400_pairs", "10201_pairs"])
def test_frame_distance_is_deterministic_and_batch_independent(lgu, N):
    poses, disps, intr = scene(23, N=N, step=0.2, angle=0.1, bad=0.05)
    P, D, K = dev(poses), dev(disps), dev(intr)
    ii, jj = all_pairs(N)
    I, J = dev(ii), dev(jj)
    a = lgu.geom.frame_distance(P, D, K, I, J, 0.3)
    b = lgu.geom.frame_distance(P, D, K, I, J, 0.3)
    assert torch.equal(a, b)
    perm = torch.from_numpy(np.random.default_rng(N).permutation(len(ii))).cuda()
    c = lgu.geom.frame_distance(P, D, K, I[perm].contiguous(), J[perm].contiguous(), 0.3)
    assert torch.equal(c, a[perm])
    for k in np.random.default_rng(1).choice(len(ii), 24, replace=False).tolist() + [0, len(ii) - 1]:
        one = lgu.geom.frame_distance(P, D, K, I[k:k + 1].contiguous(), J[k:k + 1].contiguous(), 0.3)
        assert torch.equal(one[0], a[k]), k


@pytest.mark.gpu
def test_bidirectional_distance_through_droid_backends(lgu):
    """DepthVideo.distance (depth_video.py:150-180): 0.5 * (fd(ii, jj) + fd(jj, ii)) over the all-pairs grid, with
    poses[:counter] against the whole disparity buffer."""
    _, b = lgu.install_dropins()
    poses, disps, intr = scene(31, N=24, step=0.2, angle=0.1)
    counter = 16
    ii, jj = all_pairs(counter)
    P, D, K = dev(poses[:counter]).clone(), dev(disps), dev(intr)
    d = 0.5 * (b.frame_distance(P, D, K, dev(ii), dev(jj), 0.3) + b.frame_distance(P, D, K, dev(jj), dev(ii), 0.3))
    m = host(d).reshape(counter, counter)
    assert np.array_equal(m, m.T)
    w1, r1 = G.frame_distance(poses[:counter], disps, intr, ii, jj, 0.3)
    w2, r2 = G.frame_distance(poses[:counter], disps, intr, jj, ii, 0.3)
    g1 = host(b.frame_distance(P, D, K, dev(ii), dev(jj), 0.3))
    _fd_check(g1, w1, r1)
    _fd_check(host(b.frame_distance(P, D, K, dev(jj), dev(ii), 0.3)), w2, r2)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(24, 40), (48, 64), (7, 5)])
def test_projmap_and_iproj_are_bit_identical_to_the_restatement(lgu, shape):
    H, W = shape
    poses, disps, intr = scene(41 + W, N=9, H=H, W=W, step=0.4, angle=0.3, bad=0.1)
    rng = np.random.default_rng(W)
    ii = np.concatenate([rng.integers(0, 9, 20), [0, 4, 8]]).astype(np.int64)
    jj = np.concatenate([rng.integers(0, 9, 20), [0, 4, 8]]).astype(np.int64)
    coords, valid = lgu.geom.projmap(dev(poses), dev(disps), dev(intr), dev(ii), dev(jj))
    wc, wv = G.projmap(poses, disps, intr, ii, jj)
    assert tuple(coords.shape) == (len(ii), H, W, 3) and tuple(valid.shape) == (len(ii), H, W, 1)
    assert same_bits(host(coords), wc) and same_bits(host(valid), wv)
    assert bool((coords[..., 2] == 0).all())
    assert 0 < float(valid.mean()) < 1
    # iproj with the callers' inverted poses, and with extra intrinsics entries (only the first four are read)
    inv = lgu.geom.se3_inverse(dev(poses))
    k8 = dev(np.concatenate([intr, [9, 9, 9, 9]]).astype(f32))
    pts = lgu.geom.iproj(inv, dev(disps), k8)
    assert tuple(pts.shape) == (9, H, W, 3)
    assert same_bits(host(pts), G.iproj(host(inv), disps, intr))


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(30, 40), (48, 64)])
def test_depth_filter_counts_equal_the_restatement(lgu, shape):
    H, W = shape
    N = 14
    poses, disps, intr = scene(53 + H, N=N, H=H, W=W, step=0.05, angle=0.02, bad=0.08)
    ix = np.array([0, 1, 2, 6, N - 5, N - 4, N - 3, N - 2, N - 1], np.int64)
    thresh = np.random.default_rng(H).uniform(0.005, 0.5, len(ix)).astype(f32)    # per-frame thresholds
    got = lgu.geom.depth_filter(dev(poses), dev(disps), dev(intr), dev(ix), dev(thresh))
    want = G.depth_filter(poses, disps, intr, ix, thresh)
    assert got.dtype == torch.float32 and tuple(got.shape) == (len(ix), H, W)
    assert np.array_equal(host(got), want)
    assert want.max() >= 3 and (want == 0).any()         # the counts span a range


@pytest.mark.gpu
def test_view_reconstruction_sequence_through_droid_backends(lgu):
    """view_reconstruction.py:67-78: iproj(SE3(poses).inv().data, ...), depth_filter(...), then masking."""
    _, b = lgu.install_dropins()
    poses, disps, intr = scene(61, N=10, H=48, W=64, step=0.05, angle=0.02)
    P, D, K = dev(poses), dev(disps), dev(intr)
    index = torch.arange(len(poses), device="cuda")
    thresh = 0.5 * torch.ones_like(D.mean(dim=[1, 2]))   # the scene's disparities are independent per frame
    points = b.iproj(lgu.geom.se3_inverse(P), D, K)
    counts = b.depth_filter(P, D, K, index, thresh)
    mask = (counts >= 2) & (D > .25 * D.mean())
    sel = points[mask]
    assert sel.shape[1] == 3 and 0 < sel.shape[0] < mask.numel() and bool(torch.isfinite(sel).all())
    assert np.array_equal(host(counts), G.depth_filter(poses, disps, intr, np.arange(10), host(thresh)))


_SENT = 1234.5


def _banded(shape, guard=4096):
    n = int(np.prod(shape))
    big = torch.full((n + 2 * guard,), _SENT, dtype=torch.float32, device="cuda")
    return big, big[guard:guard + n].view(shape), guard


def _bands_intact(big, guard):
    return bool((big[:guard] == _SENT).all()) and bool((big[-guard:] == _SENT).all())


@pytest.mark.gpu
def test_geometry_entry_points_write_nothing_outside_their_tensors(lgu):
    """Each entry point called through the C ABI into sentinel-filled memory: results equal the operators' into fresh
    tensors, every element is written, the bands are untouched."""
    from lgu_slam_amd.ops import _ptr, _stream
    lib = lgu._lib.load()
    N, H, W = 9, 13, 70
    poses, disps, intr = scene(71, N=N, H=H, W=W, step=0.2, angle=0.1, bad=0.05)
    P, D, K = dev(poses), dev(disps), dev(intr)
    ii, jj = dev(np.array([0, 3, 8, 2, 2], np.int64)), dev(np.array([1, 3, 0, 7, 5], np.int64))
    ix, th = dev(np.array([0, 4, 8], np.int64)), dev(np.array([0.05, 0.1, 0.2], f32))
    st = _stream(P)
    big, dist, g = _banded((5,))
    assert lib.lgu_frame_distance_f32(_ptr(P), N, _ptr(D), N, H, W, _ptr(K), _ptr(ii), _ptr(jj), 5, 0.3, _ptr(dist), st) == 0
    bc, coords, gc = _banded((5, H, W, 3))
    bv, valid, gv = _banded((5, H, W, 1))
    assert lib.lgu_projmap_f32(_ptr(P), N, _ptr(D), N, H, W, _ptr(K), _ptr(ii), _ptr(jj), 5, _ptr(coords), _ptr(valid), st) == 0
    bd, cnt, gd = _banded((3, H, W))
    assert lib.lgu_depth_filter_f32(_ptr(P), N, _ptr(D), N, H, W, _ptr(K), _ptr(ix), _ptr(th), 3, _ptr(cnt), st) == 0
    bp, pts, gp = _banded((N, H, W, 3))
    assert lib.lgu_iproj_f32(_ptr(P), N, _ptr(D), N, H, W, _ptr(K), _ptr(pts), st) == 0
    torch.cuda.synchronize()
    assert torch.equal(dist, lgu.geom.frame_distance(P, D, K, ii, jj, 0.3))
    wc, wv = lgu.geom.projmap(P, D, K, ii, jj)
    assert torch.equal(coords, wc) and torch.equal(valid, wv)
    assert torch.equal(cnt, lgu.geom.depth_filter(P, D, K, ix, th))
    assert same_bits(host(pts), host(lgu.geom.iproj(P, D, K)))
    for t in (dist, coords, valid, cnt, pts):
        assert not bool((t == _SENT).any())
    for bg, gg in ((big, g), (bc, gc), (bv, gv), (bd, gd), (bp, gp)):
        assert _bands_intact(bg, gg)


@pytest.mark.gpu
def test_side_stream_and_graph_capture(lgu):
    poses, disps, intr = scene(83, N=12, step=0.2, angle=0.1)
    P, D, K = dev(poses), dev(disps), dev(intr)
    ii, jj = all_pairs(12)
    I, J = dev(ii), dev(jj)
    ref = lgu.geom.frame_distance(P, D, K, I, J, 0.3)
    ref_pm = lgu.geom.projmap(P, D, K, I[:7], J[:7])
    ref_df = lgu.geom.depth_filter(P, D, K, I[:5], dev(np.full(5, 0.05, f32)))
    ref_ip = lgu.geom.iproj(P, D, K)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        fd = lgu.geom.frame_distance(P, D, K, I, J, 0.3)
        pm = lgu.geom.projmap(P, D, K, I[:7], J[:7])
        df = lgu.geom.depth_filter(P, D, K, I[:5], dev(np.full(5, 0.05, f32)))
        ip = lgu.geom.iproj(P, D, K)
    s.synchronize()
    assert torch.equal(fd, ref) and torch.equal(pm[0], ref_pm[0]) and torch.equal(pm[1], ref_pm[1])
    assert torch.equal(df, ref_df) and same_bits(host(ip), host(ref_ip))
    # one capture of frame_distance, replayed after the poses moved: equals eager mode on the new poses
    g = torch.cuda.CUDAGraph()
    s2 = torch.cuda.Stream()
    s2.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s2):
        lgu.geom.frame_distance(P, D, K, I, J, 0.3)           # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(s2)
    with torch.cuda.graph(g):
        out = lgu.geom.frame_distance(P, D, K, I, J, 0.3)
    P.copy_(dev(scene(84, N=12, step=0.3, angle=0.2)[0]))
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, lgu.geom.frame_distance(P, D, K, I, J, 0.3))
    assert not torch.equal(out, ref)


@pytest.mark.gpu
def test_zero_pairs_or_frames_give_empty_outputs(lgu):
    poses, disps, intr = scene(91, N=4, H=12, W=16)
    P, D, K = dev(poses), dev(disps), dev(intr)
    e = torch.zeros(0, dtype=torch.int64, device="cuda")
    assert tuple(lgu.geom.frame_distance(P, D, K, e, e, 0.3).shape) == (0,)
    c, v = lgu.geom.projmap(P, D, K, e, e)
    assert tuple(c.shape) == (0, 12, 16, 3) and tuple(v.shape) == (0, 12, 16, 1)
    assert tuple(lgu.geom.depth_filter(P, D, K, e, torch.zeros(0, device="cuda")).shape) == (0, 12, 16)
    assert tuple(lgu.geom.iproj(P[:0], D[:0], K).shape) == (0, 12, 16, 3)
    torch.cuda.synchronize()
