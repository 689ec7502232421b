"""Dense bundle adjustment (started in round 1).

The reference's host driver of `droid_backends.ba` (src/droid_kernels.cu:1314-1434) needs Eigen and cannot be built in
this image; its kernels are built without it and checked in tests/test_droid_kernels_vs_reference_build.py.
oracle/ba_oracle.py restates the whole BA line by line; these tests pin
the restatement by what any correct Gauss-Newton BA must do on a synthetic scene whose targets are exact
reprojections: zero residual => zero update, quadratic convergence of the reprojection cost from perturbed poses and
depths (which fails for a wrong Jacobian), motion-only mode, and the fixed-pose window [t0, t1).
The HIP implementation (GPU tests below) is held to the oracle.
"""
import ctypes

import numpy as np
import pytest

from oracle import ba_oracle as O

f32 = np.float32


def project(poses, disps, intr, ii, jj):
    E = len(ii)
    H, W = disps.shape[1:]
    fx, fy, cx, cy = [float(v) for v in intr]
    v, u = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    out = np.zeros((E, 2, H, W), f32)
    for e in range(E):
        tij, qij = O.rel_se3(poses[ii[e], :3], poses[ii[e], 3:], poses[jj[e], :3], poses[jj[e], 3:])
        X = np.stack([(u - cx) / fx, (v - cy) / fy, np.ones_like(u)], -1).reshape(-1, 3)
        uvv = 2.0 * np.cross(qij[:3], X)
        Xj = X + qij[3] * uvv + np.cross(qij[:3], uvv) + disps[ii[e]].reshape(-1, 1) * tij[None]
        out[e, 0] = (fx * Xj[:, 0] / Xj[:, 2] + cx).reshape(H, W)
        out[e, 1] = (fy * Xj[:, 1] / Xj[:, 2] + cy).reshape(H, W)
    return out


def scene(seed=0, N=5, H=12, W=16, span=2):
    rng = np.random.default_rng(seed)
    intr = np.array([20.0, 20.0, W / 2, H / 2], f32)
    poses = np.zeros((N, 7), f32)
    poses[:, 6] = 1
    for k in range(1, N):
        t, q = O.exp_se3(np.concatenate([rng.standard_normal(3) * 0.3, rng.standard_normal(3) * 0.1]))
        poses[k, :3] = t
        poses[k, 3:] = q
    disps = (0.3 + 0.7 * rng.random((N, H, W))).astype(f32)
    ii = np.array([i for i in range(N) for j in range(N) if i != j and abs(i - j) <= span])
    jj = np.array([j for i in range(N) for j in range(N) if i != j and abs(i - j) <= span])
    targets = project(poses, disps, intr, ii, jj)
    return rng, intr, poses, disps, ii, jj, targets


def perturb(rng, poses, disps, t0):
    p, d = poses.copy(), disps.copy()
    for k in range(t0, len(p)):
        t_, q_ = O.retr_se3(np.concatenate([rng.standard_normal(3) * 0.02, rng.standard_normal(3) * 0.01]),
                            p[k, :3].astype(np.float64), p[k, 3:].astype(np.float64))
        p[k, :3] = t_
        p[k, 3:] = q_
    d[t0:] *= (1 + 0.05 * rng.standard_normal(d[t0:].shape)).astype(f32)
    return p, d


def cost(p, d, intr, ii, jj, targets):
    return float(((project(p, d, intr, ii, jj) - targets) ** 2).mean())


def test_oracle_zero_residual_gives_zero_update():
    rng, intr, poses, disps, ii, jj, targets = scene()
    p, d = poses.copy(), disps.copy()
    dx, dz = O.ba(p, d, intr, np.zeros_like(d), targets, np.ones_like(targets), np.full(d.shape, 1e-4, f32), ii, jj, 1, len(p), 1,
                  1e-4, 0.1, False)
    assert np.abs(dx).max() < 1e-6 and np.abs(dz).max() < 1e-5
    assert np.allclose(p, poses, atol=1e-6) and np.allclose(d, disps, atol=1e-5)


def test_oracle_converges_quadratically_and_respects_the_window():
    rng, intr, poses, disps, ii, jj, targets = scene(1)
    t0 = 2
    p, d = perturb(rng, poses, disps, t0)
    c = [cost(p, d, intr, ii, jj, targets)]
    for _ in range(5):
        O.ba(p, d, intr, np.zeros_like(d), targets, np.ones_like(targets), np.full(d.shape, 1e-6, f32), ii, jj, t0, len(p), 1, 1e-4,
             1e-6, False)
        c.append(cost(p, d, intr, ii, jj, targets))
    assert c[1] < 0.2 * c[0] and c[2] < 0.05 * c[1] and c[-1] < 1e-8 * c[0]
    assert np.array_equal(p[:t0], poses[:t0])   # poses before t0 are fixed


def test_oracle_motion_only_recovers_poses():
    rng, intr, poses, disps, ii, jj, targets = scene(2)
    p, _ = perturb(rng, poses, disps, 1)
    d = disps.copy()
    for _ in range(6):
        O.ba(p, d, intr, np.zeros_like(d), targets, np.ones_like(targets), np.zeros(d.shape, f32), ii, jj, 1, len(p), 1, 1e-4, 1e-6, True)
    assert np.array_equal(d, disps) and np.abs(p - poses).max() < 1e-4


# ---- HIP implementation against the oracle (GPU) ----
torch = pytest.importorskip("torch")


def _to_dev(*arrs):
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrs]


def _run_both(lgu, poses, disps, intr, sens, targets, weights, eta, ii, jj, t0, t1, iters, lm, ep, motion_only):
    po, do = poses.copy(), disps.copy()
    dxo, dzo = O.ba(po, do, intr, sens, targets, weights, eta, ii, jj, t0, t1, iters, lm, ep, motion_only)
    pd, dd, idv, sd, td, wd_, ed = _to_dev(poses, disps, intr, sens, targets, weights, eta)
    iid, jjd = _to_dev(ii.astype(np.int64), jj.astype(np.int64))
    dxd, dzd = lgu.ba.ba(pd, dd, idv, sd, td, wd_, ed, iid, jjd, t0, t1, iters, lm, ep, motion_only)
    torch.cuda.synchronize()
    return (po, do, dxo, dzo), (pd.cpu().numpy(), dd.cpu().numpy(), dxd.cpu().numpy(), None if dzd is None else dzd.cpu().numpy())


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", [dict(seed=3, t0=1, motion_only=False, sens=False, stereo=False, iters=1),
                                 dict(seed=4, t0=2, motion_only=False, sens=True, stereo=False, iters=2),
                                 dict(seed=5, t0=1, motion_only=True, sens=False, stereo=False, iters=2),
                                 dict(seed=6, t0=1, motion_only=False, sens=False, stereo=True, iters=1)])
def test_hip_ba_matches_oracle(lgu, cfg):
    """One or two Gauss-Newton iterations from a perturbed state: poses, disparities and the returned dx / dz of the
    device implementation against the numpy restatement (float32 kernels vs float64 sums: 2e-4 relative to the update)."""
    rng, intr, poses, disps, ii, jj, targets = scene(cfg["seed"], N=5, H=12, W=16)
    if cfg["stereo"]:   # stereo factors ii == jj (fixed baseline): targets need not be consistent for this comparison
        ii = np.concatenate([ii, np.arange(1, 4)])
        jj = np.concatenate([jj, np.arange(1, 4)])
        targets = np.concatenate([targets, targets[:3] + 0.1], 0)
    p, d = perturb(rng, poses, disps, cfg["t0"])
    weights = (0.5 + rng.random(targets.shape)).astype(f32)
    sens = (d * (rng.random(d.shape) > 0.5)).astype(f32) if cfg["sens"] else np.zeros_like(d)
    eta = np.full(d.shape, 1e-3, f32)
    (po, do, dxo, dzo), (pd, dd, dxd, dzd) = _run_both(lgu, p, d, intr, sens, targets, weights, eta, ii, jj, cfg["t0"], len(p),
                                                       cfg["iters"], 1e-4, 0.1, cfg["motion_only"])
    scale = max(np.abs(dxo).max(), 1e-6)
    assert np.abs(dxd - dxo).max() <= 2e-4 * scale + 1e-7
    assert np.abs(pd - po).max() <= 2e-4 * max(np.abs(po - p).max(), 1e-6) + 1e-6
    if cfg["motion_only"]:
        assert dzd is None and np.array_equal(dd, d)
    else:
        assert np.abs(dzd - dzo).max() <= 2e-4 * max(np.abs(dzo).max(), 1e-6) + 1e-7
        assert np.abs(dd - do).max() <= 2e-4 * max(np.abs(do - d).max(), 1e-6) + 1e-6
    assert np.array_equal(pd[:cfg["t0"]], p[:cfg["t0"]])


@pytest.mark.gpu
def test_hip_ba_converges_on_a_frontend_sized_window(lgu):
    """12 keyframes of 48x64 (the frontend window), 5 iterations in one call: the reprojection cost of exact targets
    drops by > 8 orders of magnitude, as with the oracle on the small scene."""
    rng, intr, poses, disps, ii, jj, targets = scene(7, N=8, H=24, W=32, span=3)
    p, d = perturb(rng, poses, disps, 2)
    c0 = cost(p, d, intr, ii, jj, targets)
    pd, dd, idv, sd, td, wd_, ed = _to_dev(p, d, intr, np.zeros_like(d), targets, np.ones_like(targets), np.full(d.shape, 1e-6, f32))
    iid, jjd = _to_dev(ii.astype(np.int64), jj.astype(np.int64))
    lgu.ba.ba(pd, dd, idv, sd, td, wd_, ed, iid, jjd, 2, len(p), 6, 1e-4, 1e-6, False)
    c1 = cost(pd.cpu().numpy(), dd.cpu().numpy(), intr, ii, jj, targets)
    assert c1 < 1e-6 * c0


@pytest.mark.gpu
def test_hip_ba_larger_graph_with_fixed_source_frames(lgu):
    """40 frames, ~230 edges, window [5, 40): edges whose source or target frame lies before t0 contribute to the
    depth / pose blocks they touch but get no pose update of their own (update_lhs / update_rhs skip negative block
    indices); device result against the oracle."""
    rng, intr, poses, disps, ii, jj, targets = scene(11, N=40, H=8, W=12, span=3)
    t0 = 5
    p, d = perturb(rng, poses, disps, t0)
    weights = (0.5 + rng.random(targets.shape)).astype(f32)
    eta = np.full(d.shape, 1e-3, f32)
    (po, do, dxo, dzo), (pd, dd, dxd, dzd) = _run_both(lgu, p, d, intr, np.zeros_like(d), targets, weights, eta, ii, jj, t0, len(p), 1,
                                                       1e-4, 0.1, False)
    assert np.abs(dxd - dxo).max() <= 5e-4 * np.abs(dxo).max() + 1e-7
    assert np.abs(dzd - dzo).max() <= 5e-4 * np.abs(dzo).max() + 1e-7
    assert np.array_equal(pd[:t0], p[:t0]) and np.abs(pd - po).max() <= 5e-4 * np.abs(po - p).max() + 1e-6


@pytest.mark.gpu
def test_sharded_ba_world1_equals_plain_ba(lgu):
    """sharded.sharded_ba at world size 1: per-edge target / weight handed over in the owner's chunk order come back in
    the original edge order and the replicated BA equals the plain call bit for bit."""
    rng, intr, poses, disps, ii, jj, targets = scene(13, N=12, H=8, W=12, span=2)
    p, d = perturb(rng, poses, disps, 1)
    weights = (0.5 + rng.random(targets.shape)).astype(f32)
    eta = np.full(d.shape, 1e-3, f32)
    iid, jjd = _to_dev(ii.astype(np.int64), jj.astype(np.int64))
    edges = lgu.sharded.ShardedEdgeSet(iid, rank=0, world=1, chunk=4)
    own = edges.my_edges.cpu().numpy()
    assert not np.array_equal(own, np.arange(len(ii))) or len(own) == len(ii)
    args = _to_dev(intr, np.zeros_like(d))
    td, wd_, ed = _to_dev(targets, weights, eta)
    p1, d1 = _to_dev(p, d)
    p2, d2 = _to_dev(p, d)
    a = lgu.ba.ba(p1, d1, args[0], args[1], td, wd_, ed, iid, jjd, 1, len(p), 2, 1e-4, 0.1, False)
    b = lgu.sharded.sharded_ba(edges, td[edges.my_edges].contiguous(), wd_[edges.my_edges].contiguous(), p2, d2, args[0], args[1], ed,
                               iid, jjd, 1, len(p), 2, 1e-4, 0.1, False)
    assert torch.equal(p1, p2) and torch.equal(d1, d2) and torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    # the reference's loop bound range(0, jj.max()+1, chunk) (factor_graph.py:273) leaves the edges of late source frames
    # unprocessed: they enter the BA with their PREVIOUS target / weight, which live in the persistent tensors
    jj_low = torch.clamp(jjd, max=7)                            # bound = 8 -> chunks [0,4), [4,8): source frames >= 8 have no chunk
    edges_u = lgu.sharded.ShardedEdgeSet(iid, rank=0, world=1, chunk=4, jj=jj_low)
    assert edges_u.unprocessed.numel() > 0
    own_u = edges_u.my_edges
    with pytest.raises(ValueError, match="previous target"):
        lgu.sharded.sharded_ba(edges_u, td[own_u].contiguous(), wd_[own_u].contiguous(), p2, d2, args[0], args[1], ed, iid, jjd, 1,
                               len(p), 2, 1e-4, 0.1, False)
    t_state, w_state = td.clone(), wd_.clone()                  # previous values of every edge
    t_new, w_new = td * 1.01, wd_ * 0.9                         # this step's results for the processed edges
    p3, d3 = _to_dev(p, d)
    p4, d4 = _to_dev(p, d)
    lgu.sharded.sharded_ba(edges_u, t_new[own_u].contiguous(), w_new[own_u].contiguous(), p3, d3, args[0], args[1], ed, iid, jjd, 1,
                           len(p), 2, 1e-4, 0.1, False, target=t_state, weight=w_state)
    t_want, w_want = td.clone(), wd_.clone()
    t_want[own_u], w_want[own_u] = t_new[own_u], w_new[own_u]
    assert torch.equal(t_state, t_want) and torch.equal(w_state, w_want)
    lgu.ba.ba(p4, d4, args[0], args[1], t_want, w_want, ed, iid, jjd, 1, len(p), 2, 1e-4, 0.1, False)
    assert torch.equal(p3, p4) and torch.equal(d3, d4)


def _split_ba_worker(rank, world, port, q):
    """One rank of test_sharded_ba_split_two_ranks_on_one_gpu (spawned; both ranks use the same GPU, gloo collectives)."""
    import os
    import sys
    import torch.distributed as dist
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    import lgu_slam_amd as lgu
    dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%d" % port, rank=rank, world_size=world)
    try:
        rng, intr, poses, disps, ii, jj, targets = scene(21, N=40, H=8, W=12, span=3)
        t0 = 2
        p, d = perturb(rng, poses, disps, t0)
        weights = (0.5 + rng.random(targets.shape)).astype(f32)
        eta = (1e-3 + 1e-3 * rng.random(d.shape)).astype(f32)          # per-frame damping: rows must follow the depth frames
        iid, jjd = _to_dev(ii.astype(np.int64), jj.astype(np.int64))
        td, wd_, ed, intr_d, sens = _to_dev(targets, weights, eta, intr, np.zeros_like(d))
        edges = lgu.sharded.ShardedEdgeSet(iid, chunk=8)               # jj=None: every edge is in some chunk
        assert edges.world == world and 0 < edges.counts[rank] < len(ii)
        p1, d1 = _to_dev(p, d)
        own = edges.my_edges
        # only the owner's damping rows (and those of frames nobody owns) are read: the rows of the OTHER rank's frames
        # hold garbage here (0 * inf = NaN would be all-reduced into every rank's system)
        ed_local = ed.clone()
        ed_local[edges.frames[1 - rank]] = float("nan") if rank == 0 else 0.0
        out = lgu.sharded.sharded_ba_split(edges, td[own].contiguous(), wd_[own].contiguous(), p1, d1, intr_d, sens, ed_local, iid, jjd,
                                           t0, len(p), 2, 1e-4, 0.1, False)
        p2, d2 = _to_dev(p, d)
        kx = torch.unique(torch.cat([torch.arange(t0, len(p), device=iid.device), iid]))
        lgu.ba.ba(p2, d2, intr_d, sens, td, wd_, ed[kx].contiguous(), iid, jjd, t0, len(p), 2, 1e-4, 0.1, False)   # replicated, all edges
        sig = torch.stack([p1.double().sum(), p1.double().abs().sum(), d1.double().sum(), d1.double().abs().sum()]).cpu()
        lo, hi = sig.clone(), sig.clone()
        dist.all_reduce(lo, op=dist.ReduceOp.MIN)
        dist.all_reduce(hi, op=dist.ReduceOp.MAX)
        q.put((rank, edges.counts, bool(torch.equal(lo, hi)),
               float((p1 - p2).abs().max()), float((p2 - _to_dev(p)[0]).abs().max()),
               float((d1 - d2).abs().max()), float((d2 - _to_dev(d)[0]).abs().max()), bool(torch.isfinite(out[0]).all())))
    finally:
        dist.destroy_process_group()


@pytest.mark.gpu
def test_sharded_ba_split_two_ranks_on_one_gpu(lgu):
    """sharded.sharded_ba_split (VERDICT r1 #6b): two ranks (gloo, both on this GPU) each build the blocks of the edges
    they own and the Schur products of the depth frames they own, all-reduce the reduced camera system, solve it
    replicated and all-gather the owners' disparity rows.  Both ranks end with bit-identical poses / disps, which equal
    the replicated BA over all edges up to the order in which the system is summed (1e-4 of the update); world 1 is the
    plain call."""
    import os
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 30100 + (os.getpid() % 1500)
    procs = [ctx.Process(target=_split_ba_worker, args=(r, 2, port, q)) for r in range(2)]
    for pr in procs:
        pr.start()
    res = sorted(q.get(timeout=240) for _ in procs)
    for pr in procs:
        pr.join(timeout=60)
        assert pr.exitcode == 0
    for rank, counts, agree, dp, up, dd, ud, finite in res:
        assert agree and finite and sum(counts) > 0 and min(counts) > 0
        assert up > 1e-4 and ud > 1e-4                      # the BA moved poses and depths
        assert dp <= 1e-4 * up + 1e-7 and dd <= 1e-4 * ud + 1e-7, (dp, up, dd, ud)
    # world 1: the split form is the plain call
    rng, intr, poses, disps, ii, jj, targets = scene(13, N=12, H=8, W=12, span=2)
    p, d = perturb(rng, poses, disps, 1)
    weights = (0.5 + rng.random(targets.shape)).astype(f32)
    eta = np.full(d.shape, 1e-3, f32)
    iid, jjd = _to_dev(ii.astype(np.int64), jj.astype(np.int64))
    td, wd_, ed, intr_d, sens = _to_dev(targets, weights, eta, intr, np.zeros_like(d))
    edges = lgu.sharded.ShardedEdgeSet(iid, rank=0, world=1, chunk=4)
    p1, d1 = _to_dev(p, d)
    p2, d2 = _to_dev(p, d)
    own = edges.my_edges
    lgu.sharded.sharded_ba_split(edges, td[own].contiguous(), wd_[own].contiguous(), p1, d1, intr_d, sens, ed, iid, jjd, 1, len(p), 2,
                                 1e-4, 0.1, False)
    lgu.ba.ba(p2, d2, intr_d, sens, td[own].contiguous(), wd_[own].contiguous(), ed, iid[own].contiguous(), jjd[own].contiguous(),
              1, len(p), 2, 1e-4, 0.1, False)
    assert torch.equal(p1, p2) and torch.equal(d1, d2)


@pytest.mark.gpu
def test_hip_ba_is_bit_reproducible(lgu):
    """Replicated BA on every rank of a sharded run must give the same bits: two runs from the same state are identical
    (fixed-order block reductions and assembly, no atomics)."""
    rng, intr, poses, disps, ii, jj, targets = scene(19, N=10, H=12, W=16, span=3)
    p, d = perturb(rng, poses, disps, 1)
    outs = []
    for _ in range(2):
        pd, dd, idv, sd, td, wd_, ed = _to_dev(p, d, intr, np.zeros_like(d), targets, np.ones_like(targets), np.full(d.shape, 1e-3, f32))
        iid, jjd = _to_dev(ii.astype(np.int64), jj.astype(np.int64))
        dx, dz = lgu.ba.ba(pd, dd, idv, sd, td, wd_, ed, iid, jjd, 1, len(p), 3, 1e-4, 0.1, False)
        outs.append((pd.clone(), dd.clone(), dx.clone(), dz.clone()))
    assert all(torch.equal(a, b) for a, b in zip(*outs))


@pytest.mark.gpu
@pytest.mark.parametrize("motion_only", [False, True])
def test_fused_assembly_equals_the_scatter_sum_composition(lgu, motion_only):
    """lgu_ba_assemble_f64 (the whole reduced camera system in one launch) == zero-fill + lgu_ba_scatter_sum_f64 of the H
    blocks, minus that of the Schur blocks, + the blocked -> dense permutation, BIT FOR BIT (same per-entry arithmetic
    and summation order), on the index tables of a real graph."""
    from lgu_slam_amd import ba as B
    rng, intr, poses, disps, ii, jj, targets = scene(31, N=9, H=6, W=8, span=3)
    t0, t1 = 2, len(poses)
    P, E = t1 - t0, len(ii)
    lib = lgu._lib.load()
    pl = B._Plan(lib, ii.astype(np.int64), jj.astype(np.int64), t0, t1, motion_only, torch.device("cuda"))
    g = torch.Generator(device="cuda"); g.manual_seed(5)
    Hs = torch.randn(4 * E, 36, device="cuda", generator=g)
    vs = torch.randn(2 * E, 6, device="cuda", generator=g)
    ii_h, jj_h = ii.astype(np.int64), jj.astype(np.int64)
    bi = np.concatenate([ii_h, ii_h, jj_h, jj_h]) - t0
    bj = np.concatenate([ii_h, jj_h, ii_h, jj_h]) - t0
    st = torch.cuda.current_stream().cuda_stream
    A = torch.zeros(P * P, 36, dtype=torch.float64, device="cuda")
    b = torch.zeros(P, 6, dtype=torch.float64, device="cuda")
    B._ScatterSum(lib, np.where((bi >= 0) & (bj >= 0), bi * P + bj, -1), "cuda")(Hs, A, 1.0, st)
    B._ScatterSum(lib, np.concatenate([ii_h, jj_h]) - t0, "cuda")(vs, b, 1.0, st)
    S = sv = None
    if not motion_only:
        trip = pl.trip_t.cpu().numpy()
        ts = np.arange(t0, t1)
        jj_exp = np.concatenate([ts, jj_h])
        S = torch.randn(trip.shape[0], 36, device="cuda", generator=g)
        sv = torch.randn(P + E, 6, device="cuda", generator=g)
        B._ScatterSum(lib, (jj_exp[trip[:, 0]] - t0) * P + (jj_exp[trip[:, 1]] - t0), "cuda")(S, A, -1.0, st)
        # the plan lists the pairs a <= c of a depth frame only: block (c, a) is the transpose of block (a, c)
        assert (trip[:, 0] <= trip[:, 1]).all() and (trip[:, 0] < trip[:, 1]).any()
        St = S.view(-1, 6, 6).transpose(1, 2).reshape(-1, 36).contiguous()
        B._ScatterSum(lib, np.where(trip[:, 0] != trip[:, 1], (jj_exp[trip[:, 1]] - t0) * P + (jj_exp[trip[:, 0]] - t0), -1), "cuda")(St, A, -1.0, st)
        B._ScatterSum(lib, jj_exp - t0, "cuda")(sv, b, -1.0, st)
    want = A.view(P, P, 6, 6).permute(0, 2, 1, 3).reshape(6 * P, 6 * P).contiguous()
    Ad = torch.full((6 * P, 6 * P), 7.0, dtype=torch.float64, device="cuda")
    bd = torch.full((P, 6), 7.0, dtype=torch.float64, device="cuda")
    vp = lambda t_: ctypes.c_void_p(t_.data_ptr()) if t_ is not None else None
    cS, cs = (pl.csr_S, pl.csr_sv) if not motion_only else (None, None)
    rc = lib.lgu_ba_assemble_f64(vp(Hs), vp(pl.csr_H[0]), vp(pl.csr_H[1]), vp(S), vp(cS[0]) if cS else None, vp(cS[1]) if cS else None,
                                 vp(vs), vp(pl.csr_v[0]), vp(pl.csr_v[1]), vp(sv), vp(cs[0]) if cs else None, vp(cs[1]) if cs else None,
                                 vp(Ad), vp(bd), P, st)
    assert rc == 0
    assert torch.equal(Ad, want) and torch.equal(bd, b)
    assert float(want.abs().max()) > 0


@pytest.mark.gpu
def test_hip_ba_plan_cache_follows_the_graph(lgu):
    """The graph-dependent index tables are cached per edge set (the factor graph runs many BA calls on one graph):
    a cached plan gives the bits a fresh plan gives, a changed edge list / window / mode gets its own plan, and the
    cache stays bounded."""
    rng, intr, poses, disps, ii, jj, targets = scene(23, N=9, H=12, W=16, span=3)
    p, d = perturb(rng, poses, disps, 1)

    def run(ii_, jj_, tg, t0, motion_only, clear):
        if clear:
            lgu.ba._PLANS.clear()
        pd, dd, idv, sd, td, wd_, ed = _to_dev(p, d, intr, np.zeros_like(d), tg, np.ones_like(tg), np.full(d.shape, 1e-3, f32))
        iid, jjd = _to_dev(ii_.astype(np.int64), jj_.astype(np.int64))
        dx, dz = lgu.ba.ba(pd, dd, idv, sd, td, wd_, ed, iid, jjd, t0, len(p), 2, 1e-4, 0.1, motion_only)
        return [pd.clone(), dd.clone(), dx.clone()] + ([dz.clone()] if dz is not None else [])

    keep = np.arange(len(ii)) % 3 != 0          # a second graph: a third of the edges dropped
    cases = [(ii, jj, targets, 1, False), (ii[keep], jj[keep], targets[keep], 1, False), (ii, jj, targets, 2, False),
             (ii, jj, targets, 1, True)]
    fresh = [run(*c, clear=True) for c in cases]
    lgu.ba._PLANS.clear()
    for rep in range(2):                         # second round: every plan comes from the cache
        for c, want in zip(cases, fresh):
            got = run(*c, clear=False)
            assert all(torch.equal(a, b) for a, b in zip(got, want))
    assert len(lgu.ba._PLANS) == len(cases)
    for k in range(lgu.ba._PLANS_MAX + 3):       # bounded
        sel = np.arange(len(ii)) != k
        run(ii[sel], jj[sel], targets[sel], 1, False, clear=False)
    assert len(lgu.ba._PLANS) == lgu.ba._PLANS_MAX


@pytest.mark.gpu
@pytest.mark.parametrize("P", [1, 3, 11, 21, 25, 32])
def test_device_cholesky_solve_against_numpy(lgu, P):
    """lgu_ba_solve_f64: (A + diag(ep + lm diag A)) x = b in one workgroup with the matrix in LDS (packed lower triangle, 6P <= 192:
    frontend windows of up to 32 keyframes), against numpy.linalg in double; a matrix that is not positive definite gives x = 0, as the
    reference's Eigen path does; larger systems are reported unsupported (the glue then uses a library factorisation)."""
    import ctypes
    rng = np.random.default_rng(100 + P)
    n = 6 * P
    M = rng.standard_normal((n, n))
    A = M @ M.T + 0.5 * np.eye(n)
    b = rng.standard_normal(n)
    lm, ep = 1e-4, 0.1
    L = A.copy()
    L[np.diag_indices(n)] += ep + lm * np.diag(A)
    want = np.linalg.solve(L, b)
    lib = lgu._lib.load()

    def solve(Am, Pn=P):
        Ad = torch.from_numpy(np.ascontiguousarray(Am)).cuda()
        bd = torch.from_numpy(b).cuda()
        x = torch.full((Pn, 6), 7.0, dtype=torch.float32, device="cuda")
        rc = lib.lgu_ba_solve_f64(ctypes.c_void_p(Ad.data_ptr()), ctypes.c_void_p(bd.data_ptr()), ctypes.c_void_p(x.data_ptr()), Pn, lm,
                                  ep, None)
        torch.cuda.synchronize()
        assert torch.equal(Ad.cpu(), torch.from_numpy(np.ascontiguousarray(Am)))   # A is not modified
        return rc, x.cpu().numpy().reshape(-1)

    rc, got = solve(A)
    assert rc == 0 and np.abs(got - want).max() <= 2e-6 * max(1.0, np.abs(want).max())      # float32 output of a double solve
    Abad = A.copy()
    Abad[n // 2, n // 2] = -5.0 * np.abs(A).max()
    rc, got = solve(Abad)
    assert rc == 0 and not got.any()
    if P == 32:
        big = torch.eye(6 * 33, dtype=torch.float64, device="cuda")
        rc = lib.lgu_ba_solve_f64(ctypes.c_void_p(big.data_ptr()), ctypes.c_void_p(torch.zeros(198, dtype=torch.float64, device="cuda").data_ptr()),
                                  ctypes.c_void_p(torch.zeros(33, 6, device="cuda").data_ptr()), 33, lm, ep, None)
        assert rc == lgu._lib.LGU_E_UNSUPPORTED


@pytest.mark.gpu
@pytest.mark.parametrize("P", [33, 40, 77, 200])
def test_blocked_device_cholesky_solve_against_numpy(lgu, P):
    """lgu_ba_solve_blocked_f64 (csrc/ba_chol.hip; windows of more than 32 keyframes, e.g. the 200-keyframe global BA of
    BASELINE config 5): damping, blocked Cholesky (32-column panels, the right-hand side as row 6P), back substitution —
    against numpy.linalg in double, on a banded-plus-loop-closure matrix shaped like a reduced camera system; sizes that
    are and are not multiples of the panel width; not positive definite -> x = 0; A is overwritten, b is not."""
    import ctypes
    rng = np.random.default_rng(700 + P)
    n = 6 * P
    M = rng.standard_normal((n, n))
    band = np.abs(np.subtract.outer(np.arange(n), np.arange(n))) <= 30
    M = M * band
    M[:12, -12:] = rng.standard_normal((12, 12))           # a loop closure far off the band
    A = M @ M.T + 0.5 * np.eye(n)
    b = rng.standard_normal(n)
    lm, ep = 1e-4, 0.1
    Ld = A.copy()
    Ld[np.diag_indices(n)] += ep + lm * np.diag(A)
    want = np.linalg.solve(Ld, b)
    lib = lgu._lib.load()
    nwork = int(lib.lgu_ba_solve_blocked_work_doubles(P))
    assert nwork >= n + 1

    def solve(Am):
        Ad = torch.from_numpy(np.ascontiguousarray(Am)).cuda()
        bd = torch.from_numpy(b).cuda()
        x = torch.full((P, 6), 7.0, dtype=torch.float32, device="cuda")
        work = torch.empty(nwork, dtype=torch.float64, device="cuda")
        rc = lib.lgu_ba_solve_blocked_f64(ctypes.c_void_p(Ad.data_ptr()), ctypes.c_void_p(bd.data_ptr()), ctypes.c_void_p(x.data_ptr()),
                                          ctypes.c_void_p(work.data_ptr()), P, lm, ep, None)
        torch.cuda.synchronize()
        assert torch.equal(bd.cpu(), torch.from_numpy(b))
        return rc, x.cpu().numpy().reshape(-1), Ad.cpu().numpy()

    rc, got, fac = solve(A)
    assert rc == 0 and np.abs(got - want).max() <= 2e-6 * max(1.0, np.abs(want).max())      # float32 output of a double solve
    Lw = np.linalg.cholesky(Ld)
    assert np.abs(np.tril(fac) - Lw).max() <= 1e-9 * np.abs(Lw).max()                         # A now holds the factor
    Abad = A.copy()
    Abad[n // 2, n // 2] = -5.0 * np.abs(A).max()
    rc, got, _ = solve(Abad)
    assert rc == 0 and not got.any()


# ---- independent check of the Jacobians: central finite differences of the projection ---------------------------------
# Nothing below touches oracle/ba_oracle.py: the forward model (SE3 exponential, quaternion action on a homogeneous point
# with disparity, pinhole projection) is written out here in fp64 from the geometry, and every output of the build kernel
# (reference projective_transform_kernel, src/droid_kernels.cu:176-425) is rebuilt from numerical derivatives of it.

def _fd_quat_mul(a, b):
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx,
                     aw * bz + ax * by - ay * bx + az * bw, aw * bw - ax * bx - ay * by - az * bz])


def _fd_quat_rot(q, X):
    x, y, z, w = q
    Rm = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                   [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                   [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
    return X @ Rm.T


def _fd_exp_se3(xi):
    """exp of a twist (translation part first): rotation exp(phi), translation V(phi) tau."""
    tau, phi = xi[:3], xi[3:]
    th = np.linalg.norm(phi)
    K = np.array([[0, -phi[2], phi[1]], [phi[2], 0, -phi[0]], [-phi[1], phi[0], 0]])
    if th < 1e-12:
        V = np.eye(3) + 0.5 * K
        q = np.concatenate([0.5 * phi, [1.0]])
    else:
        V = np.eye(3) + (1 - np.cos(th)) / th ** 2 * K + (th - np.sin(th)) / th ** 3 * (K @ K)
        q = np.concatenate([np.sin(th / 2) * phi / th, [np.cos(th / 2)]])
    return V @ tau, q / np.linalg.norm(q)


def _fd_left_perturb(pose, xi):
    """exp(xi) * pose for pose = (t, q xyzw), a world-to-camera transform acting as X -> R X + t."""
    t, q = _fd_exp_se3(xi)
    return np.concatenate([_fd_quat_rot(q, pose[None, :3])[0] + t, _fd_quat_mul(q, pose[3:])])


def _fd_project(pi, pj, disp, intr, stereo):
    """Pixels of frame i (disparity `disp` (H,W)) seen in frame j: (2,H,W).  G_ij = G_j G_i^-1 (fixed baseline if stereo)."""
    fx, fy, cx, cy = intr
    H, W = disp.shape
    v, u = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    X = np.stack([(u - cx) / fx, (v - cy) / fy, np.ones_like(u)], -1).reshape(-1, 3)
    if stereo:
        tij, qij = np.array([-0.1, 0.0, 0.0]), np.array([0.0, 0.0, 0.0, 1.0])
    else:
        qi_inv = pi[3:] * np.array([-1, -1, -1, 1.0])
        qij = _fd_quat_mul(pj[3:], qi_inv)
        tij = pj[:3] - _fd_quat_rot(qij, pi[None, :3])[0]
    Xj = _fd_quat_rot(qij, X) + disp.reshape(-1, 1) * tij[None]
    return np.stack([fx * Xj[:, 0] / Xj[:, 2] + cx, fy * Xj[:, 1] / Xj[:, 2] + cy]).reshape(2, H, W), Xj[:, 2].min()


@pytest.mark.gpu
def test_build_kernel_jacobians_match_finite_differences(lgu):
    """Hs, vs, Eii, Eij, Cii, wi of lgu_ba_build_f32 against central finite differences of an independent fp64 forward
    model — for a temporal edge, its reverse, and a stereo edge (ii == jj: fixed baseline, pose terms zeroed)."""
    import torch
    rng = np.random.default_rng(12)
    N, H, W = 3, 10, 12
    intr = np.array([18.0, 17.0, W / 2 - 0.3, H / 2 + 0.2])
    poses = np.zeros((N, 7))
    poses[:, 6] = 1
    for k in range(1, N):
        poses[k] = _fd_left_perturb(poses[k], np.concatenate([rng.standard_normal(3) * 0.2, rng.standard_normal(3) * 0.08]))
    disps = 0.4 + 0.6 * rng.random((N, H, W))
    ii, jj = np.array([0, 1, 2, 1]), np.array([1, 0, 1, 1])
    E, HW = len(ii), H * W
    targets = np.stack([_fd_project(poses[i], poses[j], disps[i], intr, i == j)[0] for i, j in zip(ii, jj)])
    targets = targets + rng.standard_normal(targets.shape) * 0.7         # non-zero residuals
    weights = rng.random((E, 2, H, W)) + 0.1

    dev = "cuda"
    t = lambda a, dt=torch.float32: torch.from_numpy(np.ascontiguousarray(a)).to(dev).to(dt).contiguous()  # noqa: E731
    lib = lgu._lib.load()
    Hs = torch.empty(4, E, 6, 6, device=dev)
    vs = torch.empty(2, E, 6, device=dev)
    Eii, Eij = torch.empty(E, 6, HW, device=dev), torch.empty(E, 6, HW, device=dev)
    Cii, wi = torch.empty(E, HW, device=dev), torch.empty(E, HW, device=dev)
    scratch = torch.empty(E * lib.lgu_ba_build_slices(E) * 90, device=dev)
    args = [t(targets), t(weights), t(poses), t(disps), t(intr), t(ii, torch.int64), t(jj, torch.int64)]
    vp = ctypes.c_void_p
    rc = lib.lgu_ba_build_f32(*[vp(a.data_ptr()) for a in args], *[vp(a.data_ptr()) for a in (Hs, vs, Eii, Eij, Cii, wi, scratch)],
                              E, H, W, vp(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    torch.cuda.synchronize()
    Hs, vs, Eii, Eij, Cii, wi = [a.double().cpu().numpy() for a in (Hs, vs, Eii, Eij, Cii, wi)]

    h = 1e-5
    for e, (i, j) in enumerate(zip(ii, jj)):
        stereo = i == j
        f0, zmin = _fd_project(poses[i], poses[j], disps[i], intr, stereo)
        assert zmin > 0.3                                                    # every point in front of MIN_DEPTH
        Ji, Jj = np.zeros((6, 2, HW)), np.zeros((6, 2, HW))
        for k in range(6):
            d = np.zeros(6)
            d[k] = h
            if not stereo:
                Jj[k] = ((_fd_project(poses[i], _fd_left_perturb(poses[j], d), disps[i], intr, False)[0]
                          - _fd_project(poses[i], _fd_left_perturb(poses[j], -d), disps[i], intr, False)[0]) / (2 * h)).reshape(2, HW)
                Ji[k] = ((_fd_project(_fd_left_perturb(poses[i], d), poses[j], disps[i], intr, False)[0]
                          - _fd_project(_fd_left_perturb(poses[i], -d), poses[j], disps[i], intr, False)[0]) / (2 * h)).reshape(2, HW)
        Jz = ((_fd_project(poses[i], poses[j], disps[i] + h, intr, stereo)[0]
               - _fd_project(poses[i], poses[j], disps[i] - h, intr, stereo)[0]) / (2 * h)).reshape(2, HW)
        w = 0.001 * weights[e].reshape(2, HW)                                # the kernel's weight scale (:309-310)
        r = (targets[e] - f0).reshape(2, HW)
        wp = np.zeros_like(w) if stereo else w                               # pose terms of a stereo edge carry no weight (:331,:369)
        want_v = [np.einsum("cp,cp,kcp->k", wp, r, J) for J in (Ji, Jj)]
        want_H = [np.einsum("cp,kcp,lcp->kl", wp, A, B) for A, B in ((Ji, Ji), (Ji, Jj), (Jj, Ji), (Jj, Jj))]
        want_E = [np.einsum("cp,cp,kcp->kp", wp, Jz, J) for J in (Ji, Jj)]
        want_C = (w * Jz * Jz).sum(0)                                        # the depth terms keep the weight (:328-329)
        want_w = (w * r * Jz).sum(0)

        def close(got, want, what):
            scale = max(np.abs(want).max(), 1e-6)
            assert np.abs(got - want).max() <= 2e-4 * scale + 1e-7, (what, e, np.abs(got - want).max(), scale)
        for m in range(2):
            close(vs[m, e], want_v[m], "vs[%d]" % m)
        for m in range(4):
            close(Hs[m, e], want_H[m], "Hs[%d]" % m)
        close(Eii[e], want_E[0], "Eii")
        close(Eij[e], want_E[1], "Eij")
        close(Cii[e], want_C, "Cii")
        close(wi[e], want_w, "wi")
