"""Host-side logic that needs no GPU: operator-layer argument checking (reference error
text, loud failure without a device), drop-in module surface, offset generation, the
Gaussian-mask parameter layout, and the edge-sharding / all-gather path under gloo with
world_size 2."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ops_fail_loudly_without_a_device(lgu):
    v = torch.zeros(1, 2, 2, 2, 4)
    c = torch.zeros(1, 2, 2, 2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        lgu.ops.corr_index_forward(v, c, 1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        lgu.ops.defcorr_pyramid_forward([v], c, [None], 1)


def test_contiguity_error_text_matches_reference(lgu):
    # reference: TORCH_CHECK(x.is_contiguous(), "volume must be contiguous") (offersample_LGS/droid.cpp:48-49)
    v = torch.zeros(1, 2, 2, 4, 2).transpose(3, 4)
    with pytest.raises(RuntimeError, match="^volume must be contiguous$"):
        lgu.ops.corr_index_forward(v, torch.zeros(1, 2, 2, 2), 1)
    with pytest.raises(RuntimeError, match="^coords must be contiguous$"):
        lgu.ops.corr_index_forward(torch.zeros(1, 2, 2, 2, 4), torch.zeros(1, 2, 2, 2).transpose(2, 3), 1)


def test_missing_library_raises(lgu, monkeypatch):
    monkeypatch.setattr(lgu._lib, "_lib", None)
    monkeypatch.setattr(lgu._build, "SO_PATH", "/nonexistent/liblgu_corr.so")
    with pytest.raises(RuntimeError, match="no CPU\\s+fallback|missing"):
        lgu._lib.load()


def test_dropin_modules_expose_reference_names(lgu):
    d, b = lgu.install_dropins()
    for n in ("gaussianMask", "gaussianMask_backward", "lowMem_defSample", "corr_index_forward",
              "corr_index_backward", "defCorr_index_forward", "defCorr_index_backward"):
        assert callable(getattr(d, n))  # offersample_LGS/droid.cpp:138-147
    assert callable(b.altcorr_forward) and callable(b.altcorr_backward)  # src/droid.cpp:246-247
    with pytest.raises(NotImplementedError):
        b.ba()
    assert sys.modules["defCorrSample"] is d


def test_generate_offsets_matches_reference_formula(lgu):
    torch.manual_seed(0)
    E, h, w = 2, 12, 16
    feats = torch.randn(E, 256, h, w)
    ofsMap = nn.Conv2d(256, 98, 3, padding=1)
    ofsRes = nn.Conv2d(256, 98, 3, padding=1)
    offs, zero = lgu.corr.generate_offsets(ofsMap, ofsRes, feats, 4)
    assert [tuple(o.shape) for o in offs] == [(E, h, w, 98)] * 4 and zero == [False, False, True, True]
    assert float(offs[0].abs().max()) < 4 and float(offs[1].abs().max()) < 4
    assert not offs[2].any() and not offs[3].any()

    def pcn(x):  # reference corr.py:44-51
        m = x.mean(dim=[1, 2, 3], keepdim=True)
        return (x - m) / torch.sqrt(x.var(dim=[1, 2, 3], unbiased=False, keepdim=True) + 1e-5)
    o0 = torch.tanh(pcn(ofsMap(feats))) * 4
    o1 = nn.functional.interpolate(ofsRes(nn.functional.avg_pool2d(feats, 2, 2)), (h, w))
    o1 = (torch.tanh(pcn(o1)) * 4 + o0) / 2
    assert torch.allclose(offs[0], o0.permute(0, 2, 3, 1), atol=1e-6)
    assert torch.allclose(offs[1], o1.permute(0, 2, 3, 1), atol=1e-6)


def test_gaussian_mask_parameter_names_and_grid(lgu):
    ga = lgu.GaussianMask(6, 8)
    names = set(dict(ga.named_parameters()))
    # the reference state dict carries these keys (gaussianMask_cuda.py:38-41,58)
    assert {"meanMap.weight", "meanMap.bias", "covMap.weight", "covMap.bias", "map.weight", "map.bias"} <= names
    assert not ga.meanMap.weight.any() and not ga.meanMap.bias.any()
    assert tuple(ga.coord.shape) == (6, 8, 2) and ga.coord[2, 5].tolist() == [5.0, 2.0]  # (x, y)


def test_shard_partitions(lgu):
    sh = lgu.sharded
    for n in (0, 1, 7, 20, 2001):
        for world in (1, 2, 3, 8):
            spans = [sh.balanced_shard(n, r, world) for r in range(world)]
            assert spans[0][0] == 0 and spans[-1][1] == n
            assert all(a[1] == b[0] for a, b in zip(spans, spans[1:]))
            sizes = [hi - lo for lo, hi in spans]
            assert max(sizes) - min(sizes) <= 1
    ii = torch.tensor([0, 0, 1, 3, 8, 9, 9, 17, 17, 30, 31])
    shards = sh.chunk_shards(ii, 2, chunk=8)
    got = sorted(int(i) for r in shards for idx in r for i in idx)
    assert got == list(range(ii.numel()))  # every edge exactly once
    for r in shards:
        for idx in r:  # one source-frame chunk per index tensor, as factor_graph.py:272-276
            assert int(ii[idx].max()) // 8 == int(ii[idx].min()) // 8


def _gloo_worker(rank, world, port, q):
    import torch.distributed as dist
    sys.path.insert(0, ROOT)
    import lgu_slam_amd
    dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%d" % port, rank=rank, world_size=world)
    try:
        E = 7
        full = torch.arange(E * 3 * 2, dtype=torch.float32).view(E, 3, 2)
        counts = [lgu_slam_amd.sharded.balanced_shard(E, r, world)[1] - lgu_slam_amd.sharded.balanced_shard(E, r, world)[0]
                  for r in range(world)]
        ex = lgu_slam_amd.sharded.EdgeExchange(counts)
        out = lgu_slam_amd.sharded.sharded_pyramid_sample(lambda c, lo, hi: c * 2.0, full, rank, world, ex)
        q.put((rank, bool(torch.equal(out, full * 2.0)), counts))
    finally:
        dist.destroy_process_group()


def test_edge_exchange_gloo_world2():
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29500 + (os.getpid() % 2000)
    procs = [ctx.Process(target=_gloo_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=120) for _ in procs]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert all(ok for _, ok, _ in res) and res[0][2] == [4, 3]


def _rehearsal_worker(rank, world, port, q):
    import torch.distributed as dist
    sys.path.insert(0, ROOT)
    import lgu_slam_amd
    sh = lgu_slam_amd.sharded
    dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%d" % port, rank=rank, world_size=world)
    try:
        ii = torch.tensor([0, 0, 1, 3, 9, 9, 10, 17, 17, 18])
        x = torch.arange(10 * 3, dtype=torch.float32).view(10, 3)
        outs = []
        for rehearse in (False, True):
            sh.REHEARSE_COLLECTIVES = rehearse
            edges = sh.ShardedEdgeSet(ii)
            assert edges.world == 1 and sh._single(1) == (not rehearse)
            outs.append((edges.gather(x[edges.my_edges]), edges.gather_frames(torch.arange(float(edges.my_frames.numel())), out=torch.zeros(20)),
                         sh.replicas_agree(x)))
        q.put(bool(torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]) and torch.equal(outs[0][0], x)
                   and outs[0][2] and outs[1][2]))
    finally:
        dist.destroy_process_group()


def test_collectives_can_be_rehearsed_at_world_size_one():
    """LGU_REHEARSE_COLLECTIVES: a world of one rank with an initialised process group issues the sharded step's collectives
    instead of short-cutting them (how the exact RCCL calls are run on a one-GPU box); results equal the short cut."""
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 31500 + (os.getpid() % 2000)
    p = ctx.Process(target=_rehearsal_worker, args=(0, 1, port, q))
    p.start()
    ok = q.get(timeout=120)
    p.join(timeout=60)
    assert p.exitcode == 0 and ok


def test_torch_library_registration(lgu):
    from lgu_slam_amd import torch_ops
    assert len(torch_ops.REGISTERED) == 9
    sch = str(torch.ops.lgu.defCorr_index_forward.default._schema)
    assert "Tensor(a2!) offset" in sch and sch.endswith("-> Tensor[]")  # in/out offset, list return
    assert "Tensor fmap1" in str(torch.ops.lgu.altcorr_forward.default._schema)


def test_bench_distributed_control_flow_gloo_world2():
    """bench.py's multi-rank launch contract (torch.distributed.run, RANK/WORLD_SIZE env, barrier +
    max-over-ranks timing, exchange, ONE JSON line from rank 0) exercised on CPU with gloo."""
    import json
    import subprocess
    port = 29600 + (os.getpid() % 1500)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
           "127.0.0.1", "--master-port", str(port), os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "3",
           "--warmup", "1", "--dry-run-cpu", "--full"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["steps"] == 3 and d["scaling"] == "weak" and d["exchange"]["bytes_per_rank"] == 20 * 48 * 64 * 4 * 4
    for k in ("metric", "value", "unit", "warmup", "ms_per_step", "higher_is_better", "vs_baseline", "dtype", "data", "config"):
        assert k in d
    sc = d["strong_scaling_config5"]
    assert sc["n_gpus"] == 2 and sc["replicas_agree"] and sc["every_edge_owned"] and sum(sc["edges_per_rank"]) == sc["edges_total"]


def _run_bench(argv, env_drop=("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")):
    import subprocess
    env = {k: v for k, v in os.environ.items() if k not in env_drop}
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + argv, capture_output=True, text=True, timeout=300,
                          cwd=ROOT, env=env)


def test_bench_launches_its_own_ranks_from_a_plain_command():
    """`python bench.py --gpus 2` with NO launcher around it (VERDICT r02 missing #3: it used to run one rank silently and
    print n_gpus 1): the parent starts the two ranks itself, relays rank 0's single JSON line, and the line's n_gpus is
    the number of ranks the process group initialised.  It also carries the config-5 strong-scaling leg's record."""
    import json
    out = _run_bench(["--gpus", "2", "--steps", "3", "--warmup", "1", "--dry-run-cpu", "--full"])
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.strip()]
    assert len(lines) == 1 and lines[0].startswith("{"), out.stdout[-500:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["scaling"] == "weak" and d["exchange"]["bytes_per_rank"] == 20 * 48 * 64 * 4 * 4
    sc = d["strong_scaling_config5"]
    assert sc["n_gpus"] == 2 and sc["replicas_agree"] and sc["every_edge_owned"] and min(sc["edges_per_rank"]) > 0
    # N = 1: no launcher, no process group, one line
    one = _run_bench(["--gpus", "1", "--steps", "2", "--warmup", "0", "--dry-run-cpu", "--full"])
    assert one.returncode == 0, one.stderr[-2000:]
    d1 = json.loads([l for l in one.stdout.splitlines() if l.startswith("{")][0])
    assert d1["n_gpus"] == 1 and "exchange" not in d1 and d1["config5_backend_n1"]["n_gpus"] == 1


def test_bench_plain_run_measures_the_headline_only():
    """Without --full the line carries the headline and nothing that takes runs of its own: no config-5 leg, no exchange
    timing, no roofline, no CPU baseline — at world size 1 and 2 alike."""
    import json
    for argv in (["--gpus", "1", "--steps", "4", "--warmup", "1", "--dry-run-cpu"],
                 ["--gpus", "2", "--steps", "4", "--warmup", "1", "--dry-run-cpu"]):
        out = _run_bench(argv)
        assert out.returncode == 0, out.stderr[-2000:]
        lines = [l for l in out.stdout.splitlines() if l.strip()]
        assert len(lines) == 1 and lines[0].startswith("{"), out.stdout[-500:]
        d = json.loads(lines[0])
        assert d["steps"] == 4 and d["warmup"] == 1 and d["ms_per_step"] >= 0 and d["n_gpus"] == int(argv[1])
        for k in ("metric", "value", "unit", "higher_is_better", "dtype"):
            assert k in d
        assert "exchange" not in d and "strong_scaling_config5" not in d and "config5_backend_n1" not in d
        assert d["roofline"] is None and d["cpu_baseline"] is None


def test_bench_dump_outputs_dtypes_and_budget(tmp_path):
    """--dump-outputs: float64 stays float64, other dtypes become float32; above the budget every array is replaced by
    the same fixed sample of its elements, whatever run writes it."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    small = {"a": torch.arange(12, dtype=torch.float16).view(3, 4), "b": np.arange(5, dtype=np.float64)}
    bench.dump_outputs(str(tmp_path / "small"), small)
    a, b = np.load(tmp_path / "small" / "a.npy"), np.load(tmp_path / "small" / "b.npy")
    assert a.dtype == np.float32 and a.shape == (3, 4) and np.array_equal(a, np.arange(12).reshape(3, 4))
    assert b.dtype == np.float64 and np.array_equal(b, np.arange(5))
    n = bench.DUMP_BUDGET_BYTES // 4 + 1000             # one float32 array just above the budget
    big = {"x": torch.arange(n, dtype=torch.float32), "y": torch.ones(1000, dtype=torch.float64)}
    for run in ("one", "two"):
        bench.dump_outputs(str(tmp_path / run), big)
    total = sum(os.path.getsize(tmp_path / "one" / f) for f in os.listdir(tmp_path / "one"))
    assert total <= 64 * 1000 * 1000
    x1, x2 = np.load(tmp_path / "one" / "x.npy"), np.load(tmp_path / "two" / "x.npy")
    assert x1.dtype == np.float32 and 0 < x1.size < n and np.array_equal(x1, x2)
    assert np.all(np.diff(x1) > 0) and np.load(tmp_path / "one" / "y.npy").dtype == np.float64


def test_bench_exits_nonzero_when_a_rank_fails():
    """A failing rank must fail the whole command (no line, non-zero status), whoever launched it."""
    out = _run_bench(["--gpus", "2", "--steps", "1", "--warmup", "0", "--dry-run-cpu", "--full", "--edges", "-1"])
    assert out.returncode != 0 and not [l for l in out.stdout.splitlines() if l.startswith("{")]
    # and a launcher whose world disagrees with --gpus is refused instead of silently measuring something else
    import subprocess
    env = dict(os.environ, RANK="0", WORLD_SIZE="1", LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT="29999")
    bad = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--dry-run-cpu"], capture_output=True,
                         text=True, timeout=120, cwd=ROOT, env=env)
    assert bad.returncode != 0 and "WORLD_SIZE=1" in (bad.stderr + bad.stdout)


def test_sharded_edge_set_world1_orders(lgu):
    ii = torch.tensor([9, 0, 0, 17, 1, 3, 8, 9, 17, 30, 31])
    es = lgu.sharded.ShardedEdgeSet(ii, rank=0, world=1)
    assert sorted(es.my_edges.tolist()) == list(range(ii.numel()))
    x = torch.arange(ii.numel(), dtype=torch.float32)[:, None] * 10
    assert torch.equal(es.gather(x[es.my_edges]), x)  # back in original edge order


def _gloo_edge_set_worker(rank, world, port, q):
    import torch.distributed as dist
    sys.path.insert(0, ROOT)
    import lgu_slam_amd
    dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%d" % port, rank=rank, world_size=world)
    try:
        ii = torch.tensor([9, 0, 0, 17, 1, 3, 8, 9, 17, 30, 31, 40, 41, 2])
        es = lgu_slam_amd.sharded.ShardedEdgeSet(ii)
        full = torch.arange(ii.numel() * 2, dtype=torch.float32).view(-1, 2)
        got = es.gather(full[es.my_edges])  # each rank contributes only what it owns
        q.put((rank, bool(torch.equal(got, full)), es.counts))
    finally:
        dist.destroy_process_group()


def test_sharded_edge_set_gloo_world2():
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29700 + (os.getpid() % 1500)
    procs = [ctx.Process(target=_gloo_edge_set_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=120) for _ in procs]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert all(ok for _, ok, _ in res) and sum(res[0][2]) == 14


def _reference_chunk_loop(ii, jj, chunk_fn, target, weight, damping, upmask):
    """The single-process loop of the reference (factor_graph.py:272-292), written out: what a sharded step must equal."""
    for i in range(0, int(jj.max()) + 1, 8):
        v = torch.nonzero((ii >= i) & (ii < i + 8)).flatten()
        if v.numel() == 0:
            continue
        t, w, d, u = chunk_fn(v, ii[v])
        target[v] = t
        weight[v] = w
        damping[torch.unique(ii[v])] = d
        upmask[torch.unique(ii[v])] = u
    return target, weight, damping, upmask


def _step_inputs():
    g = torch.Generator().manual_seed(11)
    # a non-bidirectional graph: the last source frames (40, 41) lie beyond the last chunk the reference's loop bound
    # (jj.max() + 1 = 34 -> chunks start at 0, 8, 16, 24, 32) produces: processed by nobody, values stay
    ii = torch.tensor([9, 0, 0, 17, 1, 3, 8, 9, 17, 30, 31, 40, 41, 2, 33, 12, 12])
    jj = torch.tensor([8, 1, 2, 16, 0, 2, 9, 10, 18, 31, 30, 33, 33, 3, 32, 11, 13])
    E, nf, ht, wd = ii.numel(), 42, 3, 4
    state = [torch.randn(E, ht, wd, 2, generator=g), torch.randn(E, ht, wd, 2, generator=g),
             torch.randn(nf, ht, wd, generator=g), torch.randn(nf, 5, ht, wd, generator=g)]

    def chunk_fn(idx, iis):  # deterministic stand-in for lookup + update operator: depends on edge ids and frames only
        fr = torch.unique(iis).float()
        e = idx.float().view(-1, 1, 1, 1)
        return (e + torch.zeros(idx.numel(), ht, wd, 2), 2 * e + torch.ones(idx.numel(), ht, wd, 2),
                fr.view(-1, 1, 1) * 10 + torch.zeros(fr.numel(), ht, wd), fr.view(-1, 1, 1, 1) * 100 + torch.zeros(fr.numel(), 5, ht, wd))
    return ii, jj, state, chunk_fn


def _gloo_step_worker(rank, world, port, q):
    import torch.distributed as dist
    sys.path.insert(0, ROOT)
    import lgu_slam_amd
    sh = lgu_slam_amd.sharded
    dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%d" % port, rank=rank, world_size=world)
    try:
        ii, jj, state, chunk_fn = _step_inputs()
        want = _reference_chunk_loop(ii, jj, chunk_fn, *[t.clone() for t in state])
        es = sh.ShardedEdgeSet(ii, jj=jj)
        calls = []

        def counted(idx, iis):
            calls.append(idx.numel())
            return chunk_fn(idx, iis)
        got = sh.sharded_update_step(es, ii, counted, *[t.clone() for t in state])
        ok = all(torch.equal(a, b) for a, b in zip(got, want))
        # bookkeeping: every chunk on exactly one rank, frames owned once, the unprocessed edges are the reference's
        agree = sh.replicas_agree(*got)
        differ = sh.replicas_agree(got[0] + rank)  # rank-dependent tensor: must be reported as different
        q.put((rank, ok, agree, differ, sum(calls), es.unprocessed.tolist(), [f.tolist() for f in es.frames], es.counts))
    finally:
        dist.destroy_process_group()


def test_sharded_update_step_gloo_world2():
    """A complete sharded step (chunk loop on the owners, then the target / weight all-gathers by edge and the damping /
    upmask all-gathers by source frame) leaves on BOTH ranks exactly what the reference's single-process loop leaves —
    including the edges its jj.max() loop bound never processes."""
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29800 + (os.getpid() % 1500)
    procs = [ctx.Process(target=_gloo_step_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=120) for _ in procs)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for rank, ok, agree, differ, ncalls, unproc, frames, counts in res:
        assert ok and agree and not differ
        assert unproc == [11, 12]                      # ii = 40, 41 > last chunk of range(0, jj.max() + 1, 8)
        assert sum(counts) == 15 and sorted(f for fr in frames for f in fr) == [0, 1, 2, 3, 8, 9, 12, 17, 30, 31, 33]
    assert res[0][4] + res[1][4] == 15 and res[0][4] > 0 and res[1][4] > 0   # edges split over the two ranks


def test_sharded_update_step_world1_equals_reference_loop(lgu):
    ii, jj, state, chunk_fn = _step_inputs()
    want = _reference_chunk_loop(ii, jj, chunk_fn, *[t.clone() for t in state])
    es = lgu.sharded.ShardedEdgeSet(ii, rank=0, world=1, jj=jj)
    got = lgu.sharded.sharded_update_step(es, ii, chunk_fn, *[t.clone() for t in state])
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    with pytest.raises(ValueError, match="without an owner"):
        es.gather(state[0][es.my_edges])               # unprocessed edges: a destination buffer is required
    # jj=None keeps the old bound (every edge in some chunk)
    assert lgu.sharded.ShardedEdgeSet(ii, rank=0, world=1).unprocessed.numel() == 0


def test_volume_operator_dtype_dispatch_errors(lgu):
    """Half / double volumes follow the reference's AT_DISPATCH_FLOATING_TYPES_AND_HALF rule: every scalar_t operand
    has the volume's dtype, coords stays float (defCorrSample_kernel.cu:185-191) — checked before any device work."""
    ops = lgu.ops
    v = torch.zeros(1, 2, 2, 4, 4, dtype=torch.float16)
    c = torch.zeros(1, 2, 2, 2)
    o = torch.zeros(1, 2, 2, 3, 3, 2)
    with pytest.raises(RuntimeError, match="expected scalar type Half but found Float"):
        ops.defCorr_index_forward(v, c, o, 1)
    with pytest.raises(RuntimeError, match="expected scalar type Float but found Double"):
        ops.defCorr_index_forward(v, c.double(), o.half(), 1)
    with pytest.raises(RuntimeError, match="expected scalar type Double but found Float"):
        ops.gaussianMask(torch.zeros(1, 2, 2, 2), torch.ones(1, 2, 2, 2), v.double(), 1)
    with pytest.raises(RuntimeError, match="offset must be contiguous"):
        ops.defCorr_index_forward(v, c, o.half().transpose(1, 2), 1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):   # dtypes consistent: reaches the fp32 operator, which needs a GPU
        ops.corr_index_forward(v, c, 1)


def test_tiled_layout_host_logic(lgu):
    """Pure host side of the tiled slice layout: shapes, logical-size checks, and a numpy restatement of the
    address formula of include/lgu_corr.h (LGU_PYR_TILED) that round-trips every element of a padded slice."""
    import numpy as np
    ops = lgu.ops
    assert ops.tiled_shape(2, 48, 64, 48, 64) == (2, 48, 64, 12, 8, 4, 8)
    assert ops.tiled_shape(1, 3, 5, 6, 8) == (1, 3, 5, 2, 1, 4, 8)      # 6 rows pad to 8
    assert ops.tiled_shape(1, 3, 5, 15, 20) == (1, 3, 5, 4, 3, 4, 8)    # 15x20 pads to 16x24
    t = torch.zeros(ops.tiled_shape(1, 2, 2, 6, 8))
    assert ops._level_dims([t], True, [(6, 8)]) == ([6], [8])
    assert ops._level_dims([t], True, None) == ([8], [8])              # unpadded logical size assumed
    with pytest.raises(RuntimeError, match="tiled pyramid level"):
        ops._level_dims([torch.zeros(1, 2, 2, 6, 8)], True, [(6, 8)])   # row-major tensor passed as tiled
    with pytest.raises(RuntimeError, match="tiled pyramid level"):
        ops._level_dims([t], True, [(12, 8)])                           # logical size that does not match the tiles
    H2, W2 = 15, 20
    tpr = -(-W2 // 8)
    y, x = np.meshgrid(np.arange(H2), np.arange(W2), indexing="ij")
    pos = ((y // 4) * tpr + x // 8) * 32 + (y % 4) * 8 + x % 8
    assert len(np.unique(pos)) == H2 * W2 and pos.max() < (-(-H2 // 4)) * tpr * 32
    # separability used by the kernel: the +1 neighbours are one add away
    sx = np.where(x % 8 == 7, 25, 1)
    sy = np.where(y % 4 == 3, tpr * 32 - 24, 8)
    assert np.array_equal((pos + sx)[:, :-1], pos[:, 1:]) and np.array_equal((pos + sy)[:-1], pos[1:])


def test_lowmem_plan_argument_checks(lgu):
    ops = lgu.ops
    h = torch.zeros(1, 4, 4, 32, dtype=torch.float16)
    with pytest.raises(RuntimeError, match="1..4 levels"):
        ops.LowmemPyramidPlan(h, [h] * 5, [None] * 5, 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.LowmemPyramidPlan(h, [h], [None], 3)
    with pytest.raises(RuntimeError, match="no CPU fallback|expected scalar type"):
        ops.LowmemPyramidPlan(h.float(), [h], [None], 3)


def _lowmem_refusal_cases():
    """(entry, base-call overrides, expected code) for the C entries of the on-the-fly family.  Every case is refused
    before any HIP call, so fake (non-null, 64-byte aligned) addresses and a null stream are enough."""
    OK, BAD, UNS = 0, 100001, 100002
    single = [   # what every single-level entry refuses
        (dict(fmap2=None), BAD), (dict(B=-1), BAD), (dict(S=0), BAD), (dict(H2=0), BAD), (dict(radius=-1), BAD),
        (dict(B=0), OK), (dict(C=24), UNS)]
    f32 = [(dict(radius=8), BAD)]   # LGU_MAX_RADIUS = 7
    h16 = [(dict(radius=4), UNS), (dict(radius=0), UNS), (dict(fmap1="+2"), UNS), (dict(S=70000, NO=70000), UNS)]
    rows = (dict(B=2, S=2, NO=1), BAD)
    pyr = [(dict(L=5), BAD), (dict(radius=4), UNS), (dict(radius=0), UNS), (dict(C=48), UNS), (dict(jj=None), BAD),
           (dict(H2=[4, 0]), BAD), (dict(B=0), OK), (dict(coords=None), BAD), (dict(lbase=17), BAD), (dict(B=2, S=2, NO=1), BAD)]
    cases = {
        "lgu_lowmem_defsample_fwd_h16": single + h16 + [rows, (dict(offset=None), BAD)],
        "lgu_lowmem_defsample_fwd_f32": single + f32 + [rows, (dict(offset=None), BAD), (dict(C=24, offset=None), UNS)],
        "lgu_altcorr_fwd_h16": single + h16,
        "lgu_altcorr_fwd_f32": single + f32 + [(dict(radius=4), UNS)],
        "lgu_altcorr_bwd_f32": single + f32 + [(dict(radius=4), UNS), (dict(fmap2_grad=None), BAD)],
        "lgu_lowmem_pyramid_fwd_h16": pyr + [(dict(fmap1="+2"), UNS)],
        "lgu_lowmem_pyramid_fwd_f32": pyr + [(dict(fmap1="+2"), UNS)],
        "lgu_lowmem_pyramid_chunked_fwd_h16": pyr + [(dict(fmap1="+2"), UNS)],
        "lgu_lowmem_pyramid_chunked_fwd_f32": pyr + [(dict(fmap1="+2"), UNS)],
        "lgu_lowmem_pyramid_calls_fwd_h16": [c for c in pyr if "S" not in c[0]] + [(dict(off_row=None), BAD), (dict(NO=0), BAD)],
    }
    return [pytest.param(e, o, c, id="%s-%s" % (e[4:], ",".join("%s=%s" % kv for kv in o.items()))) for e, cs in cases.items() for o, c in cs]


@pytest.mark.parametrize("entry,override,code", _lowmem_refusal_cases())
def test_lowmem_entries_refuse_bad_arguments(lgu, entry, override, code):
    """The codes the family's entries answer for arguments they refuse (include/lgu_corr.h): LGU_E_BADARG for null
    pointers, non-positive sizes, too few offset rows and a radius above LGU_MAX_RADIUS; LGU_E_UNSUPPORTED for what no
    kernel serves; LGU_OK for an empty call.  The entries differ on purpose: the float entries refuse C % 32 != 0 at
    the door, the half ones when no kernel takes the call."""
    import ctypes
    lib = lgu._lib.load()
    names = ["fmap1", "fmap2", "coords", "offset", "corr", "corr_grad", "fmap1_grad", "fmap2_grad", "out", "ii", "jj", "off_row"]
    a = {n: 0x100000 * (i + 1) for i, n in enumerate(names)}   # fake addresses, 64-byte aligned
    a.update(B=1, S=1, H1=4, W1=4, C=32, NO=1, radius=3, lbase=0, chunked=0)
    pyramid = "pyramid" in entry
    a.update(dict(L=2, H2=[4, 2], W2=[4, 2]) if pyramid else dict(H2=4, W2=4))
    for k, v in override.items():
        a[k] = a[k] + 2 if v == "+2" else v
    if pyramid:
        L = max(min(a["L"], 4), 1)
        fmap2 = (ctypes.c_void_p * 4)(*[0x4000000 + 0x100000 * l for l in range(L)])
        offsets = (ctypes.c_void_p * 4)(0x5000000)   # offsets on level 0 only
        H2 = (ctypes.c_int * 4)(*(a["H2"] + [1] * 4)[:4])
        W2 = (ctypes.c_int * 4)(*(a["W2"] + [1] * 4)[:4])
        head = [a["fmap1"], fmap2, a["coords"], offsets, a["out"], a["L"], a["lbase"], a["B"]]
        if "calls" in entry:
            args = head + [a["H1"], a["W1"], H2, W2, a["C"], a["NO"], a["off_row"], a["radius"], a["ii"], a["jj"], a["chunked"], None]
        else:
            args = head + [a["S"], a["H1"], a["W1"], H2, W2, a["C"], a["NO"], a["radius"], a["ii"], a["jj"], None]
    else:
        dims = [a[k] for k in ("B", "S", "H1", "W1", "H2", "W2", "C")]
        if "defsample" in entry:
            args = [a["fmap1"], a["fmap2"], a["coords"], a["offset"], a["corr"]] + dims + [a["NO"], a["radius"], None]
        elif "bwd" in entry:
            args = [a["fmap1"], a["fmap2"], a["coords"], a["corr_grad"], a["fmap1_grad"], a["fmap2_grad"]] + dims + [a["radius"], None]
        else:
            args = [a["fmap1"], a["fmap2"], a["coords"], a["corr"]] + dims + [a["radius"], None]
    assert getattr(lib, entry)(*args) == code


def test_corr_encoder_host_logic():
    """CorrEncoder: structure check, and anything that is not a channel-last half CUDA tensor is handed to
    the wrapped module unchanged (the reference call, droid_net.py:116)."""
    import lgu_slam_amd as lgu
    torch.manual_seed(0)
    enc = torch.nn.Sequential(torch.nn.Conv2d(196, 128, 1), torch.nn.ReLU(inplace=True),
                              torch.nn.Conv2d(128, 128, 3, padding=1), torch.nn.ReLU(inplace=True)).eval()
    fused = lgu.CorrEncoder(enc)
    x = torch.randn(2, 196, 6, 8)
    assert not fused.takes(x) and not fused.takes(x.half().contiguous(memory_format=torch.channels_last))
    with torch.no_grad():
        assert torch.equal(fused(x), enc(x))
    with pytest.raises(RuntimeError):
        lgu.CorrEncoder(torch.nn.Sequential(torch.nn.Conv2d(196, 128, 3), torch.nn.ReLU()))
    with pytest.raises(RuntimeError):
        lgu.ops.DefcorrPyramidPlan.__init__(object.__new__(lgu.ops.DefcorrPyramidPlan), [], [], 3, out_format="nchw")
    assert lgu.CorrBlock.OUT_FORMAT == "planar" and set(lgu.ops.OUT_FORMATS) == {"planar", "nhwc", "nhwc_f16"}


def test_offset_conv_weight_packing_host_logic():
    """pack_offset_conv: hi + lo reproduces scale * W to 2^-21 relative, zero rows beyond Cout, and the MFMA fragment
    order [tap][kstep][part][ntile][kg][nl][8] maps back to W[n = ntile*16 + nl][c = kstep*32 + kg*8 + t][tap]."""
    import lgu_slam_amd as lgu
    torch.manual_seed(3)
    W = torch.randn(98, 256, 3, 3)
    b = torch.randn(98)
    wpack, bias, Cout, C = lgu.ops.pack_offset_conv(W, b, scale=4.0)
    assert (Cout, C) == (98, 128) and tuple(wpack.shape) == (9, 8, 2, 7, 4, 16, 8) and wpack.dtype == torch.float16
    assert bias.dtype == torch.float32 and torch.equal(bias, b)
    rec = (wpack[:, :, 0].float() + wpack[:, :, 1].float())          # [tap][kstep][ntile][kg][nl][t]
    rec = rec.permute(2, 4, 1, 3, 5, 0).reshape(112, 256, 9)        # [n][c][tap]
    want = torch.zeros(112, 256, 9)
    want[:98] = (W * 4.0).reshape(98, 256, 9)
    assert float((rec - want).abs().max()) <= 2.0 ** -21 * float(want.abs().max())
    assert float(rec[98:].abs().max()) == 0.0
    with pytest.raises(RuntimeError):
        lgu.ops.pack_offset_conv(torch.randn(120, 256, 3, 3), torch.randn(120))
    with pytest.raises(RuntimeError):
        lgu.ops.pack_offset_conv(torch.randn(98, 256, 1, 1), b)


def test_ba_assembly_tables_host_logic():
    """ba._csr: rows grouped by destination (ascending row inside a group), CSR over ALL destinations, rows pointing
    outside [0, ndst) dropped — the tables lgu_ba_assemble_f64 walks."""
    import numpy as np
    from lgu_slam_amd import ba as B
    dest = np.array([2, -1, 0, 2, 5, 0, 7, 2])
    ptr, idx = B._csr(dest, 6, torch.device("cpu"))
    assert ptr.tolist() == [0, 2, 2, 5, 5, 5, 6]
    assert idx.tolist() == [2, 5, 0, 3, 7, 4]
    ptr, idx = B._csr(np.array([-1, 9]), 3, torch.device("cpu"))
    assert ptr.tolist() == [0, 0, 0, 0] and idx.numel() == 1   # placeholder entry keeps the pointer valid


# ---- refusal census: every argument refusal an operator can raise on CPU tensors, its text and its precedence ---------
_NO_CPU = " must be a HIP device tensor: lgu_slam_amd has no CPU fallback"
_NO_GRAD = " has no autograd: its outputs would carry no gradient. Call it under torch.no_grad() or pass detached inputs"


def _z(*shape, dtype=torch.float32):
    return torch.zeros(shape, dtype=dtype)


def _nc(t):
    """Same shape and dtype, every stride doubled: not contiguous."""
    return torch.zeros(tuple(t.shape) + (2,), dtype=t.dtype)[..., 0]


def _to(dtype):
    return lambda t: t.to(dtype)


def _as(*shape):
    return lambda t: torch.zeros(shape, dtype=t.dtype)


def _grad(t):
    return t.requires_grad_()


_DBL, _HALF, _INT, _BF16 = _to(torch.float64), _to(torch.float16), _to(torch.int32), _to(torch.bfloat16)
_L = torch.int64

# operator -> (module, positional tensor arguments in signature order as name -> shape [, dtype], trailing arguments)
_CENSUS_BASE = {
    "defCorr_index_forward": ("ops", dict(volume=(1, 2, 2, 4, 4), coords=(1, 2, 2, 2), offset=(1, 2, 2, 3, 3, 2)), (1,)),
    "defCorr_index_backward": ("ops", dict(volume=(1, 2, 2, 4, 4), coords=(1, 2, 2, 2), offset=(1, 2, 2, 3, 3, 2),
                                           corr_grad=(1, 3, 3, 2, 2)), (1,)),
    "corr_index_forward": ("ops", dict(volume=(1, 2, 2, 4, 4), coords=(1, 2, 2, 2)), (1,)),
    "corr_index_backward": ("ops", dict(volume=(1, 2, 2, 4, 4), coords=(1, 2, 2, 2), corr_grad=(1, 3, 3, 2, 2)), (1,)),
    "gaussianMask": ("ops", dict(means=(1, 2, 2, 2), covs=(1, 2, 2, 2), volume=(1, 2, 2, 4, 4)), (1,)),
    "gaussianMask_backward": ("ops", dict(means=(1, 2, 2, 2), covs=(1, 2, 2, 2), volume=(1, 2, 2, 4, 4),
                                          volume_grad=(1, 2, 2, 4, 4)), (1,)),
    "lowMem_defSample": ("ops", dict(fmap1=(1, 2, 2, 32), fmap2=(1, 4, 4, 32), coords=(1, 1, 2, 2, 2),
                                     offset=(1, 2, 2, 3, 3, 2)), (1,)),
    "altcorr_forward": ("ops", dict(fmap1=(1, 2, 2, 32), fmap2=(1, 4, 4, 32), coords=(1, 1, 2, 2, 2)), (1,)),
    "altcorr_backward": ("ops", dict(fmap1=(1, 2, 2, 32), fmap2=(1, 4, 4, 32), coords=(1, 1, 2, 2, 2),
                                     corr_grad=(1, 1, 9, 2, 2)), (1,)),
    "lowMem_defSample_mixed": ("ops", dict(fmap1=((1, 2, 2, 32), torch.float16), fmap2=((1, 4, 4, 32), torch.float16),
                                           coords=(1, 1, 2, 2, 2), offset=(1, 2, 2, 3, 3, 2)), (1,)),
    "altcorr_forward_mixed": ("ops", dict(fmap1=((1, 2, 2, 32), torch.float16), fmap2=((1, 4, 4, 32), torch.float16),
                                          coords=(1, 1, 2, 2, 2)), (1,)),
    "frame_distance": ("geom", dict(poses=(2, 7), disps=(2, 2, 2), intrinsics=(4,), ii=((2,), _L), jj=((2,), _L)), (0.5,)),
    "projmap": ("geom", dict(poses=(2, 7), disps=(2, 2, 2), intrinsics=(4,), ii=((2,), _L), jj=((2,), _L)), ()),
    "depth_filter": ("geom", dict(poses=(2, 7), disps=(2, 2, 2), intrinsics=(4,), ix=((2,), _L), thresh=(2,)), ()),
    "iproj": ("geom", dict(poses=(2, 7), disps=(2, 2, 2), intrinsics=(4,)), ()),
    "projective_transform": ("geom", dict(poses=(1, 2, 7), disps=(1, 2, 2, 2), intrinsics=(1, 2, 4), ii=((2,), _L),
                                          jj=((2,), _L)), ()),
    "reproject": ("geom", dict(poses=(2, 7), disps=(2, 2, 2), intrinsics=(2, 4), ii=((2,), _L), jj=((2,), _L)), ()),
    "motion_features": ("geom", dict(poses=(1, 2, 7), disps=(1, 2, 2, 2), intrinsics=(1, 2, 4), ii=((2,), _L), jj=((2,), _L),
                                     target=(1, 2, 2, 2, 2)), ()),
    "scatter_mean": ("aggregate", dict(src=(2, 3), index=((3,), _L)), ()),
    "cvx_upsample": ("aggregate", dict(data=(1, 2, 2, 1), mask=(1, 576, 2, 2)), ()),
    "upsample_disp": ("aggregate", dict(disp=(1, 1, 2, 2), mask=(1, 1, 576, 2, 2)), ()),
    "upsample_disps_": ("aggregate", dict(disps_up=(2, 16, 16), disps=(2, 2, 2), ix=((2,), _L), mask=(2, 576, 2, 2)), ()),
    "kangru_context": ("gru", dict(net=(1, 128, 1, 1), weight=(128, 128), bias=(128,)), ()),
    "kan_heads": ("gru", dict(glo=(1, 128), grid=(3, 128, 10), wpack=(384, 896)), ()),
    "kangru_gates_": ("gru", dict(net_inp=(1, 448, 1, 1), cz=(1, 128, 1, 1), cr=(1, 128, 1, 1), kz=(1, 128), kr=(1, 128),
                                  net=(1, 128, 1, 1)), ()),
    "kangru_blend": ("gru", dict(cq=(1, 128, 1, 1), kq=(1, 128), z=(1, 128, 1, 1), net=(1, 128, 1, 1)), ()),
    "instance_norm_relu": ("features", dict(a=(1, 1, 2, 2)), ()),
    "normalize_images": ("features", dict(image=((1, 3, 2, 2), torch.uint8)), ()),
    "flow_conv7_relu": ("flow", dict(x=(1, 4, 1, 1), wpack=((7, 8, 64, 8), torch.float16), bias_h=((128,), torch.float16)), ()),
    # t = 2, t0 = t1 = 0: a window of n = 4 cells
    "proximity_edges": ("graph", dict(poses=(2, 7), disps=(2, 2, 2), intrinsics=(4,), t=None, ii_known=((2,), _L),
                                      jj_known=((2,), _L)), ()),
}


def _census_cases():
    """(operator, edits of the valid CPU call, keyword arguments, exception, message).  An edit maps an argument name to a
    function of its valid tensor; every unedited call would be refused only for living on the CPU."""
    R, V, N, I = RuntimeError, ValueError, NotImplementedError, IndexError
    c = []

    def add(op, edits, exc, msg, **kw):
        c.append((op, edits, kw, exc, msg))

    # -- ops: contiguity of every argument, then per argument HIP device and dtype; shapes only after those ------------
    for op, first, second, last in (("defCorr_index_forward", "volume", "coords", "offset"),
                                    ("defCorr_index_backward", "volume", "coords", "corr_grad"),
                                    ("corr_index_forward", "volume", "coords", "coords"),
                                    ("corr_index_backward", "volume", "coords", "corr_grad"),
                                    ("gaussianMask", "volume", "means", "covs"),
                                    ("gaussianMask_backward", "volume", "means", "volume_grad"),
                                    ("lowMem_defSample", "fmap1", "fmap2", "offset"),
                                    ("altcorr_forward", "fmap1", "fmap2", "coords"),
                                    ("altcorr_backward", "fmap1", "fmap2", "corr_grad")):
        add(op, {}, R, first + _NO_CPU)
        add(op, {last: _nc}, R, last + " must be contiguous")
        add(op, {first: _nc, second: _nc}, R, first + " must be contiguous")       # two defects: the order of the checks
        add(op, {first: _BF16, last: _nc}, R, last + " must be contiguous")        # contiguity before device and dtype
        add(op, {first: _BF16}, R, first + _NO_CPU)                                # device before dtype
    for op in ("lowMem_defSample_mixed", "altcorr_forward_mixed"):
        add(op, {}, R, "fmap1" + _NO_CPU)
        add(op, {"fmap1": _nc}, R, "fmap1 must be contiguous")
        add(op, {"fmap2": _nc}, R, "fmap1" + _NO_CPU)                              # two defects: fmap1 is checked whole first
        add(op, {"fmap1": _to(torch.float32)}, R, "fmap1" + _NO_CPU)
    # half / double volumes: every scalar operand has the volume's dtype, coords stays float; contiguity first
    add("defCorr_index_forward", {"volume": _HALF}, R, "expected scalar type Half but found Float")
    add("defCorr_index_forward", {"volume": _HALF, "offset": _HALF, "coords": _DBL}, R, "expected scalar type Float but found Double")
    add("defCorr_index_forward", {"volume": _HALF, "coords": _DBL}, R, "expected scalar type Float but found Double")
    add("defCorr_index_forward", {"volume": _HALF, "coords": _DBL, "offset": _nc}, R, "offset must be contiguous")
    add("defCorr_index_forward", {"volume": _HALF, "coords": _nc, "offset": _nc}, R, "offset must be contiguous")
    add("defCorr_index_forward", {"volume": _HALF, "offset": _HALF}, R, "volume" + _NO_CPU)
    add("defCorr_index_backward", {"volume": _DBL, "offset": _DBL}, R, "expected scalar type Double but found Float")
    add("defCorr_index_backward", {"volume": _DBL, "corr_grad": _nc}, R, "corr_grad must be contiguous")
    add("corr_index_forward", {"volume": _HALF, "coords": _HALF}, R, "expected scalar type Float but found Half")
    add("corr_index_forward", {"volume": _HALF, "coords": _nc}, R, "coords must be contiguous")
    add("corr_index_backward", {"volume": _HALF}, R, "expected scalar type Half but found Float")
    add("corr_index_backward", {"volume": _HALF, "coords": _INT}, R, "expected scalar type Float but found Int")
    add("gaussianMask", {"volume": _DBL, "means": _DBL}, R, "expected scalar type Double but found Float")
    add("gaussianMask", {"volume": _HALF, "means": _nc}, R, "means must be contiguous")
    add("gaussianMask_backward", {"volume": _HALF, "means": _HALF, "covs": _HALF, "volume_grad": _to(torch.int8)}, R,
        "expected scalar type Half but found torch.int8")
    add("gaussianMask_backward", {"volume": _HALF, "covs": _nc}, R, "covs must be contiguous")

    # -- geom: contiguity, dtypes, shapes, no-grad, device ---------------------------------------------------------------
    for op in ("frame_distance", "projmap", "depth_filter", "iproj", "projective_transform", "reproject", "motion_features"):
        ix = "ix" if op == "depth_filter" else "ii"
        add(op, {}, R, "poses" + _NO_CPU)
        add(op, {"disps": _nc}, R, "disps must be contiguous")
        add(op, {"disps": _DBL}, R, "expected scalar type Float but found Double (disps)")
        add(op, {"intrinsics": _to(torch.int8)}, R, "expected scalar type Float but found torch.int8 (intrinsics)")
        add(op, {"poses": _HALF, "intrinsics": _nc}, R, "intrinsics must be contiguous")       # two defects
        if op != "iproj":
            add(op, {ix: _INT}, R, "expected scalar type Long but found Int (%s)" % ix)
            add(op, {"intrinsics": _DBL, ix: _nc}, R, ix + " must be contiguous")              # two defects
    for op in ("frame_distance", "projmap", "depth_filter", "iproj"):
        add(op, {"poses": _as(2, 6)}, R, "poses must be (N,7) = t, q(xyzw), got (2, 6)")
        add(op, {"disps": _as(2, 2)}, R, "disps must be (N,ht,wd), got (2, 2)")
        add(op, {"intrinsics": _as(3)}, R, "intrinsics must be 1-D with fx, fy, cx, cy, got (3,)")
        add(op, {"poses": _as(2, 6), "disps": _DBL}, R, "expected scalar type Float but found Double (disps)")  # two defects
    for op in ("frame_distance", "projmap"):
        add(op, {"jj": _as(3)}, R, "ii and jj must be 1-D and of equal length, got (2,) and (3,)")
        add(op, {"jj": _as(3), "intrinsics": _as(3)}, R, "intrinsics must be 1-D with fx, fy, cx, cy, got (3,)")
    add("depth_filter", {"ix": _as(2, 1)}, R, "ix must be 1-D, got (2, 1)")
    add("depth_filter", {"thresh": _as(1)}, R, "thresh must be 1-D with one entry per index of ix (2), got (1,)")
    add("depth_filter", {"thresh": _DBL}, R, "expected scalar type Float but found Double (thresh)")
    add("depth_filter", {"thresh": _DBL, "ix": _INT}, R, "expected scalar type Long but found Int (ix)")
    for op in ("projective_transform", "motion_features"):
        add(op, {"poses": _as(2, 7)}, R, "poses must be (B,N,7) = t, q(xyzw), got (2, 7)")
        add(op, {"disps": _as(2, 2, 2)}, R, "disps must be (B,N,ht,wd), got (2, 2, 2)")
        add(op, {"intrinsics": _as(1, 2, 3)}, R, "intrinsics must be (B,N,4) = fx, fy, cx, cy per frame, got (1, 2, 3)")
        add(op, {"disps": _as(2, 2, 2, 2)}, R, "poses, disps and intrinsics must have the same batch size, got 1, 2 and 1")
        add(op, {"jj": _as(2, 1)}, R, "ii and jj must be 1-D and of equal length, got (2,) and (2, 1)")
        add(op, {"disps": _grad}, R, op + _NO_GRAD)
        add(op, {"disps": _grad, "jj": _as(3)}, R, "ii and jj must be 1-D and of equal length, got (2,) and (3,)")
    add("reproject", {"poses": _as(2, 6)}, R, "poses must be (B,N,7) = t, q(xyzw), got (1, 2, 6)")
    add("reproject", {"intrinsics": _grad}, R, "projective_transform" + _NO_GRAD)
    add("reproject", {"intrinsics": _grad, "ii": _INT}, R, "expected scalar type Long but found Int (ii)")
    add("motion_features", {"target": _as(1, 2, 2, 2, 3)}, R, "target must be (B,E,ht,wd,2) = (1, 2, 2, 2, 2), got (1, 2, 2, 2, 3)")
    add("motion_features", {"target": _DBL}, R, "expected scalar type Float but found Double (target)")
    add("motion_features", {"target": _nc}, R, "target must be contiguous")
    add("motion_features", {"target": lambda t: torch.zeros((1, 2, 2, 2, 3), dtype=torch.float64)}, R,
        "expected scalar type Float but found Double (target)")
    add("motion_features", {}, R, "clamp must be a non-negative bound, got -1.0", clamp=-1.0)
    add("motion_features", {"target": _grad}, R, "clamp must be a non-negative bound, got -1.0", clamp=-1.0)
    add("motion_features", {"target": _grad}, R, "motion_features" + _NO_GRAD)

    # -- aggregate ----------------------------------------------------------------------------------------------------------
    add("scatter_mean", {}, R, "src" + _NO_CPU)
    add("scatter_mean", {}, N, "scatter_mean: only out=None is supported (the reference's call form scatter_mean(src, index, "
        "dim=d) with a 1-D index of length src.size(d))", out=_z(2, 3))
    add("scatter_mean", {}, I, "dim 2 out of range for a 2-D src", dim=2)
    add("scatter_mean", {"index": _as(2)}, N, "scatter_mean: only a 1-D index of length src.size(dim) = 3 is supported (the "
        "reference's call form), got index of shape (2,)")
    add("scatter_mean", {"src": _nc}, R, "src must be contiguous")
    add("scatter_mean", {"src": _DBL}, R, "expected scalar type Float or Half but found Double (src)")
    add("scatter_mean", {"src": _to(torch.uint8)}, R, "expected scalar type Float or Half but found torch.uint8 (src)")
    add("scatter_mean", {"index": _INT}, R, "expected scalar type Long but found Int (index)")
    add("scatter_mean", {}, R, "dim_size must be >= 0, got -1", dim_size=-1)
    add("scatter_mean", {"src": _grad}, R, "scatter_mean" + _NO_GRAD)
    add("scatter_mean", {"src": _HALF}, R, "src" + _NO_CPU)
    add("scatter_mean", {"src": _DBL, "index": _nc}, R, "index must be contiguous")            # two defects
    add("scatter_mean", {"src": _grad, "index": _INT}, R, "expected scalar type Long but found Int (index)")
    add("cvx_upsample", {}, R, "data" + _NO_CPU)
    add("cvx_upsample", {"data": _as(1, 2, 2)}, R, "data must be (B,ht,wd,dim), got (1, 2, 2)")
    add("cvx_upsample", {"data": _as(1, 2, 2, 2)}, N, "cvx_upsample: only data width 1 (the disparity) is supported, got 2")
    add("cvx_upsample", {"mask": _nc}, R, "mask must be contiguous")
    add("cvx_upsample", {"data": _HALF}, R, "expected scalar type Float but found Half (data)")
    add("cvx_upsample", {"mask": _as(1, 575, 2, 2)}, R, "mask must be (1,576,2,2), optionally with leading 1s, got (1, 575, 2, 2)")
    add("cvx_upsample", {"mask": _DBL}, R, "expected scalar type Float or Half but found Double (mask)")
    add("cvx_upsample", {"mask": _grad}, R, "cvx_upsample" + _NO_GRAD)
    add("cvx_upsample", {"mask": _as(1, 1, 576, 2, 2)}, R, "data" + _NO_CPU)                   # leading 1s are accepted
    add("cvx_upsample", {"data": _DBL, "mask": _as(1, 575, 2, 2)}, R, "expected scalar type Float but found Double (data)")
    add("cvx_upsample", {"mask": lambda t: torch.zeros((1, 575, 2, 2), dtype=torch.float64)}, R,
        "mask must be (1,576,2,2), optionally with leading 1s, got (1, 575, 2, 2)")
    add("upsample_disp", {}, R, "data" + _NO_CPU)
    add("upsample_disp", {"disp": _as(1, 2, 2)}, R, "disp must be (batch,num,ht,wd), got (1, 2, 2)")
    add("upsample_disp", {"disp": _nc}, R, "disp must be contiguous")
    add("upsample_disp", {"mask": _as(1, 1, 575, 2, 2)}, R, "mask must be (1,1,576,2,2), got (1, 1, 575, 2, 2)")
    add("upsample_disp", {"disp": _DBL}, R, "expected scalar type Float but found Double (data)")
    add("upsample_disp", {"disp": _grad}, R, "cvx_upsample" + _NO_GRAD)
    add("upsample_disp", {"mask": lambda t: _nc(torch.zeros(1, 1, 575, 2, 2))}, R, "mask must be contiguous")   # two defects
    add("upsample_disps_", {}, R, "disps_up" + _NO_CPU)
    add("upsample_disps_", {"disps": _as(2, 2)}, R, "disps must be (N,ht,wd), got (2, 2)")
    add("upsample_disps_", {"disps_up": _as(2, 16, 15)}, R, "disps_up must be (N,8ht,8wd) = (2, 16, 16), got (2, 16, 15)")
    add("upsample_disps_", {"ix": _as(2, 1)}, R, "ix must be 1-D, got (2, 1)")
    add("upsample_disps_", {"mask": _nc}, R, "mask must be contiguous")
    add("upsample_disps_", {"disps_up": _DBL}, R, "expected scalar type Float but found Double (disps_up)")
    add("upsample_disps_", {"disps": _HALF}, R, "expected scalar type Float but found Half (disps)")
    add("upsample_disps_", {"ix": _INT}, R, "expected scalar type Long but found Int (ix)")
    add("upsample_disps_", {"mask": _as(3, 576, 2, 2)}, R, "mask must be (2,576,2,2), optionally with leading 1s, got (3, 576, 2, 2)")
    add("upsample_disps_", {"mask": _BF16}, R, "expected scalar type Float or Half but found BFloat16 (mask)")
    add("upsample_disps_", {"mask": _grad}, R, "upsample_disps_" + _NO_GRAD)
    add("upsample_disps_", {"disps": _nc, "ix": _as(2, 1)}, R, "ix must be 1-D, got (2, 1)")   # two defects: shapes first
    add("upsample_disps_", {"ix": _INT, "mask": _as(3, 576, 2, 2)}, R, "expected scalar type Long but found Int (ix)")

    # -- gru: shapes, contiguity, dtypes (the first operand's), no-grad, device ------------------------------------------
    for op, first, shaped, two in (("kangru_context", "net", "bias", "weight"), ("kan_heads", "glo", "grid", "wpack"),
                                   ("kangru_gates_", "net_inp", "kr", "net"), ("kangru_blend", "cq", "kq", "net")):
        shape = _CENSUS_BASE[op][1][shaped]
        bad = shape[:-1] + (shape[-1] + 1,)
        add(op, {}, R, first + _NO_CPU)
        add(op, {shaped: _as(*bad)}, R, "%s must be %s, got %s" % (shaped, shape, bad))
        add(op, {two: _nc}, R, two + " must be contiguous")
        add(op, {first: _DBL}, R, "expected scalar type Float or Half but found Double (%s)" % first)
        add(op, {two: _HALF}, R, "expected scalar type Float but found Half (%s)" % two)
        add(op, {two: _grad}, R, op + _NO_GRAD)
        add(op, {first: _nc, shaped: _as(*bad)}, R, "%s must be %s, got %s" % (shaped, shape, bad))   # two defects
        add(op, {first: _nc, two: _HALF}, R, first + " must be contiguous")
        add(op, {first: _HALF, two: _grad}, R, "expected scalar type Half but found Float (%s)"
            % ("wpack" if op == "kan_heads" else list(_CENSUS_BASE[op][1])[1]))
    add("kangru_context", {"net": _as(1, 127, 1, 1)}, R, "net must be (E,128,H,W), got (1, 127, 1, 1)")
    add("kangru_context", {"weight": _as(128, 128, 1, 2)}, R, "weight must be (128, 128, 1, 1), got (128, 128, 1, 2)")
    add("kangru_context", {"weight": _as(128, 127)}, R, "weight must be (128, 128), got (128, 127)")
    add("kan_heads", {"glo": _as(1, 127)}, R, "glo must be (E,128), got (1, 127)")
    add("kan_heads", {"grid": _DBL}, R, "expected scalar type Float but found Double (grid)")
    add("kan_heads", {"grid": _DBL, "wpack": _HALF}, R, "expected scalar type Float but found Half (wpack)")
    add("kangru_gates_", {"net_inp": _as(1, 447, 1, 1)}, R, "net_inp must be (E,448,H,W), got (1, 447, 1, 1)")
    add("kangru_gates_", {"cz": _as(1, 128, 1, 2), "kz": _as(2, 128)}, R, "cz must be (1, 128, 1, 1), got (1, 128, 1, 2)")
    add("kangru_blend", {"cq": _as(1, 128, 1)}, R, "cq must be (E,128,H,W), got (1, 128, 1)")
    add("kangru_blend", {"z": _as(2, 128, 1, 1)}, R, "z must be (1, 128, 1, 1), got (2, 128, 1, 1)")

    # -- features ---------------------------------------------------------------------------------------------------------
    op = "instance_norm_relu"
    add(op, {}, R, "a" + _NO_CPU)
    add(op, {"a": _as(1, 2, 2)}, R, "a must be (N,C,H,W), got (1, 2, 2)")
    add(op, {"a": _DBL}, R, "expected scalar type Float or Half but found Double (a)")
    add(op, {}, V, "norm_residual=True needs a residual", norm_residual=True)
    add(op, {}, V, "relu=False is served without a residual only", residual=_z(1, 1, 2, 2), relu=False)
    add(op, {}, R, "residual must be (1, 1, 2, 2), got (1, 1, 2, 3)", residual=_z(1, 1, 2, 3))
    add(op, {}, R, "expected scalar type Float but found Half (residual)", residual=_z(1, 1, 2, 2, dtype=torch.float16))
    add(op, {}, R, "out must be (1, 1, 2, 2), got (1, 1, 3, 2)", out=_z(1, 1, 3, 2))
    add(op, {"a": _as(1, 1, 1, 1)}, V, "Expected more than 1 spatial element when training, got input size torch.Size([1, 1, 1, 1])")
    add(op, {}, V, "eps must be >= 0, got -1.0", eps=-1.0)
    add(op, {"a": _nc}, R, "a must be contiguous")
    add(op, {}, R, "residual must be contiguous", residual=_nc(_z(1, 1, 2, 2)))
    add(op, {"a": _grad}, R, op + _NO_GRAD)
    add(op, {"a": _HALF}, R, "a" + _NO_CPU)
    add(op, {}, R, "expected scalar type Float but found Half (residual)", residual=_z(1, 1, 2, 2, dtype=torch.float16),
        out=_z(1, 1, 3, 2))                                                                    # two defects: per tensor
    add(op, {}, R, "residual must be (1, 1, 2, 2), got (1, 1, 2, 3)", residual=_z(1, 1, 2, 3, dtype=torch.float16))
    add(op, {"a": lambda t: _nc(t).requires_grad_()}, R, "a must be contiguous")
    add(op, {"a": _nc}, V, "eps must be >= 0, got -1.0", eps=-1.0)
    op = "normalize_images"
    add(op, {"image": _as(1, 2, 2, 2)}, R, "image must be (N,3,H,W), got (1, 2, 2, 2)")
    add(op, {"image": _to(torch.float32)}, R, "expected scalar type Byte but found Float (image)")
    add(op, {"image": _to(torch.int8)}, R, "expected scalar type Byte but found torch.int8 (image)")
    add(op, {}, R, "mean and std must have 3 entries", mean=(0.5, 0.5))
    add(op, {"image": lambda t: torch.zeros(1, 2, 2, 2)}, R, "image must be (N,3,H,W), got (1, 2, 2, 2)")    # two defects
    add(op, {"image": _to(torch.float32)}, R, "expected scalar type Byte but found Float (image)", std=(1.0,))

    # -- flow -------------------------------------------------------------------------------------------------------------
    op = "flow_conv7_relu"
    add(op, {}, R, "x" + _NO_CPU)
    add(op, {"x": _as(1, 3, 1, 1)}, R, "x must be (N,4,H,W), got (1, 3, 1, 1)")
    add(op, {"wpack": _as(7, 8, 64, 7)}, R, "wpack must hold 28672 halves (pack_conv7), got (7, 8, 64, 7)")
    add(op, {"bias_h": _as(127)}, R, "bias_h must be (128,), got (127,)")
    add(op, {"x": _nc}, R, "x must be contiguous")
    add(op, {"x": _DBL}, R, "expected scalar type Float or Half but found Double (x)")
    add(op, {"wpack": _to(torch.float32)}, R, "expected scalar type Half but found Float (wpack)")
    add(op, {"bias_h": _BF16}, R, "expected scalar type Half but found BFloat16 (bias_h)")
    add(op, {"x": _grad}, R, op + _NO_GRAD)
    add(op, {"x": _HALF}, R, "x" + _NO_CPU)
    add(op, {"wpack": _to(torch.float32), "bias_h": _nc}, R, "bias_h must be contiguous")      # two defects
    add(op, {"x": _nc, "bias_h": _as(127)}, R, "bias_h must be (128,), got (127,)")
    add(op, {"x": _grad, "bias_h": _to(torch.float32)}, R, "expected scalar type Half but found Float (bias_h)")

    # -- graph: contiguity and dtype per tensor in sequence, then shapes, then device ----------------------------------------
    op = "proximity_edges"
    add(op, {}, R, "poses" + _NO_CPU)
    add(op, {"disps": _nc}, R, "disps must be contiguous")
    add(op, {"disps": _DBL}, R, "expected scalar type Float but found Double (disps)")
    add(op, {"jj_known": _INT}, R, "expected scalar type Long but found Int (jj_known)")
    add(op, {"poses": _as(2, 6)}, R, "poses must be (N,7) = t, q(xyzw), got (2, 6)")
    add(op, {"jj_known": _as(3)}, R, "ii_known and jj_known must be 1-D and of equal length, got (2,) and (3,)")
    add(op, {"jj_known": lambda t: None}, R, "ii_known and jj_known must both be given or both be None")
    add(op, {"t": lambda t: 2.5}, R, "proximity_edges: t must be an integer, got 2.5")
    add(op, {}, R, "proximity_edges: form must be None, 'small' or 'sorted', got 'large'", form="large")
    add(op, {}, R, "dist" + _NO_CPU, dist=_z(4))
    add(op, {}, R, "dist must be 1-D with one value per cell (4), got (3,)", dist=_z(3))
    add(op, {}, R, "expected scalar type Float but found Double (dist)", dist=_z(4, dtype=torch.float64))
    add(op, {"poses": _DBL, "disps": _nc}, R, "expected scalar type Float but found Double (poses)")   # two defects: per tensor
    add(op, {"disps": lambda t: _nc(t.double())}, R, "disps must be contiguous")
    add(op, {"poses": _as(2, 6), "ii_known": _INT}, R, "expected scalar type Long but found Int (ii_known)")
    add(op, {"poses": _as(2, 6), "jj_known": _as(3)}, R, "ii_known and jj_known must be 1-D and of equal length, got (2,) and (3,)")
    return [pytest.param(*case, id="%s-%d" % (case[0], n)) for n, case in enumerate(c)]


@pytest.mark.parametrize("op,edits,kwargs,exc,message", _census_cases())
def test_refusal_census(lgu, op, edits, kwargs, exc, message):
    """Each operator's argument refusals on CPU tensors: the exception type, the whole message and, where a call has two
    defects, which one is reported.  None of them touches a device."""
    module, base, tail = _CENSUS_BASE[op]
    args = []
    for name, spec in base.items():
        if spec is None:
            value = 2                                            # proximity_edges' frame count t
        else:
            shape, dtype = spec if isinstance(spec[0], tuple) else (spec, torch.float32)
            value = torch.zeros(shape, dtype=dtype)
        args.append(edits[name](value) if name in edits else value)
    assert not set(edits) - set(base)
    with pytest.raises(exc) as info:
        getattr(getattr(lgu, module), op)(*args, *tail, **kwargs)
    assert type(info.value) is exc and str(info.value) == message


def test_refusal_census_covers_every_operator():
    assert {case.values[0] for case in _census_cases()} == set(_CENSUS_BASE) and len(_census_cases()) == 307
