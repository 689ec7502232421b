#!/usr/bin/env python3
"""Times the proximity-edge selection (lgu_slam_amd.graph, csrc/graphsel.hip) on one GPU against the reference-shaped
host loop.  Prints ONE JSON line.

Shapes (48x64 frames, the camera path of tests.test_geom.scene):
  frontend  t=30, t0=25, t1=5, rad 2, nms 1, thresh 16, max_factors 48, 40 known edges     (one call per keyframe)
  init      t=12, t0=0,  t1=0, rad 2, nms 2, thresh 16, max_factors 48                      (the initialisation)
  backend   t=256, t0=0, t1=0, rad 2, nms 3, thresh 22, max_factors 16 t                    (one global BA)
Per shape:
  reference_loop_ms   the selection driven as the reference drives it (factor_graph.py:319-383) over the distances ON
                      THE DEVICE: tensor masks for the row rule and the cap, one scalar device write per suppressed cell,
                      argsort on the device, then a host loop over ALL n sorted cells with one `.item()` per cell.  The
                      distances are computed before the clock starts.  Host wall time, median of --loop-reps runs.
  edges_e2e_ms        proximity_edges end to end: pair list, frame_distance over the pruned pairs, selection, the one
                      read of the count.  Host wall time (the call ends in that read), median of --reps.
  edges_dist_given_ms proximity_edges(dist=...) (selection + read) per form, host wall time.
  select_*_us         the selection launches alone, device events, no read: the one-launch form ("small", n <= 4096),
                      and keys + torch.sort + greedy ("sorted").
  share_under_thresh  the share of the window's cells whose distance passes the threshold; accepted = edges selected
                      beyond the prefix; same_edges: the loop and proximity_edges return the same list.
Usage: prof_graph.py [--reps N] [--loop-reps N]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import lgu_slam_amd  # noqa: E402
from lgu_slam_amd import graph as LG  # noqa: E402
from lgu_slam_amd.ops import _ptr, _stream  # noqa: E402
from tests.test_geom import scene  # noqa: E402

SHAPES = (
    ("frontend", dict(t=30, t0=25, t1=5, rad=2, nms=1, thresh=16.0, max_factors=48), 40),
    ("init", dict(t=12, t0=0, t1=0, rad=2, nms=2, thresh=16.0, max_factors=48), 0),
    ("backend", dict(t=256, t0=0, t1=0, rad=2, nms=3, thresh=22.0, max_factors=16 * 256), 0),
)
BETA = 0.25


def reference_loop(d, t, kii, kjj, t0, t1, rad, nms, thresh, max_factors, stereo=False):
    """The reference's way of driving the selection, on a device tensor d (n,) (modified)."""
    W = t - t1
    ii, jj = torch.meshgrid(torch.arange(t0, t), torch.arange(t1, t), indexing="ij")
    ii, jj = ii.reshape(-1), jj.reshape(-1)
    inf = float("inf")
    d[(ii - rad < jj).to(d.device)] = inf
    d[d > 100] = inf

    def suppress(i, j):
        r = max(min(abs(i - j) - 2, nms), 0)
        for di in range(-nms, nms + 1):
            for dj in range(-nms, nms + 1):
                if abs(di) + abs(dj) <= r and t0 <= i + di < t and t1 <= j + dj < t:
                    d[(i + di - t0) * W + (j + dj - t1)] = inf      # a scalar device write

    for i, j in zip(kii.cpu().tolist(), kjj.cpu().tolist()):
        suppress(i, j)
    es = []
    for i in range(t0, t):
        if stereo:
            es.append((i, i))
            d[(i - t0) * W + (i - t1)] = inf
        for j in range(max(i - rad - 1, 0), i):
            es += [(i, j), (j, i)]
            d[(i - t0) * W + (j - t1)] = inf
    for k in torch.argsort(d, stable=True):
        if d[k].item() > thresh:                                      # one read of the device per cell
            continue
        if len(es) > max_factors:
            break
        i, j = int(ii[k]), int(jj[k])
        es += [(i, j), (j, i)]
        suppress(i, j)
    e = torch.as_tensor(es, device=d.device).reshape(-1, 2)
    return e[:, 0], e[:, 1]


def wall_ms(fn, reps, warmup=2):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), float(min(ts)), float(max(ts))


def event_us(fn, reps, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    return float(np.median(ts))


def launches(p, d, kii, kjj):
    """Callables that enqueue the selection launches of each form on preallocated buffers (no read of the device)."""
    lib = lgu_slam_amd._lib.load()
    t, t0, t1, rad, nms, thresh, mf = (p[k] for k in ("t", "t0", "t1", "rad", "nms", "thresh", "max_factors"))
    n = (t - t0) * (t - t1)
    cap = LG.capacity(t, t0, t1, rad, False, mf)
    e_ii = torch.empty(cap, dtype=torch.int64, device="cuda")
    e_jj = torch.empty_like(e_ii)
    count = torch.empty(1, dtype=torch.int32, device="cuda")
    keys = torch.empty(n, dtype=torch.int64, device="cuda")
    work = torch.empty((n + 31) // 32, dtype=torch.int32, device="cuda")
    nk = kii.shape[0]
    kp = (_ptr(kii), _ptr(kjj)) if nk else (None, None)
    st = _stream(d)

    def small():
        rc = lib.lgu_proximity_select_small(_ptr(d), kp[0], kp[1], nk, t, t0, t1, rad, nms, thresh, mf, 0, _ptr(e_ii), _ptr(e_jj),
                                            cap, _ptr(count), st)
        assert rc == 0, rc

    def srt():
        rc = lib.lgu_proximity_keys(_ptr(d), kp[0], kp[1], nk, t, t0, t1, rad, nms, thresh, 0, _ptr(keys), _ptr(work), st)
        assert rc == 0, rc
        sk = torch.sort(keys).values
        rc = lib.lgu_proximity_select_sorted(_ptr(sk), _ptr(work), t, t0, t1, rad, nms, mf, 0, _ptr(e_ii), _ptr(e_jj), cap,
                                             _ptr(count), st)
        assert rc == 0, rc

    def keys_only():
        lib.lgu_proximity_keys(_ptr(d), kp[0], kp[1], nk, t, t0, t1, rad, nms, thresh, 0, _ptr(keys), _ptr(work), st)

    return ({"small": small} if n <= LG.SMALL_MAX else {}) | {"sorted": srt, "keys_only": keys_only}


def measure(reps, loop_reps):
    res = {}
    for name, p, nknown in SHAPES:
        t, t0, t1 = p["t"], p["t0"], p["t1"]
        n = (t - t0) * (t - t1)
        poses, disps, intr = scene(17, N=t, H=48, W=64)
        P, D, K = (torch.from_numpy(a).cuda() for a in (poses, disps, intr))
        rs = np.random.RandomState(3)
        ki = rs.randint(max(t1 - 2, 0), t, size=nknown).astype(np.int64)
        kj = np.clip(ki + rs.choice([-1, 1], size=nknown) * rs.randint(1, 9, size=nknown), 0, t - 1).astype(np.int64)
        kii, kjj = torch.from_numpy(ki).cuda(), torch.from_numpy(kj).cuda()
        kw = dict(t0=t0, t1=t1, rad=p["rad"], nms=p["nms"], thresh=p["thresh"], max_factors=p["max_factors"])
        # the window's distances, all pairs of it (what the reference computes), for the loop and the dist= forms
        wi, wj = torch.meshgrid(torch.arange(t0, t), torch.arange(t1, t), indexing="ij")
        wi, wj = wi.reshape(-1).cuda(), wj.reshape(-1).cuda()
        d1 = lgu_slam_amd.geom.frame_distance(P, D, K, wi, wj, BETA)
        d2 = lgu_slam_amd.geom.frame_distance(P, D, K, wj, wi, BETA)
        d = .5 * (d1 + d2)
        r = {"n": n, "known_edges": nknown, **p}
        cand = (d <= p["thresh"]) & ~(wi - p["rad"] < wj)
        r["share_under_thresh"] = float(cand.float().mean())
        ii, jj = LG.proximity_edges(P, D, K, t, kii, kjj, beta=BETA, **kw)
        li, lj = reference_loop(d.clone(), t, kii, kjj, **kw)
        r["edges"] = int(ii.shape[0])
        r["accepted"] = (int(ii.shape[0]) - LG.prefix_len(t, t0, p["rad"], False)) // 2
        r["same_edges"] = bool(torch.equal(ii, li) and torch.equal(jj, lj))
        r["reference_loop_ms"] = dict(zip(("median", "min", "max"),
                                          wall_ms(lambda: reference_loop(d.clone(), t, kii, kjj, **kw), loop_reps, warmup=1)))
        r["edges_e2e_ms"] = dict(zip(("median", "min", "max"),
                                     wall_ms(lambda: LG.proximity_edges(P, D, K, t, kii, kjj, beta=BETA, **kw), reps)))
        r["edges_dist_given_ms"] = {}
        for form in (("small", "sorted") if n <= LG.SMALL_MAX else ("sorted",)):
            r["edges_dist_given_ms"][form] = wall_ms(lambda: LG.proximity_edges(None, None, None, t, kii, kjj, dist=d, form=form, **kw),
                                                     reps)[0]
        for form, fn in launches(p, d, kii, kjj).items():
            r["select_%s_us" % form] = event_us(fn, reps)
        r["speedup_e2e_vs_loop"] = r["reference_loop_ms"]["median"] / r["edges_e2e_ms"]["median"]
        res[name] = r
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--loop-reps", type=int, default=3)
    args = ap.parse_args()
    lgu_slam_amd._lib.load()
    assert torch.cuda.is_available(), "prof_graph.py measures on a GPU"
    res = measure(args.reps, args.loop_reps)
    print(json.dumps({"tool": "prof_graph", "device": torch.cuda.get_device_name(0), "lib": lgu_slam_amd._lib.version(),
                      "reps": args.reps, "loop_reps": args.loop_reps, "shapes": res}))


if __name__ == "__main__":
    main()
