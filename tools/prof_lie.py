#!/usr/bin/env python3
"""Device-event medians of the lgu_slam_amd.lie operations (csrc/liegroup.hip).  Prints ONE JSON line and writes it to
profiles/lie_prof.json (--out; the --elem-only and --trace forms only print).

Broadcast operations — `G[:, :, None, None] * X` on 4-component points (act) and `G[:, :, None, None, None].adjT(J)`:
  c5   (1,1970,60,80,.)  the backend's edge count (BASELINE config 5)
  c2   (1,20,48,64,.)    a frontend window (config 2)
each as a time and as bytes moved per second (operand read + result written + 28 bytes per group element), next to
  copy   torch.Tensor.copy_ of a tensor of the operand's size: the same read-plus-write byte count, in the same process
         — the streaming rate this memory system gives a plain copy; and
  torch  the torch composition of the same operation on the device (lie.SE3._act / ._adjT: what a user had before).
Cold: consecutive calls rotate over --sets disjoint operand sets and the last --sets results are kept alive, so that no
call finds its lines in the L2 or the 256 MiB Infinity Cache (each set of c5 is 0.3 / 0.9 GB).  c2 fits the caches
whatever is rotated (2 MB / 6 MB per set): its numbers are launch-bound and are named so.

Per-element operations (inv, mul, retr, exp, log, matrix) at 512 poses: the time per call, events around --calls
back-to-back calls (host side included: this is what a caller pays).

Usage: prof_lie.py [--reps N] [--sets N] [--calls N] [--out PATH]
       prof_lie.py --elem-only --calls 10        (the per-element calls alone: the run to put under a kernel trace)
       prof_lie.py --trace KERNEL_TRACE_CSV --calls 10
            summarise a rocprofv3 --kernel-trace of the --elem-only run: dispatches per call of every operation (must be
            1) and the number of other kernels between the first and the last of them (must be 0); with a trace of the
            full run, the median kernel durations of the broadcast kernels and of the copy's kernel, by grid size.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import lgu_slam_amd  # noqa: E402

lie = lgu_slam_amd.lie
ELEM_OPS = ("inv", "mul", "retr", "exp", "log", "matrix")
SHAPES = (("c5", 1970, 60, 80), ("c2", 20, 48, 64))


def poses(*shape, seed=0):
    g = torch.Generator().manual_seed(seed)
    t = torch.randn(*shape, 3, generator=g)
    ax = torch.nn.functional.normalize(torch.randn(*shape, 3, generator=g), dim=-1)
    a = 1.5 * torch.rand(*shape, 1, generator=g)
    return torch.cat([t, torch.sin(a / 2) * ax, torch.cos(a / 2)], -1).cuda()


def rotate_ms(fn, nsets, reps, warmup=2):
    """Median device ms per call of fn(k), k cycling over the sets.  One timed window is 2 * nsets back-to-back calls
    between two events: the queue stays full, so the window holds kernel time (or, for a launch that is shorter than the
    host side of its call, the host's issue rate — the launch-bound case).  The last `nsets` results stay alive so that
    the allocator cannot hand a result the block of the previous one."""
    keep = [None] * nsets
    burst = 2 * nsets
    for k in range(warmup * nsets):
        keep[k % nsets] = fn(k % nsets)
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for k in range(burst):
            keep[k % nsets] = fn(k % nsets)
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) / burst)
    del keep
    return float(np.median(ts))


def elem_calls(G, H, a):
    return {"inv": lambda: G.inv(), "mul": lambda: G * H, "retr": lambda: G.retr(a), "exp": lambda: lie.SE3.exp(a),
            "log": lambda: G.log(), "matrix": lambda: G.matrix()}


def run_elem(calls, timed=True):
    n = 512
    G, H = lie.SE3(poses(n, seed=1)), lie.SE3(poses(n, seed=2))
    a = 0.3 * torch.randn(n, 6, generator=torch.Generator().manual_seed(3)).cuda()
    out = {}
    for name, fn in elem_calls(G, H, a).items():
        fn()
        torch.cuda.synchronize()
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(calls):
            fn()
        e.record()
        e.synchronize()
        out[name] = {"poses": n, "calls": calls, "us_per_call": 1e3 * s.elapsed_time(e) / calls}
    return out


def summarise_trace(path, calls):
    import csv
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"]))
    names = [r["Kernel_Name"] for r in rows]
    mine = [i for i, k in enumerate(names) if "lie_elem_kernel" in k]
    out = {"tool": "prof_lie --trace", "calls_per_operation": calls, "elem_dispatches": len(mine)}
    if mine:
        # one warm-up call + `calls` timed calls per operation, six operations, back to back
        out["dispatches_per_call"] = len(mine) / (len(ELEM_OPS) * (calls + 1))
        out["other_kernels_between_first_and_last"] = (mine[-1] - mine[0] + 1) - len(mine)
        per = {}
        for i in mine:
            per[names[i]] = per.get(names[i], 0) + 1
        out["per_kernel"] = per
        us = [(int(rows[i]["End_Timestamp"]) - int(rows[i]["Start_Timestamp"])) / 1e3 for i in mine]
        out["elem_kernel_us_median"] = float(np.median(us))
    for tag in ("lie_act4_kernel", "lie_stream12_kernel", "copyBuffer"):    # copyBuffer: the runtime's kernel behind copy_
        sel = [r for r in rows if tag in r["Kernel_Name"]]
        by_grid = {}
        for r in sel:
            by_grid.setdefault(int(r["Grid_Size_X"]), []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
        out[tag] = {str(g): {"dispatches": len(v), "kernel_us_median": float(np.median(v))} for g, v in sorted(by_grid.items())}
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--sets", type=int, default=3)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--elem-only", action="store_true")
    ap.add_argument("--trace")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lie_prof.json"))
    args = ap.parse_args()
    if args.trace:
        return summarise_trace(args.trace, args.calls)
    assert torch.cuda.is_available(), "prof_lie.py measures on the GPU"
    lgu_slam_amd._lib.load()
    if args.elem_only:
        print(json.dumps({"tool": "prof_lie --elem-only", "per_element": run_elem(args.calls)}))
        return
    res = {"tool": "prof_lie", "device": torch.cuda.get_device_name(0), "lib": lgu_slam_amd._lib.version(),
           "sets": args.sets, "reps": args.reps, "broadcast": {}, "per_element": run_elem(args.calls)}
    for tag, E, H, W in SHAPES:
        G = lie.SE3(poses(1, E, seed=E))
        for op, tail in (("act4", (4,)), ("adjT", (2, 6))):
            xs = [torch.randn((1, E, H, W) + tail, device="cuda") for _ in range(args.sets)]
            nbytes = 2 * xs[0].numel() * 4 + 28 * E
            if op == "act4":
                Gb = G[:, :, None, None]
                fn = lambda k: Gb * xs[k]  # noqa: E731
                tfn = lambda k: lie.SE3._act(Gb.data, xs[k])  # noqa: E731
            else:
                Gb = G[:, :, None, None, None]
                fn = lambda k: Gb.adjT(xs[k])  # noqa: E731
                tfn = lambda k: lie.SE3._adjT(Gb.data, xs[k])  # noqa: E731
            dsts = [torch.empty_like(x) for x in xs]
            w = {"shape": [1, E, H, W] + list(tail), "bytes": nbytes,
                 "fits_the_256MiB_cache": bool(args.sets * nbytes < 256 * 2 ** 20)}
            # alternate the three candidates twice: the spread between the two rounds is the noise of this run
            rounds = []
            for _ in range(2):
                r = {"ms": rotate_ms(fn, args.sets, args.reps),
                     "copy_ms": rotate_ms(lambda k: (dsts[k].copy_(xs[k]), None)[1], args.sets, args.reps)}
                rounds.append(r)
            w["ms"] = min(r["ms"] for r in rounds)
            w["copy_ms"] = min(r["copy_ms"] for r in rounds)
            w["rounds"] = rounds
            w["torch_ms"] = rotate_ms(tfn, args.sets, max(5, args.reps // 3), warmup=1)
            w["Bps"] = nbytes / (w["ms"] * 1e-3)
            w["copy_Bps"] = 2 * xs[0].numel() * 4 / (w["copy_ms"] * 1e-3)
            w["fraction_of_copy"] = w["Bps"] / w["copy_Bps"]
            w["speedup_vs_torch"] = w["torch_ms"] / w["ms"]
            w["vs_torch_max_abs"] = float((fn(0) - tfn(0)).abs().max())
            res["broadcast"]["%s_%s" % (op, tag)] = w
            del xs, dsts
            torch.cuda.empty_cache()
    line = json.dumps(res)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
