#!/usr/bin/env python3
"""Device-event medians of the fused KAN-bias GRU (lgu_slam_amd.gru.KanBiasGRU, csrc/kangru.hip) against the restated
reference composition (tests/kangru_restatement.py: the reference's torch calls) with the same seeded weights, on the
same GPU.  Prints ONE JSON line.

Workloads:
  gru_frontend  48 edges at 48x64, autocast (half)
  gru_c5        80 edges at 60x80, autocast (one config-5 chunk of update_lowmem)
  gru_c5_f32    the same chunk in fp32 (autocast off)
Per workload and form: the whole forward, cold (a 512 MiB buffer rewritten before every timed call, outside the
events) and warm; the three 3x3 convolutions alone (shared by both forms); the remainder (whole - convolutions); the
host wall time per call with a synchronisation.

Algorithmic bytes of the new kernels (s = element size, P = E*128*H*W elements):
  context  P*s (net, read once; the partial sums are E*ceil(HW/256)*128*4 more)
  heads    384*896*s (packed weights) + 4*E*128*s (glo in, three heads out)
  gates    5*P*s (cz, cr, net in; z, r*net out)
  blend    4*P*s (cq, z, net in; out)
share = bytes / kernel time / 8 TB/s, from the kernel trace (--trace).
Usage: prof_kangru.py [--reps N]
       prof_kangru.py --trace KERNEL_TRACE_CSV   (summarise a `rocprofv3 --kernel-trace --stats` run of this tool: the
                                                  median duration of each new kernel per workload, its share of its
                                                  HBM floor, and the kernel launches per forward of each form, counted
                                                  between the spin-kernel markers the tool's --markers pass emits)
"""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import lgu_slam_amd  # noqa: E402
from tests import kangru_restatement as R  # noqa: E402

HBM = 8e12
FLUSH_FLOATS = 128 * 1024 * 1024
# name, E, H, W, half
WORKLOADS = (("gru_frontend", 48, 48, 64, True), ("gru_c5", 80, 60, 80, True), ("gru_c5_f32", 80, 60, 80, False))
KERNELS = ("kangru_context_kernel", "kangru_context_finalize_kernel", "kan_heads_kernel", "kangru_gates_kernel",
           "kangru_blend_kernel")


def time_ms(fn, reps, warmup=3, flush=None):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        if flush is not None:
            flush.add_(1.0)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts))


def host_ms(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def case(E, H, W, half):
    m = R.set_weights(R.RefGRU(), 1234).cuda()
    ins = [t.cuda() for t in R.make_inputs(77, E, H, W)]
    if half:
        ins = [t.half() for t in ins]
    return m, ins


def kernel_bytes(E, H, W, half):
    s = 2 if half else 4
    P = E * 128 * H * W
    return {"kangru_context_kernel": P * s, "kan_heads_kernel": 384 * 896 * s + 4 * E * 128 * s,
            "kangru_gates_kernel": 5 * P * s, "kangru_blend_kernel": 4 * P * s}


def measure(reps):
    flush = torch.empty(FLUSH_FLOATS, device="cuda")
    res = {}
    for name, E, H, W, half in WORKLOADS:
        m, ins = case(E, H, W, half)
        fused = lgu_slam_amd.gru.KanBiasGRU(m)
        net_inp = torch.cat(ins, 1)

        def run(f):
            def go():
                with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16, enabled=half):
                    f()
            return go
        forms = {"fused": run(lambda: fused(*ins)), "reference": run(lambda: R.forward(m, *ins))}
        convs = run(lambda: (m.convz(net_inp), m.convr(net_inp), m.convq(net_inp)))
        r = {"E": E, "H": H, "W": W, "mode": "autocast half" if half else "fp32"}
        c_cold, c_warm = time_ms(convs, reps, flush=flush), time_ms(convs, reps)
        r["convs_ms"] = {"cold": c_cold, "warm": c_warm}
        for form, fn in forms.items():
            cold, warm = time_ms(fn, reps, flush=flush), time_ms(fn, reps)
            r[form] = {"whole_cold_ms": cold, "whole_warm_ms": warm, "remainder_cold_ms": cold - c_cold,
                       "remainder_warm_ms": warm - c_warm, "host_wall_ms": host_ms(fn, reps)}
        r["speedup_whole_cold"] = r["reference"]["whole_cold_ms"] / r["fused"]["whole_cold_ms"]
        r["speedup_remainder_cold"] = r["reference"]["remainder_cold_ms"] / max(r["fused"]["remainder_cold_ms"], 1e-6)
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16, enabled=half):
            d = (fused(*ins).double() - R.forward(m, *ins).double()).abs()
        r["parity_max_abs"] = float(d.max())
        r["parity_not_bit_identical"] = float((d > 0).double().mean())
        res[name] = r
    return res


def markers():
    """Each form of each workload once, between torch.cuda._sleep spin kernels (for the launch count in --trace)."""
    for name, E, H, W, half in WORKLOADS:
        m, ins = case(E, H, W, half)
        fused = lgu_slam_amd.gru.KanBiasGRU(m)
        for f in (lambda: fused(*ins), lambda: R.forward(m, *ins)):
            with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16, enabled=half):
                f()                                   # warm-up: caches, library algorithm choice
                torch.cuda.synchronize()
                torch.cuda._sleep(1000)
                f()
                torch.cuda._sleep(1000)
            torch.cuda.synchronize()


def summarise_trace(path):
    rows = list(csv.DictReader(open(path)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    per = {}
    for name, E, H, W, half in WORKLOADS:
        kb = kernel_bytes(E, H, W, half)
        ntiles = (H * W + 255) // 256
        out = {}
        for k in KERNELS:
            ds = []
            for r in rows:
                kn = r["Kernel_Name"]
                if k not in kn:
                    continue
                if ("_Float16" in kn or "DF16_" in kn) != half:
                    continue
                g = (int(r["Grid_Size_X"]), int(r["Grid_Size_Y"]))
                want = {"kangru_context_kernel": (ntiles * 256, E), "kangru_context_finalize_kernel":
                        (((E * 128 + 255) // 256) * 256, 1), "kan_heads_kernel": (((E + 15) // 16) * 256, 3)}.get(k)
                if want is None:
                    v = 16 // (2 if half else 4) if (H * W) % (8 if half else 4) == 0 else 1
                    want = (((E * 128 * H * W // v + 255) // 256) * 256, 1)
                if g not in (want, (want[0] // 256, want[1])):      # work-items or workgroups
                    continue
                ds.append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-3)
            if ds:
                med = float(np.median(ds))
                out[k] = {"median_us": med, "dispatches": len(ds)}
                if k in kb:
                    out[k]["bytes"] = kb[k]
                    out[k]["hbm_share"] = kb[k] / (med * 1e-6) / HBM
        per[name] = out
    # launches per forward: dispatches between consecutive spin kernels (markers pass: fused, reference per workload)
    spins = [i for i, r in enumerate(rows) if "spin" in r["Kernel_Name"].lower() or "sleep" in r["Kernel_Name"].lower()]
    counts = [spins[i + 1] - spins[i] - 1 for i in range(0, len(spins) - 1, 2)]
    labels = [(w[0], f) for w in WORKLOADS for f in ("fused", "reference")]
    launches = {"%s/%s" % lab: c for lab, c in zip(labels, counts)}
    print(json.dumps({"tool": "prof_kangru --trace", "kernels": per, "launches_per_forward": launches}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--trace", help="summarise this rocprofv3 kernel-trace CSV instead of measuring")
    ap.add_argument("--markers", action="store_true", help="the launch-count pass for a kernel trace")
    args = ap.parse_args()
    if args.trace:
        return summarise_trace(args.trace)
    lgu_slam_amd._lib.load()
    if args.markers:
        markers()
        if args.reps <= 0:
            return
    res = measure(args.reps)
    print(json.dumps({"tool": "prof_kangru", "device": torch.cuda.get_device_name(0), "lib": lgu_slam_amd._lib.version(),
                      "reps": args.reps, "workloads": res}))


if __name__ == "__main__":
    main()
