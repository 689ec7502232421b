#!/usr/bin/env python3
"""Device-event medians of the fused narrow 3x3 heads (lgu_slam_amd.heads, csrc/heads.hip) against the module's own
autocast forward (the path without `heads.install`), with the same seeded weights on the same GPU: the bare Cout 2 layer
(delta[2]; half and fp32 input), the Cout 2 layer with its sigmoid (a (conv, Identity, Sigmoid) tail) and the eta tail
(conv Cout 1, Identity, Softplus).  Writes profiles/heads_prof.json and prints it as ONE JSON line.

Workloads (N x H x W): 48 x 48x64 (frontend), 80 x 60x80 (a backend chunk), 1 x 48x64 (MotionFilter), and for eta also
12 x 48x64 (eta runs on the unique source frames).
Method (tools/prof_conv3.py's): every timed call runs on the next of ROT disjoint input sets (cold rotation), the two sides
alternate call by call in one process, and a spin kernel ahead of the first event keeps the host's enqueue time out of
the window.  Reported per side: median, quartiles and spread = p75 - p25 (ms).  `keep_fused`: the fused median beats the
module's beyond the two spreads.  `min_fused_pixels`: per Cout, the smallest N*H*W from which every measured class of
that Cout keeps the fused path, the rule by which lgu_slam_amd.heads.MIN_FUSED_PIXELS is set (0: every class keeps it).
Read floor of the kernel: its input once, N*H*W * 128 * element size bytes, at READ_RATE = 5 TB/s (what this mix of
strided plane reads gets); floor_fraction = floor / kernel time, the kernel time from a kernel trace.
Usage: prof_heads.py [--reps N] [--out PATH]
       prof_heads.py --markers --reps 0        (each form once between spin kernels, for a kernel trace)
       prof_heads.py --trace KERNEL_TRACE_CSV [--out PATH]   (adds kernel medians, floor fractions and launch counts of a
                                                `rocprofv3 --kernel-trace` run of the --markers pass to the JSON file)
"""
import argparse
import csv
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import lgu_slam_amd  # noqa: E402
from tests import heads_restatement as RH  # noqa: E402

READ_RATE = 5e12
ROT = 8
SPIN = 400000
WORKLOADS = (("frontend", 48, 48, 64), ("backend_chunk", 80, 60, 80), ("motion_filter", 1, 48, 64), ("eta_frames", 12, 48, 64))
# form -> (Cout, activation, input dtype, workloads it is timed at)
ALL3 = ("frontend", "backend_chunk", "motion_filter")
FORMS = {"bare2_h16": (2, "none", torch.float16, ALL3), "bare2_f32": (2, "none", torch.float32, ALL3),
         "sigmoid2_h16": (2, "sigmoid", torch.float16, ALL3), "eta_h16": (1, "softplus", torch.float16, ALL3 + ("eta_frames",))}
OUT = os.path.join(ROOT, "profiles", "heads_prof.json")
HD = lgu_slam_amd.heads


def stats(ts):
    q = np.percentile(ts, [25, 50, 75])
    return {"median_ms": float(q[1]), "p25_ms": float(q[0]), "p75_ms": float(q[2]), "spread_ms": float(q[2] - q[0]),
            "min_ms": float(np.min(ts))}


def sides_of(form):
    """(fused, module): callables of one input tensor, on two modules with the same weights."""
    cout, act, _, _ = FORMS[form]
    make = (lambda: RH.make_head(41, cout)) if form.startswith("bare") else (lambda: RH.make_tail(41, cout, act))
    return HD.Head(make().cuda()), make().cuda()


def make_inputs(form, N, H, W, count, seed):
    dtype = FORMS[form][2]
    g = torch.Generator().manual_seed(seed)
    xs = []
    for _ in range(count):
        x = torch.randn((N, 128, H, W), generator=g) * 2.0
        x.clamp_(min=0.0)            # behind a ReLU: exact zeros
        xs.append(x.cuda().to(dtype))
    return xs


def timed(fns, xs, reps, warmup=3):
    """{side: [ms]}: the sides alternate call by call; call k of a side uses input set k % ROT."""
    ts = {k: [] for k in fns}
    for k in range(warmup + reps):
        for name, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda._sleep(SPIN)
            a.record()
            fn(xs[k % ROT])
            b.record()
            b.synchronize()
            if k >= warmup:
                ts[name].append(a.elapsed_time(b))
    return ts


def measure(reps):
    res = {}
    for name, N, H, W in WORKLOADS:
        r = {"N": N, "H": H, "W": W, "pixels": N * H * W, "forms": {}}
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
            for form, spec in FORMS.items():
                if name not in spec[3]:
                    continue
                fused, module = sides_of(form)
                xs = make_inputs(form, N, H, W, ROT, N + H)
                got, own = fused(xs[0]), module(xs[0])
                assert fused.fused_calls == 1 and got.dtype == own.dtype and got.shape == own.shape
                ts = timed({"fused": fused, "module": module}, xs, reps)
                del xs
                torch.cuda.empty_cache()
                f, o = stats(ts["fused"]), stats(ts["module"])
                r["forms"][form] = {"fused": f, "module": o, "speedup": o["median_ms"] / f["median_ms"],
                                    "max_abs_diff_to_module": float((got.double() - own.double()).abs().max()),
                                    "keep_fused": bool(f["median_ms"] + f["spread_ms"] < o["median_ms"] - o["spread_ms"])}
        res[name] = r
    return res


def thresholds(workloads):
    """Per Cout: 0 if every class keeps the fused path, else the pixel count of the smallest class from which all larger
    ones keep it (1 << 62: none does)."""
    out = {}
    for cout in (1, 2):
        classes = sorted((w["pixels"], all(v["keep_fused"] for f, v in w["forms"].items() if FORMS[f][0] == cout))
                         for w in workloads.values() if any(FORMS[f][0] == cout for f in w["forms"]))
        need = 0
        for i, (pixels, keep) in enumerate(classes):
            if not keep:
                need = classes[i + 1][0] if i + 1 < len(classes) else 1 << 62
        out[str(cout)] = need
    return out


def labels():
    return [(w, form, side) for w in WORKLOADS for form in FORMS if w[0] in FORMS[form][3] for side in ("fused", "module")]


def markers():
    """Each side of each form of each workload between torch.cuda._sleep spin kernels (for the launch count in --trace)."""
    for (name, N, H, W), form, side in labels():
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
            x = make_inputs(form, N, H, W, 1, 9)[0]
            fn = sides_of(form)[0 if side == "fused" else 1]
            for _ in range(3):
                fn(x)                          # warm-up: caches, library algorithm choice
            torch.cuda.synchronize()
            torch.cuda._sleep(1000)
            for _ in range(5):
                fn(x)
            torch.cuda._sleep(1000)
            torch.cuda.synchronize()


def summarise_trace(path, out):
    rows = list(csv.DictReader(open(path)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    spins = [i for i, r in enumerate(rows) if "spin" in r["Kernel_Name"].lower() or "sleep" in r["Kernel_Name"].lower()]
    groups = [rows[spins[i] + 1:spins[i + 1]] for i in range(0, len(spins) - 1, 2)]
    doc = json.load(open(out)) if os.path.exists(out) else {"workloads": {}}
    for (w, form, side), rs in zip(labels(), groups):
        name, N, H, W = w
        d = doc["workloads"].setdefault(name, {}).setdefault("trace", {}).setdefault(form, {})
        per = {}
        for r in rs:
            per.setdefault(r["Kernel_Name"][:96], []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-3)
        d[side] = {"launches_per_call": len(rs) / 5.0,
                   "kernels_us": {k: float(np.median(v)) for k, v in per.items()},
                   "kernel_sum_us": float(sum(np.median(v) * len(v) for v in per.values()) / 5.0)}
        if side == "fused":
            us = [v for k, v in per.items() if "head3x3_c128_kernel" in k]
            if us:
                med = float(np.median(us[0]))
                floor = N * H * W * 128 * (4 if FORMS[form][2] == torch.float32 else 2) / READ_RATE * 1e6
                d["head3x3_c128_kernel"] = {"median_us": med, "read_floor_us": floor, "floor_fraction": floor / med}
    json.dump(doc, open(out, "w"), indent=1, sort_keys=True)
    print(json.dumps(doc, sort_keys=True))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--out", default=OUT)
    ap.add_argument("--trace", help="add the summary of this rocprofv3 kernel-trace CSV to the JSON file")
    ap.add_argument("--markers", action="store_true", help="the launch-count pass for a kernel trace")
    args = ap.parse_args()
    if args.trace:
        return summarise_trace(args.trace, args.out)
    lgu_slam_amd._lib.load()
    HD.MIN_FUSED_PIXELS = {1: 0, 2: 0}          # measure the fused path at every class; the rule is applied afterwards
    if args.markers:
        markers()
    if args.reps <= 0:
        return
    workloads = measure(args.reps)
    doc = {"tool": "prof_heads", "device": torch.cuda.get_device_name(0), "lib": lgu_slam_amd._lib.version(),
           "reps": args.reps, "rotation": ROT, "read_rate": READ_RATE, "workloads": workloads,
           "min_fused_pixels": thresholds(workloads)}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(doc, open(args.out, "w"), indent=1, sort_keys=True)
    print(json.dumps(doc, sort_keys=True))


if __name__ == "__main__":
    main()
