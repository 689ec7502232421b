#!/usr/bin/env python3
"""Device-event medians of the fused first layer of the motion encoder (lgu_slam_amd.flow, csrc/flowenc.hip) against the
module's own autocast forward (cast + convolution + ReLU: the path without `flow.install`), and of the whole encoder both
ways, with the same seeded weights on the same GPU.  Writes profiles/flowenc_prof.json and prints it as ONE JSON line.

Workloads (N x H x W): 48 x 48x64 (frontend), 80 x 60x80 (a backend chunk), 1 x 48x64 (MotionFilter).
Method: every timed call runs on the next of ROT disjoint input / output sets (cold rotation: ROT outputs of the large
workloads exceed the 256 MiB last-level cache), the two sides alternate call by call in one process, and a spin kernel
ahead of the first event keeps the host's enqueue time out of the window.  Reported per side: median, quartiles and
spread = p75 - p25 (ms).  `keep_fused`: the fused median beats the module's beyond the two spreads, the rule by which
lgu_slam_amd.flow.MIN_FUSED_PIXELS is set.
Algorithmic bytes of the kernel: N*128*H*W*2 written + N*4*H*W*4 read + 57 344 of packed weights; hbm_share = those bytes /
kernel time / 8 TB/s, the kernel time from a kernel trace (--trace).
Parity per workload: the share of first-layer elements bit-identical to the library's, and the worst error of both in
units of the derived bound of tests/flowenc_restatement.py (float64, at the smallest batch that holds the shape).
Usage: prof_flowenc.py [--reps N] [--out PATH]
       prof_flowenc.py --markers --reps 0       (each form once between spin kernels, for a kernel trace)
       prof_flowenc.py --trace KERNEL_TRACE_CSV [--out PATH]   (adds kernel medians, HBM share and launch counts of a
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
from tests import flowenc_restatement as R  # noqa: E402

HBM = 8e12
ROT = 8
SPIN = 400000
WORKLOADS = (("frontend", 48, 48, 64), ("backend_chunk", 80, 60, 80), ("motion_filter", 1, 48, 64))
FORMS = ("layer1_fused", "layer1_module", "encoder_fused", "encoder_module")
OUT = os.path.join(ROOT, "profiles", "flowenc_prof.json")


def kernel_bytes(N, H, W):
    return N * 128 * H * W * 2 + N * 4 * H * W * 4 + 2 * lgu_slam_amd.flow.WPACK_HALVES


def stats(ts):
    q = np.percentile(ts, [25, 50, 75])
    return {"median_ms": float(q[1]), "p25_ms": float(q[0]), "p75_ms": float(q[2]), "spread_ms": float(q[2] - q[0]),
            "min_ms": float(np.min(ts))}


def forms_of(m, xs):
    fused = lgu_slam_amd.flow.FlowEncoder(m)
    wpack, bias_h = fused.packed()
    return {"layer1_fused": lambda i: lgu_slam_amd.flow.flow_conv7_relu(xs[i], wpack, bias_h),
            "layer1_module": lambda i: m[1](m[0](xs[i])),
            "encoder_fused": lambda i: fused(xs[i]),
            "encoder_module": lambda i: m(xs[i])}


def timed(fns, reps, warmup=3):
    """{form: [ms]}: the forms alternate call by call; call k of a form uses input set k % ROT."""
    ts = {k: [] for k in fns}
    for k in range(warmup + reps):
        for name, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda._sleep(SPIN)
            a.record()
            fn(k % ROT)
            b.record()
            b.synchronize()
            if k >= warmup:
                ts[name].append(a.elapsed_time(b))
    return ts


def parity(m, H, W):
    x = R.make_input(9, 1, H, W)
    s64, S, want = R.conv7_relu(x, m[0].weight.cpu(), m[0].bias.cpu())
    bound, ref = R.allowance(s64, S, R.TERMS1), torch.relu(s64)
    f = forms_of(m, [x.cuda()])
    got, own = f["layer1_fused"](0), f["layer1_module"](0)
    return {"layer1_bit_identical_to_module": float((got == own).double().mean()),
            "layer1_bit_identical_to_restatement": float((got.cpu() == want).double().mean()),
            "layer1_fused_worst_error_in_bounds": float(((got.cpu().double() - ref).abs() / bound).max()),
            "layer1_module_worst_error_in_bounds": float(((own.cpu().double() - ref).abs() / bound).max()),
            "encoder_bit_identical_to_module": float((f["encoder_fused"](0) == f["encoder_module"](0)).double().mean())}


def measure(reps):
    res = {}
    m = R.make_module(41).cuda()
    for name, N, H, W in WORKLOADS:
        g = torch.Generator().manual_seed(N + H)
        xs = [(torch.randn((N, 4, H, W), generator=g) * 40.0).clamp_(-64.0, 64.0).cuda() for _ in range(ROT)]
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
            ts = timed(forms_of(m, xs), reps)
            r = {"N": N, "H": H, "W": W, "kernel_bytes": kernel_bytes(N, H, W), "parity": parity(m, H, W)}
        for k in FORMS:
            r[k] = stats(ts[k])
        for what in ("layer1", "encoder"):
            f, o = r[what + "_fused"], r[what + "_module"]
            r[what + "_speedup"] = o["median_ms"] / f["median_ms"]
            r[what + "_keep_fused"] = bool(f["median_ms"] + f["spread_ms"] < o["median_ms"] - o["spread_ms"])
        res[name] = r
    return res


def markers():
    """Each form of each workload once between torch.cuda._sleep spin kernels (for the launch count in --trace)."""
    m = R.make_module(41).cuda()
    for name, N, H, W in WORKLOADS:
        x = R.make_input(9, N, H, W).cuda()
        fns = forms_of(m, [x])
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
            for k in FORMS:
                for _ in range(3):
                    fns[k](0)                          # warm-up: caches, library algorithm choice
                torch.cuda.synchronize()
                torch.cuda._sleep(1000)
                for _ in range(5):
                    fns[k](0)
                torch.cuda._sleep(1000)
                torch.cuda.synchronize()


def summarise_trace(path, out):
    rows = list(csv.DictReader(open(path)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    spins = [i for i, r in enumerate(rows) if "spin" in r["Kernel_Name"].lower() or "sleep" in r["Kernel_Name"].lower()]
    groups = [rows[spins[i] + 1:spins[i + 1]] for i in range(0, len(spins) - 1, 2)]
    labels = [(w, k) for w in WORKLOADS for k in FORMS]
    doc = json.load(open(out)) if os.path.exists(out) else {"workloads": {}}
    for (w, form), rs in zip(labels, groups):
        name, N, H, W = w
        d = doc["workloads"].setdefault(name, {}).setdefault("trace", {})
        per = {}
        for r in rs:
            per.setdefault(r["Kernel_Name"][:96], []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-3)
        d[form] = {"launches_per_call": len(rs) / 5.0,
                   "kernels_us": {k: float(np.median(v)) for k, v in per.items()},
                   "kernel_sum_us": float(sum(np.median(v) * len(v) for v in per.values()) / 5.0)}
        if form == "layer1_fused":
            us = [v for k, v in per.items() if "flow_conv7_relu_kernel" in k]
            if us:
                med = float(np.median(us[0]))
                d["flow_conv7_relu_kernel"] = {"median_us": med, "bytes": kernel_bytes(N, H, W),
                                               "hbm_share": kernel_bytes(N, H, W) / (med * 1e-6) / HBM}
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
    if args.markers:
        markers()
    if args.reps <= 0:
        return
    doc = {"tool": "prof_flowenc", "device": torch.cuda.get_device_name(0), "lib": lgu_slam_amd._lib.version(),
           "reps": args.reps, "rotation": ROT, "min_fused_pixels": lgu_slam_amd.flow.MIN_FUSED_PIXELS,
           "workloads": measure(args.reps)}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(doc, open(args.out, "w"), indent=1, sort_keys=True)
    print(json.dumps(doc, sort_keys=True))


if __name__ == "__main__":
    main()
