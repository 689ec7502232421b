#!/usr/bin/env python3
"""Device-event medians of GaussianMask.gaussian_parameters with the fused parameter head installed
(lgu_slam_amd.gaussian_mask.install, csrc/gausshead.hip) against the same call uninstalled (three library GEMMs, their bias
passes and a tanh launch in front of ops.gaussian_params: the parent's behaviour), on two modules with the same seeded
weights on the same GPU, and of CorrBlock.__init__ at E = 20 on both routes.  Writes profiles/gausshead_prof.json and prints
it as ONE JSON line.

Workloads: E in {1, 20, 48} at 48 x 64; forms: half maps under float16 autocast, fp32 maps with autocast off.
Method (tools/prof_heads.py's): the two sides alternate call by call in one process; every timed call runs on the next of
ROT disjoint input sets after a pass over a FLUSH_BYTES buffer (cold caches: the sets of E = 1 alone would stay in the
last-level cache), and a spin kernel ahead of the first event keeps the host's enqueue time out of the window.  Reported
per side: median, quartiles and spread = p75 - p25 (ms).  `keep_fused`: the fused median beats the uninstalled one beyond
the two spreads.  `min_fused_pixels`: the smallest E*h*w from which every measured class keeps the fused route, the rule by
which lgu_slam_amd.gaussian_mask.MIN_FUSED_PIXELS is set (0: every class keeps it).
Read floor of the kernel: x once, E*h*w * 256 * element size bytes, over the measured device copy rate (a copy kernel of
the same bytes in the same trace, read + write counted) and over PEAK_RATE = 8 TB/s; floor fractions = floor / kernel time,
the kernel time from a kernel trace.
Usage: prof_gausshead.py [--reps N] [--out PATH]
       prof_gausshead.py --markers --reps 0        (each side of each form once between spin kernels, for a kernel trace)
       prof_gausshead.py --trace KERNEL_TRACE_CSV [--out PATH]   (adds kernel medians, floor fractions and launch counts of
                                                a `rocprofv3 --kernel-trace` run of the --markers pass to the JSON file)
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
from tests import gausshead_restatement as R  # noqa: E402

PEAK_RATE = 8e12
ROT = 4
SPIN = 400000
FLUSH_BYTES = 512 << 20
H, W = 48, 64
EDGES = (1, 20, 48)
FORMS = {"autocast_h16": (torch.float16, True), "fp32": (torch.float32, False)}      # x dtype, float16 autocast on
OUT = os.path.join(ROOT, "profiles", "gausshead_prof.json")
GM = lgu_slam_amd.gaussian_mask


def stats(ts):
    q = np.percentile(ts, [25, 50, 75])
    return {"median_ms": float(q[1]), "p25_ms": float(q[0]), "p75_ms": float(q[2]), "spread_ms": float(q[2] - q[0]),
            "min_ms": float(np.min(ts))}


def make_ga():
    return R.load(lgu_slam_amd.GaussianMask(H, W), *R.make_weights(7)).eval().cuda()


def sides():
    """(installed, uninstalled): two GaussianMask with the same weights."""
    fused, module = make_ga(), make_ga()
    GM.install(fused)
    return fused, module


def make_inputs(form, E, count, seed):
    g = torch.Generator().manual_seed(seed)
    return [(torch.randn((E, H, W, 256), generator=g) * 0.3).cuda().to(FORMS[form][0]) for _ in range(count)]


def timed(fns, xs, reps, flush, warmup=3):
    """{side: [ms]}: the sides alternate call by call; call k of a side uses input set k % len(xs), caches flushed."""
    ts = {k: [] for k in fns}
    for k in range(warmup + reps):
        for name, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            flush.add_(1)
            torch.cuda._sleep(SPIN)
            a.record()
            fn(xs[k % len(xs)])
            b.record()
            b.synchronize()
            if k >= warmup:
                ts[name].append(a.elapsed_time(b))
    return ts


def compare(f, o):
    return {"fused": f, "module": o, "speedup": o["median_ms"] / f["median_ms"],
            "keep_fused": bool(f["median_ms"] + f["spread_ms"] < o["median_ms"] - o["spread_ms"])}


def measure(reps, flush):
    res = {}
    for E in EDGES:
        r = {"E": E, "H": H, "W": W, "pixels": E * H * W, "forms": {}}
        for form, (dtype, ac) in FORMS.items():
            with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16, enabled=ac):
                fused, module = sides()
                xs = make_inputs(form, E, ROT, E + 11)
                got, own = fused.gaussian_parameters(xs[0]), module.gaussian_parameters(xs[0])
                assert fused.gaussian_parameters.fused_calls == 1 and [t.dtype for t in got] == [t.dtype for t in own]
                ts = timed({"fused": fused.gaussian_parameters, "module": module.gaussian_parameters}, xs, reps, flush)
                d = compare(stats(ts["fused"]), stats(ts["module"]))
                d["max_abs_diff_to_module"] = [float((a.double() - b.double()).abs().max()) for a, b in zip(got, own)]
                r["forms"][form] = d
                del xs
                torch.cuda.empty_cache()
        res["E%d" % E] = r
    return res


def corrblock_sides(E):
    """(make(installed?) -> callable of (fmap1, fmap2) that builds a CorrBlock under autocast, inputs)."""
    nn = torch.nn
    torch.manual_seed(5)
    ofsMap, ofs_residual = nn.Conv2d(256, 98, 3, padding=1).cuda().eval(), nn.Conv2d(256, 98, 3, padding=1).cuda().eval()
    fused, module = sides()

    def build(ga):
        def fn(maps):
            blk = lgu_slam_amd.CorrBlock(ofsMap, ofs_residual, ga, maps[0], maps[1])
            del blk
        return fn
    g = torch.Generator().manual_seed(77)
    maps = [tuple((torch.randn((1, E, 128, H, W), generator=g) * 0.3).cuda().half() for _ in range(2)) for _ in range(2)]
    return build(fused), build(module), maps, fused


def measure_corrblock(reps, flush, E=20):
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        f, m, maps, ga = corrblock_sides(E)
        f(maps[0]), m(maps[0])
        assert ga.gaussian_parameters.fused_calls == 1
        ts = timed({"fused": f, "module": m}, maps, reps, flush, warmup=2)
    d = compare(stats(ts["fused"]), stats(ts["module"]))
    d.update(E=E, H=H, W=W, form="autocast_h16")
    return d


def labels():
    return [(E, form, side) for E in EDGES for form in FORMS for side in ("fused", "module")]


def markers():
    """Each side of each form of each workload, then a copy of x's bytes, between torch.cuda._sleep spin kernels."""
    for E, form, side in labels():
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16, enabled=FORMS[form][1]):
            xs = make_inputs(form, E, 5, 9)
            dst = torch.empty_like(xs[0])
            ga = sides()[0 if side == "fused" else 1]
            for _ in range(3):
                ga.gaussian_parameters(xs[0])          # warm-up: caches, library algorithm choice
            torch.cuda.synchronize()
            torch.cuda._sleep(1000)
            for k in range(5):
                ga.gaussian_parameters(xs[k])
            torch.cuda._sleep(1000)
            for k in range(5):
                dst.copy_(xs[k])
            torch.cuda._sleep(1000)
            torch.cuda.synchronize()


def summarise_trace(path, out):
    rows = list(csv.DictReader(open(path)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    spins = [i for i, r in enumerate(rows) if "spin" in r["Kernel_Name"].lower() or "sleep" in r["Kernel_Name"].lower()]
    groups = [rows[spins[i] + 1:spins[i + 1]] for i in range(len(spins) - 1)]
    doc = json.load(open(out)) if os.path.exists(out) else {"workloads": {}}

    def us(r):
        return (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-3
    for n, (E, form, side) in enumerate(labels()):
        calls, copies = groups[3 * n], groups[3 * n + 1]      # groups[3 n + 2]: the next label's warm-up
        d = doc["workloads"].setdefault("E%d" % E, {}).setdefault("trace", {}).setdefault(form, {})
        per = {}
        for r in calls:
            per.setdefault(r["Kernel_Name"][:96], []).append(us(r))
        d[side] = {"launches_per_call": len(calls) / 5.0, "kernels_us": {k: float(np.median(v)) for k, v in per.items()},
                   "kernel_sum_us": float(sum(np.median(v) * len(v) for v in per.values()) / 5.0)}
        if side == "fused":
            mine = [v for k, v in per.items() if "gausshead" in k]
            nbytes = E * H * W * 256 * (4 if FORMS[form][0] == torch.float32 else 2)
            copy_us = float(np.median([us(r) for r in copies])) if copies else None
            if mine:
                med = float(np.median(mine[0]))
                k = {"median_us": med, "x_bytes": nbytes, "peak_floor_us": nbytes / PEAK_RATE * 1e6,
                     "peak_floor_fraction": nbytes / PEAK_RATE * 1e6 / med}
                if copy_us:
                    rate = 2 * nbytes / (copy_us * 1e-6)
                    k.update(copy_us=copy_us, copy_rate_bytes_per_s=rate, copy_floor_us=nbytes / rate * 1e6,
                             copy_floor_fraction=nbytes / rate * 1e6 / med)
                d["gausshead_kernel"] = k
    json.dump(doc, open(out, "w"), indent=1, sort_keys=True)
    print(json.dumps(doc, sort_keys=True))


def thresholds(workloads):
    """0 if every class keeps the fused route, else the pixel count of the smallest class from which all larger ones keep
    it (1 << 62: none does)."""
    classes = sorted((w["pixels"], all(v["keep_fused"] for v in w["forms"].values())) for w in workloads.values())
    need = 0
    for i, (pixels, keep) in enumerate(classes):
        if not keep:
            need = classes[i + 1][0] if i + 1 < len(classes) else 1 << 62
    return need


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
    GM.MIN_FUSED_PIXELS = 0          # measure the fused route at every class; the rule is applied afterwards
    if args.markers:
        markers()
    if args.reps <= 0:
        return
    flush = torch.zeros(FLUSH_BYTES // 4, device="cuda")
    workloads = measure(args.reps, flush)
    doc = {"tool": "prof_gausshead", "device": torch.cuda.get_device_name(0), "lib": lgu_slam_amd._lib.version(),
           "reps": args.reps, "rotation": ROT, "flush_bytes": FLUSH_BYTES, "peak_rate": PEAK_RATE, "workloads": workloads,
           "corrblock_init": measure_corrblock(max(args.reps // 2, 4), flush), "min_fused_pixels": thresholds(workloads)}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(doc, open(args.out, "w"), indent=1, sort_keys=True)
    print(json.dumps(doc, sort_keys=True))


if __name__ == "__main__":
    main()
