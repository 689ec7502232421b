#!/usr/bin/env python3
"""Device-event medians of GraphAgg's upmask layer on csrc/upmask.hip (lgu_slam_amd.upmask) against the paths it replaces,
with the same seeded weights on the same GPU.  Writes profiles/upmask_prof.json and prints it as ONE JSON line.

Comparisons, per shape class:
  (a) layer:    Upmask(module)(x) against the module's own autocast forward, half and fp32 input;
  (b) upsample: upsample_from_net_(disps_up, disps, ix, x, ...) against the parent path, the module's own autocast forward
                followed by aggregate.upsample_disps_, with float weights (autocast on around the upsampler) and with half
                weights (autocast off around it, as FactorGraph.update calls it), half x.
Shape classes (frames x ht x wd): 12 x 48x64 (frontend), 8 x 60x80 (a config-5 chunk), 1 x 48x64.  The disparity buffer has
frames + 4 rows and ix names `frames` of them.
Method (tools/prof_heads.py's): every timed call runs on the next of ROT disjoint input sets (cold rotation), the two sides
alternate call by call in one process, and a spin kernel ahead of the first event keeps the host's enqueue time out of
the window.  Reported per side: median, quartiles and spread = p75 - p25 (ms).  `keep_fused`: the fused median beats the
baseline's beyond the two spreads.  `min_fused_pixels`: the smallest frames*ht*wd from which every measured class keeps
the fused LAYER, the rule by which lgu_slam_amd.upmask.MIN_FUSED_PIXELS is set (0: every class keeps it).
Floors at HBM_RATE = 8 TB/s: the eager kernel's output written once (1152 B per pixel), the fused kernel's x read once plus
256 B per pixel written; floor_fraction = floor / kernel time, the kernel time from a kernel trace.
Usage: prof_upmask.py [--reps N] [--out PATH]
       prof_upmask.py --markers --reps 0        (each side once between spin kernels, for a kernel trace)
       prof_upmask.py --trace KERNEL_TRACE_CSV [--out PATH]   (adds kernel medians, floor fractions and launch counts of a
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
from tests import upmask_restatement as RU  # noqa: E402

HBM_RATE = 8e12
ROT = 8
SPIN = 400000
WORKLOADS = (("frontend", 12, 48, 64), ("config5_chunk", 8, 60, 80), ("single_frame", 1, 48, 64))
# form -> (kind, input dtype, half weights)
FORMS = {"layer_h16": ("layer", torch.float16, None), "layer_f32": ("layer", torch.float32, None),
         "upsample_f32w": ("upsample", torch.float16, False), "upsample_h16w": ("upsample", torch.float16, True)}
OUT = os.path.join(ROOT, "profiles", "upmask_prof.json")
UM = lgu_slam_amd.upmask
AG = lgu_slam_amd.aggregate


def stats(ts):
    q = np.percentile(ts, [25, 50, 75])
    return {"median_ms": float(q[1]), "p25_ms": float(q[0]), "p75_ms": float(q[2]), "spread_ms": float(q[2] - q[0]),
            "min_ms": float(np.min(ts))}


def sides_of(form):
    """(fused, baseline): callables of one input set (x, disps, ix, disps_up), on two modules with the same weights."""
    kind, _, hw = FORMS[form]
    wrapper, module = UM.Upmask(RU.make_upmask(41, 3.0).cuda()), RU.make_upmask(41, 3.0).cuda()
    if kind == "layer":
        return (lambda s: wrapper(s[0])), (lambda s: module(s[0])), wrapper
    wpack, bias_h = wrapper.packed()

    def fused(s):
        return UM.upsample_from_net_(s[3], s[1], s[2], s[0], wpack, bias_h, half_weights=hw)

    def parent(s):
        mask = module(s[0])
        with torch.autocast("cuda", enabled=not hw):
            return AG.upsample_disps_(s[3], s[1], s[2], mask)
    return fused, parent, wrapper


def make_inputs(form, U, H, W, count, seed):
    dtype = FORMS[form][1]
    g = torch.Generator().manual_seed(seed)
    sets = []
    for _ in range(count):
        x = torch.randn((U, 128, H, W), generator=g) * 2.0
        x.clamp_(min=0.0)            # behind a ReLU: exact zeros
        disps = 0.05 + 1.5 * torch.rand((U + 4, H, W), generator=g)
        ix = torch.randperm(U + 4, generator=g)[:U].sort().values
        sets.append((x.cuda().to(dtype), disps.cuda(), ix.cuda(), torch.zeros((U + 4, 8 * H, 8 * W), device="cuda")))
    return sets


def timed(fns, sets, reps, warmup=3):
    """{side: [ms]}: the sides alternate call by call; call k of a side uses input set k % ROT."""
    ts = {k: [] for k in fns}
    for k in range(warmup + reps):
        for name, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda._sleep(SPIN)
            a.record()
            fn(sets[k % ROT])
            b.record()
            b.synchronize()
            if k >= warmup:
                ts[name].append(a.elapsed_time(b))
    return ts


def measure(reps):
    res = {}
    for name, U, H, W in WORKLOADS:
        r = {"frames": U, "H": H, "W": W, "pixels": U * H * W, "forms": {}}
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
            for form in FORMS:
                fused, base, wrapper = sides_of(form)
                sets = make_inputs(form, U, H, W, ROT, U + H)
                got = fused(sets[0]).clone()
                own = base(sets[0]).clone()
                assert got.dtype == own.dtype and got.shape == own.shape
                assert FORMS[form][0] != "layer" or wrapper.fused_calls == 1
                ts = timed({"fused": fused, "baseline": base}, sets, reps)
                del sets
                torch.cuda.empty_cache()
                f, o = stats(ts["fused"]), stats(ts["baseline"])
                r["forms"][form] = {"fused": f, "baseline": o, "speedup": o["median_ms"] / f["median_ms"],
                                    "max_abs_diff_to_baseline": float((got.double() - own.double()).abs().max()),
                                    "keep_fused": bool(f["median_ms"] + f["spread_ms"] < o["median_ms"] - o["spread_ms"])}
        res[name] = r
    return res


def threshold(workloads):
    """0 if every class keeps the fused layer, else the pixel count of the smallest class from which all larger ones keep
    it (1 << 62: none does)."""
    classes = sorted((w["pixels"], all(v["keep_fused"] for f, v in w["forms"].items() if FORMS[f][0] == "layer"))
                     for w in workloads.values())
    need = 0
    for i, (pixels, keep) in enumerate(classes):
        if not keep:
            need = classes[i + 1][0] if i + 1 < len(classes) else 1 << 62
    return need


def labels():
    return [(w, form, side) for w in WORKLOADS for form in FORMS for side in ("fused", "baseline")]


def markers():
    """Each side of each form of each workload between torch.cuda._sleep spin kernels (for the launch count in --trace)."""
    for (name, U, H, W), form, side in labels():
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
            s = make_inputs(form, U, H, W, 1, 9)[0]
            fn = sides_of(form)[0 if side == "fused" else 1]
            for _ in range(3):
                fn(s)                          # warm-up: caches, library algorithm choice
            torch.cuda.synchronize()
            torch.cuda._sleep(1000)
            for _ in range(5):
                fn(s)
            torch.cuda._sleep(1000)
            torch.cuda.synchronize()


def summarise_trace(path, out):
    rows = list(csv.DictReader(open(path)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    spins = [i for i, r in enumerate(rows) if "spin" in r["Kernel_Name"].lower() or "sleep" in r["Kernel_Name"].lower()]
    groups = [rows[spins[i] + 1:spins[i + 1]] for i in range(0, len(spins) - 1, 2)]
    doc = json.load(open(out)) if os.path.exists(out) else {"workloads": {}}
    for (w, form, side), rs in zip(labels(), groups):
        name, U, H, W = w
        d = doc["workloads"].setdefault(name, {}).setdefault("trace", {}).setdefault(form, {})
        per = {}
        for r in rs:
            per.setdefault(r["Kernel_Name"][:96], []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-3)
        d[side] = {"launches_per_call": len(rs) / 5.0,
                   "kernels_us": {k: float(np.median(v)) for k, v in per.items()},
                   "kernel_sum_us": float(sum(np.median(v) * len(v) for v in per.values()) / 5.0)}
        if side == "fused":
            us = [v for k, v in per.items() if "upmask_kernel" in k]
            if us:
                med = float(np.median(us[0]))
                xbytes = 128 * (4 if FORMS[form][1] == torch.float32 else 2)
                per_pixel = 576 * 2 if FORMS[form][0] == "layer" else xbytes + 256
                floor = U * H * W * per_pixel / HBM_RATE * 1e6
                d["upmask_kernel"] = {"median_us": med, "floor_us": floor, "floor_fraction": floor / med}
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
    UM.MIN_FUSED_PIXELS = 0          # measure the fused path at every class; the rule is applied afterwards
    if args.markers:
        markers()
    if args.reps <= 0:
        return
    workloads = measure(args.reps)
    doc = {"tool": "prof_upmask", "device": torch.cuda.get_device_name(0), "lib": lgu_slam_amd._lib.version(),
           "reps": args.reps, "rotation": ROT, "hbm_rate": HBM_RATE, "workloads": workloads,
           "min_fused_pixels": threshold(workloads)}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(doc, open(args.out, "w"), indent=1, sort_keys=True)
    print(json.dumps(doc, sort_keys=True))


if __name__ == "__main__":
    main()
