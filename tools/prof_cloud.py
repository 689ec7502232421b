#!/usr/bin/env python3
"""Device-event medians of the map export (lgu_slam_amd.cloud.point_cloud, csrc/cloud.hip) against the composition of the
existing operators it replaces (cloud.point_cloud_composed: geom.iproj under geom.se3_inverse, geom.depth_filter, the mask
and one boolean index, all on the device), both in the exact-size form with float32 colours, side by side in one process.
Writes profiles/cloud_prof.json and prints it as ONE JSON line.

Workloads: 16 dirty frames of a 32-frame buffer at 48x64 (a visualiser tick), 256 of 256 at 48x64 and at 60x80 (a backend
finish: every keyframe dirty).  Scene: cameras a few centimetres apart, a near band (disparity about 1) over a third of the
image on a far background (0.2, below half the mean), so that roughly a third of the pixels survive; `kept_fraction` is what
did.
Method: the two sides alternate call by call; the time is between two device events around the call (it contains the
call's one host read); per side BLOCKS block medians of `reps` calls each, reported as their median and spread (max - min
of the block medians).  `fused_loses`: the fused median is behind the composed one beyond the two spreads.
`min_fused_pixels`: the smallest num*ht*wd from which no measured class loses, the rule by which cloud.MIN_FUSED_PIXELS is
set (0: no class loses).
Launches: library launches per call (counted at lgu_slam_amd._host.launch) and the aten operators dispatched per call
(views and metadata excluded), each of which is at least one more launch or copy.
HBM floor of the fused path: the dirty frames' disparities once, the ballot words twice (written, re-read), 24 bytes per
kept point (point + float32 colour; 12 without colours), over PEAK_RATE; `floor_fraction` = floor / fused median.
`device_only_ms`: the fused path in the capacity form (preallocated buffers, no host read), DEVICE_BATCH calls back to back
between two events, per call: what the three launches and the floor's torch operators cost on the device.
`kernels_us` (with --trace): medians per kernel from a `rocprofv3 --kernel-trace` run of this tool, attributed to a workload
by the grid of the decision (or depth_filter) launch that precedes them.
`decide_valu` / `valu_floor_ms` (with --isa; needs hipcc, no GPU): the decision kernel's VALU instructions counted in its
gfx950 ISA, compiled with the library's flags, priced as tools/prof_geom.py prices depth_filter (4 issue cycles each, 8 for
a transcendental or FP64 one, a wave per 64 pixels of whole workgroups, 1024 SIMDs at 2.4 GHz): the floor of the pass that
dominates the device time; `valu_floor_fraction` = that floor / device_only_ms.
Usage: prof_cloud.py [--reps N] [--out PATH]
       prof_cloud.py --isa [--out PATH]                       (adds decide_valu and the VALU floors to the JSON file)
       prof_cloud.py --trace KERNEL_TRACE_CSV [--out PATH]     (adds kernels_us to the JSON file)
"""
import argparse
import csv
import json
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import torch
from torch.utils._python_dispatch import TorchDispatchMode

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import lgu_slam_amd  # noqa: E402
from lgu_slam_amd import _host, cloud  # noqa: E402

PEAK_RATE = 8e12
BLOCKS = 5
DEVICE_BATCH = 10
OUT = os.path.join(ROOT, "profiles", "cloud_prof.json")
WORKLOADS = {"dirty16_of_32_48x64": (32, 16, 48, 64), "all256_48x64": (256, 256, 48, 64), "all256_60x80": (256, 256, 60, 80)}
_VIEWS = ("view", "reshape", "permute", "transpose", "slice", "select", "unsqueeze", "squeeze", "expand", "alias", "detach",
          "as_strided", "_unsafe_view", "t.default", "sym_", "size", "stride", "is_", "dim", "numel", "empty", "_local_scalar_dense")


def scene(N, ht, wd, seed):
    rng = np.random.default_rng(seed)
    poses = np.zeros((N, 7), np.float32)
    t = np.zeros(3)
    for k in range(N):
        axis = rng.standard_normal(3)
        axis /= np.linalg.norm(axis)
        a = 0.01 * rng.standard_normal()
        poses[k, :3], poses[k, 3:] = t, np.concatenate([np.sin(a / 2) * axis, [np.cos(a / 2)]])
        t = t + 0.02 * rng.standard_normal(3)
    v, u = np.meshgrid(np.linspace(0, 1, ht), np.linspace(0, 1, wd), indexing="ij")
    near = (u > 0.30) & (u < 0.68)
    field = np.where(near, 1.0 + 0.1 * np.sin(4 * v), 0.2)
    disps = (field[None] + 0.002 * rng.standard_normal((N, ht, wd))).astype(np.float32)
    intr = np.array([0.8 * wd, 0.8 * wd, wd / 2, ht / 2], np.float32)
    images = rng.integers(0, 256, (N, 3, 8 * ht, 8 * wd), dtype=np.uint8)
    return [torch.from_numpy(x).cuda() for x in (poses, disps, intr)], torch.from_numpy(images).cuda()


class OpCount(TorchDispatchMode):
    def __init__(self):
        super().__init__()
        self.n = 0

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        name = str(func)
        if not any(v in name for v in _VIEWS):
            self.n += 1
        return func(*args, **(kwargs or {}))


def count_launches(fn):
    """(library launches, aten operators) of one call of fn."""
    seen = []
    real = _host.launch

    def counted(symbol, *a):
        seen.append(symbol)
        return real(symbol, *a)
    mods = [m for m in (cloud, lgu_slam_amd.geom) if getattr(m, "launch", None) is real]
    for m in mods:
        m.launch = counted
    try:
        with OpCount() as oc:
            fn()
    finally:
        for m in mods:
            m.launch = real
    # lgu_cloud_decide_f32 is two launches (decision, scan)
    return sum(2 if s == "lgu_cloud_decide_f32" else 1 for s in seen), oc.n


def blocks(fns, reps, warmup=3):
    """{side: [block median ms]}: the sides alternate call by call."""
    med = {k: [] for k in fns}
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    for _ in range(BLOCKS):
        ts = {k: [] for k in fns}
        for _ in range(reps):
            for name, fn in fns.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn()
                b.record()
                b.synchronize()
                ts[name].append(a.elapsed_time(b))
        for k in fns:
            med[k].append(float(np.median(ts[k])))
    return med


def device_only(call, total, reps):
    """ms per fused call in the capacity form: no host read inside the window."""
    buf = (torch.empty((total, 3), device="cuda"), torch.empty((total, 3), device="cuda"))
    ts = []
    for k in range(reps + 2):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(DEVICE_BATCH):
            cloud.point_cloud(*call, out=buf)
        b.record()
        b.synchronize()
        if k >= 2:
            ts.append(a.elapsed_time(b) / DEVICE_BATCH)
    return float(np.median(ts))


def summarise_trace(path, out):
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"]))
    by_grid = {(num, (ht * wd + 255) // 256): name for name, (N, num, ht, wd) in WORKLOADS.items()}
    doc = json.load(open(out))
    per, cur = {}, None
    for r in rows:
        name = r["Kernel_Name"]
        short = next((k for k in ("cloud_decide", "cloud_scan", "cloud_write", "depth_filter", "iproj") if k in name), None)
        if short is None:
            continue
        if short in ("cloud_decide", "depth_filter"):
            cur = by_grid.get((int(r["Grid_Size_X"]) // 256, int(r["Grid_Size_Y"])))
        if cur is not None:
            per.setdefault(cur, {}).setdefault(short, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-3)
    for name, ks in per.items():
        doc["workloads"][name]["kernels_us"] = {k: float(np.median(v)) for k, v in ks.items()}
    json.dump(doc, open(out, "w"), indent=1, sort_keys=True)
    print(json.dumps(doc, sort_keys=True))


def add_isa(out):
    from lgu_slam_amd import _build
    with tempfile.TemporaryDirectory() as tmp:
        asm_path = os.path.join(tmp, "cloud.s")
        subprocess.check_call([_build._hipcc()] + _build.FLAGS + ["--cuda-device-only", "-S", os.path.join(_build.CSRC, "cloud.hip"),
                               "-o", asm_path], stderr=subprocess.DEVNULL)
        asm = open(asm_path).read()
    m = re.search(r"^(_ZN3lgu\d+cloud_decide_kernel\w*):", asm, re.M)
    valu = [l.split()[0] for l in asm[m.end():asm.index(".Lfunc_end", m.end())].splitlines() if l.strip().startswith("v_")]
    slow = sum(1 for v in valu if re.match(r"^v_(rcp|sqrt|rsq|exp|log|sin|cos)_", v) or "_f64" in v)
    doc = json.load(open(out))
    doc["decide_valu"] = {"valu": len(valu), "slow": slow, "issue_cycles": 4 * (len(valu) - slow) + 8 * slow}
    for w in doc["workloads"].values():
        waves = w["num"] * ((w["ht"] * w["wd"] + 255) // 256) * 4
        w["valu_floor_ms"] = waves * doc["decide_valu"]["issue_cycles"] / (1024 * 2.4e9) * 1e3
        w["valu_floor_fraction"] = w["valu_floor_ms"] / w["device_only_ms"]
    json.dump(doc, open(out, "w"), indent=1, sort_keys=True)
    print(json.dumps(doc, sort_keys=True))


def stats(meds):
    return {"median_ms": float(np.median(meds)), "spread_ms": float(np.max(meds) - np.min(meds)), "block_medians_ms": meds}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=OUT)
    ap.add_argument("--trace", help="add the kernel medians of this rocprofv3 kernel-trace CSV to the JSON file")
    ap.add_argument("--isa", action="store_true", help="add the decision kernel's VALU count and floors to the JSON file (no GPU)")
    args = ap.parse_args()
    if args.trace:
        return summarise_trace(args.trace, args.out)
    if args.isa:
        return add_isa(args.out)
    assert torch.cuda.is_available(), "prof_cloud.py measures on the GPU"
    lgu_slam_amd._lib.load()
    cloud.MIN_FUSED_PIXELS = 0           # measure the fused route at every class; the rule is applied afterwards
    res = {}
    with torch.no_grad():
        for name, (N, num, ht, wd) in WORKLOADS.items():
            video, images = scene(N, ht, wd, seed=N + ht)
            ix = torch.arange(N - num, N, device="cuda")
            thresh = torch.full((num,), 0.02, device="cuda")
            call = (*video, ix, thresh, images)
            fns = {"fused": lambda: cloud.point_cloud(*call), "composed": lambda: cloud.point_cloud_composed(*call)}
            got, want = fns["fused"](), fns["composed"]()
            same = all(torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b)
                       for a, b in zip(got, want))
            kept = int(got[2][-1])
            med = blocks(fns, args.reps)
            f, c = stats(med["fused"]), stats(med["composed"])
            nb = (ht * wd + 255) // 256
            floor_bytes = num * ht * wd * 4 + 2 * num * nb * 4 * 8 + 24 * kept
            lf, lc = count_launches(fns["fused"]), count_launches(fns["composed"])
            res[name] = {"buffer": N, "num": num, "ht": ht, "wd": wd, "pixels": num * ht * wd, "kept": kept,
                         "kept_fraction": kept / float(num * ht * wd), "same_bits": bool(same), "fused": f, "composed": c,
                         "speedup": c["median_ms"] / f["median_ms"],
                         "fused_loses": bool(f["median_ms"] - f["spread_ms"] > c["median_ms"] + c["spread_ms"]),
                         "launches": {"fused": {"library": lf[0], "aten_ops": lf[1]}, "composed": {"library": lc[0], "aten_ops": lc[1]}},
                         "floor_bytes": floor_bytes, "floor_ms": floor_bytes / PEAK_RATE * 1e3,
                         "floor_fraction": floor_bytes / PEAK_RATE * 1e3 / f["median_ms"],
                         "device_only_ms": device_only(call, kept, args.reps)}
            res[name]["device_only_floor_fraction"] = res[name]["floor_ms"] / res[name]["device_only_ms"]
            del video, images
            torch.cuda.empty_cache()
    classes = sorted((w["pixels"], w["fused_loses"]) for w in res.values())
    need = 0
    for i, (pixels, loses) in enumerate(classes):
        if loses:
            need = classes[i + 1][0] if i + 1 < len(classes) else 1 << 62
    doc = {"tool": "prof_cloud", "device": torch.cuda.get_device_name(0), "lib": lgu_slam_amd._lib.version(), "reps": args.reps,
           "blocks": BLOCKS, "peak_rate": PEAK_RATE, "workloads": res, "min_fused_pixels": need}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(doc, open(args.out, "w"), indent=1, sort_keys=True)
    print(json.dumps(doc, sort_keys=True))


if __name__ == "__main__":
    main()
