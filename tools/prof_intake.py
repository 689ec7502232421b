#!/usr/bin/env python3
"""Device-event medians of the frame intake (lgu_slam_amd.intake.frame, csrc/intake.hip) against the same arithmetic as a
composition of torch operators on the device (intake.frame_composed), side by side in one process.  Writes
profiles/intake_prof.json and prints it as ONE JSON line.

Workloads: 480x640 -> 384x512 with 5 distortion coefficients (the TUM camera), one frame and 16; the EuRoC pair 480x752 ->
320x512 (two cameras, rectified); 384x512 with both stages absent (a layout change plus the normalisation), where the
parent's own route is timed too: `raw.permute(0, 3, 1, 2).contiguous()` plus features.normalize_images.  All frames are
device-resident random bytes; outputs go to preallocated `out=` buffers on the fused side.
Method: the sides alternate call by call; the time is between two device events around the call; per side BLOCKS block
medians of `reps` calls each, reported as their median and spread (max - min of the block medians).  `fused_loses`: the
fused median is behind the other side's beyond the two spreads.  `min_fused_pixels`: the smallest N*H*W from which no
measured class loses to the composition, the rule by which intake.MIN_FUSED_PIXELS is set (0: no class loses).
`device_only_ms`: DEVICE_BATCH fused calls back to back between two events, per call.
Launches: library launches per call (counted at lgu_slam_amd._host.launch) and the aten operators dispatched per call (views
and metadata excluded), each of which is at least one more launch or copy.
HBM floor: the raw frame once, 3 bytes and 12 bytes of float per output pixel, over PEAK_RATE; `floor_fraction` = floor /
device_only_ms.
`crossover`: the tile kernel (path="tile") against the direct kernel (path="direct") at 480x640 with 5 coefficients, one frame
and 16, over downscales 1.25 .. 3; `tile_max_scale`: the largest measured scale up to which the tile kernel does not lose at 16
frames, the rule by which intake.TILE_MAX_SCALE is set.
The host OpenCV route of the reference cannot be timed here (OpenCV is not installed): `opencv_host_route` says so.
Usage: prof_intake.py [--reps N] [--out PATH]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch
from torch.utils._python_dispatch import TorchDispatchMode

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import lgu_slam_amd  # noqa: E402
from lgu_slam_amd import _host, features, intake  # noqa: E402

PEAK_RATE = 8e12
BLOCKS = 5
DEVICE_BATCH = 10
OUT = os.path.join(ROOT, "profiles", "intake_prof.json")
SCALES = {"1.25": (384, 512), "1.5": (320, 427), "2.0": (240, 320), "2.5": (192, 256), "3.0": (160, 213)}
_VIEWS = ("view", "reshape", "permute", "transpose", "slice", "select", "unsqueeze", "squeeze", "expand", "alias", "detach",
          "as_strided", "_unsafe_view", "t.default", "sym_", "size", "stride", "is_", "dim", "numel", "empty", "_local_scalar_dense")


def workloads():
    tum = dict(camera=intake.TUM_CAMERA, dist=intake.TUM_DIST, resize=(384, 512))
    return {"tum_480x640_to_384x512_n1": (1, intake.plan((480, 640), **tum)),
            "tum_480x640_to_384x512_n16": (16, intake.plan((480, 640), **tum)),
            "euroc_pair_480x752_to_320x512": (2, intake.plan.euroc((320, 512))),
            "passthrough_384x512_n1": (1, intake.plan((384, 512), (400.0, 400.0, 256.0, 192.0)))}


class OpCount(TorchDispatchMode):
    def __init__(self):
        super().__init__()
        self.n = 0

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        if not any(v in str(func) for v in _VIEWS):
            self.n += 1
        return func(*args, **(kwargs or {}))


def count_launches(fn):
    """(library launches, aten operators) of one call of fn."""
    seen = []
    real = _host.launch

    def counted(symbol, *a):
        seen.append(symbol)
        return real(symbol, *a)
    mods = [m for m in (intake, features) if getattr(m, "launch", None) is real]
    for m in mods:
        m.launch = counted
    try:
        with OpCount() as oc:
            fn()
    finally:
        for m in mods:
            m.launch = real
    return len(seen), oc.n


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


def device_only(fn, reps):
    ts = []
    for k in range(reps + 2):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(DEVICE_BATCH):
            fn()
        b.record()
        b.synchronize()
        if k >= 2:
            ts.append(a.elapsed_time(b) / DEVICE_BATCH)
    return float(np.median(ts))


def stats(meds):
    return {"median_ms": float(np.median(meds)), "spread_ms": float(np.max(meds) - np.min(meds)), "block_medians_ms": meds}


def loses(a, b):
    return bool(a["median_ms"] - a["spread_ms"] > b["median_ms"] + b["spread_ms"])


def buffers(N, plan):
    H, W = plan.out_size
    return (torch.empty((N, 3, H, W), dtype=torch.uint8, device="cuda"), torch.empty((1, N, 3, H, W), device="cuda"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=OUT)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "prof_intake.py measures on the GPU"
    lgu_slam_amd._lib.load()
    intake.MIN_FUSED_PIXELS = 0          # measure the fused route at every class; the rule is applied afterwards
    rng = np.random.default_rng(0)
    res = {}
    with torch.no_grad():
        for name, (N, plan) in workloads().items():
            h0, w0 = plan.src_size
            H, W = plan.out_size
            raw = torch.from_numpy(rng.integers(0, 256, (N, h0, w0, 3), dtype=np.uint8)).cuda()
            out = buffers(N, plan)
            fns = {"fused": lambda: intake.frame(raw, plan, out=out), "composed": lambda: intake.frame_composed(raw, plan)}
            if not plan.rectifies and not plan.resizes:
                fns["parent"] = lambda: features.normalize_images(raw.permute(0, 3, 1, 2).contiguous())
            got, want = fns["fused"](), fns["composed"]()
            differing = int((got[0] != want[0]).sum())
            med = blocks(fns, args.reps)
            side = {k: stats(v) for k, v in med.items()}
            floor_bytes = N * h0 * w0 * 3 + N * H * W * 15
            w = {"N": N, "src": [h0, w0], "out": [H, W], "pixels": N * H * W, "bytes_differing_from_composed": differing,
                 "launches": {k: dict(zip(("library", "aten_ops"), count_launches(fn))) for k, fn in fns.items()},
                 "speedup_over_composed": side["composed"]["median_ms"] / side["fused"]["median_ms"],
                 "fused_loses": loses(side["fused"], side["composed"]),
                 "floor_bytes": floor_bytes, "floor_ms": floor_bytes / PEAK_RATE * 1e3, "device_only_ms": device_only(fns["fused"], args.reps)}
            w.update(side)
            w["floor_fraction"] = w["floor_ms"] / w["device_only_ms"]
            if "parent" in side:
                w["fused_loses_to_parent"] = loses(side["fused"], side["parent"])
                w["speedup_over_parent"] = side["parent"]["median_ms"] / side["fused"]["median_ms"]
            res[name] = w
            del raw, out
            torch.cuda.empty_cache()
        cross = {}
        for N in (1, 16):
            raw = torch.from_numpy(rng.integers(0, 256, (N, 480, 640, 3), dtype=np.uint8)).cuda()
            for scale, size in SCALES.items():
                plan = intake.plan((480, 640), intake.TUM_CAMERA, dist=intake.TUM_DIST, resize=size)
                out = buffers(N, plan)
                fns = {"tile": lambda: intake.frame(raw, plan, out=out, path="tile"),
                       "direct": lambda: intake.frame(raw, plan, out=out, path="direct")}
                a = fns["tile"]()[0].clone()
                same = bool(torch.equal(a, fns["direct"]()[0]))
                side = {k: stats(v) for k, v in blocks(fns, args.reps).items()}
                dev = {k: device_only(fn, args.reps) for k, fn in fns.items()}
                cross["n%d_scale_%s" % (N, scale)] = {"N": N, "scale": float(scale), "out": list(size), "same_bytes": same, "tile": side["tile"],
                                                      "direct": side["direct"], "device_only_ms": dev,
                                                      "tile_loses": bool(dev["tile"] > dev["direct"] and loses(side["tile"], side["direct"]))}
            del raw
            torch.cuda.empty_cache()
    tile_max = 0.0
    for scale in sorted(float(s) for s in SCALES):
        if cross["n16_scale_%s" % scale]["tile_loses"]:
            break
        tile_max = scale
    classes = sorted((w["pixels"], w["fused_loses"]) for w in res.values())
    need = 0
    for i, (pixels, lost) in enumerate(classes):
        if lost:
            need = classes[i + 1][0] if i + 1 < len(classes) else 1 << 62
    doc = {"tool": "prof_intake", "device": torch.cuda.get_device_name(0), "lib": lgu_slam_amd._lib.version(), "reps": args.reps,
           "blocks": BLOCKS, "peak_rate": PEAK_RATE, "workloads": res, "crossover": cross, "tile_max_scale": tile_max,
           "min_fused_pixels": need, "opencv_host_route": "not measured: OpenCV is not installed where this was run"}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(doc, open(args.out, "w"), indent=1, sort_keys=True)
    print(json.dumps(doc, sort_keys=True))


if __name__ == "__main__":
    main()
