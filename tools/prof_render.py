#!/usr/bin/env python3
"""Device-event medians of the offscreen view (lgu_slam_amd.render.render_view, csrc/render.hip) in its two forms of the
pixel offer (the 64-bit atomic minimum alone; a plain load in front of it that skips the atomic when the key already there is
not larger) against a torch composition written here only (project with torch operators, `scatter_reduce_(amin)` on int64
keys, points only; its bits are torch's, it is no route of the library), side by side in one process.  Writes
profiles/render_prof.json and prints it as ONE JSON line.

Workloads, all into 540x960 with point_size 2, with and without one frustum per frame: 16 dirty frames of 48x64, 256 of 256
frames of 48x64, 32 frames at the full 384x512 (stride 1).  Scene: cameras a few centimetres apart on a path; a quarter of
each frame's pixels (a band of columns) back-projected at depths around 1 to 3; the view is pulled back behind the last
camera and looks at the middle of the cloud.
Method: the sides alternate call by call; the time is between two device events around the call (warm: the operands and the
code objects are resident, the first calls are thrown away; nothing here is a cold number); per side BLOCKS block medians of
`reps` calls each, reported as their median and spread (max - min of the block medians).  `fused_loses`: the kept form's
median is behind the composition's beyond the two spreads.
`device_ms`: DEVICE_BATCH calls back to back between two events, per call, for the whole call, for clear + resolve alone (no
points, no cameras), and by difference for the point and the line launch.  `atomics`: the offers that land inside the image
(counted with torch), what the atomic-only form issues; `atomic_rate_per_s` = atomics / the point launch's time by
difference: the observed rate of 64-bit atomic minima at this contention (`offers_per_covered_pixel`), launch included.
`kernels_us` (with --trace): medians per kernel from a `rocprofv3 --kernel-trace` run of `prof_render.py --sequence`, attributed
by the fixed order of that run's calls; `atomic_rate_per_s_kernel` = atomics / the point kernel's own time.
HBM floor: 15 bytes per point (12 + 3 colour bytes), 8 (clear) + 8 + 7 (resolve) bytes per pixel over PEAK_RATE.
Usage: prof_render.py [--reps N] [--out PATH]
       prof_render.py --sequence                                (the fixed call sequence, to be run under rocprofv3)
       prof_render.py --trace KERNEL_TRACE_CSV [--out PATH]      (adds kernels_us to the JSON file)
"""
import argparse
import csv
import json
import os
import sys

os.environ.setdefault("LGU_DEBUG_KNOBS", "1")      # the two forms of the offer are switched through LGU_RENDER_PRELOAD

import numpy as np  # noqa: E402
import torch  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import lgu_slam_amd  # noqa: E402
from lgu_slam_amd import render  # noqa: E402

PEAK_RATE = 8e12
BLOCKS = 5
DEVICE_BATCH = 10
SEQ_CALLS = 20
SIZE = (540, 960)
INTR = (600.0, 600.0, 479.5, 269.5)
OUT = os.path.join(ROOT, "profiles", "render_prof.json")
WORKLOADS = {"dirty16_48x64": (16, 48, 64), "all256_48x64": (256, 48, 64), "full32_384x512": (32, 384, 512)}
FORMS = {"atomic": "0", "preload": "1"}


def scene(frames, ht, wd, seed):
    """(points (P,3), colors (P,3) uint8, view (7,), intrinsics, cameras (frames,7)) on the device; P = frames*ht*wd/4."""
    rng = np.random.default_rng(seed)
    poses = np.zeros((frames, 7), np.float32)
    centre = np.zeros(3)
    v, u = np.meshgrid(np.arange(ht), np.arange(wd // 4, wd // 2), indexing="ij")          # a quarter of the pixels
    rays = np.stack([(u - wd / 2) / (0.8 * wd), (v - ht / 2) / (0.8 * wd), np.ones_like(u, float)], -1).reshape(-1, 3)
    pts = []
    for k in range(frames):
        poses[k] = render.look_at(centre, centre + (0.3 * np.sin(0.1 * k), 0.0, 1.0)).numpy()
        depth = 2.0 + np.sin(4.0 * rays[:, 1] + 0.05 * k) + 0.01 * rng.standard_normal(len(rays))
        fwd = np.array([0.3 * np.sin(0.1 * k), 0.0, 1.0])
        fwd /= np.linalg.norm(fwd)
        right = np.cross([0.0, 1.0, 0.0], fwd)
        right /= np.linalg.norm(right)
        down = np.cross(fwd, right)
        pts.append(centre + depth[:, None] * (rays[:, :1] * right + rays[:, 1:2] * down + rays[:, 2:] * fwd))
        centre = centre + 0.02 * rng.standard_normal(3) + (0.02, 0.0, 0.0)
    points = np.concatenate(pts).astype(np.float32)
    colors = rng.integers(0, 256, points.shape, dtype=np.uint8)
    mid = points.mean(0)
    view = render.look_at(centre - (0.0, 0.3, 1.5), mid)
    dev = [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (points, colors)]
    return (*dev, view.cuda(), torch.tensor(INTR).cuda(), torch.from_numpy(poses).cuda())


def offers(points, view, intr, s, near=0.01):
    """What the composition and the counting share: (key high word z as int64 bits, ok, x0, y0) with torch operators."""
    t, q = view[:3], view[3:]
    qv = q[:3].expand_as(points)
    uv = 2.0 * torch.linalg.cross(qv, points)
    Y = points + q[3] * uv + torch.linalg.cross(qv, uv) + t
    z = Y[:, 2]
    ok = torch.isfinite(Y).all(1) & (z > near)
    u, v = intr[0] * (Y[:, 0] / z) + intr[2], intr[1] * (Y[:, 1] / z) + intr[3]
    shift = 1.0 - 0.5 * s
    x0 = torch.nan_to_num(torch.floor(u + shift), nan=0.0).clamp(-2.0 ** 31, 2.0 ** 31 - 1).long()
    y0 = torch.nan_to_num(torch.floor(v + shift), nan=0.0).clamp(-2.0 ** 31, 2.0 ** 31 - 1).long()
    return z, ok, x0, y0


def composed(points, colors, view, intr, size, s=2, background=255):
    """The yardstick: points only, uint8 colours, int64 keys (a positive float's bits are a positive int32)."""
    H, W = size
    z, ok, x0, y0 = offers(points, view, intr, s)
    c = colors.long()
    key = (z.view(torch.int32).long() << 32) | (c[:, 0] << 16) | (c[:, 1] << 8) | c[:, 2]
    keys = torch.full((H * W + 1,), torch.iinfo(torch.int64).max, dtype=torch.int64, device=points.device)
    for dy in range(s):
        for dx in range(s):
            x, y = x0 + dx, y0 + dy
            inside = ok & (x >= 0) & (x < W) & (y >= 0) & (y < H)
            keys.scatter_reduce_(0, torch.where(inside, y * W + x, H * W), key, "amin")      # slot H*W takes the misses
    keys = keys[:-1].view(H, W)
    empty = keys == torch.iinfo(torch.int64).max
    image = torch.stack([(keys >> 16) & 255, (keys >> 8) & 255, keys & 255], -1).to(torch.uint8)
    image[empty] = background
    depth = (keys >> 32).to(torch.int32).view(torch.float32).clone()
    depth[empty] = float("inf")
    return image, depth


def count_offers(points, view, intr, size, s=2):
    H, W = size
    z, ok, x0, y0 = offers(points, view, intr, s)
    n = 0
    for dy in range(s):
        for dx in range(s):
            x, y = x0 + dx, y0 + dy
            n += int((ok & (x >= 0) & (x < W) & (y >= 0) & (y < H)).sum())
    return n


def fused(form, ops, cams=None):
    os.environ["LGU_RENDER_PRELOAD"] = FORMS[form]
    return render.render_view(*ops[:4], SIZE, cameras=cams)


def blocks(fns, reps, warmup=3):
    """{side: [block median ms]}: the sides alternate call by call, in an order drawn anew (seeded) for every round, so that
    no side always runs behind the same other one."""
    med = {k: [] for k in fns}
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    order, rng = list(fns.items()), np.random.default_rng(0)
    for _ in range(BLOCKS):
        ts = {k: [] for k in fns}
        for r in range(reps):
            for name, fn in [order[i] for i in rng.permutation(len(order))]:
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn()
                b.record()
                b.synchronize()
                ts[name].append(a.elapsed_time(b))
        for k in fns:
            med[k].append(float(np.median(ts[k])))
    return med


def batch_ms(fn, reps):
    """ms per call, DEVICE_BATCH calls back to back between two events."""
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


def sequence():
    """The fixed order a kernel trace is attributed by: per workload, per form, without and with cameras, SEQ_CALLS calls."""
    with torch.no_grad():
        for name, (frames, ht, wd) in WORKLOADS.items():
            ops = scene(frames, ht, wd, seed=frames + ht)
            for form in FORMS:
                for cams in (None, ops[4]):
                    for _ in range(SEQ_CALLS):
                        fused(form, ops, cams)
                    torch.cuda.synchronize()


def summarise_trace(path, out):
    rows = sorted((r for r in csv.DictReader(open(path)) if "render_" in r["Kernel_Name"]), key=lambda r: int(r["Start_Timestamp"]))
    short = lambda r: next(k for k in ("render_clear", "render_points", "render_lines", "render_resolve") if k in r["Kernel_Name"])  # noqa: E731
    doc = json.load(open(out))
    at = 0
    for name in WORKLOADS:
        w = doc["workloads"][name]
        w["kernels_us"] = {}
        for form in FORMS:
            for cams in (False, True):
                per = {}
                for _ in range(SEQ_CALLS * (4 if cams else 3)):
                    r = rows[at]
                    at += 1
                    per.setdefault(short(r), []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-3)
                assert ("render_lines" in per) == cams and len(per["render_points"]) == SEQ_CALLS, "the trace is not of --sequence"
                w["kernels_us"]["%s_%s" % (form, "cameras" if cams else "points")] = {k: float(np.median(v)) for k, v in per.items()}
        w["atomic_rate_per_s_kernel"] = w["atomics"] / (w["kernels_us"]["atomic_points"]["render_points"] * 1e-6)
    assert at == len(rows), "the trace holds other render calls"
    json.dump(doc, open(out, "w"), indent=1, sort_keys=True)
    print(json.dumps(doc, sort_keys=True))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=OUT)
    ap.add_argument("--sequence", action="store_true", help="run the fixed call sequence only (under rocprofv3 --kernel-trace)")
    ap.add_argument("--trace", help="add the kernel medians of this rocprofv3 kernel-trace CSV to the JSON file")
    args = ap.parse_args()
    if args.trace:
        return summarise_trace(args.trace, args.out)
    assert torch.cuda.is_available(), "prof_render.py measures on the GPU"
    lgu_slam_amd._lib.load()
    assert lgu_slam_amd._lib.debug_knobs_enabled()
    if args.sequence:
        return sequence()
    res = {}
    H, W = SIZE
    with torch.no_grad():
        for name, (frames, ht, wd) in WORKLOADS.items():
            ops = scene(frames, ht, wd, seed=frames + ht)
            points, colors, view, intr, cams = ops
            P = points.shape[0]
            got = {form: fused(form, ops) for form in FORMS}
            want = composed(points, colors, view, intr, SIZE)
            forms_agree = all(torch.equal(got["atomic"][i].view(torch.int32) if i else got["atomic"][i],
                                          got["preload"][i].view(torch.int32) if i else got["preload"][i]) for i in (0, 1))
            differs = int(((got["atomic"][0] != want[0]).any(-1) | (got["atomic"][1].view(torch.int32) != want[1].view(torch.int32))).sum())
            covered = int(torch.isfinite(got["atomic"][1]).sum())
            atomics = count_offers(points, view, intr, SIZE)
            sides = {"atomic": lambda: fused("atomic", ops), "preload": lambda: fused("preload", ops),
                     "composed": lambda: composed(points, colors, view, intr, SIZE),
                     "atomic_cameras": lambda: fused("atomic", ops, cams), "preload_cameras": lambda: fused("preload", ops, cams)}
            st = {k: stats(v) for k, v in blocks(sides, args.reps).items()}
            none = (points[:0], colors[:0], view, intr)
            dev_ms = {"clear_resolve": batch_ms(lambda: fused("atomic", none), args.reps)}
            for form in FORMS:
                dev_ms[form] = batch_ms(lambda: fused(form, ops), args.reps)
                dev_ms[form + "_cameras_only"] = batch_ms(lambda: fused(form, none, cams), args.reps)
                dev_ms[form + "_points_by_difference"] = dev_ms[form] - dev_ms["clear_resolve"]
                dev_ms[form + "_lines_by_difference"] = dev_ms[form + "_cameras_only"] - dev_ms["clear_resolve"]
            floor_bytes = 15 * P + 23 * H * W
            kept = min(FORMS, key=lambda f: st[f]["median_ms"])
            res[name] = {"frames": frames, "ht": ht, "wd": wd, "points": P, "atomics": atomics, "covered_pixels": covered,
                         "offers_per_covered_pixel": atomics / float(max(covered, 1)), "forms_agree": bool(forms_agree),
                         "pixels_differing_from_composition": differs, "sides": st, "faster_form": kept,
                         "speedup_over_composition": st["composed"]["median_ms"] / st[kept]["median_ms"],
                         "fused_loses": bool(st[kept]["median_ms"] - st[kept]["spread_ms"] >
                                             st["composed"]["median_ms"] + st["composed"]["spread_ms"]),
                         "device_ms": dev_ms,
                         "atomic_rate_per_s": atomics / max(dev_ms["atomic_points_by_difference"] * 1e-3, 1e-12),
                         "floor_bytes": floor_bytes, "floor_ms": floor_bytes / PEAK_RATE * 1e3,
                         "floor_fraction": floor_bytes / PEAK_RATE * 1e3 / dev_ms[kept]}
            del ops, points, colors, cams, got, want
            torch.cuda.empty_cache()
    doc = {"tool": "prof_render", "device": torch.cuda.get_device_name(0), "lib": lgu_slam_amd._lib.version(), "reps": args.reps,
           "blocks": BLOCKS, "peak_rate": PEAK_RATE, "size": list(SIZE), "point_size": 2, "state": "warm", "workloads": res}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(doc, open(args.out, "w"), indent=1, sort_keys=True)
    print(json.dumps(doc, sort_keys=True))


if __name__ == "__main__":
    main()
