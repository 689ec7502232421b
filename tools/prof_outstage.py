#!/usr/bin/env python3
"""Device-event medians of the update operator's output stage: the trunk fan-out
(lgu_slam_amd.conv3.conv3x3_fanout, csrc/conv3.hip) and the head pair (lgu_slam_amd.heads.head_pair, csrc/heads.hip)
against the separate launches they replace, and the whole fused forward on both routes, in one process on one GPU.
Writes profiles/outstage_prof.json and prints it as ONE JSON line.

The yardstick is always the separate launches, which stay in place bit-identical: never the new kernel against itself.
Workloads (N x H x W): 48 x 48x64 (frontend), 80 x 60x80 (a backend chunk), 1 x 48x64 (MotionFilter); x is half, which is
what the GRU hands over.
Forms:
  fanout3, fanout2    conv3x3_fanout of three / two packs against three / two conv3x3 launches
  pair_h16            head_pair against two head_conv3x3 + the reference's view / permute / [..., :2] / contiguous
  pair_f32            head_pair(coords=) against the same plus coords + delta.float() and weight.float()
  forward             UpdateOperator (gru_convs=True) with ii, both thresholds at 0 against both above every shape
  forward_coords1     the same with coords1=
Method (tools/prof_conv3.py's): every timed call runs on the next of ROT disjoint input sets, the
two sides alternate call by call, and a spin kernel ahead of the first event keeps the host's enqueue time out of the
window.  Reported per side: median, quartiles and spread = p75 - p25 (ms).  `keep_new`: the new median beats the
yardstick's beyond the two spreads.  `min_fanout_pixels` / `min_pair_pixels`: the smallest N*H*W from which every measured
class keeps the new path (0: every class; 1 << 62: none), the rule by which conv3.MIN_FANOUT_PIXELS and
heads.MIN_PAIR_PIXELS are set.
Algorithmic bytes of the fan-out: x once, G outputs once, G packs once; hbm_share = those bytes / kernel time / 8 TB/s,
the kernel time from a kernel trace.
Usage: prof_outstage.py [--reps N] [--out PATH]
       prof_outstage.py --markers --reps 0     (each side of each form between spin kernels, for a kernel trace)
       prof_outstage.py --trace KERNEL_TRACE_CSV [--out PATH]   (adds kernel medians, shares and launch counts of a
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
from tests import conv3_restatement as R  # noqa: E402
from tests import update_restatement as RU  # noqa: E402

HBM = 8e12
ROT = 8
SPIN = 400000
NEVER = 1 << 62
WORKLOADS = (("frontend", 48, 48, 64), ("backend_chunk", 80, 60, 80), ("motion_filter", 1, 48, 64))
FORMS = ("fanout3", "fanout2", "pair_h16", "pair_f32", "forward", "forward_coords1")
OUT = os.path.join(ROOT, "profiles", "outstage_prof.json")
C3, HD = lgu_slam_amd.conv3, lgu_slam_amd.heads


def stats(ts):
    q = np.percentile(ts, [25, 50, 75])
    return {"median_ms": float(q[1]), "p25_ms": float(q[0]), "p75_ms": float(q[2]), "spread_ms": float(q[2] - q[0]),
            "min_ms": float(np.min(ts))}


def relu_half(g, shape):
    x = torch.randn(shape, generator=g, device="cuda") * 2.0
    return x.clamp_(min=0.0).half()      # behind a ReLU: exact zeros


def make_inputs(form, N, H, W, count, seed):
    """`count` disjoint argument tuples of one form, drawn on the device."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    sets = []
    for _ in range(count):
        if form.startswith("fanout"):
            sets.append((relu_half(g, (N, 128, H, W)),))
        elif form.startswith("pair"):
            sets.append((relu_half(g, (N, 128, H, W)), relu_half(g, (N, 128, H, W)),
                         torch.randn((1, N, H, W, 2), generator=g, device="cuda") * 20.0))
        else:
            sets.append((torch.tanh(torch.randn((1, N, 128, H, W), generator=g, device="cuda")).half(),
                         relu_half(g, (1, N, 128, H, W)),
                         torch.randn((1, N, R.COR_PLANES, H, W), generator=g, device="cuda"),
                         torch.randn((1, N, 4, H, W), generator=g, device="cuda"),
                         torch.randn((1, N, H, W, 2), generator=g, device="cuda") * 20.0))
    return sets


def sides_of(form, u, wr, N):
    """(new, yardstick): callables of one argument tuple."""
    c3 = [C3.pack_conv3(c.weight, c.bias) for c in (u.delta[0], u.weight[0], u.agg.conv1)]
    pd, pw = (HD.pack_head(c.weight, c.bias) for c in (u.delta[2], u.weight[2]))
    if form.startswith("fanout"):
        G = int(form[-1])
        return (lambda a: C3.conv3x3_fanout(a[0], c3[:G], relu=True)), (lambda a: [C3.conv3x3(a[0], *p, relu=True) for p in c3[:G]])
    if form.startswith("pair"):
        f32 = form == "pair_f32"

        def separate(a):
            n, _, h, w = a[0].shape
            delta = HD.head_conv3x3(a[0], *pd, act="none").view(1, n, -1, h, w).permute(0, 1, 3, 4, 2)[..., :2].contiguous()
            weight = HD.head_conv3x3(a[1], *pw, act="sigmoid").view(1, n, -1, h, w).permute(0, 1, 3, 4, 2)[..., :2].contiguous()
            return (a[2] + delta.to(dtype=torch.float), weight.to(dtype=torch.float)) if f32 else (delta, weight)
        return (lambda a: HD.head_pair(a[0], a[1], pd, pw, coords=a[2] if f32 else None)), separate
    ii = (torch.arange(N, device="cuda") // 4).contiguous()
    with_coords = form == "forward_coords1"

    def forward(fan, pair):
        def run(a):
            C3.MIN_FANOUT_PIXELS, HD.MIN_PAIR_PIXELS = fan, pair
            return wr(a[0], a[1], a[2], a[3], ii, coords1=a[4] if with_coords else None)
        return run
    return forward(0, 0), forward(NEVER, NEVER)


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


def flat(out):
    return list(out) if isinstance(out, (tuple, list)) else [out]


def measure(reps, forms):
    res = {}
    u = RU.make_update(41).cuda()
    wr = lgu_slam_amd.update.UpdateOperator(u, gru_convs=True)
    for name, N, H, W in WORKLOADS:
        r = {"N": N, "H": H, "W": W, "pixels": N * H * W, "forms": {}}
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
            for form in forms:
                new, old = sides_of(form, u, wr, N)
                sets = make_inputs(form, N, H, W, ROT, N + H)
                same = all(torch.equal(a, b) for a, b in zip(flat(new(sets[0])), flat(old(sets[0]))))
                ts = timed({"new": new, "separate": old}, sets, reps)
                del sets
                torch.cuda.empty_cache()
                f, o = stats(ts["new"]), stats(ts["separate"])
                r["forms"][form] = {"new": f, "separate": o, "speedup": o["median_ms"] / f["median_ms"], "bit_identical": bool(same),
                                    "keep_new": bool(f["median_ms"] + f["spread_ms"] < o["median_ms"] - o["spread_ms"])}
        res[name] = r
    return res


def threshold(workloads, forms):
    """0 if every class keeps the new path in every one of `forms`, else the pixel count of the smallest class from which
    all larger ones keep it (1 << 62: none does)."""
    classes = sorted((w["pixels"], all(w["forms"][f]["keep_new"] for f in forms)) for w in workloads.values())
    need = 0
    for i, (pixels, keep) in enumerate(classes):
        if not keep:
            need = classes[i + 1][0] if i + 1 < len(classes) else NEVER
    return need


def markers():
    """Each side of each form of each workload between torch.cuda._sleep spin kernels (for the launch count in --trace)."""
    u = RU.make_update(41).cuda()
    wr = lgu_slam_amd.update.UpdateOperator(u, gru_convs=True)
    for name, N, H, W in WORKLOADS:
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
            for form in FORMS:
                a = make_inputs(form, N, H, W, 1, 9)[0]
                for fn in sides_of(form, u, wr, N):
                    for _ in range(3):
                        fn(a)                          # warm-up: caches, library algorithm choice
                    torch.cuda.synchronize()
                    torch.cuda._sleep(1000)
                    for _ in range(5):
                        fn(a)
                    torch.cuda._sleep(1000)
                    torch.cuda.synchronize()


def summarise_trace(path, out):
    rows = list(csv.DictReader(open(path)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    spins = [i for i, r in enumerate(rows) if "spin" in r["Kernel_Name"].lower() or "sleep" in r["Kernel_Name"].lower()]
    groups = [rows[spins[i] + 1:spins[i + 1]] for i in range(0, len(spins) - 1, 2)]
    labels = [(w, form, side) for w in WORKLOADS for form in FORMS for side in ("new", "separate")]
    doc = json.load(open(out)) if os.path.exists(out) else {"workloads": {}}
    for (w, form, side), rs in zip(labels, groups):
        name, N, H, W = w
        d = doc["workloads"].setdefault(name, {}).setdefault("trace", {}).setdefault(form, {})
        per = {}
        for r in rs:
            per.setdefault(r["Kernel_Name"][:96], []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-3)
        d[side] = {"launches_per_call": len(rs) / 5.0,
                   "kernels_us": {k: float(np.median(v)) for k, v in per.items()},
                   "kernel_sum_us": float(sum(np.median(v) * len(v) for v in per.values()) / 5.0)}
        if side == "new" and form.startswith("fanout"):
            us = [v for k, v in per.items() if "conv3x3_fanout_c128_kernel" in k]
            if us:
                G = int(form[-1])
                med = float(np.median(us[0]))
                nbytes = N * H * W * 128 * 2 * (1 + G) + G * 2 * C3.WPACK_HALVES[128]
                d["conv3x3_fanout_c128_kernel"] = {"median_us": med, "bytes": nbytes, "hbm_share": nbytes / (med * 1e-6) / HBM}
    json.dump(doc, open(out, "w"), indent=1, sort_keys=True)
    print(json.dumps(doc, sort_keys=True))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--out", default=OUT)
    ap.add_argument("--trace", help="add the summary of this rocprofv3 kernel-trace CSV to the JSON file")
    ap.add_argument("--markers", action="store_true", help="the launch-count pass for a kernel trace")
    ap.add_argument("--forms", help="comma-separated subset of the forms to time (a variant library under LGU_LIB_PATH); "
                    "no thresholds are derived from a subset")
    args = ap.parse_args()
    if args.trace:
        return summarise_trace(args.trace, args.out)
    lgu_slam_amd._lib.load()
    lgu_slam_amd.conv1.MIN_FUSED_PIXELS = 0          # the whole forward on its fused kernels at every class
    lgu_slam_amd.gru.MIN_FUSED_CONV_PIXELS = 0
    if args.markers:
        markers()
    if args.reps <= 0:
        return
    forms = args.forms.split(",") if args.forms else list(FORMS)
    workloads = measure(args.reps, forms)
    doc = {"tool": "prof_outstage", "device": torch.cuda.get_device_name(0), "lib": lgu_slam_amd._lib.version(),
           "reps": args.reps, "rotation": ROT, "workloads": workloads}
    if not args.forms:
        doc["min_fanout_pixels"] = threshold(workloads, ("fanout3", "fanout2"))
        doc["min_pair_pixels"] = threshold(workloads, ("pair_h16", "pair_f32"))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(doc, open(args.out, "w"), indent=1, sort_keys=True)
    print(json.dumps(doc, sort_keys=True))


if __name__ == "__main__":
    main()
