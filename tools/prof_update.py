#!/usr/bin/env python3
"""Device-event medians of corr_encoder[0] on csrc/conv1.hip (lgu_slam_amd.conv1) and of the whole update operator
(lgu_slam_amd.update) against the paths they replace, with the same seeded weights on the same GPU.  Writes
profiles/update_prof.json and prints it as ONE JSON line.

Comparisons:
  (a) layer:   conv1x1(relu=True) on the planar fp32 tensor the default lookup writes against corr_encoder[:2]
               (Conv2d(196, 128, 1) + ReLU) under float16 autocast.  Shape classes (edges x ht x wd): 48 x 48x64, 80 x 60x80,
               1 x 48x64 and 20 x 48x64 (DESIGN.md section 3.6's row).
  (b) forward: the whole UpdateModule.forward with ii given, half net / inp, fp32 corr / flow, three ways: the module's own
               autocast forward; every per-site install (flow, conv3.install_update, heads.install_update,
               gru.install(convs=True), upmask.install), the best before the operator; the same plus
               conv1.install(corr_encoder[0]), which separates the new layer's share from the wiring's;
               update.install(gru_convs=True).  Classes: 48 x 48x64 and 80 x 60x80.  The operator's outputs are compared at
               the timed sizes with those of the per-site side that has conv1 installed (without it corr_encoder[0] is the
               library's convolution and every value behind it has other bits): everything but `weight` bit for bit,
               `weight` (whose Sigmoid moves into the head's launch) within twice the heads restatement's sigmoid
               allowance, once for either side.
Method (tools/prof_upmask.py's): every timed call runs on the next of ROT disjoint seeded input sets (cold rotation), every
shape is warmed up, the sides alternate call by call in one process, and a spin kernel ahead of the first event keeps the
host's enqueue time out of the window.  Reported per side: median, quartiles and spread = p75 - p25 (ms).  `keep_fused`:
the fused median plus its spread is below the baseline median minus its spread.  `min_fused_pixels`: the smallest
edges*ht*wd from which every measured class keeps the fused LAYER, the rule by which lgu_slam_amd.conv1.MIN_FUSED_PIXELS is
set (0: every class keeps it).
Floor of the layer at HBM_RATE = 8 TB/s, the HBM bound: x read once (4 * 196 B per pixel) plus 256 B per pixel written;
floor_fraction = floor / kernel time, the kernel time from a kernel trace.
Usage: prof_update.py [--reps N] [--out PATH]
       prof_update.py --markers --reps 0        (each side once between spin kernels, for a kernel trace)
       prof_update.py --trace KERNEL_TRACE_CSV [--out PATH]   (adds kernel medians, the floor fraction and launch counts of a
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
from tests import update_restatement as RU  # noqa: E402

HBM_RATE = 8e12
ROT = 8
SPIN = 400000
CIN = 196
LAYER_CLASSES = (("edges48_48x64", 48, 48, 64), ("edges80_60x80", 80, 60, 80), ("frame1_48x64", 1, 48, 64),
                 ("edges20_48x64", 20, 48, 64))
FORWARD_CLASSES = (("edges48_48x64", 48, 48, 64), ("edges80_60x80", 80, 60, 80))
FORWARD_SIDES = ("module", "per_site", "per_site_conv1", "operator")
OUT = os.path.join(ROOT, "profiles", "update_prof.json")
C1 = lgu_slam_amd.conv1
U24 = 2.0 ** -24


def stats(ts):
    q = np.percentile(ts, [25, 50, 75])
    return {"median_ms": float(q[1]), "p25_ms": float(q[0]), "p75_ms": float(q[2]), "spread_ms": float(q[2] - q[0]),
            "min_ms": float(np.min(ts))}


def keep(f, o):
    return bool(f["median_ms"] + f["spread_ms"] < o["median_ms"] - o["spread_ms"])


def timed(fns, sets, reps, warmup=3):
    """{side: [ms]}: the sides alternate call by call; call k of a side uses input set k % len(sets)."""
    ts = {k: [] for k in fns}
    for k in range(warmup + reps):
        for name, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda._sleep(SPIN)
            a.record()
            fn(sets[k % len(sets)])
            b.record()
            b.synchronize()
            if k >= warmup:
                ts[name].append(a.elapsed_time(b))
    return ts


def _gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def layer_inputs(E, H, W, count, seed):
    """Planar fp32 correlation features: normals of scale 2 with about a third exact zeros."""
    g = _gen(seed)
    sets = []
    for _ in range(count):
        x = torch.randn((E, CIN, H, W), generator=g, device="cuda") * 2.0
        x[torch.rand((E, CIN, H, W), generator=g, device="cuda") < 0.3] = 0.0
        sets.append(x)
    return sets


def layer_sides():
    """(fused, baseline) of one input: conv1x1(relu=True) and corr_encoder[:2] of a twin with the same weights."""
    u = RU.make_update(61).cuda()
    conv = u.corr_encoder[0]
    wpack, bias_h = C1.pack_conv1(conv.weight, conv.bias)
    head = u.corr_encoder[:2]
    return (lambda x: C1.conv1x1(x, wpack, bias_h, relu=True)), (lambda x: head(x))


def forward_inputs(E, H, W, count, seed):
    g = _gen(seed)
    sets = []
    for _ in range(count):
        net = (torch.randn((1, E, 128, H, W), generator=g, device="cuda") * 0.4).clamp(-0.95, 0.95).half()
        inp = torch.randn((1, E, 128, H, W), generator=g, device="cuda").clamp_min(0).half()
        corr = torch.randn((1, E, CIN, H, W), generator=g, device="cuda") * 2.0
        flow = torch.randn((1, E, 4, H, W), generator=g, device="cuda") * 3.0
        ii = torch.randint(0, max(E // 4, 1), (E,), generator=g, device="cuda")
        sets.append((net, inp, corr, flow, ii))
    return sets


def forward_sides():
    """{side: callable of one input set} on three modules with the same weights."""
    L = lgu_slam_amd
    own, site, site1, op = (RU.make_update(61).cuda() for _ in range(4))
    for m in (site, site1):
        L.flow.install(m.flow_encoder)
        L.conv3.install_update(m)
        L.heads.install_update(m)
        L.gru.install(m.gru, convs=True)
        L.upmask.install(m.agg.upmask)
    L.conv1.install(site1.corr_encoder[0])
    wrapper = L.update.install(op, gru_convs=True)
    return {"module": lambda s: own(*s), "per_site": lambda s: site(*s), "per_site_conv1": lambda s: site1(*s),
            "operator": lambda s: op(*s)}, wrapper


def compare(got, want):
    """The operator's outputs against those of the per-site side with conv1 installed."""
    names = ("net", "delta", "weight", "eta", "upmask")
    res = {}
    for name, a, b in zip(names, got, want):
        same = a.shape == b.shape and a.dtype == b.dtype and bool(torch.equal(a, b))
        res[name] = {"bit_identical": same, "max_abs_diff": float((a.double() - b.double()).abs().max())}
    w = want[2].double()
    allow = 2.0 * (2.0 ** -11 * w + 4 * U24 * w + 2.0 ** -25)
    res["weight"]["within_sigmoid_allowance"] = bool(((got[2].double() - w).abs() <= allow).all())
    res["ok"] = all(res[n]["bit_identical"] for n in names if n != "weight") and res["weight"]["within_sigmoid_allowance"]
    return res


def measure(reps):
    layer, forward = {}, {}
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        fused, base = layer_sides()
        for name, E, H, W in LAYER_CLASSES:
            sets = layer_inputs(E, H, W, ROT, E + H)
            got, own = fused(sets[0]), base(sets[0])
            assert got.dtype == own.dtype and got.shape == own.shape
            ts = timed({"fused": fused, "baseline": base}, sets, reps)
            f, o = stats(ts["fused"]), stats(ts["baseline"])
            layer[name] = {"edges": E, "H": H, "W": W, "pixels": E * H * W, "fused": f, "baseline": o,
                           "speedup": o["median_ms"] / f["median_ms"], "keep_fused": keep(f, o),
                           "max_abs_diff_to_baseline": float((got.double() - own.double()).abs().max())}
            del sets, got, own
            torch.cuda.empty_cache()
            print("layer %s done" % name, file=sys.stderr, flush=True)
        sides, wrapper = forward_sides()
        for name, E, H, W in FORWARD_CLASSES:
            sets = forward_inputs(E, H, W, ROT, E + W)
            outs = {k: fn(sets[0]) for k, fn in sides.items()}
            assert wrapper.module_calls == 0
            r = {"edges": E, "H": H, "W": W, "pixels": E * H * W, "operator_vs_per_site_conv1": compare(outs["operator"], outs["per_site_conv1"]),
                 "max_abs_diff_operator_to_per_site": [float((a.double() - b.double()).abs().max())
                                                       for a, b in zip(outs["operator"], outs["per_site"])],
                 "max_abs_diff_operator_to_module": [float((a.double() - b.double()).abs().max())
                                                     for a, b in zip(outs["operator"], outs["module"])]}
            del outs
            ts = timed(sides, sets, reps)
            for k in FORWARD_SIDES:
                r[k] = stats(ts[k])
            r["operator_beats_per_site"] = keep(r["operator"], r["per_site"])
            r["operator_beats_module"] = keep(r["operator"], r["module"])
            forward[name] = r
            print("forward %s done" % name, file=sys.stderr, flush=True)
            del sets
            torch.cuda.empty_cache()
    return layer, forward


def threshold(layer):
    """0 if every class keeps the fused layer, else the pixel count of the smallest class from which all larger ones keep
    it (1 << 62: none does)."""
    classes = sorted((w["pixels"], w["keep_fused"]) for w in layer.values())
    need = 0
    for i, (pixels, kept) in enumerate(classes):
        if not kept:
            need = classes[i + 1][0] if i + 1 < len(classes) else 1 << 62
    return need


def labels():
    return [("layer", c, side) for c in LAYER_CLASSES for side in ("fused", "baseline")] + \
           [("forward", c, side) for c in FORWARD_CLASSES for side in FORWARD_SIDES]


def markers():
    """Each side of each class between torch.cuda._sleep spin kernels (for the kernel times and launch counts of --trace)."""
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        lsides = dict(zip(("fused", "baseline"), layer_sides()))
        fsides, _ = forward_sides()
        for kind, (name, E, H, W), side in labels():
            s = layer_inputs(E, H, W, 1, 9)[0] if kind == "layer" else forward_inputs(E, H, W, 1, 9)[0]
            fn = lsides[side] if kind == "layer" else fsides[side]
            for _ in range(3):
                fn(s)                          # warm-up: caches, library algorithm choice
            torch.cuda.synchronize()
            torch.cuda._sleep(1000)
            for _ in range(5):
                fn(s)
            torch.cuda._sleep(1000)
            torch.cuda.synchronize()
            del s
            torch.cuda.empty_cache()


def summarise_trace(path, out):
    rows = list(csv.DictReader(open(path)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    spins = [i for i, r in enumerate(rows) if "spin" in r["Kernel_Name"].lower() or "sleep" in r["Kernel_Name"].lower()]
    groups = [rows[spins[i] + 1:spins[i + 1]] for i in range(0, len(spins) - 1, 2)]
    doc = json.load(open(out)) if os.path.exists(out) else {}
    for (kind, (name, E, H, W), side), rs in zip(labels(), groups):
        d = doc.setdefault(kind, {}).setdefault(name, {}).setdefault("trace", {})
        per = {}
        for r in rs:
            per.setdefault(r["Kernel_Name"][:96], []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-3)
        d[side] = {"launches_per_call": len(rs) / 5.0, "kernel_sum_us": float(sum(sum(v) for v in per.values()) / 5.0)}
        if kind == "layer":
            d[side]["kernels_us"] = {k: float(np.median(v)) for k, v in per.items()}
        if kind == "layer" and side == "fused":
            us = [v for k, v in per.items() if "conv1x1_o128_kernel" in k]
            if us:
                med = float(np.median(us[0]))
                floor = E * H * W * (4 * CIN + 256) / HBM_RATE * 1e6
                d["conv1x1_kernel"] = {"median_us": med, "floor_us": floor, "floor_fraction": floor / med}
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
    C1.MIN_FUSED_PIXELS = 0          # measure the fused path at every class; the rule is applied afterwards
    if args.markers:
        markers()
    if args.reps <= 0:
        return
    layer, forward = measure(args.reps)
    doc = {"tool": "prof_update", "device": torch.cuda.get_device_name(0), "lib": lgu_slam_amd._lib.version(),
           "reps": args.reps, "rotation": ROT, "hbm_rate": HBM_RATE, "layer": layer, "forward": forward,
           "min_fused_pixels": threshold(layer)}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(doc, open(args.out, "w"), indent=1, sort_keys=True)
    print(json.dumps(doc, sort_keys=True))


if __name__ == "__main__":
    main()
