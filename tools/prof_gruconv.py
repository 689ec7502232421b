#!/usr/bin/env python3
"""Device-event medians of the KAN-bias GRU with its fused 448-channel convolutions (lgu_slam_amd.gru, csrc/gruconv.hip):
three sides in one process on the same tensors, KanBiasGRU(convs=True), KanBiasGRU(convs=False) (the parent's path and
the yardstick) and the module's own autocast forward; and the bare layers, gru_conv_zr against convz + convr + the gates
kernel, two 128-wide PLAIN launches + the gates kernel, and gru_conv_q against convq + the blend kernel.  Writes
profiles/gruconv_prof.json and prints it as ONE JSON line.

Workloads (E x H x W), half: 48 x 48x64 (frontend), 80 x 60x80 (a backend chunk), 1 x 48x64 (MotionFilter).
Method (tools/prof_conv3.py's): every timed call runs on the next of ROT disjoint input sets (cold rotation), the sides
alternate call by call, and a spin kernel ahead of the first event keeps the host's enqueue time out of the window.
Reported per side: median, quartiles and spread = p75 - p25 (ms).  `keep_fused`: convs=True beats convs=False beyond the
two spreads added together.  `min_fused_conv_pixels`: the smallest E*H*W from which every measured class keeps the fused
convolutions, the rule by which lgu_slam_amd.gru.MIN_FUSED_CONV_PIXELS is set (0: every class keeps them).
Shares of the bare kernels: mfma_share = 2 * 4032 * Cout * E*H*W flop / kernel time / 2.5 Pflop/s; hbm_share = (the 448
input channels, the outputs, net / z where read, all once) / kernel time / 8 TB/s, the kernel time from a kernel trace.
Usage: prof_gruconv.py [--reps N] [--out PATH]
       prof_gruconv.py --bare-only --variant NAME [--out profiles/gruconv_variants.json]   (a variant library under
                                                LGU_LIB_PATH: the bare layers only, added under its name)
       prof_gruconv.py --markers --reps 0        (each side once between spin kernels, for a kernel trace)
       prof_gruconv.py --trace KERNEL_TRACE_CSV [--out PATH]
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
from tests import gruconv_restatement as R  # noqa: E402

HBM = 8e12
MFMA_F16 = 2.5e15
ROT = 6
SPIN = 400000
WORKLOADS = (("frontend", 48, 48, 64), ("backend_chunk", 80, 60, 80), ("motion_filter", 1, 48, 64))
SIDES = ("convs_true", "convs_false", "module")
BARE = ("zr_fused", "zr_two_plain", "zr_parent", "q_fused", "q_parent")
OUT = os.path.join(ROOT, "profiles", "gruconv_prof.json")
G = lgu_slam_amd.gru


def stats(ts):
    q = np.percentile(ts, [25, 50, 75])
    return {"median_ms": float(q[1]), "p25_ms": float(q[0]), "p75_ms": float(q[2]), "spread_ms": float(q[2] - q[0]),
            "min_ms": float(np.min(ts))}


def make_sets(E, H, W, count, seed):
    """`count` disjoint input sets: (net, inp, corr, flow) half on the device, plus what the bare layers need.  The
    seeded data of at most 8 edges are made once on the host; a set repeats them over its edges, rolled by its index."""
    base = [t.cuda() for t in R.make_inputs(seed, min(E, 8), H, W)]
    sets = []
    for i in range(count):
        ins = [t.repeat((E + 7) // 8, 1, 1, 1)[:E].roll(i, dims=3).contiguous() for t in base]
        g = torch.Generator().manual_seed(seed + i)
        k = (torch.randn((3, E, 128), generator=g) * 0.5).half().cuda()
        z = torch.rand((1, 128, H, W), generator=g).half().cuda().expand(E, -1, -1, -1).contiguous()
        sets.append({"ins": ins, "k": k, "z": z, "net_inp": torch.cat(ins, 1)})
    return sets


def sides_of(m):
    wt, wf = G.KanBiasGRU(m, convs=True), G.KanBiasGRU(m, convs=False)
    (wzr, bzr), (wq, bq) = wt.conv_packed()
    wz, bz = G.pack_gruconv(m.convz)
    wr_, br_ = G.pack_gruconv(m.convr)

    def zr_parent(s):
        cz, cr = m.convz(s["net_inp"]), m.convr(s["net_inp"])
        return G.kangru_gates_(s["net_inp"], cz.contiguous(), cr.contiguous(), s["k"][0], s["k"][1], s["ins"][0])

    def zr_two_plain(s):
        cz, cr = G.gru_conv3x3(s["ins"], wz, bz), G.gru_conv3x3(s["ins"], wr_, br_)
        return G.kangru_gates_(s["net_inp"], cz, cr, s["k"][0], s["k"][1], s["ins"][0])

    full = {"convs_true": lambda s: wt(*s["ins"]), "convs_false": lambda s: wf(*s["ins"]), "module": lambda s: m(*s["ins"])}
    bare = {"zr_fused": lambda s: G.gru_conv_zr(s["ins"], wzr, bzr, s["k"][0], s["k"][1], s["ins"][0]),
            "zr_two_plain": zr_two_plain, "zr_parent": zr_parent,
            "q_fused": lambda s: G.gru_conv_q(s["ins"], wq, bq, s["k"][2], s["z"], s["ins"][0]),
            "q_parent": lambda s: G.kangru_blend(m.convq(s["net_inp"]).contiguous(), s["k"][2], s["z"], s["ins"][0])}
    return full, bare


def timed(fns, sets, reps, warmup=3):
    """{side: [ms]}: the sides alternate call by call; call k of a side uses input set k % ROT."""
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


def measure(reps, bare_only):
    res = {}
    m = R.make_module(1061).cuda()
    full, bare = sides_of(m)
    for name, E, H, W in WORKLOADS:
        r = {"E": E, "H": H, "W": W, "pixels": E * H * W}
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
            sets = make_sets(E, H, W, ROT, E + H)
            if not bare_only:
                got, base = full["convs_true"](sets[0]), full["convs_false"](sets[0])
                r["bit_identical_to_convs_false"] = float((got == base).double().mean())
                r["max_abs_diff_to_convs_false"] = float((got.float() - base.float()).abs().max())
                ts = timed(full, sets, reps)
                r["forward"] = {k: stats(v) for k, v in ts.items()}
                t, f = r["forward"]["convs_true"], r["forward"]["convs_false"]
                r["speedup_over_convs_false"] = f["median_ms"] / t["median_ms"]
                r["keep_fused"] = bool(t["median_ms"] + t["spread_ms"] + f["spread_ms"] < f["median_ms"])
            ts = timed(bare, sets, reps)
            r["bare"] = {k: stats(v) for k, v in ts.items()}
            del sets
            torch.cuda.empty_cache()
        res[name] = r
    return res


def threshold(workloads):
    classes = sorted((w["pixels"], w["keep_fused"]) for w in workloads.values())
    need = 0
    for i, (_, keep) in enumerate(classes):
        if not keep:
            need = classes[i + 1][0] if i + 1 < len(classes) else 1 << 62
    return need


def markers():
    """Each side of each workload between torch.cuda._sleep spin kernels (for the launch counts and kernel times of --trace)."""
    m = R.make_module(1061).cuda()
    full, bare = sides_of(m)
    for name, E, H, W in WORKLOADS:
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
            s = make_sets(E, H, W, 1, 9)[0]
            for fn in list(full.values()) + list(bare.values()):
                for _ in range(3):
                    fn(s)
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
    labels = [(w, side) for w in WORKLOADS for side in SIDES + BARE]
    doc = json.load(open(out)) if os.path.exists(out) else {"workloads": {}}
    for (w, side), rs in zip(labels, groups):
        name, E, H, W = w
        d = doc["workloads"].setdefault(name, {}).setdefault("trace", {})
        per = {}
        for r in rs:
            per.setdefault(r["Kernel_Name"][:96], []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-3)
        d[side] = {"launches_per_call": len(rs) / 5.0, "kernels_us": {k: float(np.median(v)) for k, v in per.items()},
                   "kernel_sum_us": float(sum(np.median(v) * len(v) for v in per.values()) / 5.0)}
        if side in ("zr_fused", "q_fused"):
            us = [v for k, v in per.items() if "gruconv3x3_c448_kernel" in k]
            if us:
                cout, extra = (256, 3 * 128) if side == "zr_fused" else (128, 3 * 128)   # outputs + net (+ z) per pixel
                med = float(np.median(us[0]))
                nbytes = 2 * E * H * W * (448 + extra) + 2 * G.GRUCONV_WPACK_HALVES[cout]
                d[side]["gruconv3x3_c448_kernel"] = {"median_us": med, "bytes": nbytes, "hbm_share": nbytes / (med * 1e-6) / HBM,
                                                     "mfma_share": 2.0 * 4032 * cout * E * H * W / (med * 1e-6) / MFMA_F16}
    json.dump(doc, open(out, "w"), indent=1, sort_keys=True)
    print(json.dumps(doc, sort_keys=True))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--out", default=OUT)
    ap.add_argument("--trace", help="add the summary of this rocprofv3 kernel-trace CSV to the JSON file")
    ap.add_argument("--markers", action="store_true", help="the launch-count pass for a kernel trace")
    ap.add_argument("--bare-only", action="store_true", help="time the bare layers only")
    ap.add_argument("--variant", help="store the result under this name in a variants file (with --bare-only)")
    args = ap.parse_args()
    if args.trace:
        return summarise_trace(args.trace, args.out)
    lgu_slam_amd._lib.load()
    G.MIN_FUSED_CONV_PIXELS = 0          # measure the fused path at every class; the rule is applied afterwards
    if args.markers:
        markers()
    if args.reps <= 0:
        return
    workloads = measure(args.reps, args.bare_only)
    doc = {"tool": "prof_gruconv", "device": torch.cuda.get_device_name(0), "lib": lgu_slam_amd._lib.version(),
           "reps": args.reps, "rotation": ROT, "workloads": workloads}
    if not args.bare_only:
        doc["min_fused_conv_pixels"] = threshold(workloads)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    if args.variant:
        allv = json.load(open(args.out)) if os.path.exists(args.out) else {"tool": "tools/prof_gruconv.py --bare-only --variant NAME "
                                                                            "under LGU_LIB_PATH, one process per build", "variants": {}}
        allv["variants"][args.variant] = {"lib": doc["lib"], "workloads": {
            w: {k: {"median_ms": v["median_ms"], "spread_ms": v["spread_ms"]} for k, v in r["bare"].items()}
            for w, r in workloads.items()}}
        doc = allv
    json.dump(doc, open(args.out, "w"), indent=1, sort_keys=True)
    print(json.dumps(doc, sort_keys=True))


if __name__ == "__main__":
    main()
