#!/usr/bin/env python3
"""Device-event medians of the fused 3x3 convolution with 128 input channels (lgu_slam_amd.conv3, csrc/conv3.hip) against
the module's own autocast forward (the path without `conv3.install`), for the bare layer at both Cout and for whole
corr_encoder, delta, weight, flow_encoder and GraphAgg-shaped calls, with the same seeded weights on the same GPU.  Writes
profiles/conv3_prof.json and prints it as ONE JSON line.

Workloads (N x H x W): 48 x 48x64 (frontend), 80 x 60x80 (a backend chunk), 1 x 48x64 (MotionFilter).
Method (tools/prof_flowenc.py's): every timed call runs on the next of ROT disjoint input sets (cold rotation: ROT inputs
of the large workloads exceed the 256 MiB last-level cache), the two sides alternate call by call in one process, and a
spin kernel ahead of the first event keeps the host's enqueue time out of the window.  Reported per side: median,
quartiles and spread = p75 - p25 (ms).  `keep_fused`: the fused median beats the module's beyond the two spreads.
`min_fused_pixels`: per Cout, the smallest N*H*W from which every measured class of the bare layer (fp32 and half input)
keeps the fused path, the rule by which lgu_slam_amd.conv3.MIN_FUSED_PIXELS is set (0: every class keeps it).
The flow_encoder forms have `flow.install` on both sides: the fused side adds a Conv3 on its [2].
Algorithmic bytes of the kernel: the input once, the output once, the pack once; hbm_share = those bytes / kernel time /
8 TB/s and mfma_share = 2 * 1152 * Cout * N*H*W flop / kernel time / 2.5 Pflop/s, the kernel time from a kernel trace.
Usage: prof_conv3.py [--reps N] [--out PATH]
       prof_conv3.py --markers --reps 0        (each form once between spin kernels, for a kernel trace)
       prof_conv3.py --trace KERNEL_TRACE_CSV [--out PATH]   (adds kernel medians, shares and launch counts of a
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
from tests import flowenc_restatement as RF  # noqa: E402

HBM = 8e12
MFMA_F16 = 2.5e15
ROT = 8
SPIN = 400000
WORKLOADS = (("frontend", 48, 48, 64), ("backend_chunk", 80, 60, 80), ("motion_filter", 1, 48, 64))
# form -> (Cout of the fused layer, input: channels and dtype)
FORMS = {"bare128_f32": (128, 128, torch.float32), "bare128_h16": (128, 128, torch.float16),
         "bare64_f32": (64, 128, torch.float32), "bare64_h16": (64, 128, torch.float16),
         "corr_encoder": (128, R.COR_PLANES, torch.float32), "delta": (128, 128, torch.float32),
         "weight": (128, 128, torch.float32), "flow_encoder": (64, 4, torch.float32), "agg": (128, 128, torch.float32)}
OUT = os.path.join(ROOT, "profiles", "conv3_prof.json")
C3 = lgu_slam_amd.conv3


def kernel_bytes(N, H, W, cout, x_bytes):
    return N * H * W * (128 * x_bytes + cout * 2) + 2 * C3.WPACK_HALVES[cout]


def stats(ts):
    q = np.percentile(ts, [25, 50, 75])
    return {"median_ms": float(q[1]), "p25_ms": float(q[0]), "p75_ms": float(q[2]), "spread_ms": float(q[2] - q[0]),
            "min_ms": float(np.min(ts))}


def sides_of(form, u, twin):
    """(fused, module): callables of one input tensor.  `u` and `twin` are two Updates with the same weights; conv3 (and,
    for flow_encoder, flow) is installed on `twin` only where the form says so."""
    if form.startswith("bare"):
        conv = u.agg.conv1 if FORMS[form][0] == 128 else u.flow_encoder[2]
        wr = C3.Conv3(conv, relu=True)
        return wr, (lambda x: torch.relu_(conv(x)))
    if form == "agg":
        wr1, wr2 = C3.Conv3(twin.agg.conv1), C3.Conv3(twin.agg.conv2)

        def fused(x):
            net = torch.relu_(wr1(x)).mean(dim=0, keepdim=True)
            return torch.relu_(wr2(net))
        return fused, u.agg
    if form == "flow_encoder":
        fe, fe_twin = lgu_slam_amd.flow.FlowEncoder(u.flow_encoder), lgu_slam_amd.flow.FlowEncoder(twin.flow_encoder)
        C3.install(twin.flow_encoder[2])
        return fe_twin, fe
    return C3.Conv3Stack(getattr(twin, form)), getattr(u, form)


def make_inputs(form, N, H, W, count, seed):
    _, ch, dtype = FORMS[form]
    if form == "flow_encoder":
        return [RF.make_input(seed + i, N, H, W).cuda() for i in range(count)]
    g = torch.Generator().manual_seed(seed)
    xs = []
    for _ in range(count):
        x = torch.randn((N, ch, H, W), generator=g) * 2.0
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


def parity(N, H, W):
    """The bare layers at one image of the workload's frame size against the float64 restatement."""
    res = {}
    for cout in (64, 128):
        m = R.make_conv(40 + cout, cout)
        x = R.make_input(9, 1, H, W)
        s64, S, want = R.conv3(x, m.weight, m.bias, True)
        bound, ref = R.allowance(s64, S, R.TERMS), torch.relu(s64)
        mc = m.cuda()
        got = C3.Conv3(mc, relu=True)(x.cuda())
        own = torch.relu(mc(x.cuda()))
        res["cout%d" % cout] = {"bit_identical_to_module": float((got == own).double().mean()),
                                "bit_identical_to_restatement": float((got.cpu() == want).double().mean()),
                                "fused_worst_error_in_bounds": float(((got.cpu().double() - ref).abs() / bound).max()),
                                "module_worst_error_in_bounds": float(((own.cpu().double() - ref).abs() / bound).max())}
    return res


def measure(reps, forms):
    res = {}
    u, twin = R.make_update(41).cuda(), R.make_update(41).cuda()
    for name, N, H, W in WORKLOADS:
        r = {"N": N, "H": H, "W": W, "pixels": N * H * W, "forms": {}}
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
            r["parity"] = parity(N, H, W)
            for form in forms:
                fused, module = sides_of(form, u, twin)
                xs = make_inputs(form, N, H, W, ROT, N + H)
                ts = timed({"fused": fused, "module": module}, xs, reps)
                del xs
                torch.cuda.empty_cache()
                f, o = stats(ts["fused"]), stats(ts["module"])
                r["forms"][form] = {"fused": f, "module": o, "speedup": o["median_ms"] / f["median_ms"],
                                    "keep_fused": bool(f["median_ms"] + f["spread_ms"] < o["median_ms"] - o["spread_ms"])}
        C3.uninstall(twin.flow_encoder[2])
        res[name] = r
    return res


def thresholds(workloads):
    """Per Cout: 0 if every class of the bare layer keeps the fused path, else the pixel count of the smallest class from
    which all larger ones keep it (1 << 62: none does)."""
    out = {}
    for cout in (64, 128):
        classes = sorted((w["pixels"], all(w["forms"]["bare%d_%s" % (cout, d)]["keep_fused"] for d in ("f32", "h16")))
                         for w in workloads.values())
        need = 0
        for i, (pixels, keep) in enumerate(classes):
            if not keep:
                need = classes[i + 1][0] if i + 1 < len(classes) else 1 << 62
        out[str(cout)] = need
    return out


def markers():
    """Each side of each form of each workload between torch.cuda._sleep spin kernels (for the launch count in --trace)."""
    u, twin = R.make_update(41).cuda(), R.make_update(41).cuda()
    for name, N, H, W in WORKLOADS:
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
            for form in FORMS:
                x = make_inputs(form, N, H, W, 1, 9)[0]
                for fn in sides_of(form, u, twin):
                    for _ in range(3):
                        fn(x)                          # warm-up: caches, library algorithm choice
                    torch.cuda.synchronize()
                    torch.cuda._sleep(1000)
                    for _ in range(5):
                        fn(x)
                    torch.cuda._sleep(1000)
                    torch.cuda.synchronize()
        C3.uninstall(twin.flow_encoder[2])


def summarise_trace(path, out):
    rows = list(csv.DictReader(open(path)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    spins = [i for i, r in enumerate(rows) if "spin" in r["Kernel_Name"].lower() or "sleep" in r["Kernel_Name"].lower()]
    groups = [rows[spins[i] + 1:spins[i + 1]] for i in range(0, len(spins) - 1, 2)]
    labels = [(w, form, side) for w in WORKLOADS for form in FORMS for side in ("fused", "module")]
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
        if side == "fused" and form.startswith("bare"):
            us = [v for k, v in per.items() if "conv3x3_c128_kernel" in k]
            if us:
                cout, _, dtype = FORMS[form]
                med = float(np.median(us[0]))
                nbytes = kernel_bytes(N, H, W, cout, 4 if dtype == torch.float32 else 2)
                d["conv3x3_c128_kernel"] = {"median_us": med, "bytes": nbytes, "hbm_share": nbytes / (med * 1e-6) / HBM,
                                            "mfma_share": 2.0 * 1152 * cout * N * H * W / (med * 1e-6) / MFMA_F16}
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
    C3.MIN_FUSED_PIXELS = {64: 0, 128: 0}          # measure the fused path at every class; the rule is applied afterwards
    if args.markers:
        markers()
    if args.reps <= 0:
        return
    forms = args.forms.split(",") if args.forms else list(FORMS)
    workloads = measure(args.reps, forms)
    doc = {"tool": "prof_conv3", "device": torch.cuda.get_device_name(0), "lib": lgu_slam_amd._lib.version(),
           "reps": args.reps, "rotation": ROT, "workloads": workloads}
    if not args.forms:
        doc["min_fused_pixels"] = thresholds(workloads)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(doc, open(args.out, "w"), indent=1, sort_keys=True)
    print(json.dumps(doc, sort_keys=True))


if __name__ == "__main__":
    main()
