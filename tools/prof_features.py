#!/usr/bin/env python3
"""Device-event medians of the feature encoder's fused kernels (lgu_slam_amd.features, csrc/instnorm.hip).  Prints ONE
JSON line and writes it to profiles/features_prof.json (--out; the --forward-only and --trace forms only print).

Kernels — per mode (0..3) and dtype at the three production planes of a 384x512 frame, (32, 192x256), (64, 96x128),
(128, 48x64), with N = 1 and N = 16 frames:
  ms / Bps    the fused launch, and the bytes it moves per second (operands read + result written)
  copy        torch.Tensor.copy_ of the same byte count in the same process: what this memory system gives a plain copy
  torch       the torch composition the launch replaces (F.instance_norm, relu, add, relu)
Consecutive calls rotate over enough disjoint operand sets that no call finds its lines in the 256 MiB Infinity Cache
(N = 16); at N = 1 a call moves at most 9 MB, everything stays cached and the time is the launch: those rows are
launch-bound and are named so.

Whole forward — RefEncoder (the reference's architecture, seeded weights) at (1,1,3,384,512) and (1,16,3,384,512), fp32
and float16 autocast: installed, and the module's own forward (after uninstall: the behaviour without this library's
path), alternated --repeats times; the spread of the medians over the repeats is reported for both.

Accuracy — rms against the float64 CPU forward at the two fixture shapes, installed and own, fp32 and autocast.

Usage: prof_features.py [--reps N] [--repeats N] [--out PATH]
       prof_features.py --forward-only --calls K      (1 + K installed autocast forwards of one frame: the run to trace)
       prof_features.py --trace KERNEL_TRACE_CSV --calls K
            summarise a rocprofv3 --kernel-trace of the --forward-only run: this library's dispatches per forward (must
            be 13, each one workgroup per plane: the resident path) and the kernels between the first and the last of
            them in the last forward, by full name: the convolution library's kernels, torch's half `add` that follows a
            convolution kernel directly (Conv2d adds its bias with it), and anything else (must be none).
"""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import lgu_slam_amd  # noqa: E402
from tests import features_restatement as R  # noqa: E402

F = lgu_slam_amd.features
PLANES = ((32, 192, 256), (64, 96, 128), (128, 48, 64))
CACHE = 256 * 2 ** 20
# kernel names of the convolution library and its helpers (bias, layout, GEMM for the 1x1 convolutions)
CONV_MARKS = ("conv", "igemm", "gemm", "cijk", "winograd", "sp3", "im2col", "miopen", "optensor", "transpose", "gridwise",
              "xdlops", "ck::", "ck_", "batched", "subtensorop")
BIAS_MARK = "CUDAFunctor_add<c10::Half>"      # torch's element-wise add, as Conv2d issues it for the bias


def rotate_ms(fn, nsets, reps, warmup=2):
    """Median device ms per call of fn(k), k cycling over the sets; one timed window is 2 * nsets back-to-back calls
    between two events (kernel time while the queue stays full, the host's issue rate for a launch-bound call)."""
    burst = 2 * nsets
    for k in range(warmup * nsets):
        fn(k % nsets)
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for k in range(burst):
            fn(k % nsets)
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) / burst)
    return float(np.median(ts))


def torch_mode(mode, a, b):
    fn = torch.nn.functional
    if mode == 0:
        return fn.relu(fn.instance_norm(a))
    if mode == 1:
        return fn.relu(b + fn.relu(fn.instance_norm(a)))
    if mode == 2:
        return fn.relu(fn.instance_norm(b) + fn.relu(fn.instance_norm(a)))
    return fn.instance_norm(a)


def run_kernels(reps):
    out = {}
    for dt, dtype in (("h16", torch.float16), ("f32", torch.float32)):
        for C, H, W in PLANES:
            for N in (1, 16):
                one = N * C * H * W * (2 if dt == "h16" else 4)
                nsets = max(3, min(12, math.ceil(2 * CACHE / (3 * one))))
                a = [torch.randn(N, C, H, W, device="cuda").to(dtype) for _ in range(nsets)]
                b = [torch.randn(N, C, H, W, device="cuda").to(dtype) for _ in range(nsets)]
                o = [torch.empty_like(x) for x in a]
                for mode in range(4):
                    nops = 3 if mode in (1, 2) else 2
                    nbytes = nops * one
                    bb = (lambda k: b[k]) if mode in (1, 2) else (lambda k: None)
                    w = {"shape": [N, C, H, W], "bytes": nbytes, "sets": nsets,
                         "launch_bound": bool(nsets * 3 * one < CACHE),
                         "ms": rotate_ms(lambda k: F.instance_norm_relu(a[k], bb(k), norm_residual=mode == 2,
                                                                        relu=mode != 3, out=o[k]), nsets, reps)}
                    if nops == 3:     # the same bytes as a copy: a -> o and the read of b as a second, half-size copy
                        half = a[0].numel() // 2
                        w["copy_ms"] = rotate_ms(lambda k: (o[k].copy_(a[k]), o[(k + 1) % nsets].view(-1)[:half].copy_(
                            b[k].view(-1)[:half])), nsets, reps)
                    else:
                        w["copy_ms"] = rotate_ms(lambda k: o[k].copy_(a[k]), nsets, reps)
                    w["torch_ms"] = rotate_ms(lambda k: torch_mode(mode, a[k], b[k]), nsets, max(3, reps // 2), warmup=1)
                    w["Bps"] = nbytes / (w["ms"] * 1e-3)
                    w["copy_Bps"] = nbytes / (w["copy_ms"] * 1e-3)
                    w["fraction_of_copy"] = w["Bps"] / w["copy_Bps"]
                    w["speedup_vs_torch"] = w["torch_ms"] / w["ms"]
                    out["mode%d_%s_%dx%dx%d_N%d" % (mode, dt, C, H, W, N)] = w
                del a, b, o
                torch.cuda.empty_cache()
    return out


def encoder():
    return R.set_weights(R.RefEncoder(), 1234).eval().cuda()


def forward_ms(m, x, half, reps):
    def fn(_):
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16, enabled=half):
            m(x)
    return rotate_ms(fn, 1, reps)


def run_forward(reps, repeats):
    out = {}
    m = encoder()
    for N in (1, 16):
        x = torch.randn(1, N, 3, 384, 512, device="cuda")
        for half in (True, False):
            inst, own = [], []
            for _ in range(repeats):
                wr = F.install(m)
                inst.append(forward_ms(m, x, half, reps))
                assert wr.fused_calls > 0
                F.uninstall(m)
                own.append(forward_ms(m, x, half, reps))
            w = {"shape": [1, N, 3, 384, 512], "installed_ms": float(np.median(inst)), "own_ms": float(np.median(own)),
                 "installed_repeats_ms": inst, "own_repeats_ms": own,
                 "installed_spread": (max(inst) - min(inst)) / min(inst), "own_spread": (max(own) - min(own)) / min(own)}
            w["speedup"] = w["own_ms"] / w["installed_ms"]
            out["N%d_%s" % (N, "autocast_half" if half else "fp32")] = w
    return out


def run_accuracy():
    out = {}
    for name in sorted(R.CASES):
        m, images = R.make_case(name)
        m64 = R.RefEncoder().double()
        m64.load_state_dict(m.state_dict())
        with torch.no_grad():
            ref = m64.eval()(images.double())
        m, images = m.cuda(), images.cuda()
        for half in (False, True):
            with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16, enabled=half):
                own = m(images)
                F.install(m)
                got = m(images)
                F.uninstall(m)
            r = [float(((t.double().cpu() - ref) ** 2).mean().sqrt()) for t in (got, own)]
            out["%s_%s" % (name, "autocast_half" if half else "fp32")] = {"rms_installed": r[0], "rms_own": r[1],
                                                                         "ratio": r[0] / r[1]}
    return out


def run_forward_only(calls):
    m = encoder()
    wr = F.install(m)
    x = torch.randn(1, 1, 3, 384, 512, device="cuda")
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        for _ in range(calls + 1):
            m(x)
    torch.cuda.synchronize()
    print(json.dumps({"tool": "prof_features --forward-only", "forwards": calls + 1, "fused_calls": wr.fused_calls}))


def summarise_trace(path, calls):
    import csv
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"]))
    names = [r["Kernel_Name"] for r in rows]
    mine = [i for i, k in enumerate(names) if "instnorm_" in k]
    out = {"tool": "prof_features --trace", "forwards": calls + 1, "instnorm_dispatches": len(mine)}
    if mine:
        out["dispatches_per_forward"] = len(mine) / (calls + 1)
        last = mine[-13:]
        out["last_forward"] = [{"kernel": names[i].split("(")[0][-60:], "workgroups": int(rows[i]["Grid_Size_X"]) //
                                int(rows[i]["Workgroup_Size_X"]), "workgroup_size": int(rows[i]["Workgroup_Size_X"]),
                                "us": (int(rows[i]["End_Timestamp"]) - int(rows[i]["Start_Timestamp"])) / 1e3} for i in last]
        out["resident_dispatches_in_last_forward"] = sum("resident" in names[i] for i in last)
        conv, bias, other = {}, {}, {}

        def is_conv(i):
            return any(mk in names[i].lower() for mk in CONV_MARKS)
        for i in range(last[0], last[-1] + 1):
            if i in last:
                continue
            if is_conv(i):
                tgt = conv
            elif BIAS_MARK in names[i] and is_conv(i - 1):
                tgt = bias
            else:
                tgt = other
            tgt[names[i][:240]] = tgt.get(names[i][:240], 0) + 1
        out["convolution_kernels_between"] = conv
        out["bias_adds_after_a_convolution_kernel_between"] = bias
        out["other_kernels_between"] = other
        out["instnorm_us_in_last_forward"] = sum(d["us"] for d in out["last_forward"])
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--forward-only", action="store_true")
    ap.add_argument("--trace")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "features_prof.json"))
    args = ap.parse_args()
    if args.trace:
        return summarise_trace(args.trace, args.calls)
    assert torch.cuda.is_available(), "prof_features.py measures on the GPU"
    lgu_slam_amd._lib.load()
    if args.forward_only:
        return run_forward_only(args.calls)
    res = {"tool": "prof_features", "device": torch.cuda.get_device_name(0), "lib": lgu_slam_amd._lib.version(),
           "reps": args.reps, "repeats": args.repeats,
           "note": "rows with launch_bound = true (N = 1) fit the caches whatever is rotated: their time is the launch, not "
                   "the memory system",
           "forward": run_forward(args.reps, args.repeats), "accuracy": run_accuracy(), "kernels": run_kernels(args.reps)}
    line = json.dumps(res)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
