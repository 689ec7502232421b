#!/usr/bin/env python3
"""Device-event medians of lgu_slam_amd.aggregate (csrc/aggregate.hip), cold and warm, against torch compositions of
the same math on the same GPU.  Prints ONE JSON line.

Workloads:
  seg_frontend   scatter_mean, GraphAgg frontend: 48 edges at 48x64 over 12 frames, half, (1,48,128,48,64)
  seg_c5         scatter_mean, one config-5 chunk: 80 edges at 60x80 over 8 frames, half, (1,80,128,60,80)
  ups_12_h16w    upsample_disps_, 12 frames at 48x64, half mask, half weights (FactorGraph.update)
  ups_12_f32w    upsample_disps_, 12 frames at 48x64, half mask under autocast, float weights (update_lowmem)
  ups_c5_f32w    upsample_disps_, 8 frames at 60x80, half mask under autocast

Torch compositions: for scatter_mean what torch_scatter computes (zeros + scatter_add_ + a count by scatter_add_ +
clamp + true_divide_, in the input dtype); for the upsampler the reference's DepthVideo.upsample (softmax, unfold,
product, sum, permute, reshape, then index_put into disps_up).
Algorithmic bytes: segment mean outer*(n + M)*inner*sizeof + 8n; upsampling U*ht*wd*(576*sizeof(mask) + 4 + 64*4).
fraction = bytes / time / 8 TB/s.  Cold: a 512 MiB buffer is rewritten before every timed launch (outside the events);
warm: the same launches without it (the window then also holds the host side of the call).
Usage: prof_aggregate.py [--reps N] [--skip-torch]
       prof_aggregate.py --trace KERNEL_TRACE_CSV   (summarise a rocprofv3 --kernel-trace of this tool: per workload, the
                                                     median kernel duration of its cold dispatches, found by grid size)
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import lgu_slam_amd  # noqa: E402

A = lgu_slam_amd.aggregate
HBM = 8e12
FLUSH_FLOATS = 128 * 1024 * 1024
XV = int(os.environ.get("LGU_PROF_CVX_XV", "1"))  # coarse pixels per upsampling thread (aggregate.hip LGU_CVX_XV)

# name, kind, (E or U, N, ht, wd), autocast
WORKLOADS = (("seg_frontend", "seg", (48, 12, 48, 64), None), ("seg_c5", "seg", (80, 8, 60, 80), None),
             ("ups_12_h16w", "ups", (12, 12, 48, 64), False), ("ups_12_f32w", "ups", (12, 12, 48, 64), True),
             ("ups_c5_f32w", "ups", (8, 8, 60, 80), True))


def time_ms(fn, reps, warmup=3, flush=None):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        if flush is not None:
            flush.add_(1.0)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts))


def seg_bytes(E, N, ht, wd):
    inner = 128 * ht * wd
    return (E + N) * inner * 2 + 8 * E


def ups_bytes(U, ht, wd):
    return U * ht * wd * (576 * 2 + 4 + 64 * 4)


def torch_scatter_mean(src, index, dim, M):
    shape = list(src.shape)
    shape[dim] = M
    view = [1] * src.dim()
    view[dim] = -1
    out = torch.zeros(shape, dtype=src.dtype, device=src.device).scatter_add_(dim, index.view(view).expand_as(src), src)
    cnt = torch.zeros(M, dtype=src.dtype, device=src.device).scatter_add_(0, index, torch.ones_like(index, dtype=src.dtype))
    return out.true_divide_(cnt.clamp_(1).view(view))


def torch_upsample_(disps_up, disps, ix, mask):
    """DepthVideo.upsample's work as torch GPU ops: gather the rows, softmax over the 9 neighbours (in the mask's dtype,
    as torch picks it), 3x3 unfold with zero padding, product, sum over the neighbours, sub-pixels to their fine
    positions, index_put into disps_up (the composition of tests/test_aggregate.py, plus the gather and the put)."""
    data = disps[ix]
    B, ht, wd = data.shape
    w = torch.softmax(mask.view(B, 9, 64, ht, wd), dim=1)
    nb = torch.nn.functional.unfold(data[:, None], [3, 3], padding=1).view(B, 9, 1, ht, wd)
    up = (w * nb).sum(1).view(B, 8, 8, ht, wd)
    disps_up[ix] = up.permute(0, 3, 1, 4, 2).reshape(B, 8 * ht, 8 * wd)


def inputs(kind, sizes, seed=0):
    g = torch.Generator().manual_seed(seed)
    if kind == "seg":
        E, N, ht, wd = sizes
        ii = torch.cat([torch.arange(N), torch.randint(0, N, (E - N,), generator=g)])
        _, ix = torch.unique(ii, return_inverse=True)
        src = torch.randn(1, E, 128, ht, wd, generator=g).half()
        return src.cuda(), ix.cuda()
    U, N, ht, wd = sizes
    disps = (0.05 + torch.rand(2 * N, ht, wd, generator=g)).cuda()
    ix = torch.sort(torch.randperm(2 * N, generator=g)[:U])[0].cuda()
    mask = (3 * torch.randn(1, U, 576, ht, wd, generator=g)).half().cuda()
    up = torch.zeros(2 * N, 8 * ht, 8 * wd, device="cuda")
    return up, disps, ix, mask


def _is_flush(r):
    return "CUDAFunctorOnSelf_add" in r["Kernel_Name"] and int(r["Grid_Size_X"]) == FLUSH_FLOATS // 4


def summarise_trace(path):
    """Cold dispatches only: those launched right after the 512 MiB flush (the previous dispatch on the queue is the
    flush's add_).  Warm-ups and the warm loop are left out, so the medians are HBM-served launches."""
    import csv
    out = {}
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"]))
    rows = [r for p, r in zip(rows, rows[1:]) if _is_flush(p)]
    for name, kind, sizes, ac in WORKLOADS:
        if kind == "seg":
            E, N, ht, wd = sizes
            chunks = (128 * ht * wd + 2047) // 2048
            grid = (chunks * N * 256, 1)
            kern, nbytes = "segment_mean_kernelIDF16_Lb1E", seg_bytes(*sizes)       # <_Float16, true>, mangled
        else:
            U, N, ht, wd = sizes
            total = U * ht * 8 * (wd // XV)
            grid = ((total + 255) // 256 * 256, 1)
            kern = "cvx_upsample_kernelIDF16_Lb%dELi%dE" % (0 if ac else 1, XV)  # <_Float16, half weights, XV>
            nbytes = ups_bytes(U, ht, wd)
        us = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows
              if kern in r["Kernel_Name"] and (int(r["Grid_Size_X"]), int(r["Grid_Size_Y"])) == grid]
        med = float(np.median(us)) if us else None
        out[name] = {"kernel": kern, "cold_dispatches": len(us), "kernel_us_median": med,
                     "kernel_us_min": min(us) if us else None, "kernel_us_max": max(us) if us else None,
                     "bytes": nbytes, "frac_8TBps": (nbytes / HBM * 1e6 / med) if med else None}
    print(json.dumps({"tool": "prof_aggregate --trace", "dispatches": "cold only (each right after the flush)",
                      "workloads": out}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--skip-torch", action="store_true")
    ap.add_argument("--trace", help="summarise this rocprofv3 kernel-trace CSV instead of measuring")
    args = ap.parse_args()
    if args.trace:
        return summarise_trace(args.trace)
    assert torch.cuda.is_available(), "prof_aggregate.py measures on the GPU"
    lgu_slam_amd._lib.load()
    res = {"tool": "prof_aggregate", "device": torch.cuda.get_device_name(0), "lib": lgu_slam_amd._lib.version(),
           "hbm_peak_Bps": HBM, "workloads": {}}
    flush = torch.zeros(FLUSH_FLOATS, device="cuda")   # 512 MiB
    R_ = args.reps
    for name, kind, sizes, ac in WORKLOADS:
        w = {"sizes": list(sizes)}
        if kind == "seg":
            src, ix = inputs(kind, sizes)
            N = sizes[1]
            nbytes = seg_bytes(*sizes)
            fn = lambda: A.scatter_mean(src, ix, dim=1, dim_size=N)  # noqa: E731
            tfn = lambda: torch_scatter_mean(src, ix, 1, N)  # noqa: E731
            ctx = torch.autocast("cuda", enabled=False)
        else:
            up, disps, ix, mask = inputs(kind, sizes)
            nbytes = ups_bytes(sizes[0], sizes[2], sizes[3])
            fn = lambda: A.upsample_disps_(up, disps, ix, mask)  # noqa: E731
            up_t = up.clone()
            tfn = lambda: torch_upsample_(up_t, disps, ix, mask)  # noqa: E731
            ctx = torch.autocast("cuda", enabled=ac)
        w["bytes"] = nbytes
        with ctx:
            w["ms_warm"] = time_ms(fn, R_)
            w["ms_cold"] = time_ms(fn, R_, flush=flush)
            w["floor_ms"] = 1e3 * nbytes / HBM
            w["frac_8TBps_warm"] = w["floor_ms"] / w["ms_warm"]
            w["frac_8TBps_cold"] = w["floor_ms"] / w["ms_cold"]
            if not args.skip_torch:
                w["torch_ms_warm"] = time_ms(tfn, max(5, R_ // 5), warmup=2)
                w["torch_ms_cold"] = time_ms(tfn, max(5, R_ // 5), warmup=1, flush=flush)
                w["speedup_vs_torch_warm"] = w["torch_ms_warm"] / w["ms_warm"]
                w["speedup_vs_torch_cold"] = w["torch_ms_cold"] / w["ms_cold"]
                if kind == "seg":
                    a, b = fn(), tfn()
                else:
                    fn()
                    tfn()
                    a, b = up[ix], up_t[ix]
                w["vs_torch_max_abs"] = float((a.double() - b.double()).abs().max())
                del a, b
        torch.cuda.empty_cache()
        res["workloads"][name] = w
    print(json.dumps(res))


if __name__ == "__main__":
    main()
