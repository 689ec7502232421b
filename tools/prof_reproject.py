#!/usr/bin/env python3
"""Device-event medians of lgu_slam_amd.geom.motion_features / projective_transform (csrc/reproject.hip) on the
factor-graph sizes, cold and warm, against a torch composition of the same math on the same GPU.  Prints ONE JSON line.

Workloads (BASELINE configs):
  motn_c5   motion_features, 1970 edges at 60x80 (config 5: the backend's update_lowmem)
  motn_c2   motion_features, 20 edges at 48x64 (config 2: a frontend window)
  motn_c3   motion_features, 40 edges at 48x64, a quarter of them stereo edges ii == jj (config 3)
  jac_c5    projective_transform(jacobian=True), 1970 edges at 60x80 (the training-side BA's call)

Torch composition: what geom/projective_ops.py:projective_transform + the motion lines of FactorGraph.update compute,
written as torch GPU ops on batched quaternion tensors (no lietorch): G_ij = G_j * G_i^-1 as quaternion products, the
stereo override, the homogeneous point cloud, the action, the projection, cat / permute / clamp, and with jacobian the
stacked Jp / Ja, matmul and the adjoint-transpose.

Cold: a 512 MiB buffer is rewritten before every timed launch (outside the events), so inputs and outputs start out of
the L2 and the 256 MiB Infinity Cache; the flush keeps the queue busy, so the events time the GPU work alone.  Warm:
the same launches without the flush on the same inputs; the queue is idle when the start event is recorded, so the
window also holds the host side of the call (argument checks, ctypes): for short launches that is what it measures.
The kernel time itself comes from a kernel trace of this tool (--trace below).
Algorithmic bytes per pixel.edge: motion_features 32 (target 8 read; coords1 8 + motn 16 written), projective_transform
with Jacobians 116 (coords 8 + valid 4 + Ji 48 + Jj 48 + Jz 8 written); fraction = bytes / time / 8 TB/s.
Usage: prof_reproject.py [--reps N] [--skip-torch] [--skip-parity]
       prof_reproject.py --trace KERNEL_TRACE_CSV   (summarise a rocprofv3 --kernel-trace of this tool: per workload,
                                                     the median kernel duration of its dispatches, found by grid size)
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

geom = lgu_slam_amd.geom
HBM = 8e12


# ---- timing -------------------------------------------------------------------------------------------------------
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


# ---- inputs -------------------------------------------------------------------------------------------------------
def scene(N, H, W, E, stereo_every=0, seed=0):
    g = torch.Generator().manual_seed(seed)
    t = torch.cumsum(0.05 * torch.randn(1, N, 3, generator=g), 1)
    ax = torch.nn.functional.normalize(torch.randn(1, N, 3, generator=g), dim=-1)
    a = 0.05 * torch.randn(1, N, 1, generator=g)
    poses = torch.cat([t, torch.sin(a / 2) * ax, torch.cos(a / 2)], -1).float()
    disps = (0.2 + torch.rand(1, N, H, W, generator=g)).float()
    intr = torch.tensor([0.8 * W, 0.8 * W, W / 2, H / 2]).repeat(1, N, 1).float()
    ii = torch.randint(0, N, (E,), generator=g)
    jj = (ii + torch.randint(1, 6, (E,), generator=g)) % N
    if stereo_every:
        jj[::stereo_every] = ii[::stereo_every]
    target = torch.randn(1, E, H, W, 2, generator=g) * 30
    target[..., 0] += torch.arange(W).float()
    target[..., 1] += torch.arange(H).float()[:, None]
    return [x.cuda().contiguous() for x in (poses, disps, intr, ii, jj, target)]


# ---- torch composition --------------------------------------------------------------------------------------------
def _qmul(a, b):
    av, aw, bv, bw = a[..., :3], a[..., 3:], b[..., :3], b[..., 3:]
    return torch.cat([aw * bv + bw * av + torch.cross(av, bv, dim=-1), aw * bw - (av * bv).sum(-1, keepdim=True)], -1)


def _rot(q, X):
    uv = 2.0 * torch.cross(q[..., :3].expand_as(X), X, dim=-1)
    return X + q[..., 3:] * uv + torch.cross(q[..., :3].expand_as(X), uv, dim=-1)


def _inv(G):
    qi = torch.cat([-G[..., 3:6], G[..., 6:]], -1)
    return torch.cat([-_rot(qi, G[..., :3]), qi], -1)


def _mul(A, B):
    return torch.cat([A[..., :3] + _rot(A[..., 3:], B[..., :3]), _qmul(A[..., 3:], B[..., 3:])], -1)


def torch_projective_transform(poses, disps, intr, ii, jj, jacobian=False):
    ht, wd = disps.shape[2:]
    y, x = torch.meshgrid(torch.arange(ht, device=disps.device).float(), torch.arange(wd, device=disps.device).float(),
                          indexing="ij")
    fx, fy, cx, cy = intr[:, ii, None, None, :].unbind(-1)
    d0 = disps[:, ii]
    X0 = torch.stack([(x - cx) / fx, (y - cy) / fy, torch.ones_like(d0), d0], -1)
    G = _mul(poses[:, jj], _inv(poses[:, ii]))
    G[:, ii == jj] = torch.tensor([-0.1, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0], device=G.device)
    Gp = G[:, :, None, None]
    X1 = torch.cat([_rot(Gp[..., 3:], X0[..., :3]) + Gp[..., :3] * X0[..., 3:], X0[..., 3:]], -1)
    fx, fy, cx, cy = intr[:, jj, None, None, :].unbind(-1)
    X, Y, Z, D = X1.unbind(-1)
    Z = torch.where(Z < 0.1, torch.ones_like(Z), Z)
    d = 1.0 / Z
    coords = torch.stack([fx * (X * d) + cx, fy * (Y * d) + cy], -1)
    valid = ((X1[..., 2] > 0.2) & (X0[..., 2] > 0.2)).float().unsqueeze(-1)
    if not jacobian:
        return coords, valid
    o = torch.zeros_like(d)
    B, N, H, W = d.shape
    Jp = torch.stack([fx * d, o, -fx * X * d * d, o, o, fy * d, -fy * Y * d * d, o], -1).view(B, N, H, W, 2, 4)
    Xa, Ya, Za, Da = X1.unbind(-1)
    Ja = torch.stack([Da, o, o, o, Za, -Ya, o, Da, o, -Za, o, Xa, o, o, Da, Ya, -Xa, o, o, o, o, o, o, o],
                     -1).view(B, N, H, W, 4, 6)
    Jj = torch.matmul(Jp, Ja)
    # -Gij.adjT(Jj): (R^T a_t, R^T (a_r + a_t x t)) per row
    qc = torch.cat([-Gp[..., 3:6], Gp[..., 6:]], -1)[..., None, :]
    at, ar = Jj[..., :3], Jj[..., 3:]
    t = Gp[..., None, :3]
    Ji = -torch.cat([_rot(qc, at), _rot(qc, ar + torch.cross(at, t.expand_as(at), dim=-1))], -1)
    Jz = torch.matmul(Jp, torch.cat([Gp[..., :3], torch.ones_like(Gp[..., :1])], -1).unsqueeze(-1))
    return coords, valid, (Ji, Jj, Jz)


def torch_motion_features(poses, disps, intr, ii, jj, target, coords0):
    coords1, _ = torch_projective_transform(poses, disps, intr, ii, jj)
    motn = torch.cat([coords1 - coords0, target - coords1], dim=-1)
    return coords1, motn.permute(0, 1, 4, 2, 3).clamp(-64.0, 64.0)


def _maxabs(a, b):
    m = torch.isfinite(a) & torch.isfinite(b)
    return float((a.double() - b.double()).abs()[m].max()) if bool(m.any()) else 0.0


def _parity_vs_restatement(args_cpu, jacobian, got):
    """Bit comparison with the float32 CPU restatement of the tests (tests/reproject_restatement.py)."""
    from tests import reproject_restatement as R
    from tests.test_reproject import same_bits
    poses, disps, intr, ii, jj, target = args_cpu
    if jacobian:
        want = R.projective_transform32(poses, disps, intr, ii, jj, jacobian=True)
        return all(same_bits(g, w) for g, w in zip(list(got[:2]) + list(got[2]), list(want[:2]) + list(want[2])))
    want = R.motion_features32(poses, disps, intr, ii, jj, target)
    return same_bits(got[0], want[0]) and same_bits(got[1], want[1])


WORKLOADS = (("motn_c5", 128, 60, 80, 1970, 0, False), ("motn_c2", 32, 48, 64, 20, 0, False),
             ("motn_c3", 32, 48, 64, 40, 4, False), ("jac_c5", 128, 60, 80, 1970, 0, True))


def summarise_trace(path):
    import csv
    out = {}
    rows = [r for r in csv.DictReader(open(path)) if "reproject_kernel" in r["Kernel_Name"]]
    for name, N, H, W, E, stereo, jac in WORKLOADS:
        grid = (E * 256, (H * W + 255) // 256)
        kern = "reproject_kernel<true, false, false>" if jac else "reproject_kernel<false, false, true>"
        us = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows
              if kern in r["Kernel_Name"] and (int(r["Grid_Size_X"]), int(r["Grid_Size_Y"])) == grid]
        nbytes = E * H * W * (116 if jac else 32)
        med = float(np.median(us)) if us else None
        out[name] = {"dispatches": len(us), "kernel_us_median": med, "kernel_us_min": min(us) if us else None,
                     "kernel_us_max": max(us) if us else None,
                     "frac_8TBps": (nbytes / HBM * 1e6 / med) if med else None}
    print(json.dumps({"tool": "prof_reproject --trace", "workloads": out}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--skip-torch", action="store_true")
    ap.add_argument("--skip-parity", action="store_true")
    ap.add_argument("--trace", help="summarise this rocprofv3 kernel-trace CSV instead of measuring")
    args = ap.parse_args()
    if args.trace:
        return summarise_trace(args.trace)
    assert torch.cuda.is_available(), "prof_reproject.py measures on the GPU"
    lgu_slam_amd._lib.load()
    res = {"tool": "prof_reproject", "device": torch.cuda.get_device_name(0), "lib": lgu_slam_amd._lib.version(),
           "hbm_peak_Bps": HBM, "workloads": {}}
    flush = torch.zeros(128 * 1024 * 1024, device="cuda")   # 512 MiB
    R_ = args.reps
    for name, N, H, W, E, stereo, jac in WORKLOADS:
        P, D, K, I, J, T = scene(N, H, W, E, stereo, seed=E + H)
        px = E * H * W
        nbytes = px * (116 if jac else 32)
        if jac:
            fn = lambda: geom.projective_transform(P, D, K, I, J, jacobian=True)  # noqa: E731
        else:
            fn = lambda: geom.motion_features(P, D, K, I, J, T)  # noqa: E731
        w = {"edges": E, "ht": H, "wd": W, "stereo_edges": int((I == J).sum()), "pixel_edges": px, "bytes": nbytes}
        w["ms_warm"] = time_ms(fn, R_)
        w["ms_cold"] = time_ms(fn, R_, flush=flush)
        w["floor_ms"] = 1e3 * nbytes / HBM
        w["frac_8TBps_warm"] = w["floor_ms"] / w["ms_warm"]
        w["frac_8TBps_cold"] = w["floor_ms"] / w["ms_cold"]
        if not args.skip_torch:
            y, x = torch.meshgrid(torch.arange(H, device="cuda").float(), torch.arange(W, device="cuda").float(), indexing="ij")
            c0 = torch.stack([x, y], -1)
            if jac:
                tfn = lambda: torch_projective_transform(P, D, K, I, J, jacobian=True)  # noqa: E731
            else:
                tfn = lambda: torch_motion_features(P, D, K, I, J, T, c0)  # noqa: E731
            w["torch_ms_warm"] = time_ms(tfn, max(5, R_ // 5), warmup=2)
            w["torch_ms_cold"] = time_ms(tfn, max(5, R_ // 5), warmup=1, flush=flush)
            w["speedup_vs_torch_warm"] = w["torch_ms_warm"] / w["ms_warm"]
            w["speedup_vs_torch_cold"] = w["torch_ms_cold"] / w["ms_cold"]
            a, b = fn(), tfn()
            w["vs_torch_max_abs_coords"] = _maxabs(a[0], b[0])
            if jac:
                w["vs_torch_max_abs_J"] = [_maxabs(p, q) for p, q in zip(a[2], b[2])]
                w["vs_torch_valid_mismatch"] = int((a[1] != b[1]).sum())
            else:
                w["vs_torch_max_abs_motn"] = _maxabs(a[1], b[1])
            del a, b
        if not args.skip_parity and name in ("motn_c5", "jac_c5", "motn_c3"):
            got = fn()
            got = (got[0].cpu(), got[1].cpu(), tuple(t.cpu() for t in got[2])) if jac else tuple(t.cpu() for t in got)
            w["bit_identical_to_restatement"] = _parity_vs_restatement([t.cpu() for t in (P, D, K, I, J, T)], jac, got)
            del got
        torch.cuda.empty_cache()
        res["workloads"][name] = w
    print(json.dumps(res))


if __name__ == "__main__":
    main()
