#!/usr/bin/env python3
"""Device-event medians of the geometry operators (lgu_slam_amd.geom) on their reference workloads, against a chunked
pure-torch composition of the same formulas on the same GPU (baseline + large-shape parity check) and a floor.
Prints ONE JSON line.

Workloads (the reference's call forms):
  fd_allpairs_256 / _512  DepthVideo.distance() with no indices: frame_distance over all t x t pairs of t frames at
                          48x64, both directions (two calls, depth_video.py:165-170)
  fd_frontend_pair        the frontend's one-pair bidirectional query (droid_frontend.py:55)
  depth_filter_512        depth_filter over 512 frames at 192x256 (view_reconstruction.py:76)
  iproj_512               iproj over 512 frames at 192x256 (view_reconstruction.py:73)
  projmap_1970            projmap for 1970 edges at 48x64

Floors.  frame_distance / depth_filter: the VALU-issue floor from the kernel's own instructions, read from the gfx950
ISA of csrc/geom.hip (compiled here with the library's flags): per pixel, every VALU instruction costs 4 cycles of its
SIMD's issue, a transcendental (v_rcp / v_sqrt / v_rsq / v_exp / v_log / v_sin / v_cos) or an FP64 instruction 8
(MI355X_MICROARCH: one wave's issue cost), over 1024 SIMDs at 2.4 GHz.  frame_distance's count is its innermost
(per-pixel) loop; depth_filter's is the whole kernel per thread (one thread per pixel, all six neighbours).
iproj / projmap: the HBM write floor, bytes written / 6.29 TB/s (measured copy bandwidth).
Usage: prof_geom.py [--reps N] [--skip-torch]
"""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import lgu_slam_amd  # noqa: E402
from lgu_slam_amd import _build  # noqa: E402

geom = lgu_slam_amd.geom
SIMDS, CLOCK, HBM = 1024, 2.4e9, 6.29e12
MIN_DEPTH = 0.25
_TRANS = re.compile(r"^v_(rcp|sqrt|rsq|exp|log|sin|cos)_")


# ---- ISA: per-pixel instruction counts ----------------------------------------------------------------------------
def _kernel_asm(asm, name):
    m = re.search(r"^(_ZN3lgu\d+%s\w*):" % name, asm, re.M)
    end = asm.index(".Lfunc_end", m.end())
    return asm[m.end():end]


def _count(lines):
    valu = [l.split()[0] for l in lines if l.strip().startswith("v_")]
    trans = sum(1 for v in valu if _TRANS.match(v) or v.endswith("_f64"))
    return {"valu": len(valu), "slow": trans, "issue_cycles": 4 * (len(valu) - trans) + 8 * trans}


def isa_counts():
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "geom.s")
        subprocess.check_call([_build._hipcc()] + _build.FLAGS + ["--cuda-device-only", "-S",
                              os.path.join(_build.CSRC, "geom.hip"), "-o", out], stderr=subprocess.DEVNULL)
        asm = open(out).read()
    # frame_distance: the blocks of its deepest loop (header annotated "Inner Loop Header: Depth=d", members
    # "in Loop: Header=<header> Depth=d"); one iteration = one pixel per lane
    blocks, cur = [], None
    for l in _kernel_asm(asm, "frame_distance_kernel").splitlines():
        m = re.match(r"^(?:\.L(BB\d+_\d+)|; %bb\.\d+):(.*)$", l)
        if m:
            cur = [m.group(1), m.group(2), []]
            blocks.append(cur)
        elif cur is not None and l.strip().startswith(";") and not cur[2]:
            cur[1] += l
        elif cur is not None:
            cur[2].append(l)
    depth = lambda b: int(re.search(r"Inner Loop Header: Depth=(\d+)", b[1]).group(1))  # noqa: E731
    hdr = max((b for b in blocks if "Inner Loop Header" in b[1]), key=depth)
    body = [l for b in blocks if b is hdr or ("Header=%s Depth" % hdr[0]) in b[1] for l in b[2]]
    fdc = _count(body)
    dfc = _count(_kernel_asm(asm, "depth_filter_kernel").splitlines())
    return fdc, dfc


def valu_floor(lane_pixels, counts):
    return lane_pixels / 64.0 * counts["issue_cycles"] / (SIMDS * CLOCK)


# ---- timing -------------------------------------------------------------------------------------------------------
def time_ms(fn, reps, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts))


# ---- scene --------------------------------------------------------------------------------------------------------
def scene(N, H, W, seed=0, dev="cuda"):
    g = torch.Generator().manual_seed(seed)
    t = torch.cumsum(0.05 * torch.randn(N, 3, generator=g), 0)
    ax = torch.nn.functional.normalize(torch.randn(N, 3, generator=g), dim=1)
    a = 0.05 * torch.randn(N, 1, generator=g)
    poses = torch.cat([t, torch.sin(a / 2) * ax, torch.cos(a / 2)], 1).float()
    disps = (0.2 + torch.rand(N, H, W, generator=g)).float()
    intr = torch.tensor([0.8 * W, 0.8 * W, W / 2, H / 2], dtype=torch.float32)
    return poses.to(dev).contiguous(), disps.to(dev).contiguous(), intr.to(dev)


# ---- pure-torch composition (same formulas, float32, chunked) -----------------------------------------------------
def _cross(a, b):
    return torch.cross(a, b, dim=-1)


def _act_so3(q, X):
    uv = 2.0 * _cross(q[..., :3], X)
    return X + q[..., 3:] * uv + _cross(q[..., :3], uv)


def _rel(poses, ii, jj):
    ti, qi, tj, qj = poses[ii, :3], poses[ii, 3:], poses[jj, :3], poses[jj, 3:]
    a0, a1, a2, a3 = qi.unbind(-1)
    b0, b1, b2, b3 = qj.unbind(-1)
    qij = torch.stack([-b3 * a0 + b0 * a3 - b1 * a2 + b2 * a1, -b3 * a1 + b1 * a3 - b2 * a0 + b0 * a2,
                       -b3 * a2 + b2 * a3 - b0 * a1 + b1 * a0, b3 * a3 + b0 * a0 + b1 * a1 + b2 * a2], -1)
    return tj - _act_so3(qij, ti), qij


def _grid(H, W, intr, dev):
    v, u = torch.meshgrid(torch.arange(H, device=dev, dtype=torch.float32), torch.arange(W, device=dev, dtype=torch.float32),
                          indexing="ij")
    u, v = u.reshape(-1), v.reshape(-1)
    return u, v, (u - intr[2]) / intr[0], (v - intr[3]) / intr[1]


def torch_frame_distance(poses, disps, intr, ii, jj, beta, chunk=2048):
    H, W = disps.shape[1:]
    u, v, x, y = _grid(H, W, intr, disps.device)
    fx, fy, cx, cy = intr[:4]
    out = []
    for s in range(0, len(ii), chunk):
        i, j = ii[s:s + chunk], jj[s:s + chunk]
        t, q = _rel(poses, i, j)
        d = disps[i].reshape(len(i), -1, 1)
        X = torch.stack([x, y, torch.ones_like(x)], -1)[None]
        Y = _act_so3(q[:, None], X) + d * t[:, None]
        Z = X + d * t[:, None]
        acc = val = tot = 0
        for P, w in ((Y, beta), (Z, 1 - beta)):
            du = fx * (P[..., 0] / P[..., 2]) + cx - u
            dv = fy * (P[..., 1] / P[..., 2]) + cy - v
            ok = P[..., 2] > MIN_DEPTH
            acc = acc + (w * torch.sqrt(du * du + dv * dv) * ok).double().sum(1)
            val = val + (w * ok).double().sum(1)
            tot = tot + w * P.shape[1]
        out.append(torch.where(val / (tot + 1e-8) < 0.75, torch.full_like(val, 1000.0), acc / val).float())
    return torch.cat(out)


def torch_depth_filter(poses, disps, intr, ix, thresh, chunk=32):
    N, H, W = disps.shape
    u, v, x, y = _grid(H, W, intr, disps.device)
    fx, fy, cx, cy = intr[:4]
    out = []
    for s in range(0, len(ix), chunk):
        i = ix[s:s + chunk]
        cnt = torch.zeros(len(i), H * W, device=disps.device)
        di = disps[i].reshape(len(i), -1)
        X = torch.stack([x, y, torch.ones_like(x)], -1)[None]
        for n in (-1, -2, -3, 3, 4, 5):
            j = i + n
            okf = (j >= 0) & (j < N)
            jc = j.clamp(0, N - 1)
            t, q = _rel(poses, i, jc)
            Y = _act_so3(q[:, None], X) + di[..., None] * t[:, None]
            uj = fx * (Y[..., 0] / Y[..., 2]) + cx
            vj = fy * (Y[..., 1] / Y[..., 2]) + cy
            dj = di / Y[..., 2]
            u0 = torch.nan_to_num(torch.floor(uj), nan=0.0).clamp(-2 ** 31, 2 ** 31 - 1).long()
            v0 = torch.nan_to_num(torch.floor(vj), nan=0.0).clamp(-2 ** 31, 2 ** 31 - 1).long()
            inside = (u0 >= 0) & (v0 >= 0) & (u0 < W - 1) & (v0 < H - 1) & okf[:, None]
            uc, vc = torch.where(inside, u0, 0), torch.where(inside, v0, 0)
            r = 1.0 / dj.double()
            Dj = disps[jc].reshape(len(i), -1)
            hit = torch.zeros_like(inside)
            for dv_, du_ in ((0, 0), (0, 1), (1, 0), (1, 1)):
                c = torch.gather(Dj, 1, ((vc + dv_).clamp(max=H - 1) * W + (uc + du_).clamp(max=W - 1)))
                hit |= (r - 1.0 / c.double()).abs() < thresh[s:s + chunk, None].double()
            cnt += (inside & hit).float()
        out.append(cnt.reshape(len(i), H, W))
    return torch.cat(out)


def torch_iproj(poses, disps, intr, chunk=64):
    N, H, W = disps.shape
    u, v, x, y = _grid(H, W, intr, disps.device)
    X = torch.stack([x, y, torch.ones_like(x)], -1)[None]
    out = []
    for s in range(0, N, chunk):
        p = poses[s:s + chunk]
        d = disps[s:s + chunk].reshape(len(p), -1, 1)
        out.append(((_act_so3(p[:, None, 3:], X) + d * p[:, None, :3]) / d).reshape(len(p), H, W, 3))
    return torch.cat(out)


def torch_projmap(poses, disps, intr, ii, jj, chunk=512):
    H, W = disps.shape[1:]
    u, v, x, y = _grid(H, W, intr, disps.device)
    fx, fy, cx, cy = intr[:4]
    X = torch.stack([x, y, torch.ones_like(x)], -1)[None]
    cs, vs = [], []
    for s in range(0, len(ii), chunk):
        i, j = ii[s:s + chunk], jj[s:s + chunk]
        t, q = _rel(poses, i, j)
        Y = _act_so3(q[:, None], X) + disps[i].reshape(len(i), -1, 1) * t[:, None]
        near = Y[..., 2].double() > 0.01
        cu = torch.where(near, fx * (Y[..., 0] / Y[..., 2]) + cx, u)
        cv = torch.where(near, fy * (Y[..., 1] / Y[..., 2]) + cy, v)
        cs.append(torch.stack([cu, cv, torch.zeros_like(cu)], -1).reshape(len(i), H, W, 3))
        vs.append((Y[..., 2] > MIN_DEPTH).float().reshape(len(i), H, W, 1))
    return torch.cat(cs), torch.cat(vs)


def _maxrel(a, b):
    a, b = a.double(), b.double()
    m = torch.isfinite(a) & torch.isfinite(b)
    return float(((a - b).abs()[m] / b.abs()[m].clamp(min=1e-6)).max()) if bool(m.any()) else 0.0


def _maxabs(a, b):
    """Largest |a - b| over entries finite in both (coordinates / points: relative error is meaningless near 0)."""
    m = torch.isfinite(a) & torch.isfinite(b)
    return float((a.double() - b.double()).abs()[m].max()) if bool(m.any()) else 0.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--skip-torch", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "prof_geom.py measures on the GPU"
    lgu_slam_amd._lib.load()
    fdc, dfc = isa_counts()
    res = {"tool": "prof_geom", "device": torch.cuda.get_device_name(0), "lib": lgu_slam_amd._lib.version(),
           "isa": {"frame_distance_per_pixel": fdc, "depth_filter_per_thread": dfc}, "workloads": {}}
    R = args.reps
    tr = max(2, R // 8)

    for N in (256, 512):
        P, D, K = scene(N, 48, 64, seed=N)
        ii, jj = torch.meshgrid(torch.arange(N, device="cuda"), torch.arange(N, device="cuda"), indexing="ij")
        ii, jj = ii.reshape(-1).contiguous(), jj.reshape(-1).contiguous()

        def run(P=P, D=D, K=K, ii=ii, jj=jj):
            return .5 * (geom.frame_distance(P, D, K, ii, jj, 0.3) + geom.frame_distance(P, D, K, jj, ii, 0.3))
        w = {"pairs": N * N, "calls": 2, "ms": time_ms(run, R)}
        w["floor_ms"] = 1e3 * valu_floor(2 * N * N * 48 * 64, fdc)
        w["share_of_floor"] = w["floor_ms"] / w["ms"]
        if not args.skip_torch:
            tfn = lambda: .5 * (torch_frame_distance(P, D, K, ii, jj, 0.3) + torch_frame_distance(P, D, K, jj, ii, 0.3))  # noqa: E731
            w["torch_ms"] = time_ms(tfn, tr, warmup=1)
            w["speedup_vs_torch"] = w["torch_ms"] / w["ms"]
            a, b = run(), tfn()
            fin = (a != 1000) & (b != 1000)
            w["parity_max_rel"] = _maxrel(a[fin], b[fin])
            w["parity_branch_mismatch"] = int(((a == 1000) != (b == 1000)).sum())
        res["workloads"]["fd_allpairs_%d" % N] = w

    P, D, K = scene(64, 48, 64, seed=1)
    i1, j1 = torch.tensor([63], device="cuda"), torch.tensor([62], device="cuda")
    w = {"pairs": 1, "calls": 2,
         "ms": time_ms(lambda: .5 * (geom.frame_distance(P, D, K, i1, j1, 0.3) + geom.frame_distance(P, D, K, j1, i1, 0.3)), R)}
    w["floor_ms"] = 1e3 * valu_floor(2 * 48 * 64, fdc)
    if not args.skip_torch:
        w["torch_ms"] = time_ms(lambda: .5 * (torch_frame_distance(P, D, K, i1, j1, 0.3) + torch_frame_distance(P, D, K, j1, i1, 0.3)), R)
    res["workloads"]["fd_frontend_pair"] = w

    P, D, K = scene(512, 192, 256, seed=2)
    ix = torch.arange(512, device="cuda")
    th = torch.full((512,), 0.005, device="cuda")
    w = {"frames": 512, "ms": time_ms(lambda: geom.depth_filter(P, D, K, ix, th), R)}
    w["floor_ms"] = 1e3 * valu_floor(512 * 192 * 256, dfc)
    w["share_of_floor"] = w["floor_ms"] / w["ms"]
    if not args.skip_torch:
        w["torch_ms"] = time_ms(lambda: torch_depth_filter(P, D, K, ix, th), tr, warmup=1)
        w["speedup_vs_torch"] = w["torch_ms"] / w["ms"]
        w["parity_count_mismatch"] = int((geom.depth_filter(P, D, K, ix, th) != torch_depth_filter(P, D, K, ix, th)).sum())
    res["workloads"]["depth_filter_512"] = w

    Pi = geom.se3_inverse(P)
    w = {"frames": 512, "ms": time_ms(lambda: geom.iproj(Pi, D, K), R)}
    w["floor_ms"] = 1e3 * 512 * 192 * 256 * 12 / HBM
    w["share_of_floor"] = w["floor_ms"] / w["ms"]
    if not args.skip_torch:
        w["torch_ms"] = time_ms(lambda: torch_iproj(Pi, D, K), tr, warmup=1)
        w["speedup_vs_torch"] = w["torch_ms"] / w["ms"]
        w["parity_max_abs"] = _maxabs(geom.iproj(Pi, D, K), torch_iproj(Pi, D, K))
    res["workloads"]["iproj_512"] = w

    P, D, K = scene(128, 48, 64, seed=3)
    g = torch.Generator().manual_seed(4)
    ii = torch.randint(0, 128, (1970,), generator=g).cuda()
    jj = ((ii + torch.randint(1, 6, (1970,), generator=g).cuda()) % 128).contiguous()
    w = {"edges": 1970, "ms": time_ms(lambda: geom.projmap(P, D, K, ii, jj), R)}
    w["floor_ms"] = 1e3 * 1970 * 48 * 64 * 16 / HBM
    w["share_of_floor"] = w["floor_ms"] / w["ms"]
    if not args.skip_torch:
        w["torch_ms"] = time_ms(lambda: torch_projmap(P, D, K, ii, jj), tr, warmup=1)
        w["speedup_vs_torch"] = w["torch_ms"] / w["ms"]
        a, b = geom.projmap(P, D, K, ii, jj), torch_projmap(P, D, K, ii, jj)
        w["parity_max_abs"] = _maxabs(a[0], b[0])
        w["parity_valid_mismatch"] = int((a[1] != b[1]).sum())
    res["workloads"]["projmap_1970"] = w
    print(json.dumps(res))


if __name__ == "__main__":
    main()
