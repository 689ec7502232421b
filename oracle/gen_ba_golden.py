#!/usr/bin/env python3
"""Writes tests/golden/ba_ref_<case>.npz: one or two Gauss-Newton steps of the REFERENCE's own Python bundle adjustment
(droid_slam/geom/ba.py `BA` and `MoBA`, with geom/chol.py and geom/projective_ops.py), run unchanged on the CPU in float64
and in float32 on seeded scenes.  tests/test_ba_reference.py holds oracle/ba_oracle.py (CPU) and lgu_slam_amd.ba (GPU) to
them.  TEST INFRASTRUCTURE: needs a checkout of the reference (--reference DIR); the fixtures hold arrays only.

How the reference's modules come to run here (nothing of their text is copied, no bytecode is written):
  lietorch       lgu_slam_amd.install_dropins(lietorch=True): the CPU torch composition of lgu_slam_amd.lie, any dtype
  torch_scatter  a module of this file with scatter_sum (index_add_ along `dim` into zeros of `dim_size`)
  projective_ops.torch
                 a proxy that forwards every attribute to torch, except as_tensor, which drops device="cuda" and takes
                 the dtype of the run (projective_ops.py:108 builds a CUDA tensor unconditionally)
  ba.schur_solve, ba.block_solve
                 wrapped in the imported module's namespace: the wrappers call the originals with the case's lm and ep
                 and record the operands H, E, C, v, w, the returned dx and dz, and dz_cuda (below)

The reference has two implementations of this step, the Python one run here and `ba_cuda` (src/droid_kernels.cu), the
one this project ships.  They differ on purpose (DESIGN.md 3.5 lists the departures); the fixtures keep to the ground on
which they agree, and state the one difference that remains:
  * lm = 0 (the two damp different matrices otherwise), and ep = 0 for MoBA (block_solve damps off-diagonal blocks too);
  * the reference solves with C + eta + 1e-7, ba_cuda with C + eta: the device gets `eta` (float32), the reference
    float64(eta) - 1e-7, so both solve with the same C;
  * no stereo edge (ii == jj), every transformed depth above 0.3, every disparity inside (0, 10): no threshold or clamp
    of either implementation is reached (asserted here before and after every step);
  * EvT6x1_kernel skips pose index 0 (src/droid_kernels.cu:1095-1115), so ba_cuda's depth update is
    dz_cuda = Q (w - E^T dx0), dx0 = dx with the first window pose's row zeroed, where the Python form uses dx itself.
    dz_cuda is formed here from the very operands the reference hands to schur_solve; dz_python is stored next to it.
    Between the two iterations of a chained case the disparities move by dz_cuda, without the reference's clamp.

Per file (float32 inputs in lgu_slam_amd.ba.ba's layouts; results of the float64 run as float64):
  poses (N,7)  disps (N,H,W)  intrinsics (4,)  targets, weights (E,2,H,W)  eta (K,H,W), rows = ba_cuda's depth frames
  ii, jj (E,) int64   t0, t1, iterations   lm, ep   motion_only
  kx (M,)               the reference's depth frames (unique(ii)): the rows of dz_cuda and dz_python
  dx (P,6)              of the last iteration
  dz_cuda, dz_python (M,HW)   of the last iteration (full BA only)
  dz_cuda_step1, dz_python_step1   of the first iteration, where there are two: by the second, dx is small and so is the
                        difference between the two forms
  kx_cuda (K,)          ba_cuda's depth frames (unique(cat(ts, ii))): the rows of eta
  poses_after (N,7), disps_after (N,H,W)
  e32_<quantity>        the largest distance between the float32 run and the float64 run of that quantity
  full_t1 only: H (P,P,6,6), v (P,6), E (P,M,6,HW), C (M,HW), w (M,HW) as handed to schur_solve, with e32_H ... e32_w and
  e32_S, e32_sv for the Schur products E Q E^T and E Q w formed from them.

Usage: gen_ba_golden.py [--reference DIR] [--out DIR] [--check]   (--check: regenerate and compare with the committed files)
"""
import argparse
import os
import sys
import types

sys.dont_write_bytecode = True

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
_here = os.path.dirname(os.path.abspath(__file__))
sys.path[:] = [q for q in sys.path if os.path.abspath(q or ".") != _here]   # `oracle` must be the package, not oracle/oracle.py
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import ba_oracle as O  # noqa: E402  (scene construction only: exp_se3, rel_se3, retr_se3)

f32 = np.float32
MIN_Z = 0.3          # above both implementations' thresholds (0.2 / 0.1 in Python, 0.25 in CUDA)
MAX_DISP = 10.0      # the Python form zeroes disparities above it

# name -> scene and call.  `drop_source`: frames that are the source (ii) of no edge.
CASES = {
    "full_t1":          dict(seed=101, N=5, H=12, W=16, span=2, t0=1, iters=1, motion=False, ep=0.1, system=True),
    "full_t2_it2":      dict(seed=102, N=5, H=12, W=16, span=2, t0=2, iters=2, motion=False, ep=0.1),
    "full_eta":         dict(seed=103, N=6, H=12, W=16, span=2, t0=3, iters=1, motion=False, ep=0.1, eta_rows=True),
    "full_target_only": dict(seed=104, N=6, H=8, W=12, span=2, t0=1, iters=1, motion=False, ep=0.1, drop_source=(4,)),
    "full_blocked":     dict(seed=105, N=36, H=6, W=8, span=2, t0=1, iters=1, motion=False, ep=0.1),
    "motion_t1":        dict(seed=106, N=5, H=12, W=16, span=2, t0=1, iters=2, motion=True, ep=0.0),
    "motion_t2":        dict(seed=107, N=5, H=12, W=16, span=2, t0=2, iters=2, motion=True, ep=0.0),
}
LM = 0.0
QUANTITIES = ("dx", "dz_cuda", "dz_python", "dz_cuda_step1", "dz_python_step1", "poses_after", "disps_after")
SYSTEM = ("H", "v", "E", "C", "w", "S", "sv")


# ---- scenes -----------------------------------------------------------------------------------------------------------
def project(poses, disps, intr, ii, jj):
    """Exact reprojections (float64 arithmetic on the float32 state) of every pixel of frame ii[e] into frame jj[e]."""
    H, W = disps.shape[1:]
    fx, fy, cx, cy = [float(v) for v in intr]
    v, u = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    X = np.stack([(u - cx) / fx, (v - cy) / fy, np.ones_like(u)], -1).reshape(-1, 3)
    out = np.zeros((len(ii), 2, H, W), f32)
    for e in range(len(ii)):
        tij, qij = O.rel_se3(poses[ii[e], :3], poses[ii[e], 3:], poses[jj[e], :3], poses[jj[e], 3:])
        uv = 2.0 * np.cross(qij[:3], X)
        Xj = X + qij[3] * uv + np.cross(qij[:3], uv) + disps[ii[e]].reshape(-1, 1).astype(np.float64) * tij[None]
        out[e, 0] = (fx * Xj[:, 0] / Xj[:, 2] + cx).reshape(H, W)
        out[e, 1] = (fy * Xj[:, 1] / Xj[:, 2] + cy).reshape(H, W)
    return out


def make_case(cfg):
    """The float32 inputs of one case, in lgu_slam_amd.ba.ba's layouts: exact targets of a seeded scene, then poses and
    disparities of the window perturbed (as tests/test_ba.py does), seeded weights."""
    rng = np.random.default_rng(cfg["seed"])
    N, H, W, span, t0 = cfg["N"], cfg["H"], cfg["W"], cfg["span"], cfg["t0"]
    intr = np.array([20.0, 20.0, W / 2, H / 2], f32)
    poses = np.zeros((N, 7), f32)
    poses[:, 6] = 1
    for k in range(1, N):
        t, q = O.exp_se3(np.concatenate([rng.standard_normal(3) * 0.08, rng.standard_normal(3) * 0.1]))
        poses[k, :3], poses[k, 3:] = t, q
    disps = (0.3 + 0.7 * rng.random((N, H, W))).astype(f32)
    drop = set(cfg.get("drop_source", ()))
    pairs = [(i, j) for i in range(N) for j in range(N) if i != j and abs(i - j) <= span and i not in drop]
    ii = np.array([p[0] for p in pairs], np.int64)
    jj = np.array([p[1] for p in pairs], np.int64)
    targets = project(poses, disps, intr, ii, jj)
    for k in range(t0, N):
        t_, q_ = O.retr_se3(np.concatenate([rng.standard_normal(3) * 0.02, rng.standard_normal(3) * 0.01]),
                            poses[k, :3].astype(np.float64), poses[k, 3:].astype(np.float64))
        poses[k, :3], poses[k, 3:] = t_, q_
    disps[t0:] *= (1 + 0.05 * rng.standard_normal(disps[t0:].shape)).astype(f32)
    weights = (0.5 + rng.random(targets.shape)).astype(f32)
    kx_cuda = np.unique(np.concatenate([np.arange(t0, N), ii]))          # ba_cuda's depth frames: cat(ts, ii)
    if cfg.get("eta_rows"):
        eta = (1e-3 + 1e-3 * rng.random((len(kx_cuda), H, W))).astype(f32)
    else:
        eta = np.full((len(kx_cuda), H, W), 1e-3, f32)
    return dict(poses=poses, disps=disps, intrinsics=intr, targets=targets, weights=weights, eta=eta, ii=ii, jj=jj,
                t0=np.int64(t0), t1=np.int64(N), iterations=np.int64(cfg["iters"]), lm=np.float64(LM), ep=np.float64(cfg["ep"]),
                motion_only=np.bool_(cfg["motion"]), kx_cuda=kx_cuda)


# ---- the reference, imported unchanged ----------------------------------------------------------------------------------
def _scatter_module():
    m = types.ModuleType("torch_scatter")

    def scatter_sum(src, index, dim=-1, out=None, dim_size=None):
        dim = dim if dim >= 0 else dim + src.dim()
        shape = list(src.shape)
        shape[dim] = int(dim_size) if dim_size is not None else (int(index.max()) + 1 if index.numel() else 0)
        res = torch.zeros(shape, dtype=src.dtype, device=src.device)
        return res.index_add_(dim, index.to(torch.int64), src)

    m.scatter_sum = scatter_sum
    return m


class _TorchProxy:
    """`torch` as projective_ops sees it: everything is torch's own, except as_tensor."""

    def __init__(self):
        self.run_dtype = torch.float64

    def __getattr__(self, name):
        return getattr(torch, name)

    def as_tensor(self, data, *args, **kwargs):
        kwargs.pop("device", None)
        kwargs["dtype"] = self.run_dtype
        return torch.as_tensor(data, *args, **kwargs)


class Reference:
    """The reference's droid_slam.geom.ba over the stand-ins, with the two solvers wrapped."""

    def __init__(self, reference):
        if not os.path.isdir(os.path.join(reference, "droid_slam", "geom")):
            raise RuntimeError("%s holds no droid_slam/geom: pass --reference DIR" % reference)
        import lgu_slam_amd
        lgu_slam_amd.install_dropins(lietorch=True)
        if "torch_scatter" in sys.modules:
            raise RuntimeError("a torch_scatter is already imported; the generator brings its own scatter_sum")
        sys.modules["torch_scatter"] = _scatter_module()
        sys.path.insert(0, reference)
        import droid_slam.geom.ba as ref_ba
        import droid_slam.geom.projective_ops as pops
        assert os.path.abspath(ref_ba.__file__).startswith(os.path.abspath(reference))
        self.ba, self.pops, self.SE3 = ref_ba, pops, sys.modules["lietorch"].SE3
        self.proxy = pops.torch = _TorchProxy()
        self.lm = self.ep = None
        self.record = None
        schur, block = ref_ba.schur_solve, ref_ba.block_solve

        def schur_solve(H, E, C, v, w):
            dx, dz = schur(H, E, C, v, w, ep=self.ep, lm=self.lm)
            B, P, M, D, HW = E.shape
            Ef = E.permute(0, 1, 3, 2, 4).reshape(B, P * D, M * HW)
            Q = (1.0 / C).view(B, M * HW, 1)
            dx0 = dx.clone()
            dx0[:, 0] = 0                                           # EvT6x1_kernel skips pose index 0
            dz_cuda = (Q * (w.reshape(B, M * HW, 1) - Ef.transpose(1, 2) @ dx0.reshape(B, P * D, 1))).reshape(B, M, HW)
            S = Ef @ (Q * Ef.transpose(1, 2))
            sv = Ef @ (Q * w.reshape(B, M * HW, 1))
            self.record = dict(H=H, E=E, C=C, v=v, w=w, dx=dx, dz_python=dz, dz_cuda=dz_cuda, S=S, sv=sv)
            return dx, dz

        def block_solve(H, b):
            dx = block(H, b, ep=self.ep, lm=self.lm)
            self.record = dict(H=H, v=b, dx=dx)
            return dx

        ref_ba.schur_solve, ref_ba.block_solve = schur_solve, block_solve

    def depths(self, poses, disps, intr, ii, jj):
        """Z of every pixel of frame ii[e] in frame jj[e], by the reference's own iproj and actp."""
        X0, _ = self.pops.iproj(disps[:, ii], intr[:, ii])
        X1, _ = self.pops.actp(poses[:, jj] * poses[:, ii].inv(), X0)
        return X1[..., 2]

    def check_state(self, what, poses, disps, intr, ii, jj):
        z = float(self.depths(poses, disps, intr, ii, jj).min())
        lo, hi = float(disps.min()), float(disps.max())
        if not z > MIN_Z:
            raise AssertionError("%s: a transformed depth of %.4f is not above %.1f" % (what, z, MIN_Z))
        if not (lo > 0.0 and hi < MAX_DISP):
            raise AssertionError("%s: disparities [%.4f, %.4f] leave (0, %g)" % (what, lo, hi, MAX_DISP))

    def run(self, name, case, dtype):
        """The case's iterations in `dtype`; every quantity as a float64 numpy array."""
        self.proxy.run_dtype = dtype
        self.lm, self.ep = float(case["lm"]), float(case["ep"])
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dtype)  # noqa: E731
        ii, jj = torch.from_numpy(case["ii"]), torch.from_numpy(case["jj"])
        if bool((ii == jj).any()):
            raise AssertionError("%s: stereo edges cannot go into a reference fixture" % name)
        t0, N = int(case["t0"]), int(case["t1"])
        poses = self.SE3(t(case["poses"])[None])
        disps = t(case["disps"])[None]
        intr = t(case["intrinsics"])[None, None].repeat(1, N, 1)
        target = t(case["targets"]).permute(0, 2, 3, 1)[None].contiguous()
        weight = t(case["weights"]).permute(0, 2, 3, 1)[None].contiguous()
        kx = torch.unique(ii)
        rows = torch.from_numpy(np.searchsorted(case["kx_cuda"], kx.numpy()))
        eta = (torch.from_numpy(case["eta"]).double()[rows] - 1e-7).to(dtype)[None]      # + 1e-7 again in geom/ba.py:91
        motion = bool(case["motion_only"])
        out = {}
        with torch.no_grad():
            for it in range(int(case["iterations"])):
                self.check_state("%s, before step %d" % (name, it), poses, disps, intr, ii, jj)
                self.record = None
                if motion:
                    poses = self.ba.MoBA(target, weight, eta, poses, disps, intr, ii, jj, fixedp=t0, rig=1)
                else:
                    poses, _ = self.ba.BA(target, weight, eta, poses, disps, intr, ii, jj, fixedp=t0, rig=1)
                rec = self.record
                if rec is None or not float(rec["dx"].abs().max()) > 0.0:
                    raise AssertionError("%s: the Cholesky factorisation fell back to zeros" % name)
                if not motion:
                    if it == 0 and int(case["iterations"]) > 1:
                        out["dz_cuda_step1"], out["dz_python_step1"] = rec["dz_cuda"][0], rec["dz_python"][0]
                    disps = disps.clone()
                    disps[:, kx] += rec["dz_cuda"].view(1, -1, *disps.shape[2:])        # disp_retr_kernel: no clamp
                self.check_state("%s, after step %d" % (name, it), poses, disps, intr, ii, jj)
        out["dx"] = rec["dx"][0]
        if not motion:
            out["dz_cuda"], out["dz_python"] = rec["dz_cuda"][0], rec["dz_python"][0]
            for k in ("H", "v", "E", "C", "w", "S", "sv"):
                out["sys_" + k] = rec[k][0]
        out["poses_after"], out["disps_after"] = poses.data[0], disps[0]
        out = {k: v.double().numpy().copy() for k, v in out.items()}
        out["kx"] = kx.numpy().astype(np.int64)
        return out


def generate(reference, names=None):
    ref = Reference(reference)
    res = {}
    for name, cfg in CASES.items():
        if names and name not in names:
            continue
        case = make_case(cfg)
        r64 = ref.run(name, case, torch.float64)
        r32 = ref.run(name, case, torch.float32)
        arrays = dict(case)
        arrays["kx"] = r64["kx"]
        keep = [q for q in QUANTITIES if q in r64]
        for q in keep:
            arrays[q] = r64[q]
            arrays["e32_" + q] = np.float64(np.abs(r32[q] - r64[q]).max())
        if cfg.get("system"):
            for q in SYSTEM:
                if q not in ("S", "sv"):
                    arrays[q] = r64["sys_" + q]
                arrays["e32_" + q] = np.float64(np.abs(r32["sys_" + q] - r64["sys_" + q]).max())
        res[name] = arrays
    return res


def _compare(name, key, have, want):
    """Inputs bit for bit; float64 results to 1e-9 of their scale (another CPU's BLAS may sum in another order, far below
    every bound a test derives); e32 to a factor 2."""
    if key.startswith("e32_"):
        ok = 0.5 * float(want) <= float(have) <= 2.0 * float(want) or float(have) == float(want)
    elif want.dtype == np.float64 and key not in ("lm", "ep"):
        ok = have.shape == want.shape and np.abs(have - want).max() <= 1e-9 * max(np.abs(want).max(), 1e-30)
    else:
        ok = have.dtype == want.dtype and np.array_equal(have, want)
    if not ok:
        raise AssertionError("%s: %s differs from the committed fixture" % (name, key))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("LGU_REFERENCE", "/root/reference"))
    ap.add_argument("--out", default=GOLDEN)
    ap.add_argument("--check", action="store_true")
    ap.add_argument("cases", nargs="*")
    args = ap.parse_args()
    for name, arrays in generate(args.reference, args.cases).items():
        path = os.path.join(args.out, "ba_ref_%s.npz" % name)
        if args.check:
            with np.load(path, allow_pickle=False) as z:
                assert sorted(z.files) == sorted(arrays), (name, sorted(z.files), sorted(arrays))
                for k, v in arrays.items():
                    _compare(name, k, z[k], np.asarray(v))
            print("%s: matches" % path)
        else:
            np.savez_compressed(path, **arrays)
            e32 = "  ".join("%s %.2e" % (k[4:], float(v)) for k, v in arrays.items() if k.startswith("e32_"))
            print("%s: %d bytes  e32: %s" % (path, os.path.getsize(path), e32))


if __name__ == "__main__":
    main()
