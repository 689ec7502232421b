"""Dense bundle adjustment against the REFERENCE's own Python BA (droid_slam/geom/ba.py `BA` / `MoBA`).

tests/golden/ba_ref_<case>.npz (oracle/gen_ba_golden.py) hold one or two Gauss-Newton steps of the reference's Python
implementation, run unchanged in float64 and in float32 on the same float32 inputs, on the ground where it and `ba_cuda`
agree (lm = 0, no stereo edge, no depth threshold or clamp reached).  The one difference that remains,
EvT6x1_kernel skipping pose index 0, is in the fixture as `dz_cuda` next to `dz_python`.

Held to the fixtures: oracle/ba_oracle.py (CPU tests: the whole step, and on `full_t1` its build, assembly and Schur
stages one by one) and lgu_slam_amd.ba (GPU tests: the whole call on every case, the build kernel's outputs on `full_t1`,
the sharded form at world size 1).

Bound, per quantity, as in tests/test_lie.py: 4 * e32 + one float32 ulp of the largest |expected| value, where e32 is
the distance between the reference's own float32 run and its float64 run, read from the fixture.  The factor 4 covers
another summation order and this build's float64 assembly and solve.  Every test prints the error it finds next to its
bound.

e32 as the generator measured it (absolute; scale = largest |expected|), recorded here and in DESIGN.md 3.5; the tests
read the fixtures, not this table:

  case              quantity     scale     e32       bound
  full_t1           dx           3.4e-2    1.1e-6    4.4e-6
                    dz           1.3e-1    2.2e-6    8.7e-6
                    poses after  1.0       1.1e-6    4.4e-6
                    disps after  1.0       2.2e-6    8.8e-6
  full_t2_it2       dx           1.4e-3    3.5e-7    1.4e-6
                    dz           1.4e-1    1.2e-6    4.9e-6
                    poses after  1.0       6.7e-8    3.9e-7
                    disps after  1.0       8.5e-7    3.5e-6
  full_eta          dx           4.4e-2    2.3e-7    9.3e-7
                    dz           2.3e-1    8.6e-7    3.4e-6
                    poses after  1.0       2.4e-7    1.1e-6
                    disps after  1.0       8.4e-7    3.5e-6
  full_target_only  dx           6.4e-2    9.3e-7    3.7e-6
                    dz           2.4e-1    1.8e-6    7.1e-6
                    poses after  1.0       8.6e-7    3.5e-6
                    disps after  1.1       1.8e-6    7.2e-6
  full_blocked      dx           6.3e-2    8.2e-7    3.3e-6
                    dz           3.9e-1    1.7e-6    6.8e-6
                    poses after  1.0       8.8e-7    3.7e-6
                    disps after  1.2       1.7e-6    6.9e-6
  motion_t1         dx           5.3e-4    6.1e-7    2.4e-6
                    poses after  1.0       5.3e-8    3.3e-7
  motion_t2         dx           6.1e-4    2.7e-7    1.1e-6
                    poses after  1.0       6.2e-8    3.7e-7
  full_t1 system    H 1.4e-4 of 7.2e2 (bound 6.1e-4), v 5.6e-6 of 14 (2.3e-5), E 1.5e-7 of 0.54 (6.7e-7),
                    C 4.4e-8 of 0.17 (1.9e-7), w 3.6e-8 of 0.028 (1.5e-7), S 8.4e-5 of 3.2e2 (3.6e-4), sv 3.8e-6 of 7.6 (1.6e-5)

(dx of the chained cases is the second iteration's, hence its small scale.)
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import ba_oracle as O

f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
REFERENCE = os.environ.get("LGU_REFERENCE", "/root/reference")
FULL = ("full_t1", "full_t2_it2", "full_eta", "full_target_only", "full_blocked")
MOTION = ("motion_t1", "motion_t2")
CASES = FULL + MOTION

_fixtures, _oracle_runs = {}, {}


def fixture(name):
    if name not in _fixtures:
        with np.load(os.path.join(GOLDEN, "ba_ref_%s.npz" % name), allow_pickle=False) as z:
            _fixtures[name] = {k: z[k] for k in z.files}
    return _fixtures[name]


def ulp32(x):
    return float(np.spacing(np.float32(x)))


def bound_of(z, quantity, want):
    """4 e32 + one float32 ulp of the largest |expected| value; e32 is the fixture's."""
    return 4.0 * float(z["e32_" + quantity]) + ulp32(np.abs(want).max())


def held(what, got, want, bound):
    err = float(np.abs(np.asarray(got, np.float64) - want).max())
    print("%-32s err %.3e  bound %.3e  (scale %.3e)" % (what, err, bound, float(np.abs(want).max())))
    return err <= bound


def dz_by_frame(z, dz):
    """`dz` (K,HW), rows = ba_cuda's depth frames cat(ts, ii), split into the rows of the reference's depth frames
    (unique(ii), the fixture's `kx`) and the rows of window frames that are the source of no edge."""
    kx_cuda = np.unique(np.concatenate([np.arange(int(z["t0"]), int(z["t1"])), z["ii"]]))
    assert dz.shape[0] == len(kx_cuda) and np.isin(z["kx"], kx_cuda).all()
    mine = np.searchsorted(kx_cuda, z["kx"])
    extra = np.setdiff1d(np.arange(len(kx_cuda)), mine)
    return dz[mine], dz[extra], kx_cuda[extra]


def call_args(z):
    return (int(z["t0"]), int(z["t1"]), int(z["iterations"]), float(z["lm"]), float(z["ep"]), bool(z["motion_only"]))


def oracle_run(name):
    """oracle/ba_oracle.py on the fixture's inputs, computed once: (dx, dz, poses after, disps after)."""
    if name not in _oracle_runs:
        z = fixture(name)
        p, d = z["poses"].copy(), z["disps"].copy()
        dx, dz = O.ba(p, d, z["intrinsics"], np.zeros_like(d), z["targets"], z["weights"], z["eta"], z["ii"], z["jj"], *call_args(z))
        _oracle_runs[name] = (dx, dz, p, d)
    return _oracle_runs[name]


def check_step(name, who, dx, dz, poses, disps):
    """dx, dz, poses and disps after one call of `who` against the fixture's float64 values."""
    z = fixture(name)
    t0 = int(z["t0"])
    ok = [held("%s %s dx" % (name, who), dx, z["dx"], bound_of(z, "dx", z["dx"])),
          held("%s %s poses after" % (name, who), poses, z["poses_after"], bound_of(z, "poses_after", z["poses_after"]))]
    assert np.array_equal(poses[:t0], z["poses"][:t0])                     # poses before t0 are bit-unchanged
    if bool(z["motion_only"]):
        assert dz is None and np.array_equal(disps, z["disps"])
    else:
        mine, extra, frames = dz_by_frame(z, np.asarray(dz, np.float64))
        b = bound_of(z, "dz_cuda", z["dz_cuda"])
        ok.append(held("%s %s dz" % (name, who), mine, z["dz_cuda"], b))
        if name == "full_target_only":
            assert list(frames) == [4]
        if len(frames):   # a window frame that is the source of no edge: its depth does not move
            ok.append(held("%s %s dz of frames %s" % (name, who, list(frames)), extra, np.zeros_like(extra), b))
        ok.append(held("%s %s disps after" % (name, who), disps, z["disps_after"], bound_of(z, "disps_after", z["disps_after"])))
    assert all(ok)


def reference_system(Hs, vs, Eii, Eij, Cii, wi, z):
    """The per-edge outputs of the build stage aggregated, in float64, to the operands the reference hands to schur_solve:
    H (P,P,6,6), v (P,6), E (P,M,6,HW), C (M,HW), w (M,HW), by the oracle's pose_system and accum."""
    ii, jj, kx, t0 = z["ii"], z["jj"], z["kx"], int(z["t0"])
    P, HW = int(z["t1"]) - t0, Cii.shape[1]
    A, b = O.pose_system(np.asarray(Hs, np.float64), np.asarray(vs, np.float64), ii, jj, t0, P)
    H = A.reshape(P, 6, P, 6).transpose(0, 2, 1, 3)
    Eii, Eij = np.asarray(Eii, np.float64), np.asarray(Eij, np.float64)
    E = np.zeros((P, len(kx), 6, HW))
    for p in range(P):    # block (pose p, depth frame m): Ei of the edges with i = p + t0 = kx[m], Ej of those with i = kx[m], j = p + t0
        for m, fr in enumerate(kx):
            E[p, m] = Eii[(ii == fr) & (ii - t0 == p)].sum(0) + Eij[(ii == fr) & (jj - t0 == p)].sum(0)
    kx_cuda = np.unique(np.concatenate([np.arange(t0, int(z["t1"])), ii]))
    eta = z["eta"].reshape(len(kx_cuda), HW).astype(np.float64)[np.searchsorted(kx_cuda, kx)]
    C = O.accum(np.asarray(Cii), ii, kx) + eta
    w = O.accum(np.asarray(wi), ii, kx)
    return dict(H=H, v=b.reshape(P, 6), E=E, C=C, w=w)


def check_system(who, got, z):
    ok = [held("full_t1 %s %s" % (who, k), got[k], z[k], bound_of(z, k, z[k])) for k in ("H", "v", "E", "C", "w")]
    assert all(ok)


def reference_schur(z):
    """E Q E^T (6P,6P) and E Q w (6P,) from the fixture's operands, float64."""
    P, M, _, HW = z["E"].shape
    Ef = z["E"].transpose(0, 2, 1, 3).reshape(6 * P, M * HW)
    Q = 1.0 / z["C"].reshape(-1)
    return Ef @ (Q[:, None] * Ef.T), Ef @ (Q * z["w"].reshape(-1))


# ---- CPU: the oracle against the reference ----------------------------------------------------------------------------
def test_fixtures_hold_arrays_only():
    for name in CASES:
        z = fixture(name)
        assert all(v.dtype.kind in "fiub" for v in z.values()), name
        assert os.path.getsize(os.path.join(GOLDEN, "ba_ref_%s.npz" % name)) < 1 << 20
        assert float(z["lm"]) == 0.0 and not (z["ii"] == z["jj"]).any()
        for q in ("dx", "poses_after", "disps_after"):
            assert z[q].dtype == np.float64 and float(z["e32_" + q]) >= 0.0
        assert z["poses"].dtype == f32 and z["eta"].dtype == f32
    assert int(fixture("full_blocked")["t1"] - fixture("full_blocked")["t0"]) > 32      # the blocked solve
    assert set(("H", "v", "E", "C", "w")) <= set(fixture("full_t1"))


@pytest.mark.parametrize("name", CASES)
def test_oracle_matches_the_reference(name):
    """oracle/ba_oracle.py (the restatement of ba_cuda) against the reference's Python BA in float64: dx, dz in ba_cuda's
    form, poses and disparities after the call."""
    dx, dz, p, d = oracle_run(name)
    check_step(name, "oracle", dx, dz, p, d)


@pytest.mark.parametrize("name", FULL)
def test_comparison_would_see_the_python_depth_update(name):
    """ba_cuda's depth update leaves out the first window pose (EvT6x1_kernel, src/droid_kernels.cu:1095-1115); the Python
    form does not.  The oracle's dz is far outside the bound of `dz_python`: a kernel that "fixed" the skip would fail the
    dz comparisons of this module.  The skipped term is E^T dx of one pose, so it is as large as dx is: the gap of 0.1 of the
    scale is asked of a case's FIRST step (0.5 to 1.0 of the scale on these scenes).  By the second step of `full_t2_it2` dx
    has shrunk 25-fold and the gap with it, to 0.04 of the scale; that is still 1700 bounds, which is asserted too."""
    z = fixture(name)

    def gap_of(dz, key):
        want = z[key]
        mine, _, _ = dz_by_frame(z, dz)
        scale, gap, bound = float(np.abs(want).max()), float(np.abs(mine - want).max()), bound_of(z, key, want)
        print("%-20s oracle dz against %s: gap %.3e = %.2f of scale %.3e = %.0f bounds of %.3e"
              % (name, key, gap, gap / scale, scale, gap / bound, bound))
        return gap, scale, bound

    gap, scale, bound = gap_of(oracle_run(name)[1], "dz_python")
    assert gap > 100 * bound
    if int(z["iterations"]) > 1:
        args = list(call_args(z))
        args[2] = 1
        p, d = z["poses"].copy(), z["disps"].copy()
        _, dz1 = O.ba(p, d, z["intrinsics"], np.zeros_like(d), z["targets"], z["weights"], z["eta"], z["ii"], z["jj"], *args)
        assert held("%s oracle dz of step 1" % name, dz_by_frame(z, dz1)[0], z["dz_cuda_step1"],
                    bound_of(z, "dz_cuda_step1", z["dz_cuda_step1"]))
        gap, scale, bound = gap_of(dz1, "dz_python_step1")
    assert gap > bound and gap >= 0.1 * scale


def test_oracle_stages_on_full_t1():
    """The build stage and the assembly pinned apart from the solve: the oracle's projective_transform aggregated by
    pose_system and accum to the reference's H, v, E, C, w; then its Schur stage (schur_pairs, the EEt / Ev products,
    schur_system) against E Q E^T and E Q w of the reference's operands."""
    z = fixture("full_t1")
    ii, jj, t0, t1 = z["ii"], z["jj"], int(z["t0"]), int(z["t1"])
    P = t1 - t0
    Hs, vs, Eii, Eij, Cii, wi = O.projective_transform(z["targets"], z["weights"], z["poses"], z["disps"], z["intrinsics"], ii, jj)
    got = reference_system(Hs, vs, Eii, Eij, Cii, wi, z)
    check_system("oracle", got, z)
    # the Schur stage, from the oracle's own C and w
    E, HW = len(ii), Cii.shape[1]
    ts = np.arange(t0, t1)
    ii_exp, jj_exp = np.concatenate([ts, ii]), np.concatenate([ts, jj])
    kx, kk = np.unique(ii_exp, return_inverse=True)
    assert np.array_equal(kx, z["kx"])
    Q = 1.0 / got["C"]
    Eall = np.concatenate([O.accum(Eii.reshape(E, 6 * HW), ii, ts).reshape(P, 6, HW), Eij.astype(np.float64)], 0)
    il, jl, idx = O.schur_pairs(jj_exp, kk, t0, t1)
    S = np.stack([(Eall[a] * Q[k][None]) @ Eall[c].T for a, c, k in idx])
    sv = np.stack([Eall[n] @ (Q[kk[n]] * got["w"][kk[n]]) for n in range(len(ii_exp))])
    A, b = O.schur_system(S, sv, il, jl, jj_exp - t0, P)
    S_ref, sv_ref = reference_schur(z)
    ok = [held("full_t1 oracle S", A, S_ref, bound_of(z, "S", S_ref)), held("full_t1 oracle sv", b, sv_ref, bound_of(z, "sv", sv_ref))]
    assert all(ok)


@pytest.mark.skipif(not os.path.isdir(os.path.join(REFERENCE, "droid_slam")), reason="reference tree not present")
def test_fixtures_regenerate_from_the_live_reference():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "oracle", "gen_ba_golden.py"), "--reference", REFERENCE, "--check"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count("matches") == len(CASES)


# ---- GPU: the HIP implementation against the reference ------------------------------------------------------------------
torch = pytest.importorskip("torch")


def _to_dev(*arrs):
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrs]


def _device_operands(z):
    return _to_dev(z["poses"], z["disps"], z["intrinsics"], np.zeros_like(z["disps"]), z["targets"], z["weights"], z["eta"],
                   z["ii"].astype(np.int64), z["jj"].astype(np.int64))


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_hip_ba_matches_the_reference(lgu, name):
    """lgu_slam_amd.ba.ba on the fixture's inputs: returned dx and dz, poses and disparities after, against the reference's
    float64 values; `full_blocked` (35 window poses) goes through lgu_ba_solve_blocked_f64."""
    z = fixture(name)
    pd, dd, idv, sd, td, wd_, ed, iid, jjd = _device_operands(z)
    dx, dz = lgu.ba.ba(pd, dd, idv, sd, td, wd_, ed, iid, jjd, *call_args(z))
    torch.cuda.synchronize()
    assert dx.dtype == torch.float32 and tuple(dx.shape) == z["dx"].shape
    check_step(name, "hip", dx.cpu().numpy(), None if dz is None else dz.cpu().numpy(), pd.cpu().numpy(), dd.cpu().numpy())


@pytest.mark.gpu
def test_hip_build_kernel_matches_the_reference_system(lgu):
    """lgu_ba_build_f32's Hs, vs, Eii, Eij, Cii, wi on `full_t1`, aggregated on the host in float64 exactly as
    test_oracle_stages_on_full_t1 aggregates the oracle's, against the operands the reference hands to schur_solve."""
    z = fixture("full_t1")
    pd, dd, idv, _, td, wd_, _, iid, jjd = _device_operands(z)
    E, (ht, wd) = len(z["ii"]), z["disps"].shape[1:]
    HW = ht * wd
    lib = lgu._lib.load()
    dev = "cuda"
    Hs, vs = torch.empty(4, E, 6, 6, device=dev), torch.empty(2, E, 6, device=dev)
    Eii, Eij = torch.empty(E, 6, HW, device=dev), torch.empty(E, 6, HW, device=dev)
    Cii, wi = torch.empty(E, HW, device=dev), torch.empty(E, HW, device=dev)
    scratch = torch.empty(E * lib.lgu_ba_build_slices(E) * 90, device=dev)
    vp = ctypes.c_void_p
    rc = lib.lgu_ba_build_f32(*[vp(a.data_ptr()) for a in (td, wd_, pd, dd, idv, iid, jjd, Hs, vs, Eii, Eij, Cii, wi, scratch)],
                              E, ht, wd, vp(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    torch.cuda.synchronize()
    got = reference_system(*[a.double().cpu().numpy() for a in (Hs, vs, Eii, Eij, Cii, wi)], z)
    check_system("hip", got, z)


@pytest.mark.gpu
def test_sharded_ba_world1_matches_the_reference(lgu):
    """sharded.sharded_ba at world size 1 on `full_t2_it2`: bit-equal to the plain call, and inside the fixture's bounds."""
    name = "full_t2_it2"
    z = fixture(name)
    p1, d1, idv, sd, td, wd_, ed, iid, jjd = _device_operands(z)
    p2, d2 = _to_dev(z["poses"], z["disps"])
    edges = lgu.sharded.ShardedEdgeSet(iid, rank=0, world=1, chunk=4)
    own = edges.my_edges
    assert own.numel() == len(z["ii"])
    a = lgu.ba.ba(p1, d1, idv, sd, td, wd_, ed, iid, jjd, *call_args(z))
    b = lgu.sharded.sharded_ba(edges, td[own].contiguous(), wd_[own].contiguous(), p2, d2, idv, sd, ed, iid, jjd, *call_args(z))
    torch.cuda.synchronize()
    assert torch.equal(p1, p2) and torch.equal(d1, d2) and torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    check_step(name, "sharded", b[0].cpu().numpy(), b[1].cpu().numpy(), p2.cpu().numpy(), d2.cpu().numpy())
