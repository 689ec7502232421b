"""projective_transform, reproject and motion_features (lgu_slam_amd.geom, csrc/reproject.hip): the reference's
geom/projective_ops.py:projective_transform and FactorGraph.update's motion features without lietorch.

The kernels are held bit for bit to the float32 restatement tests/reproject_restatement.py (coordinates, valid,
Ji / Jj / Jz, motion channels, NaN for out-of-range edges).  The float32 restatement is held to a float64 one in plain
math, whose Jacobians are checked against central finite differences under left perturbations of the poses.
"""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import reproject_restatement as R  # noqa: E402

f32 = torch.float32
ENTRIES = ("lgu_projective_transform_f32", "lgu_motion_features_f32")


def scene(seed, B=1, N=8, H=48, W=64, step=0.1, angle=0.1):
    """Poses (B,N,7) float32 (a random walk, rotations of ~`angle`), disparities in [0.2, 1.2), per-frame intrinsics
    around a DROID-like frame (fx = fy = 0.8 W, each entry scaled by up to 5 %)."""
    g = torch.Generator().manual_seed(seed)
    t = torch.cumsum(step * torch.randn(B, N, 3, generator=g, dtype=torch.float64), 1)
    ax = torch.nn.functional.normalize(torch.randn(B, N, 3, generator=g, dtype=torch.float64), dim=-1)
    a = angle * torch.randn(B, N, 1, generator=g, dtype=torch.float64)
    poses = torch.cat([t, torch.sin(a / 2) * ax, torch.cos(a / 2)], -1).to(f32)
    disps = (0.2 + torch.rand(B, N, H, W, generator=g)).to(f32)
    K = torch.tensor([0.8 * W, 0.8 * W, W / 2, H / 2], dtype=torch.float64).repeat(B, N, 1)
    intr = (K * (1 + 0.05 * torch.rand(B, N, 4, generator=g, dtype=torch.float64))).to(f32)
    return poses, disps, intr


def edges(seed, N, E, stereo=2, invalid=()):
    """E random edges ii != jj, `stereo` edges ii == jj, then the `invalid` (ii, jj) pairs."""
    g = torch.Generator().manual_seed(seed)
    ii = torch.randint(0, N, (E,), generator=g)
    jj = (ii + torch.randint(1, N, (E,), generator=g)) % N
    ii = torch.cat([ii, torch.arange(stereo), torch.tensor([p[0] for p in invalid], dtype=torch.int64)])
    jj = torch.cat([jj, torch.arange(stereo), torch.tensor([p[1] for p in invalid], dtype=torch.int64)])
    return ii, jj


def same_bits(a, b):
    a, b = torch.as_tensor(a).detach().cpu(), torch.as_tensor(b).detach().cpu()
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    na, nb = torch.isnan(a), torch.isnan(b)
    return bool(torch.equal(na, nb)) and bool(torch.equal(a[~na].view(torch.int32), b[~nb].view(torch.int32)))


NEXT_BELOW = lambda x: float(np.nextafter(np.float32(x), np.float32(0)))  # noqa: E731
THRESHOLDS = (float(np.float32(0.2)), NEXT_BELOW(0.2), float(np.float32(0.1)), NEXT_BELOW(0.1),
              float(np.nextafter(np.float32(0.2), np.float32(1))))


def threshold_scene(H=48, W=64):
    """Frame 0 at the identity, frame 1 turned by 70 degrees about x and moved by t = (0, 0, -1): on edge 0 -> 1,
    X1.z = a - disp with a the rotated z of the pixel's ray.  For up to 12 pixels each, the disparity is chosen so that
    X1.z lands exactly on float32(0.2), the float below it, float32(0.1), the float below it, the float above
    0.2 (in turn).  Returns poses, disps, intrinsics (B = 1) and the map of the value each pixel was placed on (NaN: none)."""
    th = np.deg2rad(70.0)
    poses = torch.zeros(1, 2, 7, dtype=f32)
    poses[0, :, 6] = 1
    poses[0, 1, 2] = -1.0
    poses[0, 1, 3], poses[0, 1, 6] = float(np.sin(th / 2)), float(np.cos(th / 2))
    intr = torch.tensor([0.8 * W, 0.8 * W, W / 2, H / 2], dtype=f32).repeat(1, 2, 1)
    disps = torch.full((1, 2, H, W), 0.5, dtype=f32)
    ii, jj = torch.tensor([0]), torch.tensor([1])
    zero = torch.zeros_like(disps)
    a = R.points32(poses, zero, intr, ii, jj)[2][2][0, 0].double()      # X1.z with disparity 0: the rotated ray
    placed = torch.full((H, W), float("nan"), dtype=torch.float64)
    for want in THRESHOLDS:
        n = 0
        for y, x in ((want + 0.01 < a) & (a < 0.5) & torch.isnan(placed)).nonzero().tolist():
            d = float(a[y, x]) - want
            if float(np.float32(d)) == d and n < 12:                   # representable: a - d is exactly `want`
                disps[0, 0, y, x] = d
                placed[y, x] = want
                n += 1
    Z = R.points32(poses, disps, intr, ii, jj)[2][2][0, 0].double()
    hit = ~torch.isnan(placed)
    assert torch.equal(Z[hit], placed[hit])                            # every placed pixel is exactly on its value
    for want in THRESHOLDS:
        assert int((placed == want).sum()) >= 5, want
    return poses, disps, intr, placed


# ---------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------

def test_header_declares_and_library_exports_the_reproject_entries(lgu):
    from tests.test_abi import declared_symbols
    syms = declared_symbols()
    lib = ctypes.CDLL(lgu.build())
    for s in ENTRIES:
        assert s in syms, s
        assert hasattr(lib, s), s
        assert s in lgu._lib.SIGNATURES, s


def test_float32_restatement_agrees_with_float64():
    poses, disps, intr = scene(3, B=2, N=8, H=24, W=32, step=0.3, angle=0.3)
    ii, jj = edges(4, 8, 30)
    c32, v32, J32 = R.projective_transform32(poses, disps, intr, ii, jj, jacobian=True, return_depth=True)
    c64, v64, J64 = R.projective_transform64(poses, disps, intr, ii, jj, jacobian=True, return_depth=True)
    Z = R.points32(poses, disps, intr, ii, jj)[2][2].double()
    away = ((Z - 0.1).abs() > 1e-3) & ((Z - 0.2).abs() > 1e-5)
    assert bool(away.float().mean() > 0.9)
    err = (c32.double() - c64).abs()[..., :2][away]
    assert float(err.max()) < 1e-3
    assert torch.equal(v32.double()[away], v64[away])
    assert 0 < float(v64.mean()) < 1
    for a, b in zip(J32, J64):
        b = b[away]
        assert float((a.double()[away] - b).abs().max()) <= 1e-4 * float(b.abs().max())


@pytest.mark.parametrize("seed", [0, 1])
def test_float64_jacobians_match_central_differences(seed):
    """Jj: G_j <- Exp(xi) G_j; Ji: G_i <- Exp(xi) G_i (lietorch's left perturbation, tangent = (translation, rotation));
    Jz: the disparity.  Non-stereo edges only; pixels not clamped (Z > 0.1)."""
    poses, disps, intr = scene(10 + seed, B=1, N=6, H=12, W=16, step=0.3, angle=0.4)
    ii, jj = edges(seed, 6, 10, stereo=0)
    T = R.pose_matrix(poses)
    Ti, Tj = T[:, ii], T[:, jj]
    D, Ki, Kj = disps.double()[:, ii], intr.double()[:, ii], intr.double()[:, jj]
    G = Tj @ torch.linalg.inv(Ti)
    coords, _, X1, (Ji, Jj, Jz) = R.transform64(G, D, Ki, Kj, jacobian=True)
    away = X1[..., 2] > 0.1 + 1e-3          # Jp keeps d = 1 / Z where Z is clamped: no derivative of the clamp
    assert bool(away.float().mean() > 0.8)
    proj = lambda G_, D_=D: R.transform64(G_, D_, Ki, Kj)[0]  # noqa: E731
    eps = 1e-6
    for n in range(6):
        xi = torch.zeros(6, dtype=torch.float64)
        xi[n] = eps
        fd_j = (proj(R.se3_exp(xi) @ G) - proj(R.se3_exp(-xi) @ G)) / (2 * eps)
        fd_i = (proj(Tj @ torch.linalg.inv(R.se3_exp(xi) @ Ti)) - proj(Tj @ torch.linalg.inv(R.se3_exp(-xi) @ Ti))) / (2 * eps)
        scale = float(Jj[..., n].abs().max()) + 1.0
        assert float((fd_j - Jj[..., n]).abs()[away].max()) < 1e-6 * scale, n
        assert float((fd_i - Ji[..., n]).abs()[away].max()) < 1e-6 * (float(Ji[..., n].abs().max()) + 1.0), n
    fd_z = (proj(G, D + eps) - proj(G, D - eps)) / (2 * eps)
    assert float((fd_z - Jz[..., 0]).abs()[away].max()) < 1e-6 * (float(Jz.abs().max()) + 1.0)


def test_stereo_edges_use_the_baseline():
    """ii == jj: G_ij = (t = (-0.1, 0, 0), identity), whatever the pose: x1 = fx (x - 0.1 disp) + cx, y1 = v."""
    poses, disps, intr = scene(5, B=1, N=4, H=6, W=8, step=0.5, angle=0.5)
    ii = jj = torch.tensor([0, 2, 3])
    c32, v32 = R.projective_transform32(poses, disps, intr, ii, jj, return_depth=True)
    K = intr.double()[:, ii, :, None, None]
    D = disps.double()[:, ii]
    u = torch.arange(8, dtype=torch.float64)
    x = (u - K[:, :, 2]) / K[:, :, 0]
    assert float((c32[..., 0].double() - (K[:, :, 0] * (x - 0.1 * D) + K[:, :, 2])).abs().max()) < 1e-4
    assert float((c32[..., 1].double() - torch.arange(6, dtype=torch.float64)[:, None]).abs().max()) < 1e-4
    assert torch.equal(c32[..., 2], disps[:, ii])                           # Z = 1: the depth channel is the disparity
    assert bool((v32 == 1).all())
    c64, _ = R.projective_transform64(poses, disps, intr, ii, jj)
    assert float((c32[..., :2].double() - c64).abs().max()) < 1e-4
    # the override replaces the true (identity) relative pose: different from the same frame under ii != jj semantics
    assert float((c32[..., 0] - torch.arange(8, dtype=f32)).abs().max()) > 0.5


def test_thresholds_are_float32_comparisons():
    assert not bool(torch.tensor([0.2]) > 0.2)                              # torch compares against float32(0.2)
    poses, disps, intr, placed = threshold_scene()
    ii, jj = torch.tensor([0]), torch.tensor([1])
    coords, valid = R.projective_transform32(poses, disps, intr, ii, jj)
    v = valid[0, 0, ..., 0]
    z2, z2m, z1, z1m, z2p = THRESHOLDS
    assert bool((v[placed == z2] == 0).all()) and bool((v[placed == z2m] == 0).all())
    assert bool((v[placed == z2p] == 1).all())
    # Z == float32(0.1) is kept (d = 1 / Z); the float below it is replaced by 1 (d = 1)
    X = R.points32(poses, disps, intr, ii, jj)[2][0][0, 0]
    fx, cx = intr[0, 1, 0], intr[0, 1, 2]
    below = placed == z1m
    assert torch.equal(coords[0, 0, ..., 0][below], (fx * X + cx)[below])
    at = placed == z1
    d = torch.ones(()) / torch.tensor(z1, dtype=f32)
    assert torch.equal(coords[0, 0, ..., 0][at], (fx * (X * d) + cx)[at])


def _cpu_args(B=1, N=4, H=6, W=8):
    poses = torch.zeros(B, N, 7)
    poses[..., 6] = 1
    intr = torch.tensor([8.0, 8.0, 4.0, 3.0]).repeat(B, N, 1)
    return poses, torch.ones(B, N, H, W), intr, torch.arange(3), torch.arange(1, 4) % N


@pytest.mark.parametrize("op", ["projective_transform", "motion_features", "reproject"])
def test_input_checks_raise_before_any_launch(lgu, monkeypatch, op):
    def no_launch():
        raise AssertionError("the library was reached")
    monkeypatch.setattr(lgu._lib, "load", no_launch)
    fn = getattr(lgu.geom, op)
    poses, disps, intr, ii, jj = _cpu_args()
    target = torch.zeros(1, 3, 6, 8, 2)

    def call(p=poses, d=disps, k=intr, i=ii, j=jj, tg=target, **kw):
        if op == "reproject":
            return fn(p[0] if p.dim() == 3 else p, d[0] if d.dim() == 4 else d, k[0] if k.dim() == 3 else k, i, j)
        if op == "motion_features":
            return fn(p, d, k, i, j, tg, **kw)
        return fn(p, d, k, i, j, **kw)

    with pytest.raises(RuntimeError, match="^disps must be contiguous$"):
        call(d=torch.ones(1, 4, 8, 6).transpose(2, 3))
    with pytest.raises(RuntimeError, match="^poses must be contiguous$"):
        call(p=torch.zeros(1, 7, 4).transpose(1, 2))
    with pytest.raises(RuntimeError, match="expected scalar type Long but found Int"):
        call(i=ii.int())
    with pytest.raises(RuntimeError, match="expected scalar type Float but found Double"):
        call(d=disps.double())
    with pytest.raises(RuntimeError, match="ii and jj must be 1-D and of equal length"):
        call(j=torch.arange(2))
    with pytest.raises(RuntimeError, match="intrinsics must be"):
        call(k=torch.ones(1, 4, 5))
    if op != "reproject":
        with pytest.raises(RuntimeError, match="poses must be"):
            call(p=torch.zeros(4, 7))
        with pytest.raises(RuntimeError, match="same batch size"):
            call(p=torch.zeros(2, 4, 7))
    if op == "motion_features":
        with pytest.raises(RuntimeError, match="target must be"):
            call(tg=torch.zeros(1, 3, 8, 6, 2))
        with pytest.raises(RuntimeError, match="^target must be contiguous$"):
            call(tg=torch.zeros(1, 3, 6, 2, 8).transpose(3, 4))
        with pytest.raises(RuntimeError, match="clamp"):
            call(clamp=-1.0)
    # autograd: inputs that require grad are refused while grad mode is on, before any launch or device check
    with pytest.raises(RuntimeError, match="no autograd"):
        call(p=poses.clone().requires_grad_())
    with pytest.raises(RuntimeError, match="no autograd"):
        call(d=disps.clone().requires_grad_())
    with torch.no_grad():
        with pytest.raises(RuntimeError, match="must be a HIP device tensor"):
            call(p=poses.clone().requires_grad_())
    with pytest.raises(RuntimeError, match="must be a HIP device tensor"):   # all other arguments are valid
        call()


def test_pose_objects_with_data_are_accepted(lgu, monkeypatch):
    """A lietorch-style group object is read through `.data`; a tensor is used as it is (its .data would drop the
    autograd check)."""
    monkeypatch.setattr(lgu._lib, "load", lambda: (_ for _ in ()).throw(AssertionError("the library was reached")))
    poses, disps, intr, ii, jj = _cpu_args()

    class Group:
        data = poses
    with pytest.raises(RuntimeError, match="must be a HIP device tensor"):
        lgu.geom.projective_transform(Group(), disps, intr, ii, jj)
    with pytest.raises(RuntimeError, match="no autograd"):
        lgu.geom.projective_transform(poses.clone().requires_grad_(), disps, intr, ii, jj)


def test_torch_ops_registration(lgu):
    from lgu_slam_amd import torch_ops
    assert sorted(torch_ops.REPROJ_REGISTERED) == ["motion_features", "projective_transform"]
    s = str(torch.ops.lgu.projective_transform.default._schema)
    assert "bool jacobian=False" in s and "bool return_depth=False" in s and s.endswith("-> Tensor[]")
    s = str(torch.ops.lgu.motion_features.default._schema)
    assert "Tensor target" in s and "float clamp=64." in s and s.endswith("-> Tensor[]")


# ---------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------

def cu(*ts):
    out = tuple(t.cuda().contiguous() for t in ts)
    return out if len(out) > 1 else out[0]


def _check_transform(lgu, poses, disps, intr, ii, jj, jacobian, return_depth):
    got = lgu.geom.projective_transform(*cu(poses, disps, intr, ii, jj), jacobian=jacobian, return_depth=return_depth)
    want = R.projective_transform32(poses, disps, intr, ii, jj, jacobian=jacobian, return_depth=return_depth)
    assert len(got) == len(want)
    assert same_bits(got[0], want[0]) and same_bits(got[1], want[1])
    if jacobian:
        for g, w in zip(got[2], want[2]):
            assert same_bits(g, w)
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("shape", [(48, 64), (60, 80), (7, 5)])
def test_projective_transform_is_bit_identical_to_the_restatement(lgu, B, shape):
    H, W = shape
    N = 9
    poses, disps, intr = scene(20 + H + B, B=B, N=N, H=H, W=W, step=0.4, angle=0.3)
    disps[:, 3] -= 0.5                                # some points behind / near the camera: both sides of 0.1 and 0.2
    ii, jj = edges(H + B, N, 17, stereo=2, invalid=[(N, 0), (1, N), (-1, 2), (2 ** 40, 3)])
    bad = torch.zeros(len(ii), dtype=torch.bool)
    bad[-4:] = True
    for jacobian in (False, True):
        for return_depth in (False, True):
            got = _check_transform(lgu, poses, disps, intr, ii, jj, jacobian, return_depth)
            C = 3 if return_depth else 2
            assert tuple(got[0].shape) == (B, len(ii), H, W, C) and tuple(got[1].shape) == (B, len(ii), H, W, 1)
            assert bool(torch.isnan(got[0][:, bad.cuda()]).all()) and bool((got[1][:, bad.cuda()] == 0).all())
            assert bool(torch.isfinite(got[0][:, ~bad.cuda()]).all())
            if jacobian:
                assert [tuple(J.shape) for J in got[2]] == [(B, len(ii), H, W, 2, 6)] * 2 + [(B, len(ii), H, W, 2, 1)]
                assert all(bool(torch.isnan(J[:, bad.cuda()]).all()) for J in got[2])
    v = got[1][:, ~bad.cuda()]
    assert 0 < float(v.mean()) < 1


@pytest.mark.gpu
def test_threshold_values_on_the_gpu(lgu):
    poses, disps, intr, placed = threshold_scene()
    ii, jj = torch.tensor([0, 1, 0]), torch.tensor([1, 0, 0])
    got = _check_transform(lgu, poses, disps, intr, ii, jj, True, True)
    v = got[1][0, 0, ..., 0].cpu()
    assert bool((v[placed == THRESHOLDS[0]] == 0).all()) and bool((v[placed == THRESHOLDS[4]] == 1).all())


@pytest.mark.gpu
@pytest.mark.parametrize("B", [1, 2])
def test_motion_features_are_bit_identical_with_saturation_and_nan(lgu, B):
    H, W, N = 30, 40, 7
    poses, disps, intr = scene(60 + B, B=B, N=N, H=H, W=W, step=0.6, angle=0.4)
    disps[:, 2] -= 0.6
    ii, jj = edges(B, N, 12, stereo=1, invalid=[(N, 1)])
    E = len(ii)
    g = torch.Generator().manual_seed(B)
    c1 = R.projective_transform32(poses, disps, intr, ii, jj)[0]
    target = c1 + 200 * torch.randn(B, E, H, W, 2, generator=g)            # many channels saturate at +-64
    target[torch.rand(B, E, H, W, 2, generator=g) < 0.05] = float("nan")
    target[..., 0, 0, :] = float("inf")
    target[..., 0, 1, :] = -float("inf")
    got = lgu.geom.motion_features(*cu(poses, disps, intr, ii, jj, target))
    want = R.motion_features32(poses, disps, intr, ii, jj, target)
    assert tuple(got[1].shape) == (B, E, 4, H, W) and got[1].is_contiguous()
    assert same_bits(got[0], want[0]) and same_bits(got[1], want[1])
    m = got[1].cpu()
    assert bool((m.abs() == 64).any()) and bool(torch.isnan(m[:, :, 2:]).any())
    assert float(m[~torch.isnan(m)].abs().max()) == 64.0
    assert bool(torch.isnan(m[:, -1]).all())                               # the out-of-range edge
    nan_t = torch.isnan(target).permute(0, 1, 4, 2, 3)
    assert bool(torch.isnan(m[:, :, 2:][nan_t]).all())                     # a NaN target stays NaN through the clamp
    # another bound
    got8 = lgu.geom.motion_features(*cu(poses, disps, intr, ii, jj, target), clamp=8.0)
    assert same_bits(got8[1], R.motion_features32(poses, disps, intr, ii, jj, target, clamp=8.0)[1])


@pytest.mark.gpu
def test_motion_features_at_the_config5_size(lgu):
    """1970 edges at 60x80 (BASELINE config 5), restatement on the CPU."""
    H, W, N = 60, 80, 128
    poses, disps, intr = scene(77, B=1, N=N, H=H, W=W, step=0.05, angle=0.05)
    g = torch.Generator().manual_seed(5)
    ii = torch.randint(0, N, (1970,), generator=g)
    jj = (ii + torch.randint(-5, 6, (1970,), generator=g)).clamp(0, N - 1)  # neighbours, some ii == jj (stereo)
    target = R.projective_transform32(poses, disps, intr, ii, jj)[0] + torch.randn(1, 1970, H, W, 2, generator=g)
    got = lgu.geom.motion_features(*cu(poses, disps, intr, ii, jj, target))
    want = R.motion_features32(poses, disps, intr, ii, jj, target)
    assert same_bits(got[0], want[0]) and same_bits(got[1], want[1])


@pytest.mark.gpu
def test_reproject_and_torch_ops_equal_projective_transform(lgu):
    import lgu_slam_amd.torch_ops  # noqa: F401
    poses, disps, intr = scene(91, B=1, N=10, H=24, W=32)
    ii, jj = edges(91, 10, 15)
    P, D, K, I, J = cu(poses, disps, intr, ii, jj)
    c, v = lgu.geom.reproject(P[0], D[0], K[0], I, J)
    c2, v2 = lgu.geom.projective_transform(P, D, K, I, J)
    assert tuple(c.shape) == (1, len(ii), 24, 32, 2) and tuple(v.shape) == (1, len(ii), 24, 32, 1)
    assert same_bits(c, c2) and same_bits(v, v2)
    ops = torch.ops.lgu.projective_transform(P, D, K, I, J, True, True)
    ref = lgu.geom.projective_transform(P, D, K, I, J, jacobian=True, return_depth=True)
    assert len(ops) == 5 and all(same_bits(a, b) for a, b in zip(ops, list(ref[:2]) + list(ref[2])))
    tg = c2 + 1
    mf = torch.ops.lgu.motion_features(P, D, K, I, J, tg, 64.0)
    ref = lgu.geom.motion_features(P, D, K, I, J, tg)
    assert same_bits(mf[0], ref[0]) and same_bits(mf[1], ref[1]) and same_bits(mf[0], c2)


_SENT = 1234.5


def _banded(shape, guard=4096):
    n = int(np.prod(shape))
    big = torch.full((n + 2 * guard,), _SENT, dtype=f32, device="cuda")
    return big, big[guard:guard + n].view(shape), guard


def _bands_intact(big, guard):
    return bool((big[:guard] == _SENT).all()) and bool((big[-guard:] == _SENT).all())


@pytest.mark.gpu
def test_reproject_entry_points_write_nothing_outside_their_tensors(lgu):
    """Both entries called through the C ABI into sentinel-filled memory: results equal the operators' into fresh
    tensors, every element is written, the bands are untouched."""
    from lgu_slam_amd.ops import _ptr, _stream
    lib = lgu._lib.load()
    B, N, H, W = 2, 6, 13, 70
    poses, disps, intr = scene(101, B=B, N=N, H=H, W=W, step=0.3, angle=0.2)
    ii, jj = edges(101, N, 3, stereo=1, invalid=[(N, 0)])
    E = len(ii)
    P, D, K, I, J = cu(poses, disps, intr, ii, jj)
    st = _stream(P)
    bands = []
    for flags in range(4):
        C = 3 if flags & 2 else 2
        bc, coords, gc = _banded((B, E, H, W, C))
        bv, valid, gv = _banded((B, E, H, W, 1))
        bi, Ji, gi = _banded((B, E, H, W, 2, 6))
        bj, Jj, gj = _banded((B, E, H, W, 2, 6))
        bz, Jz, gz = _banded((B, E, H, W, 2, 1))
        jac = (_ptr(Ji), _ptr(Jj), _ptr(Jz)) if flags & 1 else (None, None, None)
        assert lib.lgu_projective_transform_f32(_ptr(P), _ptr(D), _ptr(K), _ptr(I), _ptr(J), B, N, N, N, H, W, E, flags,
                                                _ptr(coords), _ptr(valid), *jac, st) == 0
        torch.cuda.synchronize()
        ref = lgu.geom.projective_transform(P, D, K, I, J, jacobian=bool(flags & 1), return_depth=bool(flags & 2))
        assert same_bits(coords, ref[0]) and same_bits(valid, ref[1])
        outs = [(bc, gc, coords), (bv, gv, valid)]
        if flags & 1:
            assert all(same_bits(a, b) for a, b in zip((Ji, Jj, Jz), ref[2]))
            outs += [(bi, gi, Ji), (bj, gj, Jj), (bz, gz, Jz)]
        else:
            assert bool((Ji == _SENT).all()) and bool((Jz == _SENT).all())     # not requested: not touched
        bands += outs
    tg = torch.randn(B, E, H, W, 2, device="cuda") * 50
    bc, c1, gc = _banded((B, E, H, W, 2))
    bm, mo, gm = _banded((B, E, 4, H, W))
    bv, va, gv = _banded((B, E, H, W))
    assert lib.lgu_motion_features_f32(_ptr(P), _ptr(D), _ptr(K), _ptr(I), _ptr(J), _ptr(tg), B, N, N, N, H, W, E, 64.0,
                                       _ptr(c1), _ptr(mo), _ptr(va), st) == 0
    torch.cuda.synchronize()
    ref = lgu.geom.motion_features(P, D, K, I, J, tg)
    assert same_bits(c1, ref[0]) and same_bits(mo, ref[1])
    assert same_bits(va, lgu.geom.projective_transform(P, D, K, I, J)[1][..., 0])
    bands += [(bc, gc, c1), (bm, gm, mo), (bv, gv, va)]
    for big, g, t in bands:
        assert not bool((t == _SENT).any())
        assert _bands_intact(big, g)
    # argument errors of the ABI
    e = lgu._lib.LGU_E_BADARG
    assert lib.lgu_projective_transform_f32(_ptr(P), _ptr(D), _ptr(K), _ptr(I), _ptr(J), B, N, N, N, H, W, E, 4,
                                            _ptr(coords), None, None, None, None, st) == e
    assert lib.lgu_projective_transform_f32(_ptr(P), _ptr(D), _ptr(K), _ptr(I), _ptr(J), B, N, N, N, H, W, E, 1,
                                            _ptr(coords), None, None, None, None, st) == e
    assert lib.lgu_motion_features_f32(_ptr(P), _ptr(D), _ptr(K), _ptr(I), _ptr(J), _ptr(tg), B, N, N, N, H, W, E, -1.0,
                                       _ptr(c1), _ptr(mo), None, st) == e
    assert lib.lgu_projective_transform_f32(None, None, None, None, None, B, N, N, N, H, W, 0, 0,
                                            None, None, None, None, None, st) == 0       # no edges: nothing launched


@pytest.mark.gpu
def test_side_stream_and_graph_capture(lgu):
    poses, disps, intr = scene(111, B=1, N=10, H=48, W=64)
    ii, jj = edges(111, 10, 40, stereo=2)
    P, D, K, I, J = cu(poses, disps, intr, ii, jj)
    tg = torch.zeros(1, len(ii), 48, 64, 2, device="cuda")
    ref = lgu.geom.projective_transform(P, D, K, I, J, jacobian=True)
    ref_m = lgu.geom.motion_features(P, D, K, I, J, tg)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        pt = lgu.geom.projective_transform(P, D, K, I, J, jacobian=True)
        mf = lgu.geom.motion_features(P, D, K, I, J, tg)
    s.synchronize()
    assert same_bits(pt[0], ref[0]) and same_bits(pt[2][0], ref[2][0]) and same_bits(mf[1], ref_m[1])
    # one capture of motion_features, replayed after the poses and the target moved: equals eager mode on the new inputs
    g = torch.cuda.CUDAGraph()
    s2 = torch.cuda.Stream()
    s2.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s2):
        lgu.geom.motion_features(P, D, K, I, J, tg)               # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(s2)
    with torch.cuda.graph(g):
        out = lgu.geom.motion_features(P, D, K, I, J, tg)
    P.copy_(cu(scene(112, B=1, N=10, H=48, W=64)[0]))
    tg.fill_(3.0)
    g.replay()
    torch.cuda.synchronize()
    now = lgu.geom.motion_features(P, D, K, I, J, tg)
    assert same_bits(out[0], now[0]) and same_bits(out[1], now[1])
    assert not same_bits(out[1], ref_m[1])


@pytest.mark.gpu
def test_zero_edges_or_frames_give_empty_outputs(lgu):
    poses, disps, intr = scene(121, B=2, N=4, H=12, W=16)
    P, D, K = cu(poses, disps, intr)
    e = torch.zeros(0, dtype=torch.int64, device="cuda")
    c, v, (Ji, Jj, Jz) = lgu.geom.projective_transform(P, D, K, e, e, jacobian=True)
    assert tuple(c.shape) == (2, 0, 12, 16, 2) and tuple(v.shape) == (2, 0, 12, 16, 1) and tuple(Jz.shape) == (2, 0, 12, 16, 2, 1)
    c1, m = lgu.geom.motion_features(P, D, K, e, e, torch.zeros(2, 0, 12, 16, 2, device="cuda"))
    assert tuple(c1.shape) == (2, 0, 12, 16, 2) and tuple(m.shape) == (2, 0, 4, 12, 16)
    i1 = torch.tensor([0], device="cuda")
    c, v = lgu.geom.projective_transform(P, D[:, :, :0], K, i1, i1)
    assert tuple(c.shape) == (2, 1, 0, 16, 2)
    c, v = lgu.geom.reproject(P[0], D[0], K[0], e, e)
    assert tuple(c.shape) == (1, 0, 12, 16, 2)
    torch.cuda.synchronize()
