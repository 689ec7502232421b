"""CPU restatements of projective_transform (the reference's geom/projective_ops.py:98-128) and of FactorGraph.update's
motion features (factor_graph.py:210-212).  TEST INFRASTRUCTURE ONLY.

* `projective_transform32` / `motion_features32`: torch float32 on the CPU, in the operation order of
  csrc/reproject.hip.  Every step is one elementwise torch operation (correctly rounded, no contraction) and every sum
  is written out, so the kernels are held to it bit for bit.
* `projective_transform64` / `transform64`: float64 in plain math (rotation matrices, 4x4 poses, matmul), for the
  precision and finite-difference tests.

Rules shared with the kernels:
  * an edge is valid when 0 <= ii, jj < min(poses, disps, intrinsics frames); another edge gets NaN coordinates,
    Jacobians and motion channels and valid 0;
  * ii == jj edges use the stereo baseline t = (-0.1, 0, 0), q = identity;
  * the 0.1 clamp and the 0.2 validity threshold are float32 comparisons (what torch does with a Python scalar):
    Z == float32(0.2) is invalid, Z == float32(0.1) is not clamped;
  * quaternions are used as given, not normalised;
  * Jj's structural zeros are written as 0 (Jj = Jp Ja with the zero products left out).
"""
import torch

f32, f64 = torch.float32, torch.float64
CLAMP_Z = torch.tensor(0.1, dtype=f32)          # 0.5 * MIN_DEPTH as float32
MIN_DEPTH = torch.tensor(0.2, dtype=f32)
STEREO = (-0.1, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0)


# ---- float32, kernel order ------------------------------------------------------------------------------------------
def _cross(a, b):
    """se3.hpp cross3, component by component."""
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def act_so3(q, X):
    """se3.hpp act_so3: q, X tuples of tensors (4 and 3 entries)."""
    uv = _cross(q, X)
    uv = tuple(c * 2.0 for c in uv)
    t = _cross(q, uv)
    return tuple(X[k] + q[3] * uv[k] + t[k] for k in range(3))


def rel_se3(pi, pj):
    """se3.hpp rel_se3 (G_j * G_i^-1) on (...,7) float32 tensors -> (t tuple, q tuple)."""
    ti, qi = pi[..., :3].unbind(-1), pi[..., 3:].unbind(-1)
    tj, qj = pj[..., :3].unbind(-1), pj[..., 3:].unbind(-1)
    q = (-qj[3] * qi[0] + qj[0] * qi[3] - qj[1] * qi[2] + qj[2] * qi[1],
         -qj[3] * qi[1] + qj[1] * qi[3] - qj[2] * qi[0] + qj[0] * qi[2],
         -qj[3] * qi[2] + qj[2] * qi[3] - qj[0] * qi[1] + qj[1] * qi[0],
         qj[3] * qi[3] + qj[0] * qi[0] + qj[1] * qi[1] + qj[2] * qi[2])
    r = act_so3(q, ti)
    return tuple(tj[k] - r[k] for k in range(3)), q


def _edges(poses, disps, intrinsics, ii, jj):
    nv = min(poses.shape[1], disps.shape[1], intrinsics.shape[1])
    ii, jj = torch.as_tensor(ii, dtype=torch.int64), torch.as_tensor(jj, dtype=torch.int64)
    ok = (ii >= 0) & (ii < nv) & (jj >= 0) & (jj < nv)
    return ok, torch.where(ok, ii, 0), torch.where(ok, jj, 0), ii == jj


def relative_poses32(poses, ii, jj):
    """G_ij per batch and edge, float32 (B,E,7) = t, q; the stereo baseline where ii == jj.  Indices must be valid."""
    poses = torch.as_tensor(poses, dtype=f32)
    t, q = rel_se3(poses[:, ii], poses[:, jj])
    G = torch.stack(t + q, -1)
    stereo = torch.as_tensor(ii) == torch.as_tensor(jj)
    G[:, stereo] = torch.tensor(STEREO, dtype=f32)
    return G


def _grid(ht, wd):
    v, u = torch.meshgrid(torch.arange(ht, dtype=f32), torch.arange(wd, dtype=f32), indexing="ij")
    return u, v


def points32(poses, disps, intrinsics, ii, jj):
    """The float32 intermediates: X0 (x, y, 1), X1 (3 tuple) and D, each (B,E,ht,wd); G_ij (B,E,7); intrinsics of jj."""
    poses, disps, intrinsics = (torch.as_tensor(a, dtype=f32) for a in (poses, disps, intrinsics))
    ok, ic, jc, _ = _edges(poses, disps, intrinsics, ii, jj)
    ht, wd = disps.shape[2:]
    u, v = _grid(ht, wd)
    G = relative_poses32(poses, ic, jc)
    Ki, Kj = intrinsics[:, ic, :, None, None], intrinsics[:, jc, :, None, None]
    D = disps[:, ic]
    X0 = ((u - Ki[:, :, 2]) / Ki[:, :, 0], (v - Ki[:, :, 3]) / Ki[:, :, 1], torch.ones_like(D))
    g = [G[:, :, k, None, None] for k in range(7)]
    R = act_so3(g[3:], X0)
    X1 = tuple(R[k] + g[k] * D for k in range(3))
    return ok, X0, X1, D, g, Kj


def projective_transform32(poses, disps, intrinsics, ii, jj, jacobian=False, return_depth=False):
    """Float32 restatement of the kernel: the reference's return structure, torch CPU tensors."""
    ok, X0, X1, D, g, Kj = points32(poses, disps, intrinsics, ii, jj)
    fx, fy, cx, cy = (Kj[:, :, k] for k in range(4))
    X, Y, Zr = X1
    Z = torch.where(Zr < CLAMP_Z, torch.ones_like(Zr), Zr)
    d = torch.ones_like(Z) / Z
    cu = fx * (X * d) + cx
    cv = fy * (Y * d) + cy
    chans = [cu, cv] + ([D * d] if return_depth else [])
    coords = torch.stack(chans, -1)
    valid = ((Zr > MIN_DEPTH) & (X0[2] > MIN_DEPTH)).to(f32)[..., None]
    bad = ~ok
    coords[:, bad] = float("nan")
    valid[:, bad] = 0.0
    if not jacobian:
        return coords, valid
    a0, a2 = fx * d, ((-fx * X) * d) * d
    b1, b2 = fy * d, ((-fy * Y) * d) * d
    zero = torch.zeros_like(d)
    r0 = (a0 * D, zero, a2 * D, a2 * Y, a0 * Zr - a2 * X, -(a0 * Y))
    r1 = (zero, b1 * D, b2 * D, b2 * Y - b1 * Zr, -(b2 * X), b1 * X)
    t, q = g[:3], g[3:]
    qc = (-q[0], -q[1], -q[2], q[3])
    ji = []
    for r in (r0, r1):
        st = act_so3(qc, r[:3])
        w = _cross(r[:3], t)
        sr = act_so3(qc, tuple(r[3 + k] + w[k] for k in range(3)))
        ji.append(tuple(-c for c in st + sr))
    Jj = torch.stack([torch.stack(r0, -1), torch.stack(r1, -1)], -2)
    Ji = torch.stack([torch.stack(ji[0], -1), torch.stack(ji[1], -1)], -2)
    Jz = torch.stack([a0 * t[0] + a2 * t[2], b1 * t[1] + b2 * t[2]], -1)[..., None]
    for J in (Ji, Jj, Jz):
        J[:, bad] = float("nan")
    return coords, valid, (Ji, Jj, Jz)


def motion_features32(poses, disps, intrinsics, ii, jj, target, clamp=64.0):
    """FactorGraph.update's two lines on the float32 coordinates: (coords1, motn (B,E,4,ht,wd) contiguous)."""
    coords1, _ = projective_transform32(poses, disps, intrinsics, ii, jj)
    ht, wd = coords1.shape[2:4]
    u, v = _grid(ht, wd)
    coords0 = torch.stack([u, v], -1)
    target = torch.as_tensor(target, dtype=f32)
    motn = torch.cat([coords1 - coords0, target - coords1], dim=-1)
    motn = motn.permute(0, 1, 4, 2, 3).clamp(-clamp, clamp).contiguous()
    return coords1, motn


# ---- float64, plain math --------------------------------------------------------------------------------------------
def quat_matrix(q):
    """Rotation matrix of unit quaternions (...,4) = x, y, z, w."""
    x, y, z, w = q.unbind(-1)
    return torch.stack([
        1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w),
        2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
        2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], -1).reshape(q.shape[:-1] + (3, 3))


def pose_matrix(p):
    """(...,7) = t, q -> (...,4,4)."""
    p = torch.as_tensor(p, dtype=f64)
    T = torch.zeros(p.shape[:-1] + (4, 4), dtype=f64)
    T[..., :3, :3] = quat_matrix(p[..., 3:])
    T[..., :3, 3] = p[..., :3]
    T[..., 3, 3] = 1
    return T


def hat(v):
    x, y, z = v.unbind(-1)
    o = torch.zeros_like(x)
    return torch.stack([o, -z, y, z, o, -x, -y, x, o], -1).reshape(v.shape[:-1] + (3, 3))


def se3_exp(xi):
    """Exp of a twist (...,6) = (translation, rotation) as a 4x4 matrix."""
    A = torch.zeros(xi.shape[:-1] + (4, 4), dtype=f64)
    A[..., :3, :3] = hat(xi[..., 3:])
    A[..., :3, 3] = xi[..., :3]
    return torch.linalg.matrix_exp(A)


def adjoint(T):
    """Adj of SE3 in the (translation, rotation) tangent order: [[R, [t]x R], [0, R]]."""
    R, t = T[..., :3, :3], T[..., :3, 3]
    A = torch.zeros(T.shape[:-2] + (6, 6), dtype=f64)
    A[..., :3, :3] = R
    A[..., :3, 3:] = hat(t) @ R
    A[..., 3:, 3:] = R
    return A


def transform64(Gij, D, Ki, Kj, jacobian=False, return_depth=False):
    """Per-pixel math of projective_transform in float64.  Gij (B,E,4,4), D (B,E,ht,wd), Ki / Kj (B,E,4).  Returns
    coords, valid, X1 and, with `jacobian`, (Ji, Jj, Jz)."""
    ht, wd = D.shape[2:]
    v, u = torch.meshgrid(torch.arange(ht, dtype=f64), torch.arange(wd, dtype=f64), indexing="ij")
    k = lambda K, n: K[:, :, n, None, None]  # noqa: E731
    X0 = torch.stack([(u - k(Ki, 2)) / k(Ki, 0), (v - k(Ki, 3)) / k(Ki, 1), torch.ones_like(D), D], -1)
    X1 = (Gij[:, :, None, None] @ X0[..., None])[..., 0]
    X, Y, Zr = X1[..., 0], X1[..., 1], X1[..., 2]
    Z = torch.where(Zr < 0.1, torch.ones_like(Zr), Zr)
    d = 1 / Z
    chans = [k(Kj, 0) * X * d + k(Kj, 2), k(Kj, 1) * Y * d + k(Kj, 3)] + ([D * d] if return_depth else [])
    coords = torch.stack(chans, -1)
    valid = ((Zr > 0.2) & (X0[..., 2] > 0.2)).to(f64)[..., None]
    if not jacobian:
        return coords, valid, X1
    o = torch.zeros_like(d)
    fx, fy = k(Kj, 0) + o, k(Kj, 1) + o
    Jp = torch.stack([fx * d, o, -fx * X * d * d, o, o, fy * d, -fy * Y * d * d, o], -1).reshape(d.shape + (2, 4))
    W = X1[..., 3]
    Ja = torch.stack([W, o, o, o, Zr, -Y,
                      o, W, o, -Zr, o, X,
                      o, o, W, Y, -X, o,
                      o, o, o, o, o, o], -1).reshape(d.shape + (4, 6))
    Jj = Jp @ Ja
    Ji = -(Jj @ adjoint(Gij)[:, :, None, None])
    tz = torch.cat([Gij[:, :, :3, 3], torch.ones_like(Gij[:, :, :1, 3])], -1)
    Jz = Jp @ tz[:, :, None, None, :, None]
    return coords, valid, X1, (Ji, Jj, Jz)


def relative_matrices64(poses, ii, jj):
    """G_j G_i^-1 (B,E,4,4) in float64 from (B,N,7) poses; the stereo baseline where ii == jj."""
    T = pose_matrix(poses)
    ii, jj = torch.as_tensor(ii), torch.as_tensor(jj)
    G = T[:, jj] @ torch.linalg.inv(T[:, ii])
    G[:, ii == jj] = pose_matrix(torch.tensor(STEREO, dtype=f64))
    return G


def projective_transform64(poses, disps, intrinsics, ii, jj, jacobian=False, return_depth=False):
    """The float64 counterpart of projective_transform32 (valid indices only)."""
    disps, intrinsics = torch.as_tensor(disps, dtype=f64), torch.as_tensor(intrinsics, dtype=f64)
    ii, jj = torch.as_tensor(ii), torch.as_tensor(jj)
    G = relative_matrices64(poses, ii, jj)
    out = transform64(G, disps[:, ii], intrinsics[:, ii], intrinsics[:, jj], jacobian, return_depth)
    return out[:2] + out[3:] if jacobian else out[:2]
