"""Restatements of the SO3 / SE3 / Sim3 operations of lgu_slam_amd.lie.  TEST INFRASTRUCTURE ONLY: nothing here imports
the product.

Two forms:

(a) `truth_*`: float64 from the definitions.  An element is its 4x4 matrix [[s R, t], [0, 1]]; exp is
    torch.linalg.matrix_exp of hat(a) = [[sigma I + [phi]x, tau], [0, 0]]; mul, inv and act are matrix algebra; adj is
    vee(T hat(a) T^-1) and adjT the transpose of the matrix that adj defines; log is checked as the inverse of exp.
(b) `exp`, `log`, `mul`, `inv`, `act`, `adj`, `adjT`, `matrix`: closed forms in plain math (rotation matrices, Rodrigues'
    coefficients, the Hamilton product), computed in the dtype of their inputs.  Run in float64 they are held to (a); run
    in float32 their distance from float64 sets the tolerance of the float32 product (tests/test_lie.py).

Data layout: SO3 q = (x, y, z, w); SE3 (t, q); Sim3 (t, q, s).  Tangents: phi; (tau, phi); (tau, phi, sigma).
Quaternions are used as given.  The closed forms switch to two-term series below an angle of 1e-4 (truncation below
1e-17); the Sim3 coefficients are the closed forms away from zero only: they need |phi| >= 0.05 and |sigma| >= 0.05.
"""
import torch

f32, f64 = torch.float32, torch.float64
GROUPS = ("SO3", "SE3", "Sim3")
K = {"SO3": 4, "SE3": 7, "Sim3": 8}        # element size
T = {"SO3": 3, "SE3": 6, "Sim3": 7}        # tangent size


# ---- shared pieces --------------------------------------------------------------------------------------------------
def split(group, g):
    """(t, q, s) of element data; t = 0 for SO3, s = 1 for SO3 and SE3."""
    if group == "SO3":
        return torch.zeros_like(g[..., :3]), g, torch.ones_like(g[..., :1])
    if group == "SE3":
        return g[..., :3], g[..., 3:7], torch.ones_like(g[..., :1])
    return g[..., :3], g[..., 3:7], g[..., 7:8]


def join(group, t, q, s):
    return {"SO3": lambda: q, "SE3": lambda: torch.cat([t, q], -1), "Sim3": lambda: torch.cat([t, q, s], -1)}[group]()


def split_tangent(group, a):
    """(tau, phi, sigma)."""
    if group == "SO3":
        return torch.zeros_like(a), a, torch.zeros_like(a[..., :1])
    if group == "SE3":
        return a[..., :3], a[..., 3:6], torch.zeros_like(a[..., :1])
    return a[..., :3], a[..., 3:6], a[..., 6:7]


def join_tangent(group, tau, phi, sigma):
    return {"SO3": lambda: phi, "SE3": lambda: torch.cat([tau, phi], -1),
            "Sim3": lambda: torch.cat([tau, phi, sigma], -1)}[group]()


def cross_matrix(v):
    x, y, z = v.unbind(-1)
    o = torch.zeros_like(x)
    return torch.stack([o, -z, y, z, o, -x, -y, x, o], -1).reshape(v.shape[:-1] + (3, 3))


def rotation(q):
    x, y, z, w = q.unbind(-1)
    return torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w),
                        2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                        2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], -1).reshape(q.shape[:-1] + (3, 3))


def matrix(group, g):
    """(...,4,4) = [[s R, t], [0, 1]] in g's dtype."""
    t, q, s = split(group, g)
    M = torch.zeros(g.shape[:-1] + (4, 4), dtype=g.dtype)
    M[..., :3, :3] = s[..., None] * rotation(q)
    M[..., :3, 3] = t
    M[..., 3, 3] = 1
    return M


def mv(M, v):
    return (M @ v[..., None])[..., 0]


# ---- (a) float64 from the definitions -----------------------------------------------------------------------------
def hat(group, a):
    tau, phi, sigma = split_tangent(group, a)
    A = torch.zeros(a.shape[:-1] + (4, 4), dtype=a.dtype)
    A[..., :3, :3] = cross_matrix(phi) + sigma[..., None] * torch.eye(3, dtype=a.dtype)
    A[..., :3, 3] = tau
    return A


def vee(group, A):
    tau = A[..., :3, 3]
    phi = torch.stack([A[..., 2, 1] - A[..., 1, 2], A[..., 0, 2] - A[..., 2, 0], A[..., 1, 0] - A[..., 0, 1]], -1) / 2
    sigma = (A[..., 0, 0] + A[..., 1, 1] + A[..., 2, 2])[..., None] / 3
    return join_tangent(group, tau, phi, sigma)


def truth_exp_matrix(group, a):
    return torch.linalg.matrix_exp(hat(group, a.to(f64)))


def truth_mul_matrix(group, g, h):
    return matrix(group, g.to(f64)) @ matrix(group, h.to(f64))


def truth_inv_matrix(group, g):
    return torch.linalg.inv(matrix(group, g.to(f64)))


def truth_act(group, g, p):
    """p (...,3) or (...,4); the batch dimensions broadcast."""
    p = p.to(f64)
    M = matrix(group, g.to(f64))
    if p.shape[-1] == 4:
        return mv(M, p)
    return mv(M, torch.cat([p, torch.ones_like(p[..., :1])], -1))[..., :3]


def truth_adj(group, g, a):
    M = matrix(group, g.to(f64))
    return vee(group, M @ hat(group, a.to(f64)) @ torch.linalg.inv(M))


def truth_adj_matrix(group, g):
    """Adj(G) (...,T,T): column k = adj of the k-th basis tangent."""
    n = T[group]
    cols = [truth_adj(group, g, torch.eye(n, dtype=f64)[k].expand(g.shape[:-1] + (n,))) for k in range(n)]
    return torch.stack(cols, -1)


def truth_adjT(group, g, a):
    return mv(truth_adj_matrix(group, g).transpose(-1, -2), a.to(f64))


# ---- (b) closed forms, in the dtype of the inputs -------------------------------------------------------------------
SMALL = 1e-4


def quat_product(a, b):
    ax, ay, az, aw = a.unbind(-1)
    bx, by, bz, bw = b.unbind(-1)
    return torch.stack([aw * bx + ax * bw + ay * bz - az * by,
                        aw * by - ax * bz + ay * bw + az * bx,
                        aw * bz + ax * by - ay * bx + az * bw,
                        aw * bw - ax * bx - ay * by - az * bz], -1)


def mul(group, g, h):
    tg, qg, sg = split(group, g)
    th, qh, sh = split(group, h)
    return join(group, tg + sg * mv(rotation(qg), th), quat_product(qg, qh), sg * sh)


def inv(group, g):
    t, q, s = split(group, g)
    qi = torch.cat([-q[..., :3], q[..., 3:]], -1)
    return join(group, -mv(rotation(q).transpose(-1, -2), t) / s, qi, 1 / s)


def act(group, g, p):
    t, q, s = split(group, g)
    r = s * mv(rotation(q), p[..., :3])
    if p.shape[-1] == 3:
        return r + t
    w = p[..., 3:]
    return torch.cat([r + t * w, w + torch.zeros_like(r[..., :1])], -1)


def adj_matrix(group, g):
    """SO3: R; SE3: [[R, [t]x R], [0, R]]; Sim3: [[s R, [t]x R, -t], [0, R, 0], [0, 0, 1]]."""
    t, q, s = split(group, g)
    R = rotation(q)
    if group == "SO3":
        return R
    n = T[group]
    A = torch.zeros(g.shape[:-1] + (n, n), dtype=g.dtype)
    A[..., :3, :3] = s[..., None] * R
    A[..., :3, 3:6] = cross_matrix(t) @ R
    A[..., 3:6, 3:6] = R
    if group == "Sim3":
        A[..., :3, 6] = -t
        A[..., 6, 6] = 1
    return A


def adj(group, g, a):
    return mv(adj_matrix(group, g), a)


def adjT(group, g, a):
    return mv(adj_matrix(group, g).transpose(-1, -2), a)


def _rotation_exp(phi):
    """q = [sin(th/2) phi / th, cos(th/2)] and Rodrigues' B = (1 - cos th) / th^2 = 2 (sin(th/2) / th)^2."""
    th = phi.norm(dim=-1, keepdim=True)
    small = th < SMALL
    ths = torch.where(small, torch.ones_like(th), th)
    im = torch.where(small, 0.5 - th * th / 48, torch.sin(ths / 2) / ths)
    re = torch.where(small, 1 - th * th / 8, torch.cos(ths / 2))
    return torch.cat([im * phi, re], -1), th, 2 * im * im


def _sim3_w(phi, sigma):
    """W of Sim3's exp (the closed form for theta and sigma away from 0): A [phi]x + B [phi]x^2 + C I."""
    th = phi.norm(dim=-1, keepdim=True)
    assert float(th.min()) >= 0.05 and float(sigma.abs().min()) >= 0.05, "outside the closed form's domain"
    es = torch.exp(sigma)
    a, b, c = es * torch.sin(th), es * torch.cos(th), th * th + sigma * sigma
    C = (es - 1) / sigma
    A = (a * sigma + (1 - b) * th) / (th * c)
    B = (C - ((b - 1) * sigma + a * th) / c) / (th * th)
    P = cross_matrix(phi)
    return A[..., None] * P + B[..., None] * (P @ P) + C[..., None] * torch.eye(3, dtype=phi.dtype)


def exp(group, a):
    tau, phi, sigma = split_tangent(group, a)
    q, th, B = _rotation_exp(phi)
    if group == "Sim3":
        return join(group, mv(_sim3_w(phi, sigma), tau), q, torch.exp(sigma))
    small = th < SMALL
    ths = torch.where(small, torch.ones_like(th), th)
    C = torch.where(small, 1 / 6 - th * th / 120, (ths - torch.sin(ths)) / (ths * ths * ths))
    P = cross_matrix(phi)
    V = torch.eye(3, dtype=a.dtype) + B[..., None] * P + C[..., None] * (P @ P)
    return join(group, mv(V, tau), q, torch.ones_like(th))


def _rotation_log(q):
    flip = torch.where(q[..., 3:] < 0, -torch.ones_like(q[..., 3:]), torch.ones_like(q[..., 3:]))
    v, w = flip * q[..., :3], flip * q[..., 3:]
    n = v.norm(dim=-1, keepdim=True)
    small = n < SMALL * w
    ns = torch.where(small, torch.ones_like(n), n)
    x = n / w
    return torch.where(small, (2 / w) * (1 - x * x / 3), 2 * torch.atan2(ns, w) / ns) * v


def log(group, g):
    t, q, s = split(group, g)
    phi = _rotation_log(q)
    if group == "SO3":
        return phi
    if group == "Sim3":
        sigma = torch.log(s)
        return join_tangent(group, mv(torch.linalg.inv(_sim3_w(phi, sigma)), t), phi, sigma)
    th = phi.norm(dim=-1, keepdim=True)
    small = th < SMALL
    ths = torch.where(small, torch.ones_like(th), th)
    D = torch.where(small, 1 / 12 + th * th / 720, (1 - (ths / 2) * torch.cos(ths / 2) / torch.sin(ths / 2)) / (ths * ths))
    P = cross_matrix(phi)
    Vinv = torch.eye(3, dtype=g.dtype) - P / 2 + D[..., None] * (P @ P)
    return join_tangent(group, mv(Vinv, t), phi, torch.zeros_like(th))


def retr(group, g, a):
    return mul(group, exp(group, a), g)


# ---- inputs ---------------------------------------------------------------------------------------------------------
def _axes(shape, gen):
    return torch.nn.functional.normalize(torch.randn(shape + (3,), generator=gen, dtype=f64), dim=-1)


def tangents(group, shape, seed, max_angle=3.0, min_angle=0.0, dtype=f32):
    """tau of order 1, |phi| uniform in [min_angle, max_angle], |sigma| in [0.05, log 2] with either sign."""
    shape = tuple(shape)
    gen = torch.Generator().manual_seed(seed)
    tau = torch.randn(shape + (3,), generator=gen, dtype=f64)
    ang = min_angle + (max_angle - min_angle) * torch.rand(shape + (1,), generator=gen, dtype=f64)
    phi = _axes(shape, gen) * ang
    mag = 0.05 + (0.693 - 0.05) * torch.rand(shape + (1,), generator=gen, dtype=f64)
    sigma = mag * torch.where(torch.rand(shape + (1,), generator=gen) < 0.5, -1.0, 1.0)
    return join_tangent(group, tau, phi, sigma).to(dtype)


def elements(group, shape, seed, max_angle=3.0, min_angle=0.0, dtype=f32, flip=True):
    """Translations of order 1, unit quaternions (to the rounding of `dtype`) of angle in [min_angle, max_angle], half
    of them written as -q when `flip`, scales in [0.5, 2]."""
    shape = tuple(shape)
    gen = torch.Generator().manual_seed(seed)
    t = torch.randn(shape + (3,), generator=gen, dtype=f64)
    ang = min_angle + (max_angle - min_angle) * torch.rand(shape + (1,), generator=gen, dtype=f64)
    q = torch.cat([torch.sin(ang / 2) * _axes(shape, gen), torch.cos(ang / 2)], -1)
    if flip:
        q = q * torch.where(torch.rand(shape + (1,), generator=gen) < 0.5, -1.0, 1.0)
    s = torch.exp(tangents("Sim3", shape, seed + 1000)[..., 6:7].to(f64))
    return join(group, t, q, s).to(dtype)
