"""SO3, SE3 and Sim3 group objects with the surface the reference's droid_slam uses of lietorch — without lietorch
(a CUDA extension with no build for this platform).  `install_dropins(lietorch=True)` serves this module as `lietorch`.

Conventions (the contract; real lietorch cannot be consulted here):

* `.data` is the stored tensor itself, last dimension = the element: SO3 `[qx,qy,qz,qw]` (4), SE3 `[tx,ty,tz,qx,qy,qz,qw]`
  (7), Sim3 `[t, q, s]` (8).  `G.data[:, mask] = v` writes through.  `shape` is `data.shape[:-1]`.
* Quaternions are used as given: never renormalised, never sign-flipped (real lietorch may normalise non-unit ones) — the
  same statement as `geom.projective_transform`'s.
* Tangents: SO3 `phi` (3), SE3 `[tau, phi]` (6, translation first), Sim3 `[tau, phi, sigma]` (7): the order
  `geom.projective_transform` emits for Ji and Jj.
* `matrix()` is (...,4,4) = `[[s R, t], [0, 1]]` for all three groups.
* `Group.exp(a)`: `matrix(exp(a))` is the matrix exponential of `hat(a) = [[sigma I + [phi]x, tau], [0, 0]]`, the
  quaternion `[sin(th/2) phi / th, cos(th/2)]` without sign normalisation.  `log` is the inverse with a rotation part of
  norm <= pi (q and -q give the same result).  Both are finite at every angle; `exp(0)` is the identity and
  `log(identity)` is 0, exactly.
* `G * H` (same group): Hamilton product, `t = t_G + s_G R_G t_H`.  `G.retr(a) = exp(a) * G`, bit for bit.
* `G * p` = `G.act(p)`: last dimension 3: `s R p + t`; 4: `(X,Y,Z,W) -> (s R XYZ + t W, W)`.
* `G.adj(a) = Adj(G) a`, `G.adjT(a) = Adj(G)^T a`, `Adj(G) a = vee(T hat(a) T^-1)`; SE3: `Adj = [[R, [t]x R], [0, R]]`.
* Batch dimensions of the two operands broadcast like torch tensors (`(B,E,1,1,1)` against `(B,E,ht,wd,2,6)`).

Where it runs: float32 tensors on the HIP device go through the kernels of csrc/liegroup.hip for SO3 and SE3 — inv, mul,
retr, exp, log, matrix: one launch each; act, adj, adjT: one streaming launch that reads the group operand from its
compact tensor whenever its broadcast dimensions are all trailing (`G[:, :, None, None] * X`), and from an expanded
contiguous copy otherwise (the slow path).  CPU tensors, float64 tensors on either device and every Sim3 operation go
through the torch composition in this module (the same formulas and series thresholds).  Mixed devices or dtypes raise
before anything is launched.  There is no autograd: an input that requires grad in grad mode is refused.
"""
import math

import torch

from ._host import check_no_grad, launch
from ._host import ptr as _ptr, stream as _stream

LIE_SO3, LIE_SE3 = 0, 1     # include/lgu_corr.h LGU_LIE_*


# ---- torch composition (any float dtype, any device) ----------------------------------------------------------------
def _cross(a, b):
    a, b = torch.broadcast_tensors(a, b)
    return torch.cross(a, b, dim=-1)


def _rot(q, X):
    """R(q) X = X + w (2 v x X) + v x (2 v x X)."""
    v, w = q[..., :3], q[..., 3:]
    uv = 2.0 * _cross(v, X)
    return X + w * uv + _cross(v, uv)


def _conj(q):
    return torch.cat([-q[..., :3], q[..., 3:]], -1)


def _qmul(a, b):
    a, b = torch.broadcast_tensors(a, b)
    ax, ay, az, aw = a.unbind(-1)
    bx, by, bz, bw = b.unbind(-1)
    return torch.stack([aw * bx + ax * bw + ay * bz - az * by,
                        aw * by + ay * bw + az * bx - ax * bz,
                        aw * bz + az * bw + ax * by - ay * bx,
                        aw * bw - ax * bx - ay * by - az * bz], -1)


def _so3_exp(phi):
    """(q, im) with im = sin(th/2) / th; series through th^4 for th^2 < 1e-4."""
    th2 = (phi * phi).sum(-1, keepdim=True)
    small = th2 < 1e-4
    th = torch.sqrt(torch.where(small, torch.ones_like(th2), th2))
    im = torch.where(small, 0.5 - th2 * (1.0 / 48.0) + th2 * th2 * (1.0 / 3840.0), torch.sin(0.5 * th) / th)
    re = torch.where(small, 1.0 - th2 * (1.0 / 8.0) + th2 * th2 * (1.0 / 384.0), torch.cos(0.5 * th))
    return torch.cat([im * phi, re], -1), im


def _so3_log(q):
    s = torch.where(q[..., 3:] < 0, -torch.ones_like(q[..., 3:]), torch.ones_like(q[..., 3:]))
    v, w = s * q[..., :3], s * q[..., 3:]
    n2 = (v * v).sum(-1, keepdim=True)
    small = n2 < 1e-4 * (w * w)
    x2 = n2 / (w * w)
    n = torch.sqrt(torch.where(small, torch.ones_like(n2), n2))
    k = torch.where(small, (2.0 / w) * (1.0 - x2 * (1.0 / 3.0) + x2 * x2 * (1.0 / 5.0) - x2 * x2 * x2 * (1.0 / 7.0)),
                    2.0 * torch.atan2(n, w) / n)
    return k * v


def _coef_c(th2):
    """(th - sin th) / th^3; series through th^6 for th^2 < 1e-2."""
    small = th2 < 1e-2
    th = torch.sqrt(torch.where(small, torch.ones_like(th2), th2))
    return torch.where(small, 1.0 / 6.0 - th2 * (1.0 / 120.0) + th2 * th2 * (1.0 / 5040.0) - th2 * th2 * th2 * (1.0 / 362880.0),
                       (th - torch.sin(th)) / (th2 * th))


def _coef_d(th2):
    """(1 - (th/2) cot(th/2)) / th^2; series through th^6 for th^2 < 1e-2."""
    small = th2 < 1e-2
    safe = torch.where(small, torch.ones_like(th2), th2)
    h = 0.5 * torch.sqrt(safe)
    return torch.where(small, 1.0 / 12.0 + th2 * (1.0 / 720.0) + th2 * th2 * (1.0 / 30240.0) + th2 * th2 * th2 * (1.0 / 1209600.0),
                       (1.0 - h * torch.cos(h) / torch.sin(h)) / safe)


def _se3_exp(a):
    tau, phi = a[..., :3], a[..., 3:6]
    q, im = _so3_exp(phi)
    th2 = (phi * phi).sum(-1, keepdim=True)
    c1 = _cross(phi, tau)
    c2 = _cross(phi, c1)
    return torch.cat([tau + (2.0 * (im * im)) * c1 + _coef_c(th2) * c2, q], -1)


def _se3_log(g):
    t, q = g[..., :3], g[..., 3:7]
    phi = _so3_log(q)
    th2 = (phi * phi).sum(-1, keepdim=True)
    c1 = _cross(phi, t)
    c2 = _cross(phi, c1)
    return torch.cat([t - 0.5 * c1 + _coef_d(th2) * c2, phi], -1)


def _hat3(v):
    x, y, z = v.unbind(-1)
    o = torch.zeros_like(x)
    return torch.stack([o, -z, y, z, o, -x, -y, x, o], -1).reshape(v.shape[:-1] + (3, 3))


def _sim3_w(phi, sigma):
    """W = int_0^1 exp(s (sigma I + [phi]x)) ds, the block that maps tau to the translation of exp: the upper right
    3x3 block of the matrix exponential of [[M, I], [0, 0]], M = sigma I + [phi]x (exact at every angle and scale)."""
    M = _hat3(phi) + sigma[..., None] * torch.eye(3, dtype=phi.dtype, device=phi.device)
    A = torch.zeros(phi.shape[:-1] + (6, 6), dtype=phi.dtype, device=phi.device)
    A[..., :3, :3] = M
    A[..., :3, 3:] = torch.eye(3, dtype=phi.dtype, device=phi.device)
    return torch.linalg.matrix_exp(A)[..., :3, 3:]


def _sim3_exp(a):
    tau, phi, sigma = a[..., :3], a[..., 3:6], a[..., 6:7]
    q, _ = _so3_exp(phi)
    t = (_sim3_w(phi, sigma) @ tau[..., None])[..., 0]
    return torch.cat([t, q, torch.exp(sigma)], -1)


def _sim3_log(g):
    t, q, s = g[..., :3], g[..., 3:7], g[..., 7:8]
    phi = _so3_log(q)
    sigma = torch.log(s)
    r0, r1, r2 = _sim3_w(phi, sigma).unbind(-2)      # W^-1 t by the adjugate: no device solver involved
    c0, c1, c2 = _cross(r1, r2), _cross(r2, r0), _cross(r0, r1)
    det = (r0 * c0).sum(-1, keepdim=True)
    tau = (c0 * t[..., 0:1] + c1 * t[..., 1:2] + c2 * t[..., 2:3]) / det
    return torch.cat([tau, phi, sigma], -1)


# ---- argument checks and broadcasting -------------------------------------------------------------------------------
def _same_kind(what, *tensors):
    """Mixed devices or dtypes raise before anything is launched."""
    first = tensors[0]
    for t in tensors[1:]:
        if t.dtype != first.dtype:
            raise RuntimeError("%s: operands have different dtypes (%s and %s)" % (what, first.dtype, t.dtype))
        if t.device != first.device:
            raise RuntimeError("%s: operands are on different devices (%s and %s)" % (what, first.device, t.device))
    check_no_grad("lie.%s" % what, [(t, "operand") for t in tensors])


def _on_hip(t):
    return t.is_cuda and t.dtype == torch.float32


def _compact(gshape, bshape):
    """g_div if the group operand's broadcast dimensions are all trailing in the broadcast batch shape, else None.
    gshape is aligned to bshape from the right; g_div = the product of the trailing dimensions where it has size 1."""
    gs = (1,) * (len(bshape) - len(gshape)) + tuple(gshape)
    k = 0
    for d, n in enumerate(gs):
        if n != 1:
            k = d + 1
    if any(gs[d] != bshape[d] for d in range(k)):
        return None
    return int(math.prod(bshape[k:]))


class _Group:
    """Common container surface; SO3, SE3 and Sim3 below set the sizes and the composition."""
    _K = 0          # element size
    _T = 0          # tangent size
    _QW = 0         # index of qw in the element
    _code = None    # LGU_LIE_* for the groups with kernels

    manifold_dim = 0    # lietorch's names for _T and _K, on the class and on every object
    embedded_dim = 0    # (droid_slam/geom/ba.py reads poses.manifold_dim)

    def __init__(self, data):
        if isinstance(data, _Group):
            data = data.data
        if not isinstance(data, torch.Tensor):
            raise TypeError("%s expects a tensor, got %s" % (type(self).__name__, type(data).__name__))
        if data.dim() < 1 or data.shape[-1] != self._K:
            raise ValueError("%s data must have last dimension %d, got shape %s"
                             % (type(self).__name__, self._K, tuple(data.shape)))
        if not data.is_floating_point():
            raise TypeError("%s data must be a floating-point tensor, got %s" % (type(self).__name__, data.dtype))
        self.data = data

    # -- construction ---------------------------------------------------------------------------------------------
    @classmethod
    def Identity(cls, *batch, device=None, dtype=None):
        if len(batch) == 1 and isinstance(batch[0], (tuple, list, torch.Size)):
            batch = tuple(batch[0])
        data = torch.zeros(tuple(batch) + (cls._K,), device=device, dtype=dtype or torch.float32)
        data[..., cls._QW:] = 1.0     # qw, and the scale of Sim3 behind it
        return cls(data)

    @classmethod
    def InitFromVec(cls, data):
        return cls(data)

    def vec(self):
        return self.data

    # -- container ------------------------------------------------------------------------------------------------
    @property
    def shape(self):
        return self.data.shape[:-1]

    @property
    def device(self):
        return self.data.device

    @property
    def dtype(self):
        return self.data.dtype

    def view(self, *batch):
        if len(batch) == 1 and isinstance(batch[0], (tuple, list, torch.Size)):
            batch = tuple(batch[0])
        return type(self)(self.data.view(tuple(batch) + (self._K,)))

    def _index(self, index):
        """Indices address batch dimensions only: the element dimension is kept whole."""
        index = index if isinstance(index, tuple) else (index,)
        if not any(i is Ellipsis for i in index):
            index = index + (Ellipsis,)
        return index + (slice(None),)

    def __getitem__(self, index):
        return type(self)(self.data[self._index(index)])

    def __setitem__(self, index, item):
        if isinstance(item, _Group):
            if type(item) is not type(self):
                raise TypeError("cannot assign a %s into a %s" % (type(item).__name__, type(self).__name__))
            item = item.data
        self.data[self._index(index)] = item

    def to(self, *args, **kwargs):
        return type(self)(self.data.to(*args, **kwargs))

    def cpu(self):
        return type(self)(self.data.cpu())

    def cuda(self, *args, **kwargs):
        return type(self)(self.data.cuda(*args, **kwargs))

    def float(self):
        return type(self)(self.data.float())

    def double(self):
        return type(self)(self.data.double())

    def detach(self):
        return type(self)(self.data.detach())

    def __repr__(self):
        return "%s: size=%s, device=%s, dtype=%s" % (type(self).__name__, tuple(self.shape), self.device, self.dtype)

    # -- per-element operations -----------------------------------------------------------------------------------
    def _elem(self, name, others, out_last, compose):
        """One per-element operation: `others` are (tensor, last dimension) operands with this object's batch shape
        after broadcasting; out_last the output's last dimension(s)."""
        tensors = [self.data] + [o for o, _ in others]
        _same_kind(name, *tensors)
        for o, last in others:
            if o.dim() < 1 or o.shape[-1] != last:
                raise ValueError("%s.%s: operand must have last dimension %d, got shape %s"
                                 % (type(self).__name__, name, last, tuple(o.shape)))
        if self._code is None or not _on_hip(self.data):
            return compose()
        batch = torch.broadcast_shapes(*[tuple(t.shape[:-1]) for t in tensors])
        flat = [t.expand(batch + t.shape[-1:]).contiguous() for t in tensors]
        out = torch.empty(batch + out_last, dtype=torch.float32, device=self.data.device)
        n = int(math.prod(batch))
        if n > 0:
            launch("lgu_lie_%s_f32" % name, "lie.%s" % name, self.data.device, self._code, *[_ptr(t) for t in flat], n, _ptr(out),
                   _stream(out))
        return out

    def inv(self):
        return type(self)(self._elem("inv", [], (self._K,), lambda: self._inv(self.data)))

    def log(self):
        return self._elem("log", [], (self._T,), lambda: self._log(self.data))

    def matrix(self):
        return self._elem("matrix", [], (4, 4), lambda: self._matrix(self.data))

    def mul(self, other):
        if type(other) is not type(self):
            raise TypeError("%s * %s is not a group product" % (type(self).__name__, type(other).__name__))
        return type(self)(self._elem("mul", [(other.data, self._K)], (self._K,), lambda: self._mul(self.data, other.data)))

    def retr(self, a):
        """exp(a) * self: the left update of bundle adjustment."""
        return type(self)(self._elem("retr", [(a, self._T)], (self._K,),
                                     lambda: self._mul(self._exp(a), self.data)))

    @classmethod
    def exp(cls, a):
        if not isinstance(a, torch.Tensor) or not a.is_floating_point() or a.dim() < 1 or a.shape[-1] != cls._T:
            raise ValueError("%s.exp expects a floating-point tensor with last dimension %d" % (cls.__name__, cls._T))
        check_no_grad("lie.exp", [(a, "a")])
        if cls._code is None or not _on_hip(a):
            return cls(cls._exp(a))
        ac = a.contiguous()
        out = torch.empty(a.shape[:-1] + (cls._K,), dtype=torch.float32, device=a.device)
        n = int(math.prod(a.shape[:-1]))
        if n > 0:
            launch("lgu_lie_exp_f32", "lie.exp", a.device, cls._code, _ptr(ac), n, _ptr(out), _stream(out))
        return cls(out)

    # -- broadcast operations -------------------------------------------------------------------------------------
    def _bcast(self, name, x, widths, entry, flag, compose):
        if not isinstance(x, torch.Tensor):
            raise TypeError("%s.%s expects a tensor, got %s" % (type(self).__name__, name, type(x).__name__))
        if x.dim() < 1 or x.shape[-1] not in widths:
            raise ValueError("%s.%s: operand must have last dimension %s, got shape %s"
                             % (type(self).__name__, name, " or ".join(str(w) for w in widths), tuple(x.shape)))
        _same_kind(name, self.data, x)
        width = x.shape[-1]
        bshape = torch.broadcast_shapes(tuple(self.shape), tuple(x.shape[:-1]))
        if self._code is None or not _on_hip(x):
            return compose(self.data, x)
        G = self.data
        g_div = _compact(self.shape, bshape)
        if g_div is None:                         # slow path: a non-trailing broadcast of G is expanded first
            G = G.expand(bshape + (self._K,))
            g_div = 1
        G = G.contiguous()
        xc = x.expand(bshape + (width,)).contiguous()
        out = torch.empty(bshape + (width,), dtype=torch.float32, device=x.device)
        rows = int(math.prod(bshape))
        if rows > 0:
            ng = G.numel() // self._K
            launch(entry, "lie.%s" % name, x.device, self._code, _ptr(G), ng, _ptr(xc), flag if flag is not None else width, rows,
                   g_div, _ptr(out), _stream(out))
        return out

    def act(self, p):
        return self._bcast("act", p, (3, 4), "lgu_lie_act_f32", None, self._act)

    def adj(self, a):
        return self._bcast("adj", a, (self._T,), "lgu_lie_adj_f32", 0, self._adj)

    def adjT(self, a):
        return self._bcast("adjT", a, (self._T,), "lgu_lie_adj_f32", 1, self._adjT)

    def __mul__(self, other):
        if isinstance(other, _Group):
            return self.mul(other)
        if isinstance(other, torch.Tensor):
            return self.act(other)
        return NotImplemented


class SO3(_Group):
    _K, _T, _QW, _code = 4, 3, 3, LIE_SO3
    manifold_dim, embedded_dim = _T, _K

    @staticmethod
    def _inv(g):
        return _conj(g)

    @staticmethod
    def _mul(g, h):
        return _qmul(g, h)

    @staticmethod
    def _exp(a):
        return _so3_exp(a)[0]

    @staticmethod
    def _log(g):
        return _so3_log(g)

    @staticmethod
    def _matrix(g):
        return _matrix(torch.zeros_like(g[..., :3]), g, None)

    @staticmethod
    def _act(g, p):
        r = _rot(g, p[..., :3])
        return r if p.shape[-1] == 3 else torch.cat([r, p[..., 3:].expand(r.shape[:-1] + (1,))], -1)

    @staticmethod
    def _adj(g, a):
        return _rot(g, a)

    @staticmethod
    def _adjT(g, a):
        return _rot(_conj(g), a)


class SE3(_Group):
    _K, _T, _QW, _code = 7, 6, 6, LIE_SE3
    manifold_dim, embedded_dim = _T, _K

    @staticmethod
    def _inv(g):
        qi = _conj(g[..., 3:7])
        return torch.cat([-_rot(qi, g[..., :3]), qi], -1)

    @staticmethod
    def _mul(g, h):
        return torch.cat([g[..., :3] + _rot(g[..., 3:7], h[..., :3]), _qmul(g[..., 3:7], h[..., 3:7])], -1)

    @staticmethod
    def _exp(a):
        return _se3_exp(a)

    @staticmethod
    def _log(g):
        return _se3_log(g)

    @staticmethod
    def _matrix(g):
        return _matrix(g[..., :3], g[..., 3:7], None)

    @staticmethod
    def _act(g, p):
        r = _rot(g[..., 3:7], p[..., :3])
        if p.shape[-1] == 3:
            return r + g[..., :3]
        w = p[..., 3:]
        return torch.cat([r + g[..., :3] * w, w.expand(r.shape[:-1] + (1,))], -1)

    @staticmethod
    def _adj(g, a):
        t, q = g[..., :3], g[..., 3:7]
        rt, rp = _rot(q, a[..., :3]), _rot(q, a[..., 3:])
        return torch.cat([rt + _cross(t, rp), rp], -1)

    @staticmethod
    def _adjT(g, a):
        t, qc = g[..., :3], _conj(g[..., 3:7])
        tau, phi = a[..., :3], a[..., 3:]
        return torch.cat([_rot(qc, tau), _rot(qc, phi + _cross(tau, t))], -1)


class Sim3(_Group):
    """Similarity transforms.  Every operation is the torch composition, on either device: no inference path of the
    reference uses Sim3."""
    _K, _T, _QW, _code = 8, 7, 6, None
    manifold_dim, embedded_dim = _T, _K

    @staticmethod
    def _inv(g):
        qi = _conj(g[..., 3:7])
        si = 1.0 / g[..., 7:8]
        return torch.cat([-(si * _rot(qi, g[..., :3])), qi, si], -1)

    @staticmethod
    def _mul(g, h):
        return torch.cat([g[..., :3] + g[..., 7:8] * _rot(g[..., 3:7], h[..., :3]), _qmul(g[..., 3:7], h[..., 3:7]),
                          g[..., 7:8] * h[..., 7:8]], -1)

    @staticmethod
    def _exp(a):
        return _sim3_exp(a)

    @staticmethod
    def _log(g):
        return _sim3_log(g)

    @staticmethod
    def _matrix(g):
        return _matrix(g[..., :3], g[..., 3:7], g[..., 7:8])

    @staticmethod
    def _act(g, p):
        r = g[..., 7:8] * _rot(g[..., 3:7], p[..., :3])
        if p.shape[-1] == 3:
            return r + g[..., :3]
        w = p[..., 3:]
        return torch.cat([r + g[..., :3] * w, w.expand(r.shape[:-1] + (1,))], -1)

    @staticmethod
    def _adj(g, a):
        """vee(T hat(a) T^-1): (s R tau + t x (R phi) - sigma t, R phi, sigma)."""
        t, q, s = g[..., :3], g[..., 3:7], g[..., 7:8]
        tau, phi, sigma = a[..., :3], a[..., 3:6], a[..., 6:7]
        rp = _rot(q, phi)
        return torch.cat([s * _rot(q, tau) + _cross(t, rp) - sigma * t, rp, sigma + torch.zeros_like(rp[..., :1])], -1)

    @staticmethod
    def _adjT(g, a):
        """The transpose of the matrix of _adj: (s R^T tau, R^T (phi + tau x t), sigma - t . tau)."""
        t, q, s = g[..., :3], g[..., 3:7], g[..., 7:8]
        qc = _conj(q)
        tau, phi, sigma = a[..., :3], a[..., 3:6], a[..., 6:7]
        return torch.cat([s * _rot(qc, tau), _rot(qc, phi + _cross(tau, t)),
                          sigma - (t * tau).sum(-1, keepdim=True)], -1)


def _matrix(t, q, s):
    x, y, z, w = q.unbind(-1)
    R = torch.stack([1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y - z * w), 2.0 * (x * z + y * w),
                     2.0 * (x * y + z * w), 1.0 - 2.0 * (x * x + z * z), 2.0 * (y * z - x * w),
                     2.0 * (x * z - y * w), 2.0 * (y * z + x * w), 1.0 - 2.0 * (x * x + y * y)], -1).reshape(q.shape[:-1] + (3, 3))
    if s is not None:
        R = s[..., None] * R
    M = torch.zeros(q.shape[:-1] + (4, 4), dtype=q.dtype, device=q.device)
    M[..., :3, :3] = R
    M[..., :3, 3] = t
    M[..., 3, 3] = 1.0
    return M


def _joined(fn, what, groups, dim):
    groups = list(groups)
    if not groups or not all(type(g) is type(groups[0]) and isinstance(g, _Group) for g in groups):
        raise TypeError("lie.%s expects a non-empty list of objects of one group" % what)
    nb = len(groups[0].shape) + (1 if what == "stack" else 0)
    if not -nb <= dim < nb:
        raise IndexError("lie.%s: dim %d is outside the %d batch dimensions" % (what, dim, nb))
    return type(groups[0])(fn([g.data for g in groups], dim if dim >= 0 else dim + nb))


def cat(groups, dim=0):
    """Concatenate group objects along a batch dimension."""
    return _joined(torch.cat, "cat", groups, dim)


def stack(groups, dim=0):
    """Stack group objects along a new batch dimension."""
    return _joined(torch.stack, "stack", groups, dim)
