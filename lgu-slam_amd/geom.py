"""The geometry entries of the reference's `droid_backends` (src/droid.cpp:237-249 -> src/droid_kernels.cu:427-851,
1436-1541): `frame_distance`, `projmap`, `depth_filter` and `iproj`, on the HIP kernels of csrc/geom.hip.

Same positional arguments and return types as the reference (a tensor; a list for projmap).  poses (Np,7) float32 as
t, q(xyzw); disps (Nd,ht,wd) float32; intrinsics 1-D float32 with fx, fy, cx, cy first; index tensors int64.  Every
input must be contiguous and live on a HIP device.  Per-pixel values are bit-identical to the reference's fp32
arithmetic; frame_distance sums its pixels in a fixed order of its own (independent of the batch).

`poses` may have fewer rows than `disps` has frames (DepthVideo.distance passes poses[:counter] with the whole
buffer).  A frame index is valid when 0 <= index < min(Np, Nd); where the reference would read out of bounds, the
result is NaN (frame_distance), NaN coordinates with channel 2 = 0 and valid = 0 (projmap), a zero row (depth_filter;
an invalid neighbour is skipped) or NaN points (iproj, frames without a pose).

Kernels are enqueued on the current stream of the inputs' device, without host synchronisation (graph-capturable).
"""
import torch

from . import _lib
from .ops import _TORCH_NAME, _ptr, _stream


def _check_inputs(*named):
    """_check_inputs(poses, "poses", ..., ii, "ii"): CHECK_INPUT (src/droid.cpp:84-85, "x must be contiguous") on every
    argument in the reference's order, then the dtypes of the reference's accessors: float32 data, int64 (`long`)
    indices — an argument named ii, jj or ix is an index.  Returns the pairs for _check_device, which runs after the
    shape checks: every argument error is raised before anything is launched, and without a device."""
    pairs = list(zip(named[0::2], named[1::2]))
    for t, name in pairs:
        if not t.is_contiguous():
            raise RuntimeError("%s must be contiguous" % name)
    for t, name in pairs:
        want = torch.int64 if name in _INDEX_NAMES else torch.float32
        if t.dtype != want:
            raise RuntimeError("expected scalar type %s but found %s (%s)" % (_TORCH_NAME[want], _TORCH_NAME.get(t.dtype, str(t.dtype)),
                                                                         name))
    return pairs


def _check_device(pairs):
    for t, name in pairs:
        if not t.is_cuda:
            raise RuntimeError("%s must be a HIP device tensor: lgu_slam_amd has no CPU fallback" % name)
    for t, name in pairs:
        if t.device != pairs[0][0].device:
            raise RuntimeError("%s is on %s, expected %s" % (name, t.device, pairs[0][0].device))


_INDEX_NAMES = ("ii", "jj", "ix")


def _check_geometry(poses, disps, intrinsics):
    if poses.dim() != 2 or poses.shape[1] != 7:
        raise RuntimeError("poses must be (N,7) = t, q(xyzw), got %s" % (tuple(poses.shape),))
    if disps.dim() != 3:
        raise RuntimeError("disps must be (N,ht,wd), got %s" % (tuple(disps.shape),))
    if intrinsics.dim() != 1 or intrinsics.shape[0] < 4:
        raise RuntimeError("intrinsics must be 1-D with fx, fy, cx, cy, got %s" % (tuple(intrinsics.shape),))


def _pairs(ii, jj):
    if ii.dim() != 1 or jj.dim() != 1 or ii.shape[0] != jj.shape[0]:
        raise RuntimeError("ii and jj must be 1-D and of equal length, got %s and %s" % (tuple(ii.shape), tuple(jj.shape)))
    return ii.shape[0]


def frame_distance(poses, disps, intrinsics, ii, jj, beta):
    """dist[k] (num,): mean flow magnitude from frame ii[k] to jj[k], a beta : 1-beta blend of the full transform and
    the translation alone, or 1000 when less than 75 % of the weight has depth > MIN_DEPTH (:518-658)."""
    named = _check_inputs(poses, "poses", disps, "disps", intrinsics, "intrinsics", ii, "ii", jj, "jj")
    _check_geometry(poses, disps, intrinsics)
    num = _pairs(ii, jj)
    _check_device(named)
    dist = torch.empty((num,), dtype=torch.float32, device=poses.device)
    if num == 0:
        return dist
    Nd, ht, wd = disps.shape
    with torch.cuda.device(poses.device):
        rc = _lib.load().lgu_frame_distance_f32(_ptr(poses), poses.shape[0], _ptr(disps), Nd, ht, wd, _ptr(intrinsics),
                                                _ptr(ii), _ptr(jj), num, float(beta), _ptr(dist), _stream(poses))
    _lib.check(rc, "frame_distance")
    return dist


def projmap(poses, disps, intrinsics, ii, jj):
    """[coords (num,ht,wd,3), valid (num,ht,wd,1)]: pixels of frame ii[k] projected into jj[k] (:427-516).  coords =
    (u, v) unless the point's depth exceeds 0.01, then its projection; channel 2 is 0.  valid = depth > MIN_DEPTH."""
    named = _check_inputs(poses, "poses", disps, "disps", intrinsics, "intrinsics", ii, "ii", jj, "jj")
    _check_geometry(poses, disps, intrinsics)
    num = _pairs(ii, jj)
    _check_device(named)
    Nd, ht, wd = disps.shape
    coords = torch.empty((num, ht, wd, 3), dtype=torch.float32, device=poses.device)
    valid = torch.empty((num, ht, wd, 1), dtype=torch.float32, device=poses.device)
    if num == 0 or ht * wd == 0:
        return [coords, valid]
    with torch.cuda.device(poses.device):
        rc = _lib.load().lgu_projmap_f32(_ptr(poses), poses.shape[0], _ptr(disps), Nd, ht, wd, _ptr(intrinsics),
                                         _ptr(ii), _ptr(jj), num, _ptr(coords), _ptr(valid), _stream(poses))
    _lib.check(rc, "projmap")
    return [coords, valid]


def depth_filter(poses, disps, intrinsics, ix, thresh):
    """counter (num,ht,wd): for every pixel of frame ix[b], how many of the neighbours ix-1, ix-2, ix-3, ix+3, ix+4,
    ix+5 inside the buffer see a disparity of one of the four pixels around its projection within thresh[b] (compared
    as |1/d_proj - 1/d_corner| in double) (:661-776)."""
    named = _check_inputs(poses, "poses", disps, "disps", intrinsics, "intrinsics", ix, "ix", thresh, "thresh")
    _check_geometry(poses, disps, intrinsics)
    if ix.dim() != 1:
        raise RuntimeError("ix must be 1-D, got %s" % (tuple(ix.shape),))
    num = ix.shape[0]
    if thresh.dim() != 1 or thresh.shape[0] < num:
        raise RuntimeError("thresh must be 1-D with one entry per index of ix (%d), got %s" % (num, tuple(thresh.shape)))
    _check_device(named)
    Nd, ht, wd = disps.shape
    counter = torch.empty((num, ht, wd), dtype=torch.float32, device=disps.device)
    if num == 0 or ht * wd == 0:
        return counter
    with torch.cuda.device(disps.device):
        rc = _lib.load().lgu_depth_filter_f32(_ptr(poses), poses.shape[0], _ptr(disps), Nd, ht, wd, _ptr(intrinsics),
                                              _ptr(ix), _ptr(thresh), num, _ptr(counter), _stream(disps))
    _lib.check(rc, "depth_filter")
    return counter


def iproj(poses, disps, intrinsics):
    """points (Nd,ht,wd,3): every pixel back-projected with its disparity and moved by poses[n],
    act_se3(T_n, (x, y, 1, d))[0:3] / d (:779-851).  The reference's callers pass camera-to-world poses:
    iproj(se3_inverse(poses), disps, intrinsics)."""
    named = _check_inputs(poses, "poses", disps, "disps", intrinsics, "intrinsics")
    _check_geometry(poses, disps, intrinsics)
    _check_device(named)
    Nd, ht, wd = disps.shape
    points = torch.empty((Nd, ht, wd, 3), dtype=torch.float32, device=disps.device)
    if Nd == 0 or ht * wd == 0:
        return points
    with torch.cuda.device(disps.device):
        rc = _lib.load().lgu_iproj_f32(_ptr(poses), poses.shape[0], _ptr(disps), Nd, ht, wd, _ptr(intrinsics), _ptr(points),
                                       _stream(disps))
    _lib.check(rc, "iproj")
    return points


def se3_inverse(poses):
    """Inverse of SE3 poses (...,7) = t, q(xyzw) with unit q: (-R(q)^-1 t, conj(q)) — what the reference's callers of
    iproj compute with lietorch as `SE3(poses).inv().data`."""
    t, q = poses[..., :3], poses[..., 3:]
    qi = torch.cat([-q[..., :3], q[..., 3:]], -1)
    v = qi[..., :3]
    uv = 2.0 * torch.cross(v, t, dim=-1)
    ti = -(t + qi[..., 3:] * uv + torch.cross(v, uv, dim=-1))
    return torch.cat([ti, qi], -1)
