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

`projective_transform`, `reproject` and `motion_features` (geom/projective_ops.py:98-128 and the motion features of
FactorGraph.update, without lietorch) run on csrc/reproject.hip; see their docstrings.

Kernels are enqueued on the current stream of the inputs' device, without host synchronisation (graph-capturable).
"""
import torch

from ._host import check_contiguous, check_device, check_dtype, check_no_grad, launch
from ._host import ptr as _ptr, stream as _stream


def _operands(data, index=(), tail=()):
    """CHECK_INPUT (src/droid.cpp:84-85, "x must be contiguous") on every argument in the reference's order, then the dtypes
    of the reference's accessors: float32 for `data` and `tail`, int64 (`long`) for `index`.  Returns the pairs for
    check_device, which runs after the shape checks: every argument error is raised before anything is launched, and
    without a device."""
    named = list(data) + list(index) + list(tail)
    check_contiguous(named)
    check_dtype(data, torch.float32)
    check_dtype(index, torch.int64)
    check_dtype(tail, torch.float32)
    return named


def _video(poses, disps, intrinsics):
    return [(poses, "poses"), (disps, "disps"), (intrinsics, "intrinsics")]


def check_geometry(poses, disps, intrinsics):
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
    named = _operands(_video(poses, disps, intrinsics), [(ii, "ii"), (jj, "jj")])
    check_geometry(poses, disps, intrinsics)
    num = _pairs(ii, jj)
    check_device(named)
    dist = torch.empty((num,), dtype=torch.float32, device=poses.device)
    if num == 0:
        return dist
    Nd, ht, wd = disps.shape
    launch("lgu_frame_distance_f32", "frame_distance", poses.device, _ptr(poses), poses.shape[0], _ptr(disps), Nd, ht, wd,
           _ptr(intrinsics), _ptr(ii), _ptr(jj), num, float(beta), _ptr(dist), _stream(poses))
    return dist


def projmap(poses, disps, intrinsics, ii, jj):
    """[coords (num,ht,wd,3), valid (num,ht,wd,1)]: pixels of frame ii[k] projected into jj[k] (:427-516).  coords =
    (u, v) unless the point's depth exceeds 0.01, then its projection; channel 2 is 0.  valid = depth > MIN_DEPTH."""
    named = _operands(_video(poses, disps, intrinsics), [(ii, "ii"), (jj, "jj")])
    check_geometry(poses, disps, intrinsics)
    num = _pairs(ii, jj)
    check_device(named)
    Nd, ht, wd = disps.shape
    coords = torch.empty((num, ht, wd, 3), dtype=torch.float32, device=poses.device)
    valid = torch.empty((num, ht, wd, 1), dtype=torch.float32, device=poses.device)
    if num == 0 or ht * wd == 0:
        return [coords, valid]
    launch("lgu_projmap_f32", "projmap", poses.device, _ptr(poses), poses.shape[0], _ptr(disps), Nd, ht, wd,
           _ptr(intrinsics), _ptr(ii), _ptr(jj), num, _ptr(coords), _ptr(valid), _stream(poses))
    return [coords, valid]


def depth_filter(poses, disps, intrinsics, ix, thresh):
    """counter (num,ht,wd): for every pixel of frame ix[b], how many of the neighbours ix-1, ix-2, ix-3, ix+3, ix+4,
    ix+5 inside the buffer see a disparity of one of the four pixels around its projection within thresh[b] (compared
    as |1/d_proj - 1/d_corner| in double) (:661-776)."""
    named = _operands(_video(poses, disps, intrinsics), [(ix, "ix")], [(thresh, "thresh")])
    check_geometry(poses, disps, intrinsics)
    if ix.dim() != 1:
        raise RuntimeError("ix must be 1-D, got %s" % (tuple(ix.shape),))
    num = ix.shape[0]
    if thresh.dim() != 1 or thresh.shape[0] < num:
        raise RuntimeError("thresh must be 1-D with one entry per index of ix (%d), got %s" % (num, tuple(thresh.shape)))
    check_device(named)
    Nd, ht, wd = disps.shape
    counter = torch.empty((num, ht, wd), dtype=torch.float32, device=disps.device)
    if num == 0 or ht * wd == 0:
        return counter
    launch("lgu_depth_filter_f32", "depth_filter", disps.device, _ptr(poses), poses.shape[0], _ptr(disps), Nd, ht, wd,
           _ptr(intrinsics), _ptr(ix), _ptr(thresh), num, _ptr(counter), _stream(disps))
    return counter


def iproj(poses, disps, intrinsics):
    """points (Nd,ht,wd,3): every pixel back-projected with its disparity and moved by poses[n],
    act_se3(T_n, (x, y, 1, d))[0:3] / d (:779-851).  The reference's callers pass camera-to-world poses:
    iproj(se3_inverse(poses), disps, intrinsics)."""
    named = _operands(_video(poses, disps, intrinsics))
    check_geometry(poses, disps, intrinsics)
    check_device(named)
    Nd, ht, wd = disps.shape
    points = torch.empty((Nd, ht, wd, 3), dtype=torch.float32, device=disps.device)
    if Nd == 0 or ht * wd == 0:
        return points
    launch("lgu_iproj_f32", "iproj", disps.device, _ptr(poses), poses.shape[0], _ptr(disps), Nd, ht, wd, _ptr(intrinsics),
           _ptr(points), _stream(disps))
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


# ---- projective_transform and the motion features (csrc/reproject.hip) ----------------------------------------------
# The reference's geom/projective_ops.py:projective_transform (:98-128) without lietorch, and FactorGraph.update's motion
# features (factor_graph.py:210-212, :268-270) in one launch.  Forward only: no autograd.

REPROJ_JACOBIAN, REPROJ_DEPTH = 1, 2     # include/lgu_corr.h LGU_REPROJ_*


def _pose_tensor(poses):
    """A (B,N,7) tensor as it is, or the `.data` of a group object (a lietorch SE3)."""
    return poses if isinstance(poses, torch.Tensor) else poses.data


def _check_batched(poses, disps, intrinsics, ii, jj):
    if poses.dim() != 3 or poses.shape[2] != 7:
        raise RuntimeError("poses must be (B,N,7) = t, q(xyzw), got %s" % (tuple(poses.shape),))
    if disps.dim() != 4:
        raise RuntimeError("disps must be (B,N,ht,wd), got %s" % (tuple(disps.shape),))
    if intrinsics.dim() != 3 or intrinsics.shape[2] != 4:
        raise RuntimeError("intrinsics must be (B,N,4) = fx, fy, cx, cy per frame, got %s" % (tuple(intrinsics.shape),))
    if not poses.shape[0] == disps.shape[0] == intrinsics.shape[0]:
        raise RuntimeError("poses, disps and intrinsics must have the same batch size, got %d, %d and %d"
                           % (poses.shape[0], disps.shape[0], intrinsics.shape[0]))
    return _pairs(ii, jj)


def _sizes(poses, disps, intrinsics, num):
    B, Nd, ht, wd = disps.shape
    return B, poses.shape[1], Nd, intrinsics.shape[1], ht, wd, num


def projective_transform(poses, disps, intrinsics, ii, jj, jacobian=False, return_depth=False):
    """Map the pixels of frames ii into frames jj (geom/projective_ops.py:98-128): `(coords, valid)`, or
    `(coords, valid, (Ji, Jj, Jz))` with `jacobian`.

    poses (B,N,7) float32 = t, q(xyzw) (or an object whose `.data` is that tensor, e.g. a lietorch SE3); disps
    (B,N,ht,wd); intrinsics (B,N,4) per frame (back-projection reads frame ii's, projection frame jj's); ii, jj int64
    (E,).  coords (B,E,ht,wd,2), a third channel disp / Z with `return_depth`; valid (B,E,ht,wd,1) float; Ji, Jj
    (B,E,ht,wd,2,6) in lietorch's tangent order (translation, rotation); Jz (B,E,ht,wd,2,1).  Edges with ii == jj use the
    stereo baseline t = (-0.1, 0, 0).  An index outside [0, min of the three frame counts) gives NaN values and valid 0.
    Quaternions are used as given (lietorch may normalise non-unit ones)."""
    poses = _pose_tensor(poses)
    named = _operands(_video(poses, disps, intrinsics), [(ii, "ii"), (jj, "jj")])
    num = _check_batched(poses, disps, intrinsics, ii, jj)
    check_no_grad("projective_transform", named)
    check_device(named)
    B, Np, Nd, Ni, ht, wd, num = _sizes(poses, disps, intrinsics, num)
    dev = disps.device
    C = 3 if return_depth else 2
    coords = torch.empty((B, num, ht, wd, C), dtype=torch.float32, device=dev)
    valid = torch.empty((B, num, ht, wd, 1), dtype=torch.float32, device=dev)
    if jacobian:
        Ji = torch.empty((B, num, ht, wd, 2, 6), dtype=torch.float32, device=dev)
        Jj = torch.empty_like(Ji)
        Jz = torch.empty((B, num, ht, wd, 2, 1), dtype=torch.float32, device=dev)
    if B * num * ht * wd > 0:
        flags = (REPROJ_JACOBIAN if jacobian else 0) | (REPROJ_DEPTH if return_depth else 0)
        jac_ptrs = (_ptr(Ji), _ptr(Jj), _ptr(Jz)) if jacobian else (None, None, None)
        launch("lgu_projective_transform_f32", "projective_transform", dev, _ptr(poses), _ptr(disps), _ptr(intrinsics),
               _ptr(ii), _ptr(jj), B, Np, Nd, Ni, ht, wd, num, flags, _ptr(coords), _ptr(valid), *jac_ptrs, _stream(disps))
    if jacobian:
        return coords, valid, (Ji, Jj, Jz)
    return coords, valid


def reproject(poses, disps, intrinsics, ii, jj):
    """DepthVideo.reproject (depth_video.py:140-148) on the video's buffers: poses (N,7), disps (N,ht,wd), intrinsics
    (N,4) -> coords (1,E,ht,wd,2), valid (1,E,ht,wd,1)."""
    poses = _pose_tensor(poses)
    return projective_transform(poses[None], disps[None], intrinsics[None], ii, jj)


def motion_features(poses, disps, intrinsics, ii, jj, target, clamp=64.0):
    """The motion features of FactorGraph.update (factor_graph.py:210-212) in one launch: `(coords1, motn)` with
    coords1 = projective_transform(...)[0] (B,E,ht,wd,2) and motn (B,E,4,ht,wd) contiguous =
    cat([coords1 - coords0, target - coords1], -1).permute(0,1,4,2,3).clamp(-clamp, clamp) (a NaN stays NaN).
    Arguments as projective_transform's; target (B,E,ht,wd,2) float32."""
    poses = _pose_tensor(poses)
    named = _operands(_video(poses, disps, intrinsics), [(ii, "ii"), (jj, "jj")], [(target, "target")])
    num = _check_batched(poses, disps, intrinsics, ii, jj)
    B, Np, Nd, Ni, ht, wd, num = _sizes(poses, disps, intrinsics, num)
    if tuple(target.shape) != (B, num, ht, wd, 2):
        raise RuntimeError("target must be (B,E,ht,wd,2) = %s, got %s" % ((B, num, ht, wd, 2), tuple(target.shape)))
    if not float(clamp) >= 0:
        raise RuntimeError("clamp must be a non-negative bound, got %r" % (clamp,))
    check_no_grad("motion_features", named)
    check_device(named)
    dev = disps.device
    coords1 = torch.empty((B, num, ht, wd, 2), dtype=torch.float32, device=dev)
    motn = torch.empty((B, num, 4, ht, wd), dtype=torch.float32, device=dev)
    if B * num * ht * wd > 0:
        launch("lgu_motion_features_f32", "motion_features", dev, _ptr(poses), _ptr(disps), _ptr(intrinsics), _ptr(ii),
               _ptr(jj), _ptr(target), B, Np, Nd, Ni, ht, wd, num, float(clamp), _ptr(coords1), _ptr(motn), None,
               _stream(disps))
    return coords1, motn
