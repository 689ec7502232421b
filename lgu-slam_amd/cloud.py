"""The map export: the filtered, coloured point cloud of a set of keyframes, on the HIP kernels of csrc/cloud.hip.

What the reference's visualiser callback (droid_slam/visualization.py:92-129) and anyone who saves a reconstruction does
with `iproj`, `depth_filter`, a per-frame mean, four copies to the host and a boolean index per frame:

    points, colors, offsets = cloud.point_cloud(video.poses, video.disps, video.intrinsics[0], dirty_index, thresh,
                                                video.images)

decides, back-projects, colours and compacts on the device, in three launches; only surviving points reach memory.  Entry
b of `ix` owns the rows offsets[b] : offsets[b + 1], its pixels in row-major order: the concatenation the reference's loop
produces.  Counts are `geom.depth_filter`'s and points `geom.iproj(geom.se3_inverse(poses[ix]), disps[ix], intrinsics)`'s,
bit for bit (one device definition each, csrc/geom_pixel.hpp); `point_cloud_composed` is that composition of the existing
operators, kept as the route below `MIN_FUSED_PIXELS` and as the tests' yardstick.

Kernels are enqueued on the current stream of the operands' device.  With `out=None` the call reads one number on the host
(the total, to size the results); with `out=(points_buf, colors_buf_or_None)` it reads nothing.
"""
import torch

from . import _lib, geom
from ._host import check_contiguous, check_device, check_dtype, check_no_grad, launch
from ._host import ptr as _ptr, stream as _stream

MIN_FUSED_PIXELS = 0        # num*ht*wd below which point_cloud takes point_cloud_composed (read at the call)
launches = {"fused": 0, "composed": 0}      # calls served by each route (empty calls launch nothing and count nowhere)

_COLOR_DTYPES = (torch.float32, torch.uint8)


def _check(poses, disps, intrinsics, ix, thresh, images, disp_floor, stride, phase, color_dtype, out):
    """Every refusal of point_cloud, before any launch: contiguity, HIP device, dtype, then the shapes in geom.depth_filter's
    wording, then images, disp_floor and out.  Returns num."""
    named = [(poses, "poses"), (disps, "disps"), (intrinsics, "intrinsics"), (ix, "ix"), (thresh, "thresh")]
    extra = ([(images, "images")] if images is not None else []) + ([(disp_floor, "disp_floor")] if disp_floor is not None else [])
    outs = []
    if out is not None:
        if not isinstance(out, (tuple, list)) or len(out) != 2 or not isinstance(out[0], torch.Tensor) \
                or not (out[1] is None or isinstance(out[1], torch.Tensor)):
            raise RuntimeError("out must be a pair (points buffer, colors buffer or None)")
        outs = [(out[0], "out points")] + ([(out[1], "out colors")] if out[1] is not None else [])
    if color_dtype not in _COLOR_DTYPES:
        raise RuntimeError("color_dtype must be torch.float32 or torch.uint8, got %s" % (color_dtype,))
    everything = named + extra + outs
    check_contiguous(everything)
    check_device(everything)
    check_dtype(named[:3], torch.float32)
    check_dtype(named[3:4], torch.int64)
    check_dtype(named[4:], torch.float32)
    if images is not None:
        check_dtype([(images, "images")], torch.uint8)
    if disp_floor is not None:
        check_dtype([(disp_floor, "disp_floor")], torch.float32)
    if outs:
        check_dtype(outs[:1], torch.float32)
        check_dtype(outs[1:], color_dtype)
    check_no_grad("point_cloud", everything)
    geom.check_geometry(poses, disps, intrinsics)
    if ix.dim() != 1:
        raise RuntimeError("ix must be 1-D, got %s" % (tuple(ix.shape),))
    num = ix.shape[0]
    if thresh.dim() != 1 or thresh.shape[0] < num:
        raise RuntimeError("thresh must be 1-D with one entry per index of ix (%d), got %s" % (num, tuple(thresh.shape)))
    Nd, ht, wd = disps.shape
    if images is not None:
        if int(stride) < 1 or int(phase) < 0:
            raise RuntimeError("stride must be >= 1 and phase >= 0, got stride %r and phase %r" % (stride, phase))
        if images.dim() != 4 or images.shape[1] != 3:
            raise RuntimeError("images must be (N,3,H,W) uint8 BGR, got %s" % (tuple(images.shape),))
        H, W = images.shape[2:]
        sampled = (len(range(phase, H, stride)), len(range(phase, W, stride)))
        if sampled != (ht, wd):
            raise RuntimeError("images of %dx%d sampled at [%d::%d] give %dx%d pixels, disps has %dx%d"
                               % (H, W, phase, stride, sampled[0], sampled[1], ht, wd))
        if images.shape[0] < min(poses.shape[0], Nd):
            raise RuntimeError("images must hold a frame for every frame with a pose and a disparity (%d), got %d"
                               % (min(poses.shape[0], Nd), images.shape[0]))
    if disp_floor is not None and tuple(disp_floor.shape) != (num,):
        raise RuntimeError("disp_floor must be (num,) = (%d,), got %s" % (num, tuple(disp_floor.shape)))
    if outs:
        for t, name in outs:
            if t.dim() != 2 or t.shape[1] != 3:
                raise RuntimeError("%s must be (capacity,3), got %s" % (name, tuple(t.shape)))
        if (out[1] is None) != (images is None):
            raise RuntimeError("out colors must be given with images and only with them")
        if out[1] is not None and out[1].shape[0] != out[0].shape[0]:
            raise RuntimeError("out colors must have the capacity of out points (%d rows), got %d" % (out[0].shape[0], out[1].shape[0]))
    return num


def _floor(disps, ix, disp_ratio):
    """disp_ratio * disps[ix].mean(dim=[1,2]) with those torch calls (the bits of the reference's `.5*disps.mean(...)`);
    out-of-range ix clamped for this gather only."""
    Nd = disps.shape[0]
    if Nd == 0 or disps.shape[1] * disps.shape[2] == 0:
        return torch.zeros((ix.shape[0],), dtype=torch.float32, device=disps.device)
    return disp_ratio * disps[ix.clamp(0, Nd - 1)].mean(dim=[1, 2])


def _empty(num, images, color_dtype, out, device):
    offsets = torch.zeros((num + 1,), dtype=torch.int64, device=device)
    if out is not None:
        return out[0], out[1], offsets
    points = torch.empty((0, 3), dtype=torch.float32, device=device)
    return points, (None if images is None else torch.empty((0, 3), dtype=color_dtype, device=device)), offsets


def point_cloud_composed(poses, disps, intrinsics, ix, thresh, images=None, *, min_count=2, disp_ratio=0.5, disp_floor=None,
                         stride=8, phase=3, color_dtype=torch.float32, out=None):
    """point_cloud as the composition of the existing operators the reference's callback is (visualization.py:92-129), all
    on the device: geom.iproj under geom.se3_inverse, geom.depth_filter, the mask `(count >= min_count) & (disps >
    floor)`, one boolean index over the batch.  Same arguments, results and refusals as point_cloud."""
    num = _check(poses, disps, intrinsics, ix, thresh, images, disp_floor, stride, phase, color_dtype, out)
    Nd, ht, wd = disps.shape
    dev = disps.device
    if num == 0 or ht * wd == 0:
        return _empty(num, images, color_dtype, out, dev)
    launches["composed"] += 1
    floor = _floor(disps, ix, disp_ratio) if disp_floor is None else disp_floor
    count = geom.depth_filter(poses, disps, intrinsics, ix, thresh)
    nvalid = min(poses.shape[0], Nd)
    safe = ix.clamp(0, max(nvalid - 1, 0))
    if nvalid == 0:         # no frame has both a pose and a disparity: depth_filter counted 0 everywhere
        mask = torch.zeros((num, ht, wd), dtype=torch.bool, device=dev)
        points = torch.empty((num, ht, wd, 3), dtype=torch.float32, device=dev)
    else:
        d = disps[safe]
        inside = (ix >= 0) & (ix < nvalid)              # an entry outside the buffer keeps nothing, whatever min_count
        mask = (count >= min_count) & (d > floor[:, None, None]) & inside[:, None, None]
        points = geom.iproj(geom.se3_inverse(poses[safe]).contiguous(), d.contiguous(), intrinsics)
    offsets = torch.zeros((num + 1,), dtype=torch.int64, device=dev)
    offsets[1:] = torch.cumsum(mask.reshape(num, -1).sum(dim=1), 0)
    colors = None
    if images is not None:
        rgb = images[safe][:, [2, 1, 0], phase::stride, phase::stride].permute(0, 2, 3, 1)
        colors = (rgb / 255.0) if color_dtype == torch.float32 else rgb
    if out is None:
        return points[mask], (None if colors is None else colors[mask]), offsets
    kept = points[mask]
    n = min(out[0].shape[0], kept.shape[0])
    out[0][:n] = kept[:n]
    if colors is not None:
        out[1][:n] = colors[mask][:n]
    return out[0], out[1], offsets


def point_cloud(poses, disps, intrinsics, ix, thresh, images=None, *, min_count=2, disp_ratio=0.5, disp_floor=None, stride=8,
                phase=3, color_dtype=torch.float32, out=None):
    """`(points, colors, offsets)`: the filtered point cloud of the frames `ix` (visualization.py:92-129).

    poses (Np,7) float32 world-to-camera = t, q(xyzw); disps (Nd,ht,wd) float32; intrinsics 1-D float32 with fx, fy, cx, cy
    first; ix (num,) int64; thresh (>= num,) float32 as geom.depth_filter's; images (Ni,3,H,W) uint8 BGR with
    len(range(phase, H, stride)) == ht and the same for W, or None.  A pixel of frame ix[b] is kept when depth_filter counts
    at least `min_count` neighbours for it and its disparity exceeds the entry's floor: `disp_floor[b]` ((num,) float32) if
    given, else `disp_ratio * disps[ix].mean(dim=[1,2])`.  An ix[b] outside [0, min(Np, Nd)) keeps nothing.

    points (total,3) float32 in world coordinates; colors (total,3) RGB, float32 in [0,1] or with color_dtype=torch.uint8
    the bytes, None without images; offsets (num+1,) int64: entry b owns the rows offsets[b]:offsets[b+1], pixels ascending.

    out=None: exact-size results; the call reads offsets[-1] on the host, its one synchronisation.  out=(points_buf,
    colors_buf or None), (capacity,3) each: nothing is read on the host, rows below the capacity are written and the rest
    of the buffers is untouched; the caller compares offsets[-1] with the capacity.  The buffers themselves are returned.
    num == 0 or an empty frame: empty results and zero offsets, nothing is launched.  No autograd."""
    num = _check(poses, disps, intrinsics, ix, thresh, images, disp_floor, stride, phase, color_dtype, out)
    Nd, ht, wd = disps.shape
    dev = disps.device
    if num == 0 or ht * wd == 0:
        return _empty(num, images, color_dtype, out, dev)
    if num * ht * wd < MIN_FUSED_PIXELS:
        return point_cloud_composed(poses, disps, intrinsics, ix, thresh, images, min_count=min_count, disp_ratio=disp_ratio,
                                    disp_floor=disp_floor, stride=stride, phase=phase, color_dtype=color_dtype, out=out)
    floor = (_floor(disps, ix, disp_ratio) if disp_floor is None else disp_floor).contiguous()
    scratch = torch.empty((int(_lib.load().lgu_cloud_scratch_bytes(num, ht, wd)),), dtype=torch.uint8, device=dev)
    offsets = torch.empty((num + 1,), dtype=torch.int64, device=dev)
    args = _lib.CloudArgs(poses=_ptr(poses), disps=_ptr(disps), intrinsics=_ptr(intrinsics), ix=_ptr(ix), thresh=_ptr(thresh),
                          floor=_ptr(floor), scratch=_ptr(scratch), offsets=_ptr(offsets), np=poses.shape[0], nd=Nd, ht=ht, wd=wd,
                          num=num, min_count=int(min_count), color_u8=int(color_dtype == torch.uint8))
    if images is not None:
        args.images, args.ni, args.H, args.W = _ptr(images), images.shape[0], images.shape[2], images.shape[3]
        args.stride, args.phase = int(stride), int(phase)
    launch("lgu_cloud_decide_f32", "point_cloud", dev, args, _stream(disps))
    if out is None:
        total = int(offsets[-1])                 # the call's one host read
        points = torch.empty((total, 3), dtype=torch.float32, device=dev)
        colors = None if images is None else torch.empty((total, 3), dtype=color_dtype, device=dev)
    else:
        points, colors = out
    args.points, args.colors, args.cap = _ptr(points), (None if colors is None else _ptr(colors)), points.shape[0]
    launch("lgu_cloud_write_f32", "point_cloud", dev, args, _stream(disps))
    launches["fused"] += 1
    return points, colors, offsets
