"""The offscreen view of the map: coloured points and one wireframe frustum per keyframe, z-buffered, on the HIP kernels of
csrc/render.hip.

The drawing half of the reference's visualiser callback (droid_slam/visualization.py:36-51, 121-134, in the 540x960 window
of :144-153 with misc/renderoption.json: white background, point size 2), without Open3D and without a display:

    points, colors, _ = cloud.point_cloud(video.poses, video.disps, video.intrinsics[0], index, thresh, video.images)
    image, depth = render.render_view(points, colors, view, intrinsics, (540, 960), cameras=video.poses[:t])

`view` is a world-to-camera pose as `video.poses` holds them; `look_at` makes one on the host.  The definition of the picture
is tests/render_restatement.py: one 64-bit key per pixel, depth bits above the packed colour, the
minimum wins, so the bytes do not depend on the order of points or on timing.  It is this project's own definition of the
view and was never compared with an Open3D render.

Kernels are enqueued on the current stream of the operands' device; the call reads nothing on the host.
"""
import math

import numpy as np
import torch

from . import _lib
from ._host import check_contiguous, check_device, check_dtype, check_no_grad, launch
from ._host import ptr as _ptr, stream as _stream

launches = {"fused": 0}         # calls served by the kernels
MAX_PIXELS = 1 << 28
MAX_POINT_SIZE = 8

_COLOR_DTYPES = (torch.float32, torch.uint8)


def _rgb(value, name):
    try:
        c = tuple(int(v) for v in value)
    except (TypeError, ValueError):
        c = ()
    if len(c) != 3 or any(v < 0 or v > 255 for v in c) or any(int(v) != v for v in value):
        raise RuntimeError("%s must be three integers in 0..255, got %r" % (name, value))
    return c


def _check(points, colors, view, intrinsics, size, point_size, background, near, cameras, camera_scale, camera_color, out):
    """Every refusal of render_view, before any launch: contiguity, HIP device, dtype, then the shapes, then point_size, size,
    near and the colours, then out.  Returns (P, K, H, W, background, camera_color)."""
    named = [(points, "points"), (colors, "colors"), (view, "view"), (intrinsics, "intrinsics")]
    cams = [(cameras, "cameras")] if cameras is not None else []
    outs = []
    if out is not None:
        if not isinstance(out, (tuple, list)) or len(out) != 2 or not all(isinstance(t, torch.Tensor) for t in out):
            raise RuntimeError("out must be a pair (image buffer, depth buffer)")
        outs = [(out[0], "out image"), (out[1], "out depth")]
    everything = named + cams + outs
    check_contiguous(everything)
    check_device(everything)
    check_dtype(named[:1], torch.float32)
    check_dtype(named[1:2], _COLOR_DTYPES)
    check_dtype(named[2:] + cams, torch.float32)
    if outs:
        check_dtype(outs[:1], torch.uint8)
        check_dtype(outs[1:], torch.float32)
    check_no_grad("render_view", everything)
    if points.dim() != 2 or points.shape[1] != 3:
        raise RuntimeError("points must be (P,3), got %s" % (tuple(points.shape),))
    P = points.shape[0]
    if tuple(colors.shape) != (P, 3):
        raise RuntimeError("colors must be (P,3) = (%d, 3), got %s" % (P, tuple(colors.shape)))
    if tuple(view.shape) != (7,):
        raise RuntimeError("view must be (7,) = t, q(xyzw), got %s" % (tuple(view.shape),))
    if intrinsics.dim() != 1 or intrinsics.shape[0] < 4:
        raise RuntimeError("intrinsics must be 1-D with fx, fy, cx, cy, got %s" % (tuple(intrinsics.shape),))
    if cameras is not None and (cameras.dim() != 2 or cameras.shape[1] != 7):
        raise RuntimeError("cameras must be (K,7) = t, q(xyzw), got %s" % (tuple(cameras.shape),))
    K = 0 if cameras is None else cameras.shape[0]
    if isinstance(point_size, bool) or not isinstance(point_size, int) or not 1 <= point_size <= MAX_POINT_SIZE:
        raise RuntimeError("point_size must be an integer in 1..%d, got %r" % (MAX_POINT_SIZE, point_size))
    try:
        H, W = (int(v) for v in size)
    except (TypeError, ValueError):
        raise RuntimeError("size must be (H, W), got %r" % (size,)) from None
    if H < 0 or W < 0 or H * W == 0 or H * W > MAX_PIXELS:
        raise RuntimeError("size must have between 1 and 2^28 pixels, got %dx%d" % (H, W))
    if not (isinstance(near, (int, float)) and math.isfinite(near) and near > 0):
        raise RuntimeError("near must be finite and positive, got %r" % (near,))
    if not (isinstance(camera_scale, (int, float)) and math.isfinite(camera_scale)):
        raise RuntimeError("camera_scale must be finite, got %r" % (camera_scale,))
    background, camera_color = _rgb(background, "background"), _rgb(camera_color, "camera_color")
    if outs:
        if tuple(out[0].shape) != (H, W, 3):
            raise RuntimeError("out image must be (H,W,3) = (%d, %d, 3), got %s" % (H, W, tuple(out[0].shape)))
        if tuple(out[1].shape) != (H, W):
            raise RuntimeError("out depth must be (H,W) = (%d, %d), got %s" % (H, W, tuple(out[1].shape)))
    return P, K, H, W, background, camera_color


def render_view(points, colors, view, intrinsics, size, *, point_size=2, background=(255, 255, 255), near=0.01, cameras=None,
                camera_scale=0.05, camera_color=(255, 0, 0), out=None):
    """`(image, depth)`: the points and the cameras' frustums as the camera `view` sees them.

    points (P,3) float32 in world coordinates, P may be 0; colors (P,3) RGB, uint8 or float32 in [0,1] (the two forms
    cloud.point_cloud returns); a point with a non-finite coordinate is skipped.  view (7,) float32 world-to-camera = t,
    q(xyzw), the convention of video.poses; intrinsics 1-D float32 with fx, fy, cx, cy of the output image first; size =
    (H, W).  A point covers point_size x point_size pixels (1..8) around its projection when its depth exceeds `near`.
    cameras (K,7) float32 world-to-camera poses (rows of video.poses) or None: each is drawn as a wireframe frustum of
    `camera_scale` in `camera_color`, clipped at `near`.

    image (H,W,3) uint8 RGB, `background` where nothing was drawn; depth (H,W) float32: the camera-space z of the nearest
    primitive of the pixel, +inf on background.  Among primitives of equal depth the smaller packed colour wins: the result
    does not depend on the order of the points.  out=(image_buf, depth_buf): written and returned.  Nothing is read on the
    host.  No autograd."""
    P, K, H, W, background, camera_color = _check(points, colors, view, intrinsics, size, point_size, background, near, cameras,
                                                  camera_scale, camera_color, out)
    dev = points.device
    if out is None:
        image = torch.empty((H, W, 3), dtype=torch.uint8, device=dev)
        depth = torch.empty((H, W), dtype=torch.float32, device=dev)
    else:
        image, depth = out
    scratch = torch.empty((int(_lib.load().lgu_render_scratch_bytes(H, W)),), dtype=torch.uint8, device=dev)
    args = _lib.RenderArgs(points=_ptr(points) if P else None, colors=_ptr(colors) if P else None, view=_ptr(view),
                           intrinsics=_ptr(intrinsics), cameras=_ptr(cameras) if K else None, scratch=_ptr(scratch),
                           image=_ptr(image), depth=_ptr(depth), npoints=P, near=float(near), camera_scale=float(camera_scale),
                           ncam=K, H=H, W=W, point_size=point_size, color_u8=int(colors.dtype == torch.uint8),
                           background=background, camera_color=camera_color)
    launch("lgu_render_view", "render_view", dev, args, _stream(points))
    launches["fused"] += 1
    return image, depth


def look_at(eye, target, up=(0.0, -1.0, 0.0)):
    """The world-to-camera pose (7,) = t, q(xyzw), float32 on the CPU, of the camera that sits at `eye` and looks along its
    +z at `target` with its image y pointing down (the DROID camera frame): `up` maps into the half plane x = 0, y < 0.
    Computed on the host in float64.  `eye == target` and an `up` along the line of sight are refused."""
    eye, target, up = (np.asarray(v, np.float64).reshape(-1) for v in (eye, target, up))
    if eye.shape != (3,) or target.shape != (3,) or up.shape != (3,) or not all(np.isfinite(v).all() for v in (eye, target, up)):
        raise RuntimeError("eye, target and up must be three finite numbers each")
    z = target - eye
    if not np.linalg.norm(z) > 0:
        raise RuntimeError("look_at: eye and target coincide")
    z = z / np.linalg.norm(z)
    x = np.cross(-up, z)                      # image y is down: x = down x ahead
    if not np.linalg.norm(x) > 1e-12 * np.linalg.norm(up):
        raise RuntimeError("look_at: up is along the line of sight")
    x = x / np.linalg.norm(x)
    y = np.cross(z, x)
    R = np.stack([x, y, z])                   # world-to-camera: the rows are the camera's axes
    t = -R @ eye
    # the quaternion of R by the branch with the largest pivot
    tr = R[0, 0] + R[1, 1] + R[2, 2]
    if tr > 0:
        s = 2.0 * math.sqrt(1.0 + tr)
        q = [(R[2, 1] - R[1, 2]) / s, (R[0, 2] - R[2, 0]) / s, (R[1, 0] - R[0, 1]) / s, 0.25 * s]
    else:
        i = int(np.argmax(np.diag(R)))
        j, k = (i + 1) % 3, (i + 2) % 3
        s = 2.0 * math.sqrt(1.0 + R[i, i] - R[j, j] - R[k, k])
        q = [0.0, 0.0, 0.0, (R[k, j] - R[j, k]) / s]
        q[i], q[j], q[k] = 0.25 * s, (R[j, i] + R[i, j]) / s, (R[k, i] + R[i, k]) / s
    q = np.asarray(q)
    q = q / np.linalg.norm(q)
    if q[3] < 0:
        q = -q
    return torch.from_numpy(np.concatenate([t, q]).astype(np.float32))
