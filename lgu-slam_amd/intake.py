"""The frame intake: a decoded camera frame to `Droid.track`'s operands in one launch, on the HIP kernels of csrc/intake.hip.

What every stream of the reference does on the host with OpenCV before track sees a frame (demo.py:39-54, demo_depth.py:39-65,
evaluation_scripts/test_tum.py:34-52, test_euroc.py:29-76: undistort or rectify, resize, crop, scaled intrinsics), what
motion_filter.py:56-57 does after it (the normalisation, `features.normalize_images`) and what depth_video.py:64-66 does
with the depth image:

    p = intake.plan.tum()                                     # or plan.demo(h0, w0, calib), plan.euroc(), plan(...)
    image, inputs = intake.frame(raw_bgr_u8, p)               # (N,3,H,W) uint8 BGR, (1,N,3,H,W) float32 RGB
    disps_sens_row = intake.sensor_disparity(raw_depth_u16, p)
    intrinsics = p.intrinsics                                 # float32 (4,): fx, fy, cx, cy of the output frame

The semantics are those of tests/intake_restatement.py: OpenCV's fixed-point scheme for 8-bit images
as far as it is known here, restated; OpenCV is not a dependency and was never run against it.  `frame_composed` is the same
arithmetic as a composition of torch operators on the device, kept as the route below `MIN_FUSED_PIXELS` and as the tests'
yardstick on the device.

Kernels are enqueued on the current stream of the operands' device.  A host frame is uploaded as the bytes it is; with `out=`
buffers (and a device frame) nothing is allocated.  Every refusal comes before any launch; there is no CPU fallback.
"""
import ctypes

import numpy as np
import torch

from . import _lib, features
from ._host import check_contiguous, check_device, check_dtype, check_no_grad, check_shape, launch, no_upload_while_capturing
from ._host import ptr as _ptr, stream as _stream

MIN_FUSED_PIXELS = 0        # N*H*W below which frame takes frame_composed (read at the call)
TILE_MAX_SCALE = 1.5        # largest downscale (raw over resized, either axis) served by the LDS tile kernel; beyond it, and
                            # with a stage absent, the direct kernel (read at the call; the bytes do not depend on it).
                            # Measured (profiles/intake_prof.json): the tile wins at 1.25 and 1.5, the direct kernel from 2.0
launches = {"fused": 0, "composed": 0}      # calls served by each route (empty calls launch nothing and count nowhere)

CAMERA_DOUBLES = 22         # fx fy cx cy | fx' fy' cx' cy' | R^-1 row-major | k1 k2 p1 p2 k3
_PATHS = {None: 0, "tile": 1, "direct": 2}


def _k4(camera, what):
    """(fx, fy, cx, cy) from four numbers or a 3x3 (or 3x4) camera matrix."""
    a = np.asarray(camera, dtype=np.float64)
    if a.shape == (4,):
        return a
    if a.shape in ((3, 3), (3, 4)):
        return np.array([a[0, 0], a[1, 1], a[0, 2], a[1, 2]])
    raise RuntimeError("%s must be (fx, fy, cx, cy) or a 3x3 camera matrix, got shape %s" % (what, a.shape))


def _per_frame(value, one):
    """`value` as a list of per-frame entries and whether it was given per frame; `one(v)` says v is a single entry."""
    if value is None:
        return [None], False
    if one(value):
        return [value], False
    return list(value), True


def _is_one_camera(v):
    a = np.asarray(v, dtype=np.float64)
    return a.shape in ((4,), (3, 3))         # (3,4) is three cameras of four numbers; only rectify's P may be 3x4


def _is_one_dist(v):
    return len(v) == 0 or np.ndim(v[0]) == 0      # numbers, not sequences of them (which may differ in length)


def _is_one_rectify(v):
    try:        # (R, P): the first entry is a 3x3 matrix of numbers; in a sequence of pairs it is a pair
        return len(v) == 2 and np.asarray(v[0], dtype=np.float64).shape == (3, 3)
    except (ValueError, TypeError):
        return False


class Plan:
    """What `plan` returns: `src_size` (h0,w0), `size` (h1,w1) of the resized frame, `crop` (top, left, H, W), `out_size`
    (H,W), `cameras` (ncam,22) float64 (ncam 0: no rectification; 1: shared; else one per frame), `intrinsics` float32 (4,)
    of the output frame (of the first camera)."""

    def __init__(self, src_size, size, crop, cameras, intrinsics):
        self.src_size, self.size, self.crop = src_size, size, crop
        self.out_size = (crop[2], crop[3])
        self.cameras = cameras
        self.intrinsics = intrinsics
        self._tables = {}

    @property
    def rectifies(self):
        return self.cameras.shape[0] > 0

    @property
    def resizes(self):
        return self.size != self.src_size

    def table(self, device):
        """The cameras as a device table (ncam,22) float64, uploaded once per device."""
        t = self._tables.get(device)
        if t is None:
            no_upload_while_capturing("intake.Plan.table", device if isinstance(device, torch.device) else torch.device(device))
            t = self._tables[device] = torch.from_numpy(self.cameras).to(device)
        return t


def plan(src_size, camera, dist=None, rectify=None, resize=None, crop=None):
    """The per-camera parameters of an intake, in double.

    src_size (h0,w0) of the raw frame; camera (fx, fy, cx, cy) or a 3x3 matrix; dist 4 or 5 coefficients k1 k2 p1 p2 [k3]
    (cv2.undistort's) or None; rectify (R, P): the rectifying rotation and the new camera matrix (3x3 or 3x4,
    cv2.initUndistortRectifyMap's) or None; resize (h1,w1) or None; crop (top, left, H, W) of the resized frame or None.
    camera, dist and rectify may each be a sequence with one entry per frame of the batch (a stereo pair has two).
    With neither dist nor rectify the frame is not resampled by a map; with resize None or equal to src_size not resized."""
    h0, w0 = (int(v) for v in src_size)
    if h0 < 1 or w0 < 1:
        raise RuntimeError("src_size must be (h0,w0) with both at least 1, got %s" % (tuple(src_size),))
    cams, many_c = _per_frame(camera, _is_one_camera)
    dists, many_d = _per_frame(dist, _is_one_dist)
    rects, many_r = _per_frame(rectify, _is_one_rectify)
    counts = {len(v) for v, many in ((cams, many_c), (dists, many_d), (rects, many_r)) if many}
    if len(counts) > 1:
        raise RuntimeError("camera, dist and rectify given per frame must have the same number of entries, got %s" % sorted(counts))
    ncam = counts.pop() if counts else 1
    if ncam < 1:
        raise RuntimeError("camera, dist and rectify given per frame must have at least one entry")
    rows, news = [], []
    for i in range(ncam):
        K = _k4(cams[i if many_c else 0], "camera")
        d = dists[i if many_d else 0]
        r = rects[i if many_r else 0]
        coeff = np.zeros(5)
        if d is not None:
            d = np.asarray(d, dtype=np.float64).reshape(-1)
            if d.size not in (4, 5):
                raise RuntimeError("dist must have 4 or 5 coefficients (k1, k2, p1, p2[, k3]), got %d" % d.size)
            coeff[:d.size] = d
        if r is None:
            Kn, iR = K, np.eye(3)
        else:
            R = np.asarray(r[0], dtype=np.float64)
            if R.shape != (3, 3):
                raise RuntimeError("rectify must be (R, P) with R 3x3, got R of shape %s" % (R.shape,))
            Kn, iR = _k4(r[1], "rectify's new camera matrix"), np.linalg.inv(R)
        rows.append(np.concatenate([K, Kn, iR.reshape(9), coeff]))
        news.append(Kn)
    stage1 = dist is not None or rectify is not None
    cameras = np.ascontiguousarray(np.stack(rows)) if stage1 else np.zeros((0, CAMERA_DOUBLES))
    h1, w1 = (h0, w0) if resize is None else (int(v) for v in resize)
    if h1 < 1 or w1 < 1:
        raise RuntimeError("resize must be (h1,w1) with both at least 1, got %s" % (tuple(resize),))
    top, left, H, W = (0, 0, h1, w1) if crop is None else (int(v) for v in crop)
    if top < 0 or left < 0 or H < 0 or W < 0 or top + H > h1 or left + W > w1:
        raise RuntimeError("crop (top, left, H, W) = %s lies outside the resized frame %dx%d" % ((top, left, H, W), h1, w1))
    fx, fy, cx, cy = news[0]
    intr = np.array([fx * (w1 / w0), fy * (h1 / h0), cx * (w1 / w0) - left, cy * (h1 / h0) - top])
    return Plan((h0, w0), (h1, w1), (top, left, H, W), cameras, torch.from_numpy(intr.astype(np.float32)))


def _demo(h0, w0, calib, crop8=False):
    """demo.py / demo_depth.py: calib = fx fy cx cy [k1 k2 p1 p2 [k3]]; the frame is undistorted when coefficients are
    given, resized to (int(h0 s), int(w0 s)) with s = sqrt(384 512 / (h0 w0)); crop8 (demo_depth.py) cuts both sizes down
    to multiples of 8."""
    calib = np.asarray(calib, dtype=np.float64).reshape(-1)
    if calib.size < 4:
        raise RuntimeError("calib must start with fx, fy, cx, cy, got %d numbers" % calib.size)
    h1 = int(h0 * np.sqrt((384 * 512) / (h0 * w0)))
    w1 = int(w0 * np.sqrt((384 * 512) / (h0 * w0)))
    crop = (0, 0, h1 - h1 % 8, w1 - w1 % 8) if crop8 else None
    return plan((h0, w0), calib[:4], dist=calib[4:] if calib.size > 4 else None, resize=(h1, w1), crop=crop)


# The TUM RGB-D calibration evaluation_scripts/test_tum.py uses (freiburg1, as published with the dataset)
TUM_CAMERA = (517.3, 516.5, 318.6, 255.3)
TUM_DIST = (0.2624, -0.9531, -0.0054, 0.0026, 1.1633)


def _tum():
    """evaluation_scripts/test_tum.py: 480x640, undistort with 5 coefficients, resize to 256x352, crop 8 rows and 16
    columns on every side."""
    return plan((480, 640), TUM_CAMERA, dist=TUM_DIST, resize=(256, 352), crop=(8, 16, 240, 320))


# The EuRoC MAV stereo calibration (cam0 / cam1 intrinsics and distortion from the dataset's sensor.yaml files, the
# rectification R and P of the pair as published with the stereo examples of ORB-SLAM2's EuRoC.yaml)
EUROC_SIZE = (480, 752)
EUROC_K = ((458.654, 457.296, 367.215, 248.375), (457.587, 456.134, 379.999, 255.238))
EUROC_DIST = ((-0.28340811, 0.07395907, 0.00019359, 1.76187114e-05, 0.0), (-0.28368365, 0.07451284, -0.00010473, -3.555907e-05, 0.0))
EUROC_R = (((0.999966347530033, -0.001422739138722922, 0.008079580483432283),
            (0.001365741834644127, 0.9999741760894847, 0.007055629199258132),
            (-0.008089410156878961, -0.007044357138835809, 0.9999424675829176)),
           ((0.9999633526194376, -0.003625811871560086, 0.007755443660172947),
            (0.003680398547259526, 0.9999684752771629, -0.007035845251224894),
            (-0.007729688520722713, 0.007064130529506649, 0.999945173484644)))
EUROC_P = ((435.2046959714599, 435.2046959714599, 367.4517211914062, 252.2008514404297),) * 2


def _euroc(image_size=(320, 512), stereo=True):
    """evaluation_scripts/test_euroc.py: the rectified pair (left, right) of 480x752 frames, or the left camera alone,
    resized to image_size."""
    n = 2 if stereo else 1
    return plan(EUROC_SIZE, EUROC_K[:n], dist=EUROC_DIST[:n], rectify=[(EUROC_R[i], EUROC_P[i]) for i in range(n)], resize=image_size)


plan.demo = _demo
plan.tum = _tum
plan.euroc = _euroc


def route(plan):
    """The kernel `frame` picks for `plan`: "tile" (both stages and a downscale of at most TILE_MAX_SCALE) or "direct"."""
    (h0, w0), (h1, w1) = plan.src_size, plan.size
    return "tile" if plan.rectifies and plan.resizes and max(h0 / h1, w0 / w1) <= TILE_MAX_SCALE else "direct"


def _device(raw, outs):
    for t in outs:
        return t.device
    return raw.device if raw.is_cuda else torch.device("cuda", torch.cuda.current_device())


def _check(what, raw, p, normalized, mean, std, out):
    """Every refusal of frame / frame_composed, before any launch: the plan and the pair `out`, contiguity, HIP device (a
    host raw frame is admitted: it is uploaded), dtype, no autograd, then the shapes.  Returns (N, C, outs)."""
    if not isinstance(p, Plan):
        raise RuntimeError("plan must come from intake.plan, got %s" % type(p).__name__)
    outs = []
    if out is not None:
        if not isinstance(out, (tuple, list)) or len(out) != 2 or not isinstance(out[0], torch.Tensor) \
                or not (out[1] is None or isinstance(out[1], torch.Tensor)):
            raise RuntimeError("out must be a pair (image buffer, inputs buffer or None)")
        outs = [(out[0], "out image")] + ([(out[1], "out inputs")] if out[1] is not None else [])
    if len(mean) != 3 or len(std) != 3:
        raise RuntimeError("mean and std must have 3 entries")
    everything = [(raw, "raw")] + outs
    check_contiguous(everything)
    on_device = ([(raw, "raw")] if raw.is_cuda else []) + outs       # a host frame is uploaded; buffers are never
    if on_device:
        check_device(on_device)
    check_dtype([(raw, "raw")], torch.uint8)
    check_dtype(outs[:1], torch.uint8)
    check_dtype(outs[1:], torch.float32)
    check_no_grad(what, everything)
    h0, w0 = p.src_size
    if raw.dim() not in (3, 4) or tuple(raw.shape[1:3]) != (h0, w0) or (raw.dim() == 4 and raw.shape[3] != 3):
        raise RuntimeError("raw must be (N,%d,%d,3) uint8 BGR or (N,%d,%d) grey, got %s" % (h0, w0, h0, w0, tuple(raw.shape)))
    N = raw.shape[0]
    ncam = p.cameras.shape[0]
    if ncam > 1 and ncam != N:
        raise RuntimeError("the plan has %d cameras, one per frame, raw has %d frames" % (ncam, N))
    H, W = p.out_size
    if outs:
        check_shape(outs[:1], (N, 3, H, W))
        if (out[1] is not None) != bool(normalized):
            raise RuntimeError("out inputs must be given with normalized=True and only with it")
        check_shape(outs[1:], (1, N, 3, H, W))
    return N, (1 if raw.dim() == 3 else 3), outs


def _results(raw, p, N, normalized, out):
    dev = _device(raw, [t for t in (out or ()) if t is not None])
    H, W = p.out_size
    if out is not None:
        return dev, out[0], out[1]
    image = torch.empty((N, 3, H, W), dtype=torch.uint8, device=dev)
    return dev, image, (torch.empty((1, N, 3, H, W), dtype=torch.float32, device=dev) if normalized else None)


def frame(raw, plan, normalized=True, mean=features.IMAGENET_MEAN, std=features.IMAGENET_STD, out=None, path=None):
    """`(image, inputs)` of the decoded frames `raw` under `plan`, in one launch.

    raw (N,h0,w0,3) uint8 BGR as decoders deliver it, or (N,h0,w0) grey (replicated), on the host (uploaded as it is) or the
    device.  image (N,3,H,W) uint8 BGR planar: what track takes as `image[None]` and `video.images` stores.  inputs
    (1,N,3,H,W) float32 RGB with the bits of features.normalize_images(image, mean, std), or None with normalized=False.
    out=(image_buf, inputs_buf or None): written in place and returned, nothing is allocated.  path: None picks the kernel
    (TILE_MAX_SCALE), "tile" / "direct" ask for one (same bytes; measurements and tests).  N == 0 or an empty output:
    nothing is launched.  No autograd."""
    N, C, _ = _check("frame", raw, plan, normalized, mean, std, out)
    if path not in _PATHS:
        raise RuntimeError("path must be None, 'tile' or 'direct', got %r" % (path,))
    p = plan
    H, W = p.out_size
    if N * H * W and N * H * W < MIN_FUSED_PIXELS:
        return frame_composed(raw, p, normalized=normalized, mean=mean, std=std, out=out)
    dev, image, inputs = _results(raw, p, N, normalized, out)
    if N * H * W == 0:
        return image, inputs
    if not raw.is_cuda:
        raw = raw.to(dev)
    (h0, w0), (h1, w1), (top, left, _, _) = p.src_size, p.size, p.crop
    ncam = p.cameras.shape[0]
    if path is None:
        path = route(p)
    args = _lib.IntakeArgs(raw=_ptr(raw), image=_ptr(image), inputs=None if inputs is None else _ptr(inputs), N=N, h0=h0, w0=w0,
                           C=C, h1=h1, w1=w1, top=top, left=left, H=H, W=W, ncam=ncam, path=_PATHS[path])
    args.mean[:] = [float(v) for v in mean]
    args.std[:] = [float(v) for v in std]
    table = None
    if ncam > 2:
        table = p.table(dev)
        args.cam_table = _ptr(table)
    else:
        for i in range(ncam):
            ctypes.memmove(ctypes.byref(args.cam[i]), p.cameras[i].ctypes.data, CAMERA_DOUBLES * 8)
    launch("lgu_intake_frame_u8", "frame", dev, args, _stream(image))
    launches["fused"] += 1
    return image, inputs


def _gather(raw, n_idx, y, x):
    """raw (N,h,w,3) int64 at integer positions (N,h',w'), 0 outside the frame."""
    h, w = raw.shape[1:3]
    ok = (y >= 0) & (y < h) & (x >= 0) & (x < w)
    return raw[n_idx, y.clamp(0, h - 1), x.clamp(0, w - 1)] * ok[..., None]


def _quantise(m):
    t = torch.floor(m * 32.0 + 0.5)
    lim = float(1 << 30)
    t = torch.where(t >= -lim, t, torch.full_like(t, -lim))
    t = torch.where(t <= lim, t, torch.full_like(t, lim))
    return t.to(torch.int64)


def _rectify_composed(img, cams):
    """Stage 1 on img (N,h,w,3) int64 with cams (1|N,22) float64 on the device: every operand of a product, sum or quotient
    is a tensor (a tensor divided by a Python number would be multiplied by the reciprocal)."""
    N, h, w, _ = img.shape
    c = [cams[:, i].reshape(-1, 1, 1) for i in range(CAMERA_DOUBLES)]
    k, kn, ir, d = c[0:4], c[4:8], c[8:17], c[17:22]
    u = torch.arange(w, dtype=torch.float64, device=img.device).reshape(1, 1, w)
    v = torch.arange(h, dtype=torch.float64, device=img.device).reshape(1, h, 1)
    x = ((u - kn[2]) / kn[0]).expand(-1, h, w)
    y = ((v - kn[3]) / kn[1]).expand(-1, h, w)
    X = (ir[0] * x + ir[1] * y) + ir[2]
    Y = (ir[3] * x + ir[4] * y) + ir[5]
    Wn = (ir[6] * x + ir[7] * y) + ir[8]
    x, y = X / Wn, Y / Wn
    x2, y2 = x * x, y * y
    r2 = x2 + y2
    rad = 1.0 + r2 * (d[0] + r2 * (d[1] + r2 * d[4]))
    t = 2.0 * (x * y)
    xd = (x * rad + d[2] * t) + d[3] * (r2 + 2.0 * x2)
    yd = (y * rad + d[2] * (r2 + 2.0 * y2)) + d[3] * t
    qx, qy = _quantise(xd * k[0] + k[2]).expand(N, h, w), _quantise(yd * k[1] + k[3]).expand(N, h, w)
    ix, iy = qx >> 5, qy >> 5
    ax, ay = (qx & 31)[..., None], (qy & 31)[..., None]
    n_idx = torch.arange(N, device=img.device).reshape(N, 1, 1).expand(N, h, w)
    acc = (_gather(img, n_idx, iy, ix) * (32 - ax) * (32 - ay) + _gather(img, n_idx, iy, ix + 1) * ax * (32 - ay)
           + _gather(img, n_idx, iy + 1, ix) * (32 - ax) * ay + _gather(img, n_idx, iy + 1, ix + 1) * ax * ay)
    return (acc + 512) >> 10


def _resize_taps(n_out, n_in, device):
    o = torch.arange(n_out, dtype=torch.float64, device=device)
    f = (o + 0.5) * torch.full((), n_in / n_out, dtype=torch.float64, device=device) - 0.5
    fl = torch.floor(f)
    i0 = fl.to(torch.int64)
    a = f - fl
    low, high = i0 < 0, i0 >= n_in - 1
    zero = torch.zeros_like(a)
    i0 = torch.where(low, torch.zeros_like(i0), i0)
    a = torch.where(low, zero, a)
    i0 = torch.where(high, torch.full_like(i0, n_in - 1), i0)
    a = torch.where(high, zero, a)
    i1 = (i0 + 1).clamp(max=n_in - 1)
    return i0, i1, torch.floor(a * 2048.0 + 0.5).to(torch.int64)


def _resize_composed(img, h1, w1):
    h, w = img.shape[1:3]
    y0, y1, ky = _resize_taps(h1, h, img.device)
    x0, x1, kx = _resize_taps(w1, w, img.device)
    wy0, wy1 = (2048 - ky).reshape(1, -1, 1, 1), ky.reshape(1, -1, 1, 1)
    wx0, wx1 = (2048 - kx).reshape(1, 1, -1, 1), kx.reshape(1, 1, -1, 1)
    top, bot = img[:, y0], img[:, y1]
    acc = top[:, :, x0] * wy0 * wx0 + top[:, :, x1] * wy0 * wx1 + bot[:, :, x0] * wy1 * wx0 + bot[:, :, x1] * wy1 * wx1
    return (acc + (1 << 21)) >> 22


def frame_composed(raw, plan, normalized=True, mean=features.IMAGENET_MEAN, std=features.IMAGENET_STD, out=None):
    """`frame` as a composition of torch operators on the device (float64 tensors for the map, int64 for the pixel
    arithmetic, features.normalize_images for the floats): same arguments, results and refusals."""
    N, C, _ = _check("frame", raw, plan, normalized, mean, std, out)
    p = plan
    H, W = p.out_size
    dev, image, inputs = _results(raw, p, N, normalized, out)
    if N * H * W == 0:
        return image, inputs
    launches["composed"] += 1
    if not raw.is_cuda:
        raw = raw.to(dev)
    img = (raw[..., None].expand(-1, -1, -1, 3) if C == 1 else raw).to(torch.int64)
    if p.rectifies:
        img = _rectify_composed(img, p.table(dev))
    if p.resizes:
        img = _resize_composed(img, *p.size)
    top, left, _, _ = p.crop
    image.copy_(img[:, top:top + H, left:left + W].permute(0, 3, 1, 2))
    if normalized:
        inputs.copy_(features.normalize_images(image, mean, std))
    return image, inputs


def sensor_disparity(raw_depth, plan, scale=1e-3, out=None):
    """The `disps_sens` row of depth_video.py:64-66 from the raw depth image, in one launch: the depth `raw_depth * scale`
    resized to the plan's size as F.interpolate(mode='bilinear', align_corners=False) does in double, cropped as the
    frame, sampled at [3::8, 3::8], `where(d > 0, 1/d, d)`, rounded to float32 once.  Only the sampled points are computed.
    The depth is not undistorted (the reference does not do that either).

    raw_depth (h0,w0) or (N,h0,w0), uint16 or float32, host (uploaded as it is) or device; out: a float32 buffer of the
    result's shape, (len(range(3, H, 8)), len(range(3, W, 8))) behind the leading N if raw_depth has one."""
    p = plan
    if not isinstance(p, Plan):
        raise RuntimeError("plan must come from intake.plan, got %s" % type(p).__name__)
    outs = [(out, "out")] if out is not None else []
    everything = [(raw_depth, "raw_depth")] + outs
    check_contiguous(everything)
    on_device = ([(raw_depth, "raw_depth")] if raw_depth.is_cuda else []) + outs
    if on_device:
        check_device(on_device)
    check_dtype([(raw_depth, "raw_depth")], (torch.uint16, torch.float32))
    check_dtype(outs, torch.float32)
    check_no_grad("sensor_disparity", everything)
    h0, w0 = p.src_size
    if raw_depth.dim() not in (2, 3) or tuple(raw_depth.shape[-2:]) != (h0, w0):
        raise RuntimeError("raw_depth must be (%d,%d) or (N,%d,%d), got %s" % (h0, w0, h0, w0, tuple(raw_depth.shape)))
    H, W = p.out_size
    shape = tuple(raw_depth.shape[:-2]) + (len(range(3, H, 8)), len(range(3, W, 8)))
    check_shape(outs, shape)
    dev = _device(raw_depth, [out] if out is not None else [])
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=dev)
    if out.numel() == 0:
        return out
    if not raw_depth.is_cuda:
        raw_depth = raw_depth.to(dev)
    (h1, w1), (top, left, _, _) = p.size, p.crop
    args = _lib.IntakeDepthArgs(raw=_ptr(raw_depth), out=_ptr(out), scale=float(scale), N=(raw_depth.shape[0] if raw_depth.dim() == 3 else 1),
                                h0=h0, w0=w0, h1=h1, w1=w1, top=top, left=left, H=H, W=W, src_u16=int(raw_depth.dtype == torch.uint16))
    launch("lgu_intake_depth_f32", "sensor_disparity", dev, args, _stream(out))
    return out
