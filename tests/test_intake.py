"""The frame intake (lgu_slam_amd.intake, csrc/intake.hip): rectify, resize, crop and normalise a decoded frame in one launch.

CPU: the ABI, the refusals and their precedence, the numpy restatement tests/intake_restatement.py against facts that can be
worked out by hand and against the framework's own interpolation, the intrinsics of the three named rules, and the cap on
the pixels the GPU comparison may leave out.  GPU: `frame` against the restatement byte for byte, leaving out only pixels
where a contributing stage-1 coordinate has 32 m + 0.5 within 1e-6 of an integer (double arithmetic over about 20 operations
on coordinates up to 1e4 errs by about 1e-10) and at most 1 % of a case's pixels; `inputs` against features.normalize_images
bit for bit; `sensor_disparity` against the reference's own operators to 1 float32 ulp.
"""
import ctypes

import numpy as np
import pytest

from tests import intake_restatement as R

torch = pytest.importorskip("torch")
F = torch.nn.functional

INTAKE_ENTRIES = ("lgu_intake_frame_u8", "lgu_intake_depth_f32")
EXCLUSION_CAP = 0.01
TUM_DIST = (0.2624, -0.9531, -0.0054, 0.0026, 1.1633)


def _rot(rx, ry, rz):
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    return (np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]]) @ np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
            @ np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]]))


# name -> (seed, raw shape, plan arguments, frame arguments).  The camera of a small frame is the TUM camera scaled to it.
def _cam(h, w):
    return (517.3 * w / 640, 516.5 * h / 480, 318.6 * w / 640, 255.3 * h / 480)


_STEREO = dict(camera=[_cam(40, 56), (47.1, 44.2, 29.3, 18.9)], dist=[TUM_DIST, (-0.2834, 0.0739, 0.0002, 1.76e-05, 0.0)],
               rectify=[(_rot(0.007, 0.008, -0.0014), (43.5, 43.5, 27.4, 20.2)), (_rot(-0.007, 0.0077, 0.0037), (43.5, 43.5, 27.4, 20.2))])
CASES = {
    "tum5": (1, (1, 40, 56, 3), dict(camera=_cam(40, 56), dist=TUM_DIST, resize=(24, 32)), {}),
    "upscale4": (2, (1, 30, 44, 3), dict(camera=_cam(30, 44), dist=TUM_DIST[:4], resize=(45, 66)), {}),
    "direct": (3, (1, 48, 64, 3), dict(camera=_cam(48, 64), dist=TUM_DIST, resize=(16, 24)), {}),
    "ragged": (4, (1, 40, 56, 3), dict(camera=_cam(40, 56), dist=TUM_DIST, resize=(27, 38), crop=(3, 5, 19, 27)), {}),
    "resize_only": (5, (2, 40, 56, 3), dict(camera=_cam(40, 56), resize=(24, 32)), {}),
    "rectify_only": (6, (1, 40, 56, 3), dict(camera=_cam(40, 56), dist=TUM_DIST), {}),
    "neither": (7, (2, 19, 27, 3), dict(camera=_cam(19, 27)), {}),
    "stereo": (8, (2, 40, 56, 3), dict(resize=(24, 32), **_STEREO), {}),
    "shared16": (9, (16, 40, 56, 3), dict(camera=_cam(40, 56), dist=TUM_DIST, resize=(24, 32), crop=(0, 0, 24, 32)), {}),
    "grey": (10, (2, 40, 56), dict(camera=_cam(40, 56), dist=TUM_DIST, resize=(24, 32)), {}),
    "strong": (11, (1, 40, 56, 3), dict(camera=_cam(40, 56), dist=(3.0, 0.5, 0.01, -0.02, 0.0), resize=(24, 32)), {}),
    # further paths of the code: a device table of cameras (more than two), several tiles on both axes, a tile whose
    # rectangle exceeds the LDS budget (the tile kernel computes it directly), the kernel that is not the routed one
    "table3": (12, (3, 30, 44, 3), dict(camera=[_cam(30, 44), (40.0, 38.0, 20.0, 16.0), (33.0, 36.0, 23.5, 14.0)],
                                        dist=[TUM_DIST, TUM_DIST[:4], (0.1, -0.05, 0.001, 0.002)], resize=(20, 36)), {}),
    "tiles": (13, (1, 60, 100, 3), dict(camera=_cam(60, 100), dist=TUM_DIST, resize=(41, 70)), {}),
    "steep_tile": (14, (1, 64, 128, 3), dict(camera=_cam(64, 128), dist=TUM_DIST, resize=(16, 24)), dict(path="tile")),
    "tum5_tile": (1, (1, 40, 56, 3), dict(camera=_cam(40, 56), dist=TUM_DIST, resize=(24, 32)), dict(path="tile")),
    "ragged_direct": (4, (1, 40, 56, 3), dict(camera=_cam(40, 56), dist=TUM_DIST, resize=(27, 38), crop=(3, 5, 19, 27)), dict(path="direct")),
    # on the threshold between the two kernels (a downscale of 1.5 on both axes: the tile kernel) and just beyond it
    "at_threshold": (15, (1, 48, 60, 3), dict(camera=_cam(48, 60), dist=TUM_DIST, resize=(32, 40)), {}),
    "past_threshold": (15, (1, 48, 60, 3), dict(camera=_cam(48, 60), dist=TUM_DIST, resize=(32, 39)), {}),
    "direct_tile": (3, (1, 48, 64, 3), dict(camera=_cam(48, 64), dist=TUM_DIST, resize=(16, 24)), dict(path="tile")),
}
_REF = {}


def make_plan(lgu, name):
    _, shape, kw, _ = CASES[name]
    return lgu.intake.plan(shape[1:3], **kw)


def reference(lgu, name):
    """(raw, image, fragile) of a case: the restatement on the cameras the plan packs, computed once."""
    if name not in _REF:
        seed, shape, _, _ = CASES[name]
        raw = np.random.default_rng(seed).integers(0, 256, size=shape, dtype=np.uint8)
        p = make_plan(lgu, name)
        cams = None if p.cameras.shape[0] == 0 else (p.cameras[0] if p.cameras.shape[0] == 1 else p.cameras)
        image, fragile = R.frame(raw, cams, p.size, p.crop)
        for a in (raw, image, fragile):
            a.setflags(write=False)
        _REF[name] = (raw, image, fragile)
    return _REF[name]


# ---------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------
def test_header_declares_and_binding_carries_the_intake_entries(lgu):
    from tests.test_abi import declared_symbols
    from tests.test_alignment import pointer_entries
    syms = declared_symbols()
    lib = ctypes.CDLL(lgu.build())
    for s in INTAKE_ENTRIES:
        assert s in syms, s
        assert hasattr(lib, s), s
        assert s in lgu._lib.SIGNATURES, s
        assert s in pointer_entries(), "%s takes its operands in a block by value: the alignment audit reads the block's pointer fields" % s
    assert lgu._lib.SIGNATURES["lgu_intake_frame_u8"][0] is lgu._lib.IntakeArgs
    assert ctypes.sizeof(lgu._lib.IntakeCamera) == 22 * 8 == lgu.intake.CAMERA_DOUBLES * 8
    assert "intake" in vars(lgu) and "intake.hip" in lgu._build.SOURCES


def test_refusals_of_the_entries_need_no_device(lgu):
    lib = lgu._lib.load()
    fake = ctypes.c_void_p(4096)         # never dereferenced: every refusal below precedes the launch
    BAD, UNS = lgu._lib.LGU_E_BADARG, lgu._lib.LGU_E_UNSUPPORTED

    def args(**kw):
        base = dict(raw=fake, image=fake, N=1, h0=8, w0=8, C=3, h1=8, w1=8, top=0, left=0, H=8, W=8, ncam=0, path=0)
        base.update(kw)
        return lgu._lib.IntakeArgs(**base)

    assert lib.lgu_intake_frame_u8(args(N=0), None) == 0 and lib.lgu_intake_frame_u8(args(H=0), None) == 0
    for kw in (dict(N=-1), dict(C=2), dict(path=3), dict(top=1), dict(left=4, W=5), dict(ncam=2), dict(raw=None), dict(image=None),
               dict(h0=0, h1=4, H=4), dict(N=3, ncam=3), dict(N=3, ncam=3, cam_table=ctypes.c_void_p(4100))):
        assert lib.lgu_intake_frame_u8(args(**kw), None) == BAD, kw
    assert lib.lgu_intake_frame_u8(args(N=65536), None) == UNS
    assert lib.lgu_intake_frame_u8(args(h1=8 * 65536, H=8 * 65536), None) == UNS

    def dargs(**kw):
        base = dict(raw=fake, out=fake, scale=1e-3, N=1, h0=16, w0=16, h1=16, w1=16, top=0, left=0, H=16, W=16, src_u16=1)
        base.update(kw)
        return lgu._lib.IntakeDepthArgs(**base)

    assert lib.lgu_intake_depth_f32(dargs(N=0), None) == 0 and lib.lgu_intake_depth_f32(dargs(H=3), None) == 0
    for kw in (dict(N=-1), dict(top=1), dict(raw=None), dict(out=None), dict(h0=0)):
        assert lib.lgu_intake_depth_f32(dargs(**kw), None) == BAD, kw


@pytest.mark.parametrize("fn", ["frame", "frame_composed"])
def test_refusals_come_before_any_launch_in_their_order(lgu, monkeypatch, fn):
    def no_launch():
        raise AssertionError("the library was reached")
    monkeypatch.setattr(lgu._lib, "load", no_launch)
    I = lgu.intake
    f = getattr(I, fn)
    p = I.plan((12, 16), (10.0, 10.0, 8.0, 6.0), dist=(0.1, 0.0, 0.0, 0.0), resize=(6, 8))
    raw = torch.zeros(2, 12, 16, 3, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="^plan must come from intake.plan"):
        f(raw, (12, 16))
    with pytest.raises(RuntimeError, match="^out must be a pair"):
        f(raw, p, out=torch.zeros(2, 3, 6, 8, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="^mean and std must have 3 entries$"):
        f(raw, p, mean=(0.5, 0.5))
    # contiguity first, whatever else is wrong; then the device of the buffers; then dtype, autograd, shapes
    with pytest.raises(RuntimeError, match="^raw must be contiguous$"):
        f(torch.zeros(2, 16, 12, 3).transpose(1, 2), p)
    with pytest.raises(RuntimeError, match="^out image must be contiguous$"):
        f(raw.float(), p, out=(torch.zeros(2, 3, 8, 6, dtype=torch.uint8).transpose(2, 3), None), normalized=False)
    with pytest.raises(RuntimeError, match="^out image must be a HIP device tensor: lgu_slam_amd has no CPU fallback$"):
        f(raw.float(), p, out=(torch.zeros(2, 3, 6, 8, dtype=torch.uint8), None), normalized=False)
    monkeypatch.setattr(I, "check_device", lambda pairs: None)      # CPU tensors stand in; nothing below touches them
    with pytest.raises(RuntimeError, match=r"^expected scalar type torch.uint8 but found Float \(raw\)$"):
        f(torch.zeros(2, 12, 16, 4), p)
    with pytest.raises(RuntimeError, match=r"^expected scalar type torch.uint8 but found Float \(out image\)$"):
        f(raw, p, out=(torch.zeros(2, 3, 6, 8), None), normalized=False)
    with pytest.raises(RuntimeError, match=r"^expected scalar type Float but found Double \(out inputs\)$"):
        f(raw, p, out=(torch.zeros(2, 3, 6, 8, dtype=torch.uint8), torch.zeros(1, 2, 3, 6, 8).double()))
    with pytest.raises(RuntimeError, match="^frame has no autograd"):
        f(raw, p, out=(torch.zeros(2, 3, 6, 8, dtype=torch.uint8), torch.zeros(1, 2, 3, 6, 8).requires_grad_()))
    with pytest.raises(RuntimeError, match=r"^raw must be \(N,12,16,3\) uint8 BGR or \(N,12,16\) grey, got \(2, 12, 16, 4\)$"):
        f(torch.zeros(2, 12, 16, 4, dtype=torch.uint8), p)
    with pytest.raises(RuntimeError, match=r"^raw must be \(N,12,16,3\)"):
        f(torch.zeros(12, 16, dtype=torch.uint8), p)
    with pytest.raises(RuntimeError, match=r"^the plan has 3 cameras, one per frame, raw has 2 frames$"):
        f(raw, I.plan((12, 16), [(10.0, 10.0, 8.0, 6.0)] * 3, dist=(0.1, 0.0, 0.0, 0.0)))
    with pytest.raises(RuntimeError, match=r"^out image must be \(2, 3, 6, 8\), got \(2, 3, 6, 9\)$"):
        f(raw, p, out=(torch.zeros(2, 3, 6, 9, dtype=torch.uint8), None), normalized=False)
    with pytest.raises(RuntimeError, match="^out inputs must be given with normalized=True and only with it$"):
        f(raw, p, out=(torch.zeros(2, 3, 6, 8, dtype=torch.uint8), None))
    with pytest.raises(RuntimeError, match=r"^out inputs must be \(1, 2, 3, 6, 8\), got \(2, 3, 6, 8\)$"):
        f(raw, p, out=(torch.zeros(2, 3, 6, 8, dtype=torch.uint8), torch.zeros(2, 3, 6, 8)))
    if fn == "frame":
        with pytest.raises(RuntimeError, match="^path must be None, 'tile' or 'direct'"):
            f(raw, p, path="lds")
    # sensor_disparity
    depth = torch.zeros(12, 16)
    with pytest.raises(RuntimeError, match="^raw_depth must be contiguous$"):
        I.sensor_disparity(torch.zeros(16, 12).t(), p)
    with pytest.raises(RuntimeError, match=r"^expected scalar type torch.uint16 or Float but found Double \(raw_depth\)$"):
        I.sensor_disparity(depth.double(), p)
    with pytest.raises(RuntimeError, match=r"^raw_depth must be \(12,16\) or \(N,12,16\), got \(12, 15\)$"):
        I.sensor_disparity(torch.zeros(12, 15), p)
    with pytest.raises(RuntimeError, match=r"^out must be \(1, 1\), got \(2, 2\)$"):
        I.sensor_disparity(depth, p, out=torch.zeros(2, 2))


def test_plan_refuses_what_it_cannot_express(lgu):
    I = lgu.intake
    K = (10.0, 10.0, 8.0, 6.0)
    for n in (1, 3, 6, 8):
        with pytest.raises(RuntimeError, match=r"^dist must have 4 or 5 coefficients \(k1, k2, p1, p2\[, k3\]\), got %d$" % n):
            I.plan((12, 16), K, dist=[0.1] * n)
    with pytest.raises(RuntimeError, match="^camera must be"):
        I.plan((12, 16), (1.0, 2.0, 3.0))
    with pytest.raises(RuntimeError, match="^crop .* lies outside the resized frame 6x8$"):
        I.plan((12, 16), K, resize=(6, 8), crop=(1, 0, 6, 8))
    with pytest.raises(RuntimeError, match="must have the same number of entries"):
        I.plan((12, 16), [K, K], dist=[[0.1] * 4] * 3)
    p = I.plan((12, 16), np.array([[10.0, 0, 8.0], [0, 11.0, 6.0], [0, 0, 1]]), dist=(0.1, 0.2, 0.3, 0.4))
    assert p.cameras.shape == (1, 22) and p.cameras[0, :4].tolist() == [10.0, 11.0, 8.0, 6.0]
    assert p.cameras[0, 17:].tolist() == [0.1, 0.2, 0.3, 0.4, 0.0]
    assert np.array_equal(p.cameras[0], R.camera((10.0, 11.0, 8.0, 6.0), (0.1, 0.2, 0.3, 0.4)))
    Rm = _rot(0.01, -0.02, 0.03)
    p = I.plan((12, 16), K, rectify=(Rm, np.array([[9.0, 0, 7.0, -3.0], [0, 9.5, 5.0, 0], [0, 0, 1, 0]])))
    assert np.array_equal(p.cameras[0], R.camera(K, None, Rm, (9.0, 9.5, 7.0, 5.0)))
    assert not I.plan((12, 16), K).rectifies and not I.plan((12, 16), K, resize=(12, 16)).resizes


def test_route_picks_the_tile_kernel_up_to_the_measured_crossover(lgu):
    I = lgu.intake
    want = {"tum5": "direct", "upscale4": "tile", "direct": "direct", "ragged": "tile", "resize_only": "direct", "rectify_only": "direct",
            "neither": "direct", "tiles": "tile", "at_threshold": "tile", "past_threshold": "direct"}
    for name, kernel in want.items():
        assert I.route(make_plan(lgu, name)) == kernel, name
    assert I.TILE_MAX_SCALE == 1.5 and I.MIN_FUSED_PIXELS == 0
    assert I.route(I.plan.demo(480, 640, [500.0, 500.0, 320.0, 240.0, 0.1, 0.0, 0.0, 0.0])) == "tile"
    assert I.route(I.plan.euroc()) == "tile" and I.route(I.plan.tum()) == "direct"


def test_restatement_with_both_stages_absent_is_the_identity():
    raw = np.random.default_rng(0).integers(0, 256, size=(2, 9, 13, 3), dtype=np.uint8)
    image, fragile = R.frame(raw)
    assert np.array_equal(image, raw.transpose(0, 3, 1, 2)) and not fragile.any()
    # and each stage alone at its neutral setting: no coefficients with K' = K; a resize to the same size
    assert np.array_equal(R.rectify(raw[0], R.camera((11.0, 12.0, 6.5, 4.25)))[0], raw[0])
    assert np.array_equal(R.resize(raw[0], 9, 13), raw[0])
    grey = raw[..., 0]
    assert np.array_equal(R.frame(grey)[0], np.repeat(grey[:, None], 3, axis=1))


def test_restatement_shifts_by_three_columns_when_the_new_principal_point_is_three_to_the_right():
    """No coefficients, cx' = cx + 3, fx' = fx: pixel u of the result is pixel u - 3 of the frame, zeros enter from the border."""
    raw = np.random.default_rng(1).integers(1, 256, size=(10, 14, 3), dtype=np.uint8)
    out, _ = R.rectify(raw, R.camera((16.0, 16.0, 7.0, 5.0), None, None, (16.0, 16.0, 10.0, 5.0)))
    assert np.array_equal(out[:, 3:], raw[:, :-3]) and not out[:, :3].any()


def test_restatement_maps_the_principal_point_to_the_principal_point():
    cam = R.camera((517.25, 516.5, 318.0, 255.0), TUM_DIST, _rot(0.0, 0.0, 0.0), (400.0, 401.0, 300.0, 200.0))
    mx, my = R.rectify_coords(cam, 480, 640)
    assert mx[200, 300] == 318.0 and my[200, 300] == 255.0


@pytest.mark.parametrize("shape,size", [((40, 56), (24, 32)), ((30, 44), (45, 66)), ((48, 64), (16, 24)), ((27, 38), (27, 61))])
def test_restated_resize_lies_within_one_grey_level_of_the_float64_interpolation(shape, size):
    """12-bit weight rounding contributes at most about 0.12 grey levels and the final rounding 0.5."""
    raw = np.random.default_rng(2).integers(0, 256, size=shape + (3,), dtype=np.uint8)
    ours = R.resize(raw, *size).astype(np.float64)
    ref = F.interpolate(torch.from_numpy(raw).double().permute(2, 0, 1)[None], size, mode="bilinear", align_corners=False)
    worst = np.abs(ours - ref[0].permute(1, 2, 0).numpy()).max()
    print("worst difference %.4f grey levels" % worst)
    assert worst <= 1.0


def _ulps(a, b):
    """Distance in float32 ulps between arrays of finite values of equal sign."""
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    assert np.isfinite(a).all() and np.isfinite(b).all() and (np.signbit(a) == np.signbit(b)).all()
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


def reference_disparity(raw, scale, size, crop):
    """The reference's own operators: demo_depth.py:41,53-55 and depth_video.py:64-66."""
    depth = torch.from_numpy(np.asarray(raw).astype(np.float64) * scale)
    depth = F.interpolate(depth[None, None], size, mode="bilinear").squeeze()
    top, left, H, W = crop
    depth = depth[top:top + H, left:left + W][3::8, 3::8]
    return torch.where(depth > 0, 1.0 / depth, depth).float().numpy()


def make_depth(seed, shape, dtype):
    rng = np.random.default_rng(seed)
    d = rng.integers(300, 9000, size=shape).astype(np.float64)
    d[rng.random(shape) < 0.15] = 0
    return d.astype(np.uint16) if dtype == "u16" else (d * 1.0371).astype(np.float32)


@pytest.mark.parametrize("shape,size,crop", [((72, 104), (51, 75), (0, 0, 48, 72)), ((48, 64), (60, 81), (2, 1, 56, 80)),
                                             ((37, 53), (37, 53), (0, 0, 37, 53))])
@pytest.mark.parametrize("dtype", ["u16", "f32"])
def test_restated_sensor_disparity_is_the_reference_ops_to_one_ulp(shape, size, crop, dtype):
    raw = make_depth(3, shape, dtype)
    ours = R.sensor_disparity(raw, 1e-3, size, crop)
    ref = reference_disparity(raw, 1e-3, size, crop)
    assert ours.shape == ref.shape == (len(range(3, crop[2], 8)), len(range(3, crop[3], 8)))
    worst = int(_ulps(ours, ref).max())
    print("worst difference %d ulp" % worst)
    assert worst <= 1


def test_intrinsics_of_the_three_named_rules(lgu):
    """Against numbers typed from the reference scripts' arithmetic, to the float32 rounding of the result."""
    I = lgu.intake

    def close(p, want):
        got = p.intrinsics
        assert got.dtype == torch.float32 and tuple(got.shape) == (4,)
        assert np.allclose(got.numpy().astype(np.float64), want, rtol=2.0 ** -23, atol=0), (got.tolist(), want)

    # test_tum.py:26-50: 517.3 * 352 / 640, 516.5 * 256 / 480, 318.6 * 352 / 640 - 16, 255.3 * 256 / 480 - 8
    p = I.plan.tum()
    assert (p.src_size, p.size, p.crop, p.out_size) == ((480, 640), (256, 352), (8, 16, 240, 320), (240, 320))
    assert p.cameras.shape == (1, 22) and p.cameras[0, 17:].tolist() == [0.2624, -0.9531, -0.0054, 0.0026, 1.1633]
    close(p, [284.515, 275.46666666666667, 159.23, 128.16])
    # test_euroc.py:51-74: 435.2046959714599 * 512 / 752, * 320 / 480, 367.4517211914062 * 512 / 752, 252.2008514404297 * 320 / 480
    p = I.plan.euroc((320, 512))
    assert (p.src_size, p.size, p.out_size) == ((480, 752), (320, 512), (320, 512)) and p.cameras.shape == (2, 22)
    assert p.cameras[0, :4].tolist() == [458.654, 457.296, 367.215, 248.375] and p.cameras[1, 17] == -0.28368365
    assert np.allclose(p.cameras[0, 8:17].reshape(3, 3) @ np.array(I.EUROC_R[0]), np.eye(3), atol=1e-15)
    close(p, [296.3095802358876, 290.1364639809733, 250.17989527925528, 168.13390096028647])
    assert I.plan.euroc(stereo=False).cameras.shape == (1, 22)
    # demo.py:44-53 at 480x640: s = sqrt(384 * 512 / (480 * 640)) = 0.8, 384x512
    p = I.plan.demo(480, 640, [535.4, 539.2, 320.1, 247.6])
    assert (p.size, p.out_size) == ((384, 512), (384, 512)) and not p.rectifies
    close(p, [428.32, 431.36, 256.08, 198.08])
    # demo_depth.py:45-59 at 376x1241 (KITTI): h1 = int(376 * s) = 244, w1 = int(1241 * s) = 805, cropped to 240x800
    p = I.plan.demo(376, 1241, [718.856, 718.856, 607.1928, 185.2157, -0.1, 0.01, 0.0, 0.0], crop8=True)
    assert (p.size, p.crop, p.out_size) == ((244, 805), (0, 0, 240, 800), (240, 800)) and p.rectifies
    close(p, [718.856 * 805 / 1241, 718.856 * 244 / 376, 607.1928 * 805 / 1241, 185.2157 * 244 / 376])


@pytest.mark.parametrize("name", list(CASES))
def test_exclusion_cap_holds_for_every_gpu_case(lgu, name):
    raw, image, fragile = reference(lgu, name)
    share = float(fragile.mean())
    print("%s: %d of %d pixels left out" % (name, int(fragile.sum()), fragile.size))
    assert share <= EXCLUSION_CAP
    if name == "strong":
        outside = R.outside_share(make_plan(lgu, name).cameras[0], 40, 56)
        print("strong: %.3f of the stage-1 pixels map outside the raw frame" % outside)
        assert outside >= 0.2


# ---------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------
def dev(a):
    return torch.from_numpy(np.array(a)).cuda()         # a copy: the shared references are read-only


def check_against_reference(image, ref, fragile, what):
    got = image.cpu().numpy()
    assert got.shape == ref.shape and got.dtype == np.uint8
    keep = ~np.broadcast_to(fragile[:, None], ref.shape)
    bad = (got != ref) & keep
    print("%s: %d of %d bytes differ outside the %d pixels left out" % (what, int(bad.sum()), bad.size, int(fragile.sum())))
    assert fragile.mean() <= EXCLUSION_CAP
    assert not bad.any(), "%s: first differences at %s" % (what, np.argwhere(bad)[:5].tolist())


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_frame_has_the_bytes_of_the_restatement(lgu, name):
    raw, ref, fragile = reference(lgu, name)
    p = make_plan(lgu, name)
    image, inputs = lgu.intake.frame(dev(raw), p, **CASES[name][3])
    torch.cuda.synchronize()
    assert tuple(image.shape) == (raw.shape[0], 3) + p.out_size and tuple(inputs.shape) == (1,) + tuple(image.shape)
    check_against_reference(image, ref, fragile, name)
    if name == "neither":
        assert torch.equal(image, dev(raw).permute(0, 3, 1, 2))
    # inputs: the bits of the project's normalisation of that image, and of the restated one
    want = lgu.features.normalize_images(image)
    assert torch.equal(inputs.view(torch.int32), want.view(torch.int32))
    assert np.array_equal(inputs.cpu().numpy().view(np.int32),
                          R.normalize(image.cpu().numpy(), lgu.features.IMAGENET_MEAN, lgu.features.IMAGENET_STD).view(np.int32))


@pytest.mark.gpu
def test_inputs_follow_a_custom_mean_and_std_and_can_be_left_out(lgu):
    raw, ref, fragile = reference(lgu, "tum5")
    p = make_plan(lgu, "tum5")
    mean, std = (0.1, 0.5, 0.9), (0.3, 1.7, 0.05)
    image, inputs = lgu.intake.frame(dev(raw), p, mean=mean, std=std)
    assert torch.equal(inputs.view(torch.int32), lgu.features.normalize_images(image, mean, std).view(torch.int32))
    check_against_reference(image, ref, fragile, "tum5 with a custom mean")
    image2, none = lgu.intake.frame(dev(raw), p, normalized=False)
    assert none is None and torch.equal(image, image2)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["tum5", "upscale4", "ragged", "resize_only", "rectify_only", "neither", "stereo", "grey", "strong",
                                  "table3"])
def test_frame_equals_the_composition(lgu, name):
    raw, _, fragile = reference(lgu, name)
    p = make_plan(lgu, name)
    before = dict(lgu.intake.launches)
    image, inputs = lgu.intake.frame(dev(raw), p)
    cimage, cinputs = lgu.intake.frame_composed(dev(raw), p)
    assert lgu.intake.launches == {"fused": before["fused"] + 1, "composed": before["composed"] + 1}
    keep = ~torch.from_numpy(np.ascontiguousarray(np.broadcast_to(fragile[:, None], tuple(image.shape)))).cuda()
    bad = (image != cimage) & keep
    assert not bool(bad.any()), "%d bytes differ" % int(bad.sum())
    same = (image == cimage).flip(1)[None]          # float plane c comes from byte plane 2 - c
    assert torch.equal(inputs.view(torch.int32)[same], cinputs.view(torch.int32)[same])


@pytest.mark.gpu
def test_small_calls_route_to_the_composition(lgu, monkeypatch):
    raw, ref, fragile = reference(lgu, "tum5")
    p = make_plan(lgu, "tum5")
    size = 24 * 32
    monkeypatch.setattr(lgu.intake, "MIN_FUSED_PIXELS", size + 1)
    before = dict(lgu.intake.launches)
    image, _ = lgu.intake.frame(dev(raw), p)
    assert lgu.intake.launches == {"fused": before["fused"], "composed": before["composed"] + 1}
    check_against_reference(image, ref, fragile, "composed")
    monkeypatch.setattr(lgu.intake, "MIN_FUSED_PIXELS", size)       # read at the call: at the threshold the fused route serves
    lgu.intake.frame(dev(raw), p)
    assert lgu.intake.launches["fused"] == before["fused"] + 1


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["u16", "f32"])
def test_sensor_disparity_is_the_reference_ops_to_one_ulp(lgu, dtype):
    """72x104 -> 51x75 with 15 % zero depths, the crop of demo_depth.py (48x72)."""
    raw = make_depth(4, (72, 104), dtype)
    p = lgu.intake.plan((72, 104), _cam(72, 104), resize=(51, 75), crop=(0, 0, 48, 72))
    ref = reference_disparity(raw, 1e-3, (51, 75), (0, 0, 48, 72))
    t = torch.from_numpy(raw.view(np.uint16) if dtype == "u16" else raw)
    got = lgu.intake.sensor_disparity(t.cuda(), p)
    assert tuple(got.shape) == (6, 9) and got.dtype == torch.float32
    worst = int(_ulps(got.cpu().numpy(), ref).max())
    print("worst difference %d ulp; %d zero depths among the samples" % (worst, int((ref == 0).sum())))
    assert worst <= 1
    assert int(_ulps(got.cpu().numpy(), R.sensor_disparity(raw, 1e-3, (51, 75), (0, 0, 48, 72))).max()) <= 1
    # without a resize the samples are the raw image's own [3::8, 3::8]: a zero depth stays a zero
    same = lgu.intake.sensor_disparity(t.cuda(), lgu.intake.plan((72, 104), _cam(72, 104))).cpu().numpy()
    direct = reference_disparity(raw, 1e-3, (72, 104), (0, 0, 72, 104))
    assert (direct == 0).any() and int(_ulps(same, direct).max()) <= 1 and np.array_equal(same == 0, direct == 0)
    # a host image is uploaded as it is; a batch is served frame by frame; out= is written in place
    assert torch.equal(lgu.intake.sensor_disparity(t, p), got)
    buf = torch.full((2, 6, 9), -7.0, device="cuda")
    back = lgu.intake.sensor_disparity(torch.from_numpy(np.stack([t.numpy(), t.numpy()])).cuda(), p, out=buf)
    assert back is buf and torch.equal(buf[0], got) and torch.equal(buf[1], got)


@pytest.mark.gpu
def test_two_runs_give_identical_bits_and_host_and_device_frames_agree(lgu):
    for name in ("shared16", "stereo"):
        raw = reference(lgu, name)[0]
        p = make_plan(lgu, name)
        a = lgu.intake.frame(dev(raw), p)
        b = lgu.intake.frame(dev(raw), p)
        c = lgu.intake.frame(torch.from_numpy(np.array(raw)), p)    # host-resident
        for x, y in ((a, b), (a, c)):
            assert torch.equal(x[0], y[0]) and torch.equal(x[1].view(torch.int32), y[1].view(torch.int32))
        assert c[0].is_cuda and c[1].is_cuda


def _guarded(shape, dtype, fill, pad, offset=0):
    """A contiguous tensor of `shape` inside a sentinel-filled buffer: `pad` elements in front (plus `offset`) and behind."""
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * pad + offset,), fill, dtype=dtype, device="cuda")
    return buf, buf[pad + offset:pad + offset + n].view(shape)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["ragged", "tiles", "neither", "steep_tile"])
def test_out_buffers_are_written_in_place_and_guard_bands_stay_intact(lgu, name):
    raw, ref, fragile = reference(lgu, name)
    p = make_plan(lgu, name)
    N, (H, W) = raw.shape[0], p.out_size
    ibuf, image = _guarded((N, 3, H, W), torch.uint8, 0xA5, 64)
    fbuf, inputs = _guarded((1, N, 3, H, W), torch.float32, -12345.0, 64)
    got = lgu.intake.frame(dev(raw), p, out=(image, inputs), **CASES[name][3])
    assert got[0] is image and got[1] is inputs
    check_against_reference(image, ref, fragile, name)
    assert torch.equal(inputs.view(torch.int32), lgu.features.normalize_images(image.clone()).view(torch.int32))
    n = N * 3 * H * W
    assert bool((ibuf[:64] == 0xA5).all()) and bool((ibuf[64 + n:] == 0xA5).all())
    assert bool((fbuf[:64] == -12345.0).all()) and bool((fbuf[64 + n:] == -12345.0).all())
    dbuf, drow = _guarded((len(range(3, H, 8)), len(range(3, W, 8))), torch.float32, -12345.0, 32)
    depth = torch.from_numpy(make_depth(5, raw.shape[1:3], "u16").view(np.uint16)).cuda()
    lgu.intake.sensor_disparity(depth, p, out=drow)
    assert bool((dbuf[:32] == -12345.0).all()) and bool((dbuf[32 + drow.numel():] == -12345.0).all())
    assert bool((drow != -12345.0).all()) or drow.numel() == 0


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["tum5", "neither", "grey"])
def test_operands_at_element_alignment_are_served(lgu, name):
    """Raw frames at an odd byte address, the byte planes at an odd address, the float planes at a 4-byte address."""
    raw, ref, fragile = reference(lgu, name)
    p = make_plan(lgu, name)
    N, (H, W) = raw.shape[0], p.out_size
    rbuf = torch.zeros(raw.size + 1, dtype=torch.uint8, device="cuda")
    shifted = rbuf[1:].view(raw.shape)
    shifted.copy_(dev(raw))
    _, image = _guarded((N, 3, H, W), torch.uint8, 0, 64, offset=3)
    _, inputs = _guarded((1, N, 3, H, W), torch.float32, 0.0, 64, offset=1)
    assert shifted.data_ptr() % 2 == 1 and image.data_ptr() % 2 == 1 and inputs.data_ptr() % 8 == 4
    lgu.intake.frame(shifted, p, out=(image, inputs))
    check_against_reference(image, ref, fragile, name + " shifted")
    aligned = lgu.intake.frame(dev(raw), p)
    assert torch.equal(image, aligned[0]) and torch.equal(inputs.view(torch.int32), aligned[1].view(torch.int32))


@pytest.mark.gpu
def test_degenerate_shapes_launch_nothing(lgu, monkeypatch):
    def no_launch():
        raise AssertionError("the library was reached")
    p = make_plan(lgu, "tum5")
    empty = torch.zeros((0, 40, 56, 3), dtype=torch.uint8, device="cuda")
    monkeypatch.setattr(lgu._lib, "load", no_launch)
    image, inputs = lgu.intake.frame(empty, p)
    assert tuple(image.shape) == (0, 3, 24, 32) and tuple(inputs.shape) == (1, 0, 3, 24, 32)
    q = lgu.intake.plan((40, 56), _cam(40, 56), dist=TUM_DIST, resize=(24, 32), crop=(4, 4, 0, 8))
    image, inputs = lgu.intake.frame(torch.zeros((1, 40, 56, 3), dtype=torch.uint8, device="cuda"), q, normalized=False)
    assert tuple(image.shape) == (1, 3, 0, 8) and inputs is None
    assert tuple(lgu.intake.sensor_disparity(torch.zeros((40, 56), device="cuda"), q).shape) == (0, 1)
