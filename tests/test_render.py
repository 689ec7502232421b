"""The offscreen view of the map (lgu_slam_amd.render, csrc/render.hip): coloured points and wireframe frustums, z-buffered.

CPU: the ABI, the refusals of the entries and of render_view with their precedence, look_at, the colour-byte round trip, and
the numpy restatement tests/render_restatement.py on scenes whose image can be written down by hand.  GPU: render_view
against the restatement, the image as bytes and the depth as bit patterns; no tolerance anywhere.
"""
import ctypes

import numpy as np
import pytest

from tests import render_restatement as R

torch = pytest.importorskip("torch")

from lgu_slam_amd import render as _render  # noqa: E402,F401  the module under test: nothing here can pass without it

RENDER_ENTRIES = ("lgu_render_scratch_bytes", "lgu_render_view")
HAND_K = np.array([10.0, 10.0, 16.0, 12.0], np.float32)
HAND_SIZE = (24, 32)
IDENTITY = np.array([0, 0, 0, 0, 0, 0, 1], np.float32)
WHITE, RED = (255, 255, 255), (255, 0, 0)


# ---------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------
def test_header_declares_and_binding_carries_the_render_entries(lgu):
    from tests.test_abi import declared_symbols
    from tests.test_alignment import pointer_entries
    syms = declared_symbols()
    lib = ctypes.CDLL(lgu.build())
    for s in RENDER_ENTRIES:
        assert s in syms, s
        assert hasattr(lib, s), s
        assert s in lgu._lib.SIGNATURES, s
        # operands in a block by value: the alignment audit reads the block's pointer fields (the size helper has none)
        assert (s in pointer_entries()) == (s == "lgu_render_view"), s
    assert lgu._lib.RESTYPES["lgu_render_scratch_bytes"] is ctypes.c_longlong
    assert lgu._lib.SIGNATURES["lgu_render_view"][0] is lgu._lib.RenderArgs
    assert "render" in vars(lgu) and "render.hip" in lgu._build.SOURCES


def test_scratch_size_and_refusals_of_the_entries_need_no_device(lgu):
    """Host-side answers: 8 bytes of scratch per pixel; an image above 2^28 pixels is LGU_E_UNSUPPORTED; a scratch that is not
    16-byte aligned, a point size outside 1..8 and a near that is not finite and positive are LGU_E_BADARG; all before any
    launch."""
    lib = lgu._lib.load()
    BAD, UNS = lgu._lib.LGU_E_BADARG, lgu._lib.LGU_E_UNSUPPORTED
    for H, W in ((0, 64), (48, 0), (-1, 64), (48, -3)):
        assert lib.lgu_render_scratch_bytes(H, W) == 0
    for H, W in ((1, 1), (48, 64), (23, 37), (540, 960), (16384, 16384)):
        assert lib.lgu_render_scratch_bytes(H, W) == 8 * H * W
    fake = ctypes.c_void_p(4096)         # never dereferenced: every refusal below precedes the launch

    def args(**kw):
        base = dict(points=fake, colors=fake, view=fake, intrinsics=fake, cameras=fake, scratch=fake, image=fake, depth=fake,
                    npoints=5, near=0.01, camera_scale=0.05, ncam=2, H=48, W=64, point_size=2, color_u8=1)
        base.update(kw)
        return lgu._lib.RenderArgs(**base)

    assert lib.lgu_render_view(args(H=16385, W=16384), None) == UNS
    assert lib.lgu_render_view(args(H=0), None) == 0 and lib.lgu_render_view(args(W=0), None) == 0     # nothing to launch
    for kw in (dict(scratch=ctypes.c_void_p(4104)), dict(scratch=ctypes.c_void_p(4100)), dict(point_size=0), dict(point_size=9),
               dict(near=0.0), dict(near=-1.0), dict(near=float("nan")), dict(near=float("inf")), dict(camera_scale=float("nan")),
               dict(H=-1), dict(npoints=-1), dict(ncam=-1), dict(points=None), dict(colors=None), dict(cameras=None), dict(view=None),
               dict(intrinsics=None), dict(scratch=None), dict(image=None), dict(depth=None)):
        assert lib.lgu_render_view(args(**kw), None) == BAD, kw


def _cpu_args():
    return dict(points=torch.zeros(5, 3), colors=torch.zeros(5, 3, dtype=torch.uint8), view=torch.tensor(IDENTITY),
                intrinsics=torch.tensor(HAND_K), size=HAND_SIZE)


def test_refusals_come_before_any_launch_in_their_order(lgu, monkeypatch):
    def no_launch():
        raise AssertionError("the library was reached")
    monkeypatch.setattr(lgu._lib, "load", no_launch)

    def call(**kw):
        a = _cpu_args()
        opts = {k: kw.pop(k) for k in list(kw) if k not in a}
        a.update(kw)
        return lgu.render.render_view(a["points"], a["colors"], a["view"], a["intrinsics"], a["size"], **opts)

    cpu = "must be a HIP device tensor: lgu_slam_amd has no CPU fallback$"
    # contiguity first, whatever else is wrong; then the device, before the dtype and the shapes
    with pytest.raises(RuntimeError, match="^points must be contiguous$"):
        call(points=torch.zeros(3, 5).t(), colors=torch.zeros(5, 3).double())
    with pytest.raises(RuntimeError, match="^colors must be contiguous$"):
        call(colors=torch.zeros(3, 5).t())
    with pytest.raises(RuntimeError, match="^cameras must be contiguous$"):
        call(cameras=torch.zeros(7, 2).t())
    with pytest.raises(RuntimeError, match="^out depth must be contiguous$"):
        call(out=(torch.zeros(24, 32, 3, dtype=torch.uint8), torch.zeros(32, 24).t()))
    with pytest.raises(RuntimeError, match="^out must be a pair"):
        call(out=torch.zeros(24, 32, 3))
    with pytest.raises(RuntimeError, match="^points " + cpu):
        call(view=torch.zeros(7).double(), size=(0, 0))             # wrong dtype and size too: the device is named
    with pytest.raises(RuntimeError, match="^points " + cpu):
        call()
    # past the device check (CPU tensors stand in; nothing below touches them): dtype before shape
    monkeypatch.setattr(lgu.render, "check_device", lambda pairs: None)
    with pytest.raises(RuntimeError, match=r"^expected scalar type Float but found Double \(points\)$"):
        call(points=torch.zeros(5, 4).double())
    with pytest.raises(RuntimeError, match=r"^expected scalar type Float or torch.uint8 but found Half \(colors\)$"):
        call(colors=torch.zeros(4, 3).half())
    with pytest.raises(RuntimeError, match=r"^expected scalar type Float but found Double \(view\)$"):
        call(view=torch.zeros(6).double())
    with pytest.raises(RuntimeError, match=r"^expected scalar type Float but found Long \(intrinsics\)$"):
        call(intrinsics=torch.zeros(4).long())
    with pytest.raises(RuntimeError, match=r"^expected scalar type Float but found Double \(cameras\)$"):
        call(cameras=torch.zeros(2, 7).double())
    with pytest.raises(RuntimeError, match=r"^expected scalar type torch.uint8 but found Float \(out image\)$"):
        call(out=(torch.zeros(24, 32, 3), torch.zeros(24, 32)))
    with pytest.raises(RuntimeError, match=r"^expected scalar type Float but found Double \(out depth\)$"):
        call(out=(torch.zeros(24, 32, 3, dtype=torch.uint8), torch.zeros(24, 32).double()))
    # no autograd, after the dtypes and before the shapes
    p = torch.zeros(5, 4).requires_grad_()
    with pytest.raises(RuntimeError, match="^render_view has no autograd"):
        call(points=p)
    with torch.no_grad(), pytest.raises(RuntimeError, match=r"^points must be \(P,3\), got \(5, 4\)$"):
        call(points=p)
    # the shapes, in the order of the arguments
    with pytest.raises(RuntimeError, match=r"^points must be \(P,3\), got \(15,\)$"):
        call(points=torch.zeros(15), colors=torch.zeros(4, 3))
    with pytest.raises(RuntimeError, match=r"^colors must be \(P,3\) = \(5, 3\), got \(4, 3\)$"):
        call(colors=torch.zeros(4, 3), view=torch.zeros(6))
    with pytest.raises(RuntimeError, match=r"^view must be \(7,\) = t, q\(xyzw\), got \(1, 7\)$"):
        call(view=torch.zeros(1, 7), intrinsics=torch.zeros(3))
    with pytest.raises(RuntimeError, match="^intrinsics must be 1-D with fx, fy, cx, cy"):
        call(intrinsics=torch.zeros(3), cameras=torch.zeros(7))
    with pytest.raises(RuntimeError, match=r"^cameras must be \(K,7\) = t, q\(xyzw\), got \(7,\)$"):
        call(cameras=torch.zeros(7), point_size=0)
    # point_size, size, near and the colours; then out
    for bad in (0, 9, -1, 2.0, True, None):
        with pytest.raises(RuntimeError, match=r"^point_size must be an integer in 1\.\.8"):
            call(point_size=bad, size=(0, 0))
    for bad in ((0, 32), (24, 0), (-24, -32), (16385, 16384)):
        with pytest.raises(RuntimeError, match=r"^size must have between 1 and 2\^28 pixels"):
            call(size=bad, near=0.0)
    with pytest.raises(RuntimeError, match=r"^size must be \(H, W\)"):
        call(size=24)
    for bad in (0.0, -0.01, float("nan"), float("inf"), None):
        with pytest.raises(RuntimeError, match="^near must be finite and positive"):
            call(near=bad, background=(256, 0, 0))
    with pytest.raises(RuntimeError, match="^camera_scale must be finite"):
        call(camera_scale=float("inf"))
    with pytest.raises(RuntimeError, match=r"^background must be three integers in 0\.\.255"):
        call(background=(256, 0, 0), out=(torch.zeros(24, 32, 4, dtype=torch.uint8), torch.zeros(24, 32)))
    with pytest.raises(RuntimeError, match=r"^camera_color must be three integers in 0\.\.255"):
        call(camera_color=(0.5, 0, 0))
    with pytest.raises(RuntimeError, match=r"^out image must be \(H,W,3\) = \(24, 32, 3\), got \(24, 32, 4\)$"):
        call(out=(torch.zeros(24, 32, 4, dtype=torch.uint8), torch.zeros(24, 31)))
    with pytest.raises(RuntimeError, match=r"^out depth must be \(H,W\) = \(24, 32\), got \(24, 31\)$"):
        call(out=(torch.zeros(24, 32, 3, dtype=torch.uint8), torch.zeros(24, 31)))


def _rotate(q, X):
    """R(q) X in float64, q = (x, y, z, w)."""
    v, w = np.asarray(q[:3], np.float64), float(q[3])
    uv = 2.0 * np.cross(v, X)
    return X + w * uv + np.cross(v, uv)


@pytest.mark.parametrize("eye,target,up", [((0, 0, 0), (0, 0, 5), (0, -1, 0)), ((1, -2, -3), (0.5, 0.25, 4), (0, -1, 0)),
                                           ((3, 1, 4), (-1, 0.5, 2), (0.1, -1, 0.3)), ((0, -6, 0), (0.1, 0, 0.2), (0, 0, -1)),
                                           ((2, 2, 2), (-2, -3, -2.5), (0, 0, 1)), ((0, 0, 4), (0, 0, -1), (0, 1, 0))])
def test_look_at_places_the_camera(lgu, eye, target, up):
    pose = lgu.render.look_at(eye, target, up)
    assert pose.dtype == torch.float32 and pose.shape == (7,) and pose.device.type == "cpu"
    p = pose.double().numpy()
    t, q = p[:3], p[3:]
    eye, target, up = (np.asarray(v, np.float64) for v in (eye, target, up))
    dist = np.linalg.norm(target - eye)
    assert abs(np.linalg.norm(q) - 1) < 1e-6                                    # a unit quaternion (float32 storage)
    np.testing.assert_allclose(_rotate(q, eye) + t, 0, atol=1e-5)               # eye maps to the origin
    np.testing.assert_allclose(_rotate(q, target) + t, [0, 0, dist], atol=1e-5)  # target onto +z at its distance
    u = _rotate(q, up)
    assert abs(u[0]) < 1e-5 and u[1] < 0                                        # up into -y: x = 0, y negative
    if tuple(eye) == (0, 0, 0) and tuple(up) == (0, -1, 0):
        np.testing.assert_allclose(p, IDENTITY, atol=1e-7)                      # looking down +z from the origin: the identity


def test_look_at_refuses_degenerate_placements(lgu):
    with pytest.raises(RuntimeError, match="eye and target coincide"):
        lgu.render.look_at((1, 2, 3), (1, 2, 3))
    with pytest.raises(RuntimeError, match="up is along the line of sight"):
        lgu.render.look_at((0, 0, 0), (0, -2, 0))
    with pytest.raises(RuntimeError, match="three finite numbers"):
        lgu.render.look_at((0, 0), (0, 0, 1))


def test_colour_bytes_round_trip_in_both_float_forms():
    b = np.arange(256, dtype=np.uint8)
    fused = b.astype(np.float32) * np.float32(1.0 / 255.0)          # the fused cloud's colours
    composed = (torch.from_numpy(b) / 255.0).numpy()                # the composition's
    assert composed.dtype == np.float32
    for form in (fused, composed):
        got = R.colour_bytes(np.stack([form, form, form], -1))
        assert (got[:, 0] == b).all() and (got == got[:, :1]).all()
    odd = np.array([[np.nan, -0.2, 1.7], [np.inf, -np.inf, 0.5]], np.float32)
    assert R.colour_bytes(odd).tolist() == [[0, 0, 255], [255, 0, 128]]


def hand(points=(), colors=(), **kw):
    pts = np.asarray(points, np.float32).reshape(-1, 3)
    cols = np.asarray(colors, np.uint8).reshape(-1, 3)
    kw.setdefault("view", IDENTITY)
    return dict(points=pts, colors=cols, K=HAND_K, size=HAND_SIZE, **kw)


def restate(scene, stats=None):
    s = dict(scene)
    return R.render_view(s.pop("points"), s.pop("colors"), s.pop("view"), s.pop("K"), s.pop("size"), stats=stats, **s)


FRONT_CAMERA = np.array([[0, 0, -1.75, 0, 0, 0, 1]], np.float32)        # world-to-camera of a camera at (0, 0, 1.75)
HAND_SCENES = {
    "one_point": hand([(0, 0, 2)], [(10, 20, 30)], point_size=1),
    "size2": hand([(0, 0, 2)], [(10, 20, 30)], point_size=2),
    "size3": hand([(0, 0, 2)], [(10, 20, 30)], point_size=3),
    "occlusion": hand([(0, 0, 4), (0, 0, 2), (0, 0, 3)], [(1, 1, 1), (200, 100, 50), (2, 2, 2)], point_size=1),
    "equal_depth": hand([(0, 0, 2), (0, 0, 2), (0, 0, 2)], [(9, 0, 0), (8, 255, 255), (8, 255, 254)], point_size=1),
    "rejected": hand([(0, 0, -2), (0, 0, 0.5), (np.nan, 0, 2), (0, np.inf, 2), (0, 0, np.inf), (0, 0, 0)], [(5, 5, 5)] * 6, near=0.5),
    "corner": hand([(-3.2, -2.4, 2), (3.0, 2.2, 2)], [(1, 2, 3), (4, 5, 6)], point_size=3),
    "frustum_ahead": hand(cameras=FRONT_CAMERA, camera_scale=0.5),
    "moved_view": hand([(0.5, 0.25, 2)], [(7, 7, 7)], view=np.array([-0.5, -0.25, 2, 0, 0, 0, 1], np.float32), point_size=1),
}


def _drawn(image, background=WHITE):
    return sorted((int(y), int(x)) for y, x in zip(*np.nonzero((image != np.asarray(background, np.uint8)).any(-1))))


def test_restatement_one_point_lands_on_its_pixel_with_the_footprints_of_each_size():
    """(0,0,2) under the identity view: u = 10 * 0 + 16, v = 12.  Size 1 is the nearest pixel; size 2 starts at floor(u + 0):
    16..17 (on a pixel centre the pixel and its right / lower neighbour, between two centres the two nearest); size 3 the
    nearest +-1."""
    image, depth, _ = restate(HAND_SCENES["one_point"])
    assert _drawn(image) == [(12, 16)] and image[12, 16].tolist() == [10, 20, 30] and depth[12, 16] == 2.0
    assert np.isinf(depth).sum() == 24 * 32 - 1 and (depth[np.isinf(depth)] > 0).all()
    image, depth, _ = restate(HAND_SCENES["size2"])
    assert _drawn(image) == [(12, 16), (12, 17), (13, 16), (13, 17)] and (depth[12:14, 16:18] == 2.0).all()
    image, depth, _ = restate(HAND_SCENES["size3"])
    assert _drawn(image) == [(y, x) for y in (11, 12, 13) for x in (15, 16, 17)]
    # between two pixel centres size 2 takes the two nearest: u = 16.4 -> 16, 17; u = 15.6 -> 15, 16
    for x, cols in ((0.08, [16, 17]), (-0.08, [15, 16])):
        image, _, _ = restate(hand([(x, 0, 2)], [(1, 1, 1)], point_size=2))
        assert sorted({c for _, c in _drawn(image)}) == cols
    image, depth, _ = restate(HAND_SCENES["moved_view"])            # the view's translation moves the point to (0, 0, 4)
    assert _drawn(image) == [(12, 16)] and depth[12, 16] == 4.0


def test_restatement_orders_by_depth_then_by_packed_colour():
    image, depth, _ = restate(HAND_SCENES["occlusion"])
    assert _drawn(image) == [(12, 16)] and image[12, 16].tolist() == [200, 100, 50] and depth[12, 16] == 2.0
    image, depth, _ = restate(HAND_SCENES["equal_depth"])
    assert image[12, 16].tolist() == [8, 255, 254] and depth[12, 16] == 2.0
    for order in ([2, 1, 0], [1, 0, 2]):                             # whatever the order of the points
        s = dict(HAND_SCENES["equal_depth"])
        s["points"], s["colors"] = s["points"][order], s["colors"][order]
        assert np.array_equal(restate(s)[0], image)


def test_restatement_rejects_points_behind_at_near_and_non_finite():
    stats = {}
    image, depth, keys = restate(HAND_SCENES["rejected"], stats)
    assert _drawn(image) == [] and np.isinf(depth).all() and (keys == R.EMPTY).all()
    assert stats["points_rejected"] == 6 and stats["points_passed"] == 0
    image, _, _ = restate(hand([(0, 0, 0.5)], [(5, 5, 5)], near=0.49))     # just beyond near: drawn
    assert len(_drawn(image)) == 4


def test_restatement_clips_a_splat_at_the_corners():
    """(-3.2,-2.4,2): u = 0, v = 0, size 3 covers -1..1: the four pixels inside remain.  (3,2.2,2): u = 31, v = 23, the last
    pixel: of 30..32 by 22..24 the four pixels inside remain."""
    stats = {}
    image, _, _ = restate(HAND_SCENES["corner"], stats)
    assert _drawn(image) == [(0, 0), (0, 1), (1, 0), (1, 1), (22, 30), (22, 31), (23, 30), (23, 31)]
    assert stats["offers_inside"] == 8 and stats["offers_outside"] == 10


def test_restatement_draws_a_frustum_straight_ahead():
    """A camera at (0,0,1.75) with the view's orientation, scale 0.5: its base is the square +-0.5 at depth 1.75 + 0.75 = 2.5,
    u = 16 +- 2, v = 12 +- 2.  The base's edges are the border of rows 10..14 by columns 14..18; the apex edges and the marker
    stay inside that square (the marker's tip is at v = 12 + 10 * 0.6 / 2.5 = 14.4)."""
    stats = {}
    image, depth, _ = restate(HAND_SCENES["frustum_ahead"], stats)
    border = [(y, x) for y in range(10, 15) for x in range(14, 19) if y in (10, 14) or x in (14, 18)]
    drawn = _drawn(image)
    assert set(border) <= set(drawn) and all(10 <= y <= 14 and 14 <= x <= 18 for y, x in drawn)
    for y, x in drawn:
        assert image[y, x].tolist() == list(RED)
    for y, x in border:
        if y == 10 or x in (14, 18):        # (the lower edge shares pixels with the marker, which is at the same depth)
            assert abs(depth[y, x] - 2.5) < 1e-5
    assert (12, 16) in drawn and abs(depth[12, 16] - 1.75) < 1e-5    # the apex, in front of the base
    assert stats["segments_drawn"] == 10 and stats["segments_clipped"] == 0 and stats["segments_skipped"] == 0
    # the same camera with the view inside the frustum: the apex edges are clipped at near, the apex itself is not drawn
    stats = {}
    # (view at (0,0,1.9): apex at z = -0.15, base at 0.6; near = 0.3 cuts the apex edges at tc = 0.6, x = y = +-0.3, u = 16 +- 10)
    s = dict(HAND_SCENES["frustum_ahead"], view=np.array([0, 0, -1.9, 0, 0, 0, 1], np.float32), near=0.3)
    image, depth, _ = restate(s, stats)
    assert stats["segments_clipped"] == 4 and stats["segments_drawn"] == 10
    assert abs(depth.min() - 0.3) < 1e-6
    for y, x in ((2, 6), (2, 26), (22, 6), (22, 26)):
        assert abs(depth[y, x] - 0.3) < 1e-6 and image[y, x].tolist() == list(RED)


# ---------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------
VIEW = np.array([0.2, -0.1, 0.5, 0.05, -0.1, 0.03, 1.0])
VIEW[3:] /= np.linalg.norm(VIEW[3:])
VIEW = VIEW.astype(np.float32)


def random_scene(P=5000, seed=0, K=(40.0, 40.0, 31.5, 23.5), size=(48, 64), **kw):
    rng = np.random.default_rng(seed)
    pts = (rng.standard_normal((P, 3)) * (2.0, 1.5, 2.0) + (0.0, 0.0, 4.0)).astype(np.float32)
    cols = rng.integers(0, 256, (P, 3), dtype=np.uint8)
    return dict(points=pts, colors=cols, view=VIEW, K=np.asarray(K, np.float32), size=size, **kw)


def six_cameras():
    """World-to-camera poses of six cameras around the random scene (its centre is (0,0,4)); the view's own centre is near
    (-0.3, 0.2, -0.5).  Camera 3 sits on the view (it straddles the near plane), camera 4 at the right edge of the image,
    camera 5 behind the view."""
    import lgu_slam_amd as lgu
    centre = (0.0, 0.0, 4.0)
    eyes = [(2.5, 0.0, 1.0), (-2.0, 0.5, 2.0), (0.0, -1.5, 0.5), (-0.28, 0.18, -0.62), (2.2, 0.3, 2.0), (0.0, 0.0, -3.0)]
    return np.stack([lgu.render.look_at(e, centre).numpy() for e in eyes])


_REF = {}


def reference(name, make):
    """(scene, image, depth, stats) of a named scene: the restatement, computed once and never modified."""
    if name not in _REF:
        scene, stats = make(), {}
        image, depth, _ = restate(scene, stats)
        for a in (image, depth):
            a.setflags(write=False)
        _REF[name] = (scene, image, depth, stats)
    return _REF[name]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def run(lgu, scene, **over):
    s = dict(scene, **over)
    cams = s.pop("cameras", None)
    with torch.no_grad():
        return lgu.render.render_view(dev(s.pop("points")), dev(s.pop("colors")), dev(s.pop("view")), dev(s.pop("K")), s.pop("size"),
                                      cameras=None if cams is None else dev(cams), **s)


def assert_same(got, image, depth, what=""):
    gi, gd = got[0].cpu().numpy(), got[1].cpu().numpy()
    assert gi.dtype == np.uint8 and gd.dtype == np.float32 and gi.shape == image.shape and gd.shape == depth.shape, what
    bad_i = int((gi != image).any(-1).sum())
    bad_d = int((gd.view(np.uint32) != depth.view(np.uint32)).sum())
    assert bad_i == 0 and bad_d == 0, "%s: %d pixels differ in colour, %d in depth bits" % (what, bad_i, bad_d)


def assert_random_scene_exercises_everything(scene, stats, background=True):
    """Contested pixels, clipped offers, rejected points and (with `background`) empty pixels are all present."""
    H, W = scene["size"]
    print("points passed %d, offers inside %d, outside %d, covered %d of %d" % (stats["points_passed"], stats["offers_inside"],
                                                                               stats["offers_outside"], stats["covered"], H * W))
    assert stats["offers_inside"] > stats["covered"] > 0           # more offers than covered pixels: pixels are contested
    assert stats["offers_outside"] > 0                             # offers fall off the image
    assert stats["points_rejected"] > 0                            # points behind the near plane
    assert stats["covered"] < H * W or not background              # background remains


@pytest.mark.gpu
def test_random_scene_has_the_bytes_of_the_restatement(lgu):
    scene, image, depth, stats = reference("random", random_scene)
    assert_random_scene_exercises_everything(scene, stats)
    assert stats["offers_inside"] > 3 * stats["covered"]           # several offers per covered pixel on average
    before = lgu.render.launches["fused"]
    got = run(lgu, scene)
    assert lgu.render.launches["fused"] == before + 1
    assert_same(got, image, depth, "uint8 colours")
    # the float32 colours of the fused cloud and of the composition give the same bytes
    as_float = scene["colors"].astype(np.float32) * np.float32(1.0 / 255.0)
    assert_same(run(lgu, scene, colors=as_float), image, depth, "float32 colours")
    assert_same(run(lgu, scene, colors=(torch.from_numpy(scene["colors"]) / 255.0).numpy()), image, depth, "byte / 255.0")
    # arbitrary float colours (out of range, NaN) against the restatement of the same floats
    wild = np.random.default_rng(1).standard_normal(scene["colors"].shape).astype(np.float32) + 0.5
    wild[::97] = np.nan
    wi, wd, _ = restate(dict(scene, colors=wild))
    assert_same(run(lgu, scene, colors=wild), wi, wd, "wild float colours")


@pytest.mark.gpu
@pytest.mark.parametrize("point_size", [1, 3, 8])
def test_random_scene_at_other_point_sizes(lgu, point_size):
    scene, image, depth, stats = reference("random_s%d" % point_size, lambda: random_scene(point_size=point_size))
    assert_random_scene_exercises_everything(scene, stats, background=point_size < 8)   # 8x8 splats cover all of 48x64
    assert_same(run(lgu, scene), image, depth, "point_size %d" % point_size)


def odd_scene():
    return random_scene(P=4097, seed=3, K=(25.0, 27.0, 17.3, 11.8), size=(23, 37), cameras=six_cameras(), camera_scale=0.3,
                        background=(10, 20, 30), camera_color=(0, 200, 255))


@pytest.mark.gpu
def test_odd_view_and_point_count(lgu):
    """23x37 = 851 pixels and 4097 points: no size is a multiple of the wave, the workgroup or the vector widths of the clear
    and resolve passes."""
    scene, image, depth, stats = reference("odd", odd_scene)
    assert_random_scene_exercises_everything(scene, stats)
    assert_same(run(lgu, scene), image, depth, "odd")


@pytest.mark.gpu
def test_result_does_not_depend_on_order_run_or_atomic_form(lgu, monkeypatch):
    scene, image, depth, _ = reference("random", random_scene)
    perm = np.random.default_rng(5).permutation(len(scene["points"]))
    assert_same(run(lgu, scene, points=scene["points"][perm], colors=scene["colors"][perm]), image, depth, "permuted")
    a, b = run(lgu, scene), run(lgu, scene)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))
    assert_same(b, image, depth, "second run")
    # the other form of the offer (a load before the atomic) and a grid of two workgroups whose threads stride over the points
    assert lgu._lib.debug_knobs_enabled()
    monkeypatch.setenv("LGU_RENDER_PRELOAD", "1")
    assert_same(run(lgu, scene), image, depth, "load before the atomic")
    monkeypatch.setenv("LGU_RENDER_PRELOAD", "0")
    assert_same(run(lgu, scene), image, depth, "atomic only")
    monkeypatch.setenv("LGU_RENDER_MAX_BLOCKS", "2")
    assert_same(run(lgu, scene), image, depth, "grid stride")


def frustum_scene(with_points):
    s = random_scene(cameras=six_cameras(), camera_scale=0.5)
    if not with_points:
        s["points"], s["colors"] = s["points"][:0], s["colors"][:0]
    return s


@pytest.mark.gpu
@pytest.mark.parametrize("with_points", [False, True], ids=["alone", "with_points"])
def test_frustums_have_the_bytes_of_the_restatement(lgu, with_points):
    scene, image, depth, stats = reference("frustums_%d" % with_points, lambda: frustum_scene(with_points))
    print(stats)
    assert stats["segments_clipped"] > 0            # a camera straddles the near plane
    assert stats["segments_crossing_edge"] > 0      # a segment leaves the image
    assert stats["segments_skipped"] > 0            # a camera (or part of one) is behind the view
    assert stats["segments_drawn"] >= 30 and stats["samples_inside"] > 100
    red = int((image == np.asarray(RED, np.uint8)).all(-1).sum())
    assert red > 50                                 # frustum pixels survive in the picture
    assert_same(run(lgu, scene), image, depth, "frustums")
    if with_points:                                 # points occlude some frustum pixels and the other way round
        _, alone, _, _ = reference("frustums_0", lambda: frustum_scene(False))
        was_red = (alone == np.asarray(RED, np.uint8)).all(-1)
        now_red = (image == np.asarray(RED, np.uint8)).all(-1)
        assert (was_red & ~now_red).any() and (was_red & now_red).any()


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(HAND_SCENES))
def test_hand_scenes_on_the_device(lgu, name):
    scene, image, depth, _ = reference("hand_" + name, lambda: HAND_SCENES[name])
    assert_same(run(lgu, scene), image, depth, name)


@pytest.mark.gpu
def test_render_writes_nothing_outside_its_tensors(lgu):
    """out buffers cut from larger sentinel-filled tensors, at byte / element alignment (the scalar resolve) and at 16 bytes
    (the vector resolve): nothing outside image and depth changes, every element inside is written."""
    for name, make in (("odd", odd_scene), ("random", random_scene)):
        scene, image, depth, _ = reference(name, make)
        H, W = scene["size"]
        for pad_i, pad_d in ((5, 3), (16, 4)):
            big_i = torch.full((H * W * 3 + 2 * pad_i,), 77, dtype=torch.uint8, device="cuda")
            big_d = torch.full((H * W + 2 * pad_d,), 1234.5, device="cuda")
            buf_i, buf_d = big_i[pad_i:pad_i + H * W * 3].view(H, W, 3), big_d[pad_d:pad_d + H * W].view(H, W)
            got = run(lgu, scene, out=(buf_i, buf_d))
            torch.cuda.synchronize()
            assert got[0] is buf_i and got[1] is buf_d
            assert_same(got, image, depth, "%s pad %d" % (name, pad_i))
            assert bool((big_i[:pad_i] == 77).all()) and bool((big_i[pad_i + H * W * 3:] == 77).all())
            assert bool((big_d[:pad_d] == 1234.5).all()) and bool((big_d[pad_d + H * W:] == 1234.5).all())
    assert not (image == 77).all(-1).all() and not (depth == 1234.5).any()      # the sentinels are not the answer


@pytest.mark.gpu
def test_no_points_and_no_cameras_give_background(lgu):
    for size in ((5, 7), (48, 64)):
        empty = dict(points=np.zeros((0, 3), np.float32), colors=np.zeros((0, 3), np.uint8), view=VIEW, K=HAND_K, size=size)
        for cams in (None, np.zeros((0, 7), np.float32)):
            image, depth = run(lgu, empty, cameras=cams, background=(1, 2, 3))
            assert image.shape == (*size, 3) and depth.shape == size
            assert bool((image == torch.tensor([1, 2, 3], dtype=torch.uint8, device="cuda")).all())
            assert bool(torch.isposinf(depth).all())
        image, depth = run(lgu, dict(empty, colors=np.zeros((0, 3), np.float32)))
        assert bool((image == 255).all()) and bool(torch.isposinf(depth).all())


@pytest.mark.gpu
def test_call_enqueues_on_the_current_stream(lgu):
    scene, image, depth, _ = reference("frustums_1", lambda: frustum_scene(True))
    ops = [dev(scene[k]) for k in ("points", "colors", "view", "K", "cameras")]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s), torch.no_grad():
        big = torch.randn(1 << 22, device="cuda").sort().values        # work queued on s in front of the call
        pts = ops[0] + 0 * big[:1]                                      # the points exist only once s has got there
        got = lgu.render.render_view(pts, *ops[1:4], scene["size"], cameras=ops[4], camera_scale=0.5)
    s.synchronize()
    assert_same(got, image, depth, "side stream")


@pytest.mark.gpu
def test_call_reads_nothing_on_the_host(lgu):
    scene, image, depth, _ = reference("frustums_1", lambda: frustum_scene(True))
    ops = [dev(scene[k]) for k in ("points", "colors", "view", "K", "cameras")]
    out = (torch.empty((*scene["size"], 3), dtype=torch.uint8, device="cuda"), torch.empty(scene["size"], device="cuda"))
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with torch.no_grad():
            a = lgu.render.render_view(*ops[:4], scene["size"], cameras=ops[4], camera_scale=0.5)
            b = lgu.render.render_view(*ops[:4], scene["size"], cameras=ops[4], camera_scale=0.5, out=out)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert_same(a, image, depth, "fresh results")
    assert_same(b, image, depth, "out buffers")


@pytest.mark.gpu
@pytest.mark.parametrize("color_dtype", [torch.float32, torch.uint8], ids=["float32", "uint8"])
def test_end_to_end_from_the_video_to_the_picture(lgu, color_dtype):
    """A four-frame 12x16 video through cloud.point_cloud, then render_view with the video's poses as cameras: the picture is
    the restatement's render of the same three tensors."""
    from tests.test_cloud import make_scene
    N, ht, wd = 4, 12, 16
    poses, disps, intr, images = make_scene(41, N, ht, wd)
    video = [dev(x) for x in (poses, disps, intr)]
    ix = torch.arange(N, device="cuda")
    thresh = torch.full((N,), 0.05, device="cuda")
    with torch.no_grad():
        points, colors, offsets = lgu.cloud.point_cloud(*video, ix, thresh, dev(images), min_count=1, color_dtype=color_dtype)
    assert int(offsets[-1]) == points.shape[0] > 50 and colors.dtype == color_dtype
    view = np.array([0.05, -0.02, 0.8, 0, 0, 0, 1], np.float32)          # the scene pushed away from the view
    K = np.array([24.0, 24.0, 19.5, 14.5], np.float32)
    size, scale = (30, 40), 0.2
    with torch.no_grad():
        got = lgu.render.render_view(points, colors, dev(view), dev(K), size, cameras=video[0], camera_scale=scale)
    stats = {}
    image, depth, _ = R.render_view(points.cpu().numpy(), colors.cpu().numpy(), view, K, size, cameras=poses, camera_scale=scale,
                                    stats=stats)
    print(stats)
    assert stats["covered"] > 50 and stats["segments_drawn"] > 0 and stats["points_passed"] > 50
    assert_same(got, image, depth, "end to end")
