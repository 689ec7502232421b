"""The map export (lgu_slam_amd.cloud, csrc/cloud.hip): the filtered, coloured point cloud of a set of keyframes.

CPU: the ABI, every refusal of point_cloud with its precedence, and the float64 restatement tests/cloud_restatement.py on
scenes whose result can be worked out by hand.  GPU: the fused call against cloud.point_cloud_composed, the composition of
the project's pinned operators (geom.depth_filter, geom.iproj under geom.se3_inverse, the reference's mask and boolean
index), compared as bit patterns (int32 views), so NaN and inf points of zero disparities count.
"""
import ctypes

import numpy as np
import pytest

from tests import cloud_restatement as R

torch = pytest.importorskip("torch")

CLOUD_ENTRIES = ("lgu_cloud_scratch_bytes", "lgu_cloud_decide_f32", "lgu_cloud_write_f32")


# ---------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------
def test_header_declares_and_binding_carries_the_cloud_entries(lgu):
    from tests.test_abi import declared_symbols
    syms = declared_symbols()
    lib = ctypes.CDLL(lgu.build())
    for s in CLOUD_ENTRIES:
        assert s in syms, s
        assert hasattr(lib, s), s
        assert s in lgu._lib.SIGNATURES, s
    assert lgu._lib.RESTYPES["lgu_cloud_scratch_bytes"] is ctypes.c_longlong
    assert "cloud" in vars(lgu) and "cloud.hip" in lgu._build.SOURCES


def test_scratch_size_and_refusals_of_the_entries_need_no_device(lgu):
    """Host-side answers: the scratch holds 4 ballot words, a prefix and a count per workgroup of 256 pixels; a frame of more
    than 65535 workgroups is LGU_E_UNSUPPORTED, a misaligned scratch LGU_E_BADARG, both before any launch."""
    lib = lgu._lib.load()
    assert lib.lgu_cloud_scratch_bytes(0, 48, 64) == 0 and lib.lgu_cloud_scratch_bytes(3, 0, 64) == 0
    assert lib.lgu_cloud_scratch_bytes(-1, 48, 64) == 0
    for num, ht, wd in ((1, 5, 7), (16, 48, 64), (3, 17, 19), (7, 60, 80)):
        units = num * ((ht * wd + 255) // 256)
        assert lib.lgu_cloud_scratch_bytes(num, ht, wd) == units * 40 + (units * 4 + 7) // 8 * 8
    fake = ctypes.c_void_p(4096)         # never dereferenced: every refusal below precedes the launch
    args = lgu._lib.CloudArgs(poses=fake, disps=fake, intrinsics=fake, ix=fake, thresh=fake, floor=fake, scratch=fake, offsets=fake,
                              points=fake, cap=8, np=4, nd=4, ht=4097, wd=4096, num=1, min_count=2)
    assert lib.lgu_cloud_decide_f32(args, None) == lgu._lib.LGU_E_UNSUPPORTED
    assert lib.lgu_cloud_write_f32(args, None) == lgu._lib.LGU_E_UNSUPPORTED
    args.ht, args.wd, args.scratch = 8, 8, ctypes.c_void_p(4100)
    assert lib.lgu_cloud_decide_f32(args, None) == lgu._lib.LGU_E_BADARG
    assert lib.lgu_cloud_write_f32(args, None) == lgu._lib.LGU_E_BADARG
    args.scratch, args.images, args.colors = fake, fake, fake     # images that do not cover the frame
    args.ni, args.H, args.W, args.stride, args.phase = 4, 64, 59, 8, 3
    assert lib.lgu_cloud_write_f32(args, None) == lgu._lib.LGU_E_BADARG
    args.num = -1
    assert lib.lgu_cloud_decide_f32(args, None) == lgu._lib.LGU_E_BADARG


def _cpu_args():
    poses = torch.zeros(4, 7)
    poses[:, 6] = 1
    return dict(poses=poses, disps=torch.ones(4, 6, 8), intrinsics=torch.tensor([8.0, 8.0, 4.0, 3.0]), ix=torch.arange(3),
                thresh=torch.full((3,), 0.1))


@pytest.mark.parametrize("fn", ["point_cloud", "point_cloud_composed"])
def test_refusals_come_before_any_launch_in_their_order(lgu, monkeypatch, fn):
    def no_launch():
        raise AssertionError("the library was reached")
    monkeypatch.setattr(lgu._lib, "load", no_launch)
    f = getattr(lgu.cloud, fn)

    def call(images=None, **kw):
        a = _cpu_args()
        opts = {k: kw.pop(k) for k in list(kw) if k not in a}
        a.update(kw)
        return f(a["poses"], a["disps"], a["intrinsics"], a["ix"], a["thresh"], images, **opts)

    cpu = "must be a HIP device tensor: lgu_slam_amd has no CPU fallback$"
    # contiguity first, whatever else is wrong; then the device, before the dtype and the shapes
    with pytest.raises(RuntimeError, match="^disps must be contiguous$"):
        call(disps=torch.ones(4, 8, 6).transpose(1, 2), ix=torch.arange(3).int())
    with pytest.raises(RuntimeError, match="^poses must be contiguous$"):
        call(poses=torch.zeros(7, 4).t())
    with pytest.raises(RuntimeError, match="^images must be contiguous$"):
        call(images=torch.zeros(4, 3, 64, 48, dtype=torch.uint8).transpose(2, 3))
    with pytest.raises(RuntimeError, match="^disp_floor must be contiguous$"):
        call(disp_floor=torch.zeros(6)[::2])
    with pytest.raises(RuntimeError, match="^out points must be contiguous$"):
        call(out=(torch.zeros(3, 8).t(), None))
    with pytest.raises(RuntimeError, match="^poses " + cpu):
        call(ix=torch.arange(3).int(), thresh=torch.zeros(1))            # wrong dtype and shape too: the device is named
    with pytest.raises(RuntimeError, match="^poses " + cpu):
        call()
    # past the device check (CPU tensors stand in; nothing below touches them): dtype before shape
    monkeypatch.setattr(lgu.cloud, "check_device", lambda pairs: None)
    with pytest.raises(RuntimeError, match=r"^expected scalar type Long but found Int \(ix\)$"):
        call(ix=torch.zeros(2, 2).int())
    with pytest.raises(RuntimeError, match=r"^expected scalar type Float but found Double \(thresh\)$"):
        call(thresh=torch.zeros(1).double())
    with pytest.raises(RuntimeError, match=r"^expected scalar type Float but found Half \(disps\)$"):
        call(disps=torch.ones(4, 6, 8).half())
    with pytest.raises(RuntimeError, match=r"^expected scalar type torch.uint8 but found Float \(images\)$"):
        call(images=torch.zeros(4, 3, 48, 64))
    with pytest.raises(RuntimeError, match=r"^expected scalar type Float but found Double \(disp_floor\)$"):
        call(disp_floor=torch.zeros(3).double())
    with pytest.raises(RuntimeError, match=r"^expected scalar type Float but found Double \(out points\)$"):
        call(out=(torch.zeros(5, 3).double(), None))
    with pytest.raises(RuntimeError, match=r"found Float \(out colors\)$"):
        call(images=torch.zeros(4, 3, 48, 64, dtype=torch.uint8), color_dtype=torch.uint8, out=(torch.zeros(5, 3), torch.zeros(5, 3)))
    with pytest.raises(RuntimeError, match="^color_dtype must be torch.float32 or torch.uint8"):
        call(color_dtype=torch.float16)
    # the shape messages, in geom.depth_filter's wording and order
    with pytest.raises(RuntimeError, match=r"^poses must be \(N,7\)"):
        call(poses=torch.zeros(4, 6), ix=torch.zeros(2, 2).long())
    with pytest.raises(RuntimeError, match=r"^disps must be \(N,ht,wd\)"):
        call(disps=torch.ones(4, 48))
    with pytest.raises(RuntimeError, match="^intrinsics must be 1-D with fx, fy, cx, cy"):
        call(intrinsics=torch.ones(3))
    with pytest.raises(RuntimeError, match=r"^ix must be 1-D, got \(2, 2\)$"):
        call(ix=torch.zeros(2, 2).long(), thresh=torch.zeros(1))
    with pytest.raises(RuntimeError, match=r"^thresh must be 1-D with one entry per index of ix \(3\), got \(2,\)$"):
        call(thresh=torch.zeros(2), disp_floor=torch.zeros(9))
    # images, disp_floor, out
    with pytest.raises(RuntimeError, match=r"^images must be \(N,3,H,W\) uint8 BGR, got \(4, 48, 64\)$"):
        call(images=torch.zeros(4, 48, 64, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match=r"^images of 48x56 sampled at \[3::8\] give 6x7 pixels, disps has 6x8$"):
        call(images=torch.zeros(4, 3, 48, 56, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match=r"^images of 56x64 sampled at \[3::8\] give 7x8 pixels, disps has 6x8$"):
        call(images=torch.zeros(4, 3, 56, 64, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match=r"^images of 48x64 sampled at \[1::4\] give 12x16 pixels, disps has 6x8$"):
        call(images=torch.zeros(4, 3, 48, 64, dtype=torch.uint8), stride=4, phase=1)
    with pytest.raises(RuntimeError, match="^stride must be >= 1 and phase >= 0"):
        call(images=torch.zeros(4, 3, 48, 64, dtype=torch.uint8), stride=0)
    with pytest.raises(RuntimeError, match=r"^images must hold a frame for every frame with a pose and a disparity \(4\), got 3$"):
        call(images=torch.zeros(3, 3, 48, 64, dtype=torch.uint8), disp_floor=torch.zeros(2))
    with pytest.raises(RuntimeError, match=r"^disp_floor must be \(num,\) = \(3,\), got \(2,\)$"):
        call(disp_floor=torch.zeros(2), out=(torch.zeros(5, 4), None))
    with pytest.raises(RuntimeError, match="^out must be a pair"):
        call(out=torch.zeros(5, 3))
    with pytest.raises(RuntimeError, match=r"^out points must be \(capacity,3\), got \(5, 4\)$"):
        call(out=(torch.zeros(5, 4), None))
    with pytest.raises(RuntimeError, match="^out colors must be given with images and only with them$"):
        call(out=(torch.zeros(5, 3), torch.zeros(5, 3)))
    with pytest.raises(RuntimeError, match="^out colors must be given with images and only with them$"):
        call(images=torch.zeros(4, 3, 48, 64, dtype=torch.uint8), out=(torch.zeros(5, 3), None))
    with pytest.raises(RuntimeError, match=r"^out colors must have the capacity of out points \(5 rows\), got 4$"):
        call(images=torch.zeros(4, 3, 48, 64, dtype=torch.uint8), out=(torch.zeros(5, 3), torch.zeros(4, 3)))
    # no autograd, inside and outside torch.no_grad()
    p = _cpu_args()["poses"].requires_grad_()
    with pytest.raises(RuntimeError, match="^point_cloud has no autograd"):
        call(poses=p)
    with torch.no_grad(), pytest.raises(RuntimeError, match=r"^ix must be 1-D"):   # admitted under no_grad: the next refusal
        call(poses=p, ix=torch.zeros(2, 2).long())


def _identity_poses(n, t=None):
    poses = np.zeros((n, 7))
    poses[:, 6] = 1
    if t is not None:
        poses[:, :3] = t
    return poses


def test_restatement_on_identical_poses_counts_the_neighbours_in_the_buffer():
    """Scene 1.  Nine identical (identity) cameras, constant disparity d, intrinsics that are powers of two: every pixel
    projects exactly onto itself in every neighbour, its corner disparity equals its own, so inside floor(u) < wd-1,
    floor(v) < ht-1 the count is the number of neighbours ix-1, ix-2, ix-3, ix+3, ix+4, ix+5 inside the buffer: 3, 4, 5, 6 for
    ix = 0, 1, 2, 3 (and 3, 4 for ix = 8, 5).  The last row and column count 0.  Points are (x, y, 1) / d."""
    N, ht, wd, d = 9, 5, 6, 0.5
    K = np.array([8.0, 8.0, 4.0, 2.0])
    poses, disps = _identity_poses(N), np.full((N, ht, wd), d)
    ix = np.array([0, 1, 2, 3, 8, 5, -1, 9])
    cnt = R.counts(poses, disps, K, ix, np.full(len(ix), 1e-3))
    for b, want in enumerate((3, 4, 5, 6, 3, 4, 0, 0)):
        assert (cnt[b, :-1, :-1] == want).all(), (b, cnt[b])
        assert (cnt[b, -1, :] == 0).all() and (cnt[b, :, -1] == 0).all()
    rays = R.rays(ht, wd, K)
    for min_count, kept_entries in ((3, (0, 1, 2, 3, 4, 5)), (4, (1, 2, 3, 5)), (5, (2, 3)), (6, (3,)), (7, ())):
        pts, cols, offs = R.point_cloud(poses, disps, K, ix, np.full(len(ix), 1e-3), min_count=min_count)
        per = (ht - 1) * (wd - 1)
        want_offs = np.cumsum([0] + [per if b in kept_entries else 0 for b in range(len(ix))])
        assert cols is None and (offs == want_offs).all(), (min_count, offs)
        assert pts.shape == (per * len(kept_entries), 3)
        for n in range(len(kept_entries)):           # every entry: the interior pixels in row-major order
            np.testing.assert_allclose(pts[n * per:(n + 1) * per], (rays[:-1, :-1] / d).reshape(-1, 3), rtol=0, atol=1e-15)
    # the disparity floor: d > ratio * mean(d) fails for ratio >= 1 on a constant frame, an explicit floor overrides it
    assert R.point_cloud(poses, disps, K, ix, np.full(len(ix), 1e-3), disp_ratio=1.0)[2][-1] == 0
    assert R.point_cloud(poses, disps, K, ix[:1], np.full(1, 1e-3), disp_floor=[0.49])[2][-1] == (ht - 1) * (wd - 1)
    # colours: BGR bytes sampled at [phase::stride], RGB / 255, in the rows' order
    rng = np.random.default_rng(0)
    img = rng.integers(0, 256, (N, 3, 8 * ht, 8 * wd), dtype=np.uint8)
    pts, cols, offs = R.point_cloud(poses, disps, K, ix[3:4], np.full(1, 1e-3), images=img)
    want = img[3][::-1, 3::8, 3::8].transpose(1, 2, 0)[:-1, :-1].reshape(-1, 3) / 255.0
    np.testing.assert_allclose(cols, want, rtol=0, atol=0)
    # a moved camera: the same pixels, points moved by the inverse pose (here -t)
    moved = _identity_poses(N, t=np.array([0.25, -0.5, 1.0]))
    pts2 = R.point_cloud(moved, disps, K, ix[3:4], np.full(1, 1e-3))[0]
    np.testing.assert_allclose(pts2, pts - np.array([0.25, -0.5, 1.0]), rtol=0, atol=1e-15)


def test_restatement_keeps_nothing_when_every_projection_leaves_the_image():
    """Scene 2.  Cameras 1000 units apart along x: with d = 1, x + d t_ij is at least ~999 away from the ray, its pixel
    column beyond +-7000: no projection is inside any neighbour, nothing is kept."""
    N, ht, wd = 9, 5, 6
    K = np.array([8.0, 8.0, 4.0, 2.0])
    poses = _identity_poses(N)
    poses[:, 0] = 1000.0 * np.arange(N)
    ix = np.arange(N)
    cnt = R.counts(poses, np.ones((N, ht, wd)), K, ix, np.full(N, 1e9))
    assert (cnt == 0).all()
    pts, cols, offs = R.point_cloud(poses, np.ones((N, ht, wd)), K, ix, np.full(N, 1e9), min_count=1)
    assert pts.shape == (0, 3) and (offs == 0).all() and len(offs) == N + 1


# ---------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------
def make_scene(seed, N, ht, wd, stride=8, phase=3):
    """Cameras a few centimetres apart on a smooth path, a smooth disparity field in [0.2, 2] seen by all of them plus a
    little per-frame noise, a handful of zero and negative disparities, random BGR images."""
    rng = np.random.default_rng(seed)
    poses = np.zeros((N, 7), np.float32)
    t = np.zeros(3)
    for k in range(N):
        axis = rng.standard_normal(3)
        axis /= np.linalg.norm(axis)
        a = 0.02 * rng.standard_normal()
        poses[k, :3] = t
        poses[k, 3:] = np.concatenate([np.sin(a / 2) * axis, [np.cos(a / 2)]])
        t = t + 0.03 * rng.standard_normal(3)
    v, u = np.meshgrid(np.linspace(0, 1, ht), np.linspace(0, 1, wd), indexing="ij")
    field = 1.1 + 0.9 * np.sin(3.0 * u + 1.0) * np.cos(2.0 * v)
    disps = np.clip(field[None] + 0.01 * rng.standard_normal((N, ht, wd)), 0.2, 2.0).astype(np.float32)
    bad = rng.random((N, ht, wd)) < 0.03
    disps[bad] = np.where(rng.random(int(bad.sum())) < 0.5, 0.0, -rng.random(int(bad.sum()))).astype(np.float32)
    intr = np.array([0.8 * wd, 0.8 * wd, wd / 2, ht / 2], np.float32)
    images = rng.integers(0, 256, (N, 3, stride * ht, stride * wd), dtype=np.uint8)
    return poses, disps, intr, images


def entries(N):
    """ix unordered, with a repeat, -1 and N, and the frames 0, 1, N-1 whose neighbours are partly missing; thresh with one
    0 (keeps nothing) and one inf (keeps every pixel that projects inside two neighbours, given a floor below it)."""
    ix = [N - 1, 0, 1, N // 2, -1, N // 2, N, 2 % N, 1]
    th = [0.05] * len(ix)
    th[2] = 0.0
    th[3] = float("inf")
    return np.array(ix, np.int64), np.array(th, np.float32)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def same_bits(a, b):
    if a is None or b is None:
        return a is None and b is None
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if a.dtype == torch.float32:
        a, b = a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)
    return bool(torch.equal(a, b))


SHAPES = [(8, 5, 7), (8, 9, 13), (8, 17, 19), (3, 8, 8)]      # one partial wave; two waves; two workgroups; exactly one wave
_CASES = {}


def gpu_case(N, ht, wd, short_poses=False):
    """The operands on the device and the composed results (computed once, never modified) for float32 and uint8 colours."""
    key = (N, ht, wd, short_poses)
    if key not in _CASES:
        import lgu_slam_amd as lgu
        poses, disps, intr, images = make_scene(100 * N + ht, N, ht, wd)
        ix, th = entries(N)
        a = dict(poses=dev(poses[:N - 2] if short_poses else poses), disps=dev(disps), intrinsics=dev(intr), ix=dev(ix), thresh=dev(th),
                 images=dev(images))
        pos = (a["poses"], a["disps"], a["intrinsics"], a["ix"], a["thresh"])
        floor = 0.5 * a["disps"][a["ix"].clamp(0, N - 1)].mean(dim=[1, 2])
        floor[3] = -1.0                                         # the inf-threshold entry keeps every pixel seen twice
        a["floor"] = floor
        with torch.no_grad():
            a["want_f32"] = lgu.cloud.point_cloud_composed(*pos, a["images"])
            a["want_u8"] = lgu.cloud.point_cloud_composed(*pos, a["images"], color_dtype=torch.uint8)
            a["want_floor"] = lgu.cloud.point_cloud_composed(*pos, a["images"], disp_floor=floor)
        torch.cuda.synchronize()
        _CASES[key] = a
    return _CASES[key]


def _pos(a):
    return a["poses"], a["disps"], a["intrinsics"], a["ix"], a["thresh"]


@pytest.mark.gpu
@pytest.mark.parametrize("short_poses", [False, True], ids=["Np=Nd", "Np<Nd"])
@pytest.mark.parametrize("N,ht,wd", SHAPES)
def test_fused_has_the_bits_of_the_composition(lgu, N, ht, wd, short_poses):
    a = gpu_case(N, ht, wd, short_poses)
    C = lgu.cloud
    before = dict(C.launches)
    got = {"want_f32": C.point_cloud(*_pos(a), a["images"]),
           "want_u8": C.point_cloud(*_pos(a), a["images"], color_dtype=torch.uint8),
           "want_floor": C.point_cloud(*_pos(a), a["images"], disp_floor=a["floor"])}
    none = C.point_cloud(*_pos(a))
    torch.cuda.synchronize()
    assert C.launches["fused"] == before["fused"] + 4 and C.launches["composed"] == before["composed"]
    for name, (p, c, o) in got.items():
        wp, wc, wo = a[name]
        print("%s %dx%d of %d frames: kept %d of %d pixels" % (name, ht, wd, N, int(wo[-1]), len(a["ix"]) * ht * wd))
        assert o.dtype == torch.int64 and torch.equal(o, wo), (name, o.tolist(), wo.tolist())
        assert same_bits(p, wp), name
        assert same_bits(c, wc), name
    assert none[1] is None and same_bits(none[0], a["want_f32"][0]) and torch.equal(none[2], a["want_f32"][2])
    # what the scene is for: something is kept, something is dropped, the invalid and thresh = 0 entries keep nothing, the
    # inf entry with a floor below every disparity keeps at least what its default-floor twin keeps
    o, of = a["want_f32"][2].tolist(), a["want_floor"][2].tolist()
    nvalid = a["poses"].shape[0]
    for b, f in enumerate(a["ix"].tolist()):
        if not 0 <= f < nvalid or b == 2:
            assert o[b + 1] == o[b], (b, f)
    assert of[4] - of[3] >= o[4] - o[3]
    if N >= 8 and ht * wd >= 64:      # (the 3-frame buffer has at most two neighbours per frame, one frame with both)
        assert 0 < o[-1] < len(o) * ht * wd and of[4] - of[3] > 0
    assert a["want_u8"][1].dtype == torch.uint8 and a["want_f32"][1].dtype == torch.float32


@pytest.mark.gpu
def test_every_point_has_the_bits_of_iproj_under_arbitrary_poses(lgu):
    """min_count = 0 with a floor of -inf keeps every pixel of every valid entry, so every point is compared, under poses with
    arbitrary rotations and translations of order 1: here the inverse pose's rounding shows in the points.  (With every
    product and sum of the inverse rounded on its own, 12 % of the inverse's elements differ from geom.se3_inverse on such
    poses: torch's cross product evaluates a1 b2 - a2 b1 as fma(a1, b2, -(a2 b1)), and so does the kernel.)"""
    N, ht, wd = 8, 17, 19
    rng = np.random.default_rng(11)
    _, disps, intr, _ = make_scene(3, N, ht, wd)
    q = rng.standard_normal((N, 4))
    poses = np.concatenate([rng.standard_normal((N, 3)), q / np.linalg.norm(q, axis=1, keepdims=True)], 1).astype(np.float32)
    ix = np.array([3, 7, 0, 5, 5, 8, 1, 2, 6, 4], np.int64)
    pos = tuple(dev(x) for x in (poses, disps, intr, ix, np.zeros(len(ix), np.float32)))
    floor = torch.full((len(ix),), float("-inf"), device="cuda")
    with torch.no_grad():
        p, c, o = lgu.cloud.point_cloud(*pos, min_count=0, disp_floor=floor)
        want = lgu.geom.iproj(lgu.geom.se3_inverse(pos[0]), pos[1], pos[2])
        wp, wc, wo = lgu.cloud.point_cloud_composed(*pos, min_count=0, disp_floor=floor)
    per = ht * wd
    assert o.tolist() == [per * n for n in (0, 1, 2, 3, 4, 5, 5, 6, 7, 8, 9)] and torch.equal(o, wo)
    valid = [f for f in ix.tolist() if f < N]
    assert same_bits(p, want[torch.tensor(valid).cuda()].reshape(-1, 3)) and same_bits(p, wp)
    assert not bool(torch.isfinite(p).all())          # the planted zero disparities: inf and NaN points, compared as bits


@pytest.mark.gpu
def test_uint8_colours_are_the_gathered_bytes_and_other_strides_work(lgu):
    N, ht, wd = 8, 9, 13
    poses, disps, intr, images = make_scene(5, N, ht, wd, stride=4, phase=1)
    ix, th = entries(N)
    pos = tuple(dev(x) for x in (poses, disps, intr, ix, th))
    img = dev(images)
    with torch.no_grad():
        p, c, o = lgu.cloud.point_cloud(*pos, img, stride=4, phase=1, color_dtype=torch.uint8)
        pf, cf, of = lgu.cloud.point_cloud(*pos, img, stride=4, phase=1)
        wp, wc, wo = lgu.cloud.point_cloud_composed(*pos, img, stride=4, phase=1)
        count = lgu.geom.depth_filter(*pos)
    assert same_bits(pf, wp) and same_bits(cf, wc) and torch.equal(of, wo) and torch.equal(o, wo) and same_bits(p, wp)
    # the bytes, gathered on the host from the mask the operators give
    safe = np.clip(ix, 0, N - 1)
    mask = (count.cpu().numpy() >= 2) & (disps[safe] > (0.5 * pos[1][dev(safe)].mean(dim=[1, 2])).cpu().numpy()[:, None, None])
    rgb = images[safe][:, ::-1, 1::4, 1::4].transpose(0, 2, 3, 1)
    assert int(mask.sum()) == int(o[-1]) > 0
    assert np.array_equal(c.cpu().numpy(), rgb[mask])
    assert same_bits(cf, c.float() * torch.tensor(1.0 / 255.0, dtype=torch.float32).cuda())


@pytest.mark.gpu
def test_capacity_form_writes_a_prefix_and_reads_nothing_on_the_host(lgu):
    a = gpu_case(8, 17, 19)
    wp, wc, wo = a["want_f32"]
    total = int(wo[-1])
    assert total > 5
    SENT_F, SENT_B = 1234.5, 77
    for cap in (total, total - 5, 0):
        for color_dtype, want_c in ((torch.float32, wc), (torch.uint8, a["want_u8"][1])):
            big_p = torch.full((total + 16, 3), SENT_F, device="cuda")
            big_c = torch.full((total + 16, 3), SENT_B if color_dtype == torch.uint8 else SENT_F, dtype=color_dtype, device="cuda")
            buf_p, buf_c = big_p[7:7 + cap], big_c[7:7 + cap]
            torch.cuda.synchronize()
            torch.cuda.set_sync_debug_mode("error")
            try:
                p, c, o = lgu.cloud.point_cloud(*_pos(a), a["images"], color_dtype=color_dtype, out=(buf_p, buf_c))
            finally:
                torch.cuda.set_sync_debug_mode("default")
            torch.cuda.synchronize()
            assert p is buf_p and c is buf_c and torch.equal(o, wo), cap
            assert same_bits(big_p[7:7 + cap], wp[:cap]) and same_bits(big_c[7:7 + cap], want_c[:cap]), cap
            for big, sent in ((big_p, SENT_F), (big_c, SENT_B if color_dtype == torch.uint8 else SENT_F)):
                assert bool((big[:7] == sent).all()) and bool((big[7 + cap:] == sent).all()), cap
    # a capacity above the total: the tail of the buffer stays as it was
    big_p = torch.full((total + 9, 3), SENT_F, device="cuda")
    p, c, o = lgu.cloud.point_cloud(*_pos(a), out=(big_p, None))
    assert c is None and same_bits(big_p[:total], wp) and bool((big_p[total:] == SENT_F).all()) and torch.equal(o, wo)


def _odd(t, pad=3):
    """t's values in a fresh allocation, starting `pad` elements in: aligned to its element only (int64: 8 bytes)."""
    raw = torch.full((t.numel() + 2 * pad,), 99, dtype=t.dtype, device=t.device)
    raw[pad:pad + t.numel()] = t.reshape(-1)
    out = raw[pad:pad + t.numel()].view(t.shape)
    assert out.is_contiguous() and out.data_ptr() % 16 != 0 and out.data_ptr() % t.element_size() == 0
    return out


@pytest.mark.gpu
def test_operands_at_element_alignment_give_the_same_bits(lgu):
    a = gpu_case(8, 17, 19)
    total = int(a["want_floor"][2][-1])
    pos = tuple(_odd(t) for t in _pos(a))
    guard_p, guard_c = torch.full((3 * total + 6,), 5.0, device="cuda"), torch.full((3 * total + 2,), 9, dtype=torch.uint8, device="cuda")
    out = (guard_p[3:3 + 3 * total].view(total, 3), guard_c[1:1 + 3 * total].view(total, 3))
    assert out[0].data_ptr() % 16 != 0 and out[1].data_ptr() % 2 == 1
    p, c, o = lgu.cloud.point_cloud(*pos, _odd(a["images"], 1), disp_floor=_odd(a["floor"]), color_dtype=torch.uint8, out=out)
    torch.cuda.synchronize()
    assert torch.equal(o, a["want_floor"][2]) and same_bits(p, a["want_floor"][0])
    assert torch.equal(c, lgu.cloud.point_cloud_composed(*_pos(a), a["images"], disp_floor=a["floor"], color_dtype=torch.uint8)[1])
    assert bool((guard_p[:3] == 5.0).all()) and bool((guard_p[3 + 3 * total:] == 5.0).all())
    assert bool((guard_c[:1] == 9).all()) and bool((guard_c[1 + 3 * total:] == 9).all())
    pf, cf, of = lgu.cloud.point_cloud(*pos, _odd(a["images"], 1))
    assert same_bits(pf, a["want_f32"][0]) and same_bits(cf, a["want_f32"][1]) and torch.equal(of, a["want_f32"][2])


@pytest.mark.gpu
def test_small_calls_route_to_the_composition(lgu, monkeypatch):
    a = gpu_case(8, 9, 13)
    C = lgu.cloud
    size = len(a["ix"]) * 9 * 13
    monkeypatch.setattr(C, "MIN_FUSED_PIXELS", size + 1)
    before = dict(C.launches)
    p, c, o = C.point_cloud(*_pos(a), a["images"])
    assert C.launches == {"fused": before["fused"], "composed": before["composed"] + 1}
    assert same_bits(p, a["want_f32"][0]) and same_bits(c, a["want_f32"][1]) and torch.equal(o, a["want_f32"][2])
    monkeypatch.setattr(C, "MIN_FUSED_PIXELS", size)             # read at the call: at the threshold the fused route serves
    p, c, o = C.point_cloud(*_pos(a), a["images"])
    assert C.launches == {"fused": before["fused"] + 1, "composed": before["composed"] + 1}
    assert same_bits(p, a["want_f32"][0]) and same_bits(c, a["want_f32"][1]) and torch.equal(o, a["want_f32"][2])


@pytest.mark.gpu
def test_degenerate_shapes_launch_nothing(lgu, monkeypatch):
    a = gpu_case(8, 9, 13)
    C = lgu.cloud
    before = dict(C.launches)

    def no_launch():
        raise AssertionError("the library was reached")
    monkeypatch.setattr(lgu._lib, "load", no_launch)
    for fn in (C.point_cloud, C.point_cloud_composed):
        p, c, o = fn(a["poses"], a["disps"], a["intrinsics"], a["ix"][:0], a["thresh"], a["images"])
        assert p.shape == (0, 3) and c.shape == (0, 3) and c.dtype == torch.float32 and o.tolist() == [0]
        p, c, o = fn(a["poses"], a["disps"][:, :0].contiguous(), a["intrinsics"], a["ix"], a["thresh"])
        assert p.shape == (0, 3) and c is None and o.tolist() == [0] * (len(a["ix"]) + 1)
        buf = torch.full((4, 3), 3.0, device="cuda")
        p, c, o = fn(a["poses"], a["disps"], a["intrinsics"], a["ix"][:0], a["thresh"], out=(buf, None))
        assert p is buf and bool((buf == 3.0).all()) and o.tolist() == [0]
    assert C.launches == before


@pytest.mark.gpu
def test_call_enqueues_on_the_current_stream(lgu):
    a = gpu_case(8, 17, 19)
    wp, wc, wo = a["want_f32"]
    total = int(wo[-1])
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        buf_p = torch.zeros((total, 3), device="cuda")
        buf_c = torch.zeros((total, 3), device="cuda")
        p, c, o = lgu.cloud.point_cloud(*_pos(a), a["images"], out=(buf_p, buf_c))
        pe, ce, oe = lgu.cloud.point_cloud(*_pos(a), a["images"])
    s.synchronize()
    assert same_bits(pe, wp) and same_bits(ce, wc) and torch.equal(oe, wo)
    assert same_bits(p, wp) and same_bits(c, wc) and torch.equal(o, wo)
