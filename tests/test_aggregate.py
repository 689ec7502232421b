"""scatter_mean, cvx_upsample, upsample_disp and upsample_disps_ (lgu_slam_amd.aggregate, csrc/aggregate.hip): GraphAgg's
segment mean and the convex 8x upsampling of the disparity (droid_slam/droid_net.py:14-69, depth_video.py:124-128).

The segment mean is held bit for bit to the float32 restatement tests/aggregate_restatement.py.  The upsampler is held
to the float64 restatement within |gpu - ref| <= 4e-6 * max_k |d_k| (UPS_TOL); in the half-weight mode a weight that
lies within float32 noise of a half rounding boundary can round to the neighbouring half, so a fraction <= 6e-4 of the
outputs (HALF_FLIP_FRACTION) may instead be off by up to one half ulp of a weight, 2^-11 * max_k |d_k|.  Measured: at
most 3.7e-4 for the MI355X kernel against the float64 restatement (2.7e-5 against the reference fixture, 0 against the
torch composition) and 4.7e-4 between the float32 and float64 restatements; about 9 weights per output, each within
~2e-4 (relative) of a boundary with float32 noise, put the expected rate there.  The fixture tests/golden/cvx_upsample_*.npz holds the reference's own
cvx_upsample (tools/gen_upsample_golden.py).
"""
import ctypes
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import aggregate_restatement as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
REFERENCE = os.environ.get("LGU_REFERENCE", "/root/reference")   # the reference tree, where present (CPU tests only)
ENTRIES = ("lgu_scatter_mean_f32", "lgu_scatter_mean_h16", "lgu_cvx_upsample_f32", "lgu_upsample_disps_f32")
UPS_TOL = 4e-6
HALF_FLIP = 2.0 ** -11 + UPS_TOL
HALF_FLIP_FRACTION = 6e-4

sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_upsample_golden as G  # noqa: E402


def same_bits(a, b):
    a, b = torch.as_tensor(a).detach().cpu(), torch.as_tensor(b).detach().cpu()
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    iv = torch.int16 if a.dtype == torch.float16 else torch.int32
    return bool(torch.equal(a.contiguous().view(iv), b.contiguous().view(iv)))


def check_upsample(got, want64, bound, half_weights, what=""):
    """got, want64 (B,R,C) numpy; bound (B,R,C) = max_k |d_k| per output."""
    r = np.abs(np.asarray(got, dtype=np.float64) - want64) / bound
    if not half_weights:
        assert r.max() <= UPS_TOL, "%s: %g" % (what, r.max())
        return
    assert r.max() <= HALF_FLIP, "%s: %g" % (what, r.max())
    assert (r > UPS_TOL).mean() <= HALF_FLIP_FRACTION, "%s: %g" % (what, (r > UPS_TOL).mean())


def graph_agg_index(seed, E, N):
    """GraphAgg's ix: torch.unique(ii, return_inverse=True)[1] for E edges over N frames."""
    g = torch.Generator().manual_seed(seed)
    ii = torch.cat([torch.arange(N), torch.randint(0, N, (E - N,), generator=g)])
    ii = ii[torch.randperm(E, generator=g)]
    _, ix = torch.unique(ii, return_inverse=True)
    return ix


def seg_src(seed, shape, dtype):
    g = torch.Generator().manual_seed(seed)
    return (4 * torch.randn(shape, generator=g)).to(dtype)


def ups_inputs(seed, B, ht, wd, scale=3.0):
    g = torch.Generator().manual_seed(seed)
    data = (0.05 + 1.5 * torch.rand(B, ht, wd, generator=g)).float()
    mask = (scale * torch.randn(B, 576, ht, wd, generator=g)).float()
    return data, mask


def fixture(name):
    B, ht, wd, seed = G.CASES[name]
    z = dict(np.load(os.path.join(GOLD, name + ".npz")))
    mask = G.mask_from(int(z["mask_seed"]), B, ht, wd, float(z["mask_scale"]))
    assert hashlib.sha256(mask.tobytes()).hexdigest() == str(z["mask_sha256"]), "mask regeneration drifted"
    return z, mask


# ---- CPU ------------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_aggregate_entries(lgu):
    from tests.test_abi import declared_symbols
    syms = declared_symbols()
    lib = ctypes.CDLL(lgu._lib._build.SO_PATH)
    for s in ENTRIES:
        assert s in syms and s in lgu._lib.SIGNATURES and hasattr(lib, s), s


def test_float32_restatement_agrees_with_float64():
    g = np.random.default_rng(3)
    src = (4 * g.standard_normal((2, 40, 333))).astype(np.float32)
    ix = g.integers(-2, 9, 40)
    a, b = R.scatter_mean32(src, ix, 8), R.scatter_mean64(src, ix, 8)
    assert np.abs(a - b).max() <= 1e-6 * np.abs(src).max() * 4
    assert (a[:, [m for m in range(8) if m not in ix]] == 0).all()
    h = R.scatter_mean32(src.astype(np.float16), ix, 8)
    assert h.dtype == np.float16 and np.abs(h.astype(np.float64) - b).max() <= 2.0 ** -11 * np.abs(b).max() + 1e-6
    data = (0.05 + 1.5 * g.random((3, 17, 22))).astype(np.float32)
    mask = (3 * g.standard_normal((3, 576, 17, 22))).astype(np.float32)
    bound = R.upsample_bound(data)
    for hw in (False, True):
        m = mask.astype(np.float16).astype(np.float32) if hw else mask
        check_upsample(R.cvx_upsample32(data, m, hw), R.cvx_upsample64(data, m, hw), bound, hw, "hw=%s" % hw)
    # the mapping: a single dominant weight moves the neighbour's value to the output pixel
    one = np.full((1, 576, 3, 4), -50.0, dtype=np.float32)
    k, a_, b_ = 5, 2, 6                       # k = 5: neighbour (y, x+1)
    one[0, k * 64 + a_ * 8 + b_] = 50.0
    d = np.arange(12, dtype=np.float32).reshape(1, 3, 4) + 1
    out = R.cvx_upsample64(d, one)
    assert abs(out[0, 8 * 1 + a_, 8 * 2 + b_] - d[0, 1, 3]) < 1e-12
    assert abs(out[0, 8 * 1 + a_, 8 * 3 + b_]) < 1e-12      # neighbour outside the frame is 0


@pytest.mark.parametrize("name", sorted(G.CASES))
def test_restatement_equals_the_reference_fixture(name):
    z, mask = fixture(name)
    data, rows = z["data"], z["rows"]
    bound = R.upsample_bound(data)[:, rows]
    mh = mask.astype(np.float16).astype(np.float32)
    check_upsample(z["out_f32"], R.cvx_upsample64(data, mask)[:, rows], bound, False, "f32")
    check_upsample(z["out_h16_f32w"], R.cvx_upsample64(data, mh)[:, rows], bound, False, "h16 f32 weights")
    check_upsample(z["out_h16_h16w"], R.cvx_upsample64(data, mh, True)[:, rows], bound, True, "h16 half weights")
    # and the half-weight reading is the one the reference's half softmax gets: the other one is out of bound
    r = np.abs(z["out_h16_h16w"] - R.cvx_upsample64(data, mh)[:, rows]) / bound
    assert (r > UPS_TOL).mean() > 0.05


@pytest.mark.skipif(not os.path.isdir(os.path.join(REFERENCE, "droid_slam")), reason="reference tree not present")
def test_fixture_regenerates_from_the_live_reference():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_upsample_golden.py"), "--reference", REFERENCE,
                        "--check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count("matches") == len(G.CASES)


@pytest.mark.skipif(not os.path.isdir(os.path.join(REFERENCE, "droid_slam")), reason="reference tree not present")
def test_reference_droid_net_imports_with_the_torch_scatter_dropin():
    """With install_dropins(torch_scatter=True) the reference's droid_net imports with only lietorch and cv2 stubbed, and
    its scatter_mean is this build's."""
    code = r"""
import sys, types
class Stub(types.ModuleType):
    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return type(name, (), {})
for name in ("lietorch", "cv2"):
    sys.modules[name] = Stub(name)
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[2])
import lgu_slam_amd
lgu_slam_amd.install_dropins(torch_scatter=True)
import droid_slam.droid_net as dn
import torch_scatter
assert dn.scatter_mean is lgu_slam_amd.aggregate.scatter_mean
assert torch_scatter.scatter_mean is lgu_slam_amd.aggregate.scatter_mean
print("ok")
"""
    r = subprocess.run([sys.executable, "-c", code, ROOT, REFERENCE], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout + r.stderr


def test_install_dropins_torch_scatter_is_opt_in():
    code = r"""
import sys, types
sys.path.insert(0, sys.argv[1])
import lgu_slam_amd
ret = lgu_slam_amd.install_dropins()
assert [m.__name__ for m in ret] == ["defCorrSample", "droid_backends"]
assert lgu_slam_amd.DROPIN_SCATTER_DIR not in sys.path
try:
    import torch_scatter
    assert getattr(torch_scatter, "__file__", "").find("dropin_scatter") < 0   # a real one stays a real one
    print("real")
    sys.exit(0)
except ImportError:
    pass
ret2 = lgu_slam_amd.install_dropins(torch_scatter=True)
assert [m.__name__ for m in ret2] == ["defCorrSample", "droid_backends"]
from torch_scatter import scatter_mean, scatter_sum
assert scatter_mean is lgu_slam_amd.aggregate.scatter_mean
try:
    scatter_sum(None, None)
    raise SystemExit("scatter_sum did not raise")
except NotImplementedError:
    pass
lgu_slam_amd.install_dropins(torch_scatter=True)       # again: a no-op
sys.modules["torch_scatter"] = types.ModuleType("torch_scatter")
try:
    lgu_slam_amd.install_dropins(torch_scatter=True)
    raise SystemExit("a foreign torch_scatter was not refused")
except RuntimeError:
    pass
print("ok")
"""
    r = subprocess.run([sys.executable, "-c", code, ROOT], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() in ("ok", "real"), r.stdout + r.stderr


def _no_lib(monkeypatch, lgu):
    def boom():
        raise AssertionError("the library was touched before the argument check")
    monkeypatch.setattr(lgu._lib, "load", boom)


def test_argument_checks_raise_before_any_launch(lgu, monkeypatch):
    _no_lib(monkeypatch, lgu)
    A = lgu.aggregate
    src = torch.zeros(1, 6, 4, 5)
    ix = torch.tensor([0, 1, 0, 2, 1, 0])
    with pytest.raises(NotImplementedError, match="out=None"):
        A.scatter_mean(src, ix, dim=1, out=torch.zeros(1, 3, 4, 5))
    with pytest.raises(NotImplementedError, match="1-D index"):
        A.scatter_mean(src, ix.view(1, 6, 1, 1).expand(1, 6, 4, 5), dim=1)
    with pytest.raises(NotImplementedError, match="1-D index"):
        A.scatter_mean(src, ix[:5], dim=1)
    with pytest.raises(RuntimeError, match="src must be contiguous"):
        A.scatter_mean(src.transpose(2, 3), ix, dim=1)
    with pytest.raises(RuntimeError, match="index must be contiguous"):
        A.scatter_mean(src, torch.stack([ix, ix], 1)[:, 0], dim=1)
    with pytest.raises(RuntimeError, match="Float or Half but found Double"):
        A.scatter_mean(src.double(), ix, dim=1)
    with pytest.raises(RuntimeError, match="Long but found Int"):
        A.scatter_mean(src, ix.int(), dim=1)
    with pytest.raises(IndexError):
        A.scatter_mean(src, ix, dim=4)
    with pytest.raises(RuntimeError, match="no autograd"):
        A.scatter_mean(src.clone().requires_grad_(), ix, dim=1)
    with pytest.raises(RuntimeError, match="HIP device tensor"):
        A.scatter_mean(src, ix, dim=1, dim_size=3)
    data, mask = torch.zeros(2, 3, 4, 1), torch.zeros(2, 576, 3, 4)
    with pytest.raises(NotImplementedError, match="width 1"):
        A.cvx_upsample(torch.zeros(2, 3, 4, 2), mask)
    with pytest.raises(RuntimeError, match="mask must be"):
        A.cvx_upsample(data, mask[:1])
    with pytest.raises(RuntimeError, match="mask must be"):                 # same values, another layout
        A.cvx_upsample(data, torch.zeros(576, 2, 3, 4))
    with pytest.raises(RuntimeError, match="mask must be"):
        A.cvx_upsample(data, torch.zeros(2, 1, 576, 3, 4))
    A_ok = [(2, 576, 3, 4), (1, 2, 576, 3, 4), (1, 1, 2, 576, 3, 4)]     # leading 1s pass the shape check
    for shp in A_ok:
        with pytest.raises(RuntimeError, match="HIP device tensor"):
            A.cvx_upsample(data, torch.zeros(shp))
    with pytest.raises(RuntimeError, match="mask must be"):
        A.upsample_disp(torch.zeros(1, 2, 3, 4), torch.zeros(1, 576, 2, 3, 4))
    with pytest.raises(RuntimeError, match="disp must be contiguous"):
        A.upsample_disp(torch.zeros(1, 2, 4, 3).transpose(2, 3), torch.zeros(1, 2, 576, 3, 4))
    with pytest.raises(RuntimeError, match="mask must be contiguous"):
        A.cvx_upsample(data, torch.zeros(2, 576, 4, 3).transpose(2, 3))
    with pytest.raises(RuntimeError, match="Float or Half but found Double"):
        A.cvx_upsample(data, mask.double())
    with pytest.raises(RuntimeError, match="Float but found Half"):
        A.cvx_upsample(data.half(), mask)
    with pytest.raises(RuntimeError, match="no autograd"):
        A.cvx_upsample(data, mask.clone().requires_grad_())
    with pytest.raises(RuntimeError, match="HIP device tensor"):
        A.cvx_upsample(data, mask)
    with pytest.raises(RuntimeError, match="HIP device tensor"):
        A.upsample_disp(torch.zeros(1, 2, 3, 4), torch.zeros(1, 2, 576, 3, 4))
    disps, up = torch.zeros(5, 3, 4), torch.zeros(5, 24, 32)
    ixu, m1 = torch.tensor([1, 3]), torch.zeros(1, 2, 576, 3, 4)
    with pytest.raises(RuntimeError, match="disps_up must be"):
        A.upsample_disps_(torch.zeros(5, 24, 31), disps, ixu, m1)
    with pytest.raises(RuntimeError, match="ix must be 1-D"):
        A.upsample_disps_(up, disps, ixu[None], m1)
    with pytest.raises(RuntimeError, match="Long but found Int"):
        A.upsample_disps_(up, disps, ixu.int(), m1)
    with pytest.raises(RuntimeError, match="disps_up must be contiguous"):
        A.upsample_disps_(torch.zeros(5, 32, 24).transpose(1, 2), disps, ixu, m1)
    with pytest.raises(RuntimeError, match="mask must be"):
        A.upsample_disps_(up, disps, ixu, torch.zeros(1, 3, 576, 3, 4))
    with pytest.raises(RuntimeError, match="mask must be"):
        A.upsample_disps_(up, disps, ixu, torch.zeros(576, 2, 3, 4))
    with pytest.raises(RuntimeError, match="HIP device tensor"):
        A.upsample_disps_(up, disps, ixu, m1)


def test_torch_ops_registration(lgu):
    import lgu_slam_amd.torch_ops  # noqa: F401
    for name in ("scatter_mean", "cvx_upsample", "upsample_disp", "upsample_disps_"):
        assert hasattr(torch.ops.lgu, name), name
    schema = str(torch.ops.lgu.upsample_disps_.default._schema)
    assert "Tensor(a0!) disps_up" in schema, schema


# ---- GPU ------------------------------------------------------------------------------------------------------------
def _torch_scatter_mean(src, index, dim, M):
    """What torch_scatter.scatter_mean computes: zeros + scatter_add_ of src and of ones (the count), count clamped to
    1, true_divide_, all in src's dtype."""
    shape = list(src.shape)
    shape[dim] = M
    view = [1] * src.dim()
    view[dim] = -1
    idx = index.view(view).expand_as(src)
    out = torch.zeros(shape, dtype=src.dtype, device=src.device).scatter_add_(dim, idx, src)
    cnt = torch.zeros(M, dtype=src.dtype, device=src.device).scatter_add_(0, index, torch.ones_like(index, dtype=src.dtype))
    return out.true_divide_(cnt.clamp_(1).view(view))


SEG_CASES = {"frontend": ((1, 48, 128, 48, 64), 48, 12), "config5": ((1, 80, 128, 60, 80), 80, 8),
             "odd_inner": ((3, 20, 37), 20, 6)}


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
@pytest.mark.parametrize("case", sorted(SEG_CASES))
def test_scatter_mean_is_bit_identical_to_the_restatement(lgu, case, dtype):
    shape, E, N = SEG_CASES[case]
    src = seg_src(E, shape, dtype)
    ix = graph_agg_index(E, E, N)
    got = lgu.aggregate.scatter_mean(src.cuda(), ix.cuda(), dim=1)
    assert got.dtype == dtype and tuple(got.shape) == (shape[0], N) + shape[2:]
    outer, inner = shape[0], int(np.prod(shape[2:]))
    want = R.scatter_mean32(src.numpy().reshape(outer, E, inner), ix.numpy(), N).reshape(got.shape)
    assert same_bits(got, torch.from_numpy(want))
    # within the stated bound of the torch_scatter composition
    ref = _torch_scatter_mean(src.cuda(), ix.cuda(), 1, N)
    cmax = int(torch.bincount(ix).max())
    tol = ((cmax + 1) * 2.0 ** -11 if dtype == torch.float16 else (cmax + 1) * 2.0 ** -23) * float(src.abs().max())
    assert float((got.double() - ref.double()).abs().max()) <= tol


@pytest.mark.gpu
def test_scatter_mean_edge_cases_and_guard_bands(lgu):
    lib = lgu._lib.load()
    dev = torch.device("cuda")
    for dtype, fn in ((torch.float32, lib.lgu_scatter_mean_f32), (torch.float16, lib.lgu_scatter_mean_h16)):
        outer, n, inner, M = 2, 9, 40, 6
        src = seg_src(5, (outer, n, inner), dtype).to(dev)
        index = torch.tensor([3, -1, 0, 3, 6, 100, 0, -7, 3], device=dev)      # segments 1, 2, 4, 5 empty
        guard = 4096
        big = torch.full((outer * M * inner + 2 * guard,), 7.0, dtype=dtype, device=dev)
        out = big[guard:-guard].view(outer, M, inner)
        s = torch.cuda.current_stream()
        rc = fn(ctypes.c_void_p(src.data_ptr()), ctypes.c_void_p(index.data_ptr()), outer, n, inner, M,
                ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(s.cuda_stream))
        assert rc == 0
        torch.cuda.synchronize()
        assert bool((big[:guard] == 7).all()) and bool((big[-guard:] == 7).all())
        want = R.scatter_mean32(src.cpu().numpy(), index.cpu().numpy(), M)
        assert same_bits(out, torch.from_numpy(want))
        assert bool((out[:, [1, 2, 4, 5]] == 0).all())
        # beyond the stated limits
        assert fn(ctypes.c_void_p(src.data_ptr()), ctypes.c_void_p(index.data_ptr()), 1, 70000, 1, 1,
                  ctypes.c_void_p(out.data_ptr()), None) == lgu._lib.LGU_E_UNSUPPORTED
        assert fn(None, None, -1, 1, 1, 1, None, None) == lgu._lib.LGU_E_BADARG
    A = lgu.aggregate
    # n = 0: zeros of dim_size; M = 0: empty; dim_size=None with n = 0: empty
    z = A.scatter_mean(torch.zeros(2, 0, 5, device=dev), torch.zeros(0, dtype=torch.int64, device=dev), dim=1, dim_size=3)
    assert tuple(z.shape) == (2, 3, 5) and bool((z == 0).all())
    e = A.scatter_mean(torch.ones(2, 4, 5, device=dev), torch.tensor([5, 6, 7, 8], device=dev), dim=1, dim_size=0)
    assert tuple(e.shape) == (2, 0, 5)
    assert tuple(A.scatter_mean(torch.zeros(0, device=dev), torch.zeros(0, dtype=torch.int64, device=dev)).shape) == (0,)
    # dim=-1, dim_size=None (max + 1)
    x = seg_src(8, (3, 7, 11), torch.float32).cuda()
    ix = torch.tensor([2, 0, 2, 1, 4, 4, 0, 2, 1, 0, 3], device=dev)
    got = A.scatter_mean(x, ix)
    want = R.scatter_mean32(x.cpu().numpy().reshape(21, 11, 1), ix.cpu().numpy(), 5).reshape(3, 7, 5)
    assert same_bits(got, torch.from_numpy(want))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
@pytest.mark.parametrize("n, M, inner", [(300, 37, 1000), (4999, 13, 97), (65536, 5, 8)])
def test_scatter_mean_over_several_index_tiles(lgu, n, M, inner, dtype):
    """n > 256: the segment lists are built over several tiles of the index vector (the backend's chunks of 80-300
    edges, up to the stated limit of 65536), with out-of-range and negative entries mixed in."""
    g = torch.Generator().manual_seed(n)
    index = torch.randint(-2, M + 2, (n,), generator=g)
    src = seg_src(n + 1, (2, n, inner), dtype)
    got = lgu.aggregate.scatter_mean(src.cuda(), index.cuda(), dim=1, dim_size=M)
    want = R.scatter_mean32(src.numpy(), index.numpy(), M)
    assert same_bits(got, torch.from_numpy(want))
    # segments gather rows from more than one tile
    spans = [int(js.max()) // 256 > int(js.min()) // 256 for js in ((index == m).nonzero().flatten() for m in range(M))
             if len(js) > 0]
    assert sum(spans) >= M // 2


@pytest.mark.gpu
def test_scatter_mean_with_only_negative_indices_and_no_dim_size(lgu):
    src = torch.ones(2, 5, 3, device="cuda")
    out = lgu.aggregate.scatter_mean(src, torch.tensor([-1, -3, -1, -2, -5], device="cuda"), dim=1)
    assert tuple(out.shape) == (2, 0, 3)


@pytest.mark.gpu
def test_scatter_mean_runs_are_identical_on_side_streams_and_in_graphs(lgu):
    A = lgu.aggregate
    shape, E, N = SEG_CASES["frontend"]
    src = seg_src(1, shape, torch.float16).cuda()
    ix = graph_agg_index(2, E, N).cuda()
    a = A.scatter_mean(src, ix, dim=1)
    b = A.scatter_mean(src, ix, dim=1)
    assert same_bits(a, b)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        c = A.scatter_mean(src, ix, dim=1, dim_size=N)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    assert same_bits(a, c)
    g = torch.cuda.CUDAGraph()
    s2 = torch.cuda.Stream()
    s2.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s2):
        A.scatter_mean(src, ix, dim=1, dim_size=N)            # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(s2)
    with torch.cuda.graph(g):
        d = A.scatter_mean(src, ix, dim=1, dim_size=N)
    src.mul_(-1)
    g.replay()
    torch.cuda.synchronize()
    assert same_bits(d, A.scatter_mean(src, ix, dim=1))


def _ups_gpu(lgu, data, mask, mode):
    """mode: "f32" (float mask), "h16w" (half mask, autocast off: half weights), "f32w" (half mask under autocast)."""
    A = lgu.aggregate
    d = data.cuda()[..., None]
    if mode == "f32":
        return A.cvx_upsample(d, mask.cuda())[..., 0]
    m = mask.cuda().half()
    with torch.autocast("cuda", enabled=(mode == "f32w")):
        return A.cvx_upsample(d, m)[..., 0]


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["f32", "h16w", "f32w"])
@pytest.mark.parametrize("size", [(4, 48, 64), (2, 17, 30), (1, 1, 1)])
def test_cvx_upsample_within_bound_of_float64(lgu, mode, size):
    data, mask = ups_inputs(sum(size), *size)
    got = _ups_gpu(lgu, data, mask, mode).cpu().numpy()
    m = mask.numpy() if mode == "f32" else mask.half().float().numpy()
    want = R.cvx_upsample64(data.numpy(), m, mode == "h16w")
    check_upsample(got, want, R.upsample_bound(data.numpy()), mode == "h16w", mode)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(G.CASES))
def test_cvx_upsample_against_the_reference_fixture(lgu, name):
    z, mask = fixture(name)
    data, rows = torch.from_numpy(z["data"]), z["rows"]
    bound = R.upsample_bound(z["data"])[:, rows]
    mask = torch.from_numpy(mask)
    check_upsample(_ups_gpu(lgu, data, mask, "f32").cpu().numpy()[:, rows], z["out_f32"], bound, False, "f32")
    check_upsample(_ups_gpu(lgu, data, mask, "f32w").cpu().numpy()[:, rows], z["out_h16_f32w"], bound, False, "f32w")
    check_upsample(_ups_gpu(lgu, data, mask, "h16w").cpu().numpy()[:, rows], z["out_h16_h16w"], bound, True, "h16w")


@pytest.mark.gpu
def test_half_mask_with_float_weights_equals_the_float_mask(lgu):
    data, mask = ups_inputs(9, 3, 48, 64)
    mh = mask.half()
    a = _ups_gpu(lgu, data, mh.float(), "f32")
    b = _ups_gpu(lgu, data, mh.float(), "f32w")
    assert same_bits(a, b)


def _torch_upsample(data, mask):
    """The reference's composition written out: softmax over the 9 neighbours (in the mask's dtype, as torch picks it),
    3x3 unfold with zero padding, product, sum over the neighbours, sub-pixels to their fine positions."""
    B, ht, wd = data.shape
    w = torch.softmax(mask.view(B, 9, 64, ht, wd), dim=1)
    nb = torch.nn.functional.unfold(data[:, None], [3, 3], padding=1).view(B, 9, 1, ht, wd)
    up = (w * nb).sum(1).view(B, 8, 8, ht, wd)
    return up.permute(0, 3, 1, 4, 2).reshape(B, 8 * ht, 8 * wd)


@pytest.mark.gpu
@pytest.mark.parametrize("autocast", [False, True])
def test_cvx_upsample_against_the_torch_composition_in_both_autocast_states(lgu, autocast):
    data, mask = ups_inputs(21, 4, 48, 64)
    d, m = data.cuda(), mask.cuda().half()
    with torch.autocast("cuda", enabled=autocast):
        ref = _torch_upsample(d, m)
        got = lgu.aggregate.cvx_upsample(d[..., None], m)[..., 0]
    assert ref.dtype == torch.float32
    bound = R.upsample_bound(data.numpy())
    check_upsample(got.cpu().numpy(), ref.double().cpu().numpy(), bound, not autocast, "autocast=%s" % autocast)
    # the other weight rounding is far outside the bound
    other = lgu._lib.load().lgu_cvx_upsample_f32
    out = torch.empty_like(got)
    flags = lgu.aggregate.UPS_MASK_F16 | (lgu.aggregate.UPS_HALF_WEIGHTS if autocast else 0)
    rc = other(ctypes.c_void_p(d.data_ptr()), ctypes.c_void_p(m.data_ptr()), 4, 48, 64, flags,
               ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    r = np.abs(out.double().cpu().numpy() - ref.double().cpu().numpy()) / bound
    assert (r > UPS_TOL).mean() > 0.05


@pytest.mark.gpu
def test_upsample_disp_and_torch_ops_equal_cvx_upsample(lgu):
    import lgu_slam_amd.torch_ops  # noqa: F401
    data, mask = ups_inputs(4, 6, 24, 32)
    d, m = data.cuda(), mask.cuda()
    a = lgu.aggregate.cvx_upsample(d[..., None], m)
    b = lgu.aggregate.upsample_disp(d.view(2, 3, 24, 32), m.view(2, 3, 576, 24, 32))
    assert tuple(a.shape) == (6, 192, 256, 1) and tuple(b.shape) == (2, 3, 192, 256)
    assert same_bits(a.view(2, 3, 192, 256), b)
    assert same_bits(torch.ops.lgu.cvx_upsample(d[..., None], m), a)
    assert same_bits(torch.ops.lgu.upsample_disp(d.view(2, 3, 24, 32), m.view(2, 3, 576, 24, 32)), b)
    src, ix = seg_src(3, (1, 10, 4, 6), torch.float32).cuda(), graph_agg_index(3, 10, 4).cuda()
    assert same_bits(torch.ops.lgu.scatter_mean(src, ix, 1, None), lgu.aggregate.scatter_mean(src, ix, dim=1))


@pytest.mark.gpu
@pytest.mark.parametrize("half", [False, True])
def test_upsample_disps_writes_only_rows_ix(lgu, half):
    import lgu_slam_amd.torch_ops  # noqa: F401
    A = lgu.aggregate
    N, ht, wd = 12, 48, 64
    disps, _ = ups_inputs(1, N, ht, wd)
    ix = torch.tensor([1, 4, 5, 9, 11])
    _, mask = ups_inputs(2, len(ix), ht, wd)
    d, i = disps.cuda(), ix.cuda()
    m = mask.cuda().half() if half else mask.cuda()
    up = torch.full((N, 8 * ht, 8 * wd), -3.0, device="cuda")
    assert A.upsample_disps_(up, d, i, m[None]) is up             # GraphAgg's upmask shape (1,U,576,ht,wd)
    want = A.cvx_upsample(d[i][..., None], m)[..., 0]
    assert same_bits(up[i], want)
    rest = [r for r in range(N) if r not in ix.tolist()]
    assert bool((up[rest] == -3.0).all())
    # out-of-range entries write nothing; the valid ones are written as before
    up2 = torch.full_like(up, -3.0)
    i2 = torch.tensor([1, -1, 5, 12, 11], device="cuda")
    A.upsample_disps_(up2, d, i2, m)
    assert same_bits(up2[[1, 5, 11]], want[[0, 2, 4]])
    assert bool((up2[[r for r in range(N) if r not in (1, 5, 11)]] == -3.0).all())
    # empty ix
    up3 = torch.full_like(up, -3.0)
    A.upsample_disps_(up3, d, torch.zeros(0, dtype=torch.int64, device="cuda"), m[:0])
    assert bool((up3 == -3.0).all())
    # torch.ops form (mutating)
    up4 = torch.full_like(up, -3.0)
    torch.ops.lgu.upsample_disps_(up4, d, i, m)
    assert same_bits(up4, up)


@pytest.mark.gpu
def test_upsample_disps_on_a_side_stream_and_in_a_graph(lgu):
    A = lgu.aggregate
    N, ht, wd = 8, 60, 80
    disps, _ = ups_inputs(5, N, ht, wd)
    _, mask = ups_inputs(6, 3, ht, wd)
    d, m = disps.cuda(), mask.cuda().half()
    i = torch.tensor([0, 3, 7], device="cuda")
    ref = torch.zeros(N, 8 * ht, 8 * wd, device="cuda")
    A.upsample_disps_(ref, d, i, m)
    up = torch.zeros_like(ref)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        A.upsample_disps_(up, d, i, m)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    assert same_bits(up, ref)
    g = torch.cuda.CUDAGraph()
    up.zero_()
    s2 = torch.cuda.Stream()
    s2.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s2):
        A.upsample_disps_(up, d, i, m)
    torch.cuda.current_stream().wait_stream(s2)
    with torch.cuda.graph(g):
        A.upsample_disps_(up, d, i, m)
    up.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert same_bits(up, ref)


@pytest.mark.gpu
def test_graph_agg_composition_through_scatter_mean(lgu):
    """GraphAgg.forward's body written here: conv1 -> ReLU -> segment mean over the edges of a source frame -> conv2 ->
    ReLU, under no_grad and autocast, with this build's scatter_mean against the torch segment mean."""
    torch.manual_seed(0)
    conv1 = torch.nn.Conv2d(128, 128, 3, padding=1).cuda()
    conv2 = torch.nn.Conv2d(128, 128, 3, padding=1).cuda()
    E, N, ht, wd = 48, 12, 48, 64
    net = torch.randn(1, E, 128, ht, wd, device="cuda")
    ix = graph_agg_index(7, E, N).cuda()

    def agg(mean):
        with torch.no_grad(), torch.autocast("cuda"):
            x = torch.relu(conv1(net.view(E, 128, ht, wd))).view(1, E, 128, ht, wd)
            x = mean(x).view(-1, 128, ht, wd)
            return x, torch.relu(conv2(x))

    mid, got = agg(lambda x: lgu.aggregate.scatter_mean(x, ix, dim=1))
    mid_ref, ref = agg(lambda x: _torch_scatter_mean(x, ix, 1, N))
    assert mid.dtype == torch.float16 and got.shape == ref.shape
    cmax = int(torch.bincount(ix).max())
    src_max = float(mid.abs().max()) * 2
    assert float((mid.double() - mid_ref.double()).abs().max()) <= (cmax + 1) * 2.0 ** -11 * src_max
    assert float((got.double() - ref.double()).abs().max()) <= 2e-2 * float(ref.abs().max())
