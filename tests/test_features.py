"""The feature encoder's fused instance-norm kernels (lgu_slam_amd.features, csrc/instnorm.hip) against the float64
restatement tests/features_restatement.py and the reference's own encoder (tests/golden/features_fnet_*.npz,
tools/gen_features_golden.py).

Numerics contract, u = 2^-24, L = log2(hw) + 4, k(x) = mean|x| / sqrt(var + eps) per plane:
- E = u (L k(a) + 8 (|y_a| + 1)), mode 1 + 8 u |b|, mode 2 + u (L k(b) + 8 |y_b|): a tree sum of hw fp32 terms plus a
  handful of fp32 operations;
- fp32: |got - ref64| <= E; half: |got - ref64| <= ulp_half(|ref64| + E) / 2 + E, one rounding;
- the torch composition itself is held to the fp32 bound on the CPU, so a bound that is too tight fails there;
- frame normalisation: bit-identical to the four torch ops on the device;
- whole encoder: rms(installed - ref64) <= 1.25 rms(module's own forward - ref64) on the same device and mode (the
  convolutions are the same library calls on both paths; 25 % for the spread of an RMS over a few thousand outputs and
  the library's choice of algorithm).
The GPU tests read only the fixtures and the restatement, never the reference tree.
"""
import ctypes
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import features_restatement as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
REFERENCE = os.environ.get("LGU_REFERENCE", "/root/reference")
ENTRIES = ("lgu_instnorm_relu_f32", "lgu_instnorm_relu_h16", "lgu_instnorm_resident_limit", "lgu_image_normalize_u8")
MODES = (0, 1, 2, 3)
BADARG = 100001
DEV = "cuda"


def same_bits(a, b):
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    iv = {torch.float16: torch.int16, torch.float32: torch.int32}[a.dtype]
    return bool(torch.equal(a.view(iv), b.view(iv)))


def fixture(name):
    z = dict(np.load(os.path.join(GOLD, name + ".npz")))
    m, images = R.make_case(name)
    assert R.case_sha256(m, images) == str(z["sha256"]), "images or weights drifted from the fixture"
    return z, m, images


@functools.lru_cache(maxsize=None)
def inputs(family, dt, planes, hw):
    """a, b (planes, hw) on the CPU; cached and never written."""
    return R.family_inputs(family, R.DTYPES[dt], planes, hw)


# ---- CPU ------------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_feature_entries(lgu):
    from tests.test_abi import declared_symbols
    syms = declared_symbols()
    lib = ctypes.CDLL(lgu._lib._build.SO_PATH)
    for s in ENTRIES:
        assert s in syms and s in lgu._lib.SIGNATURES and hasattr(lib, s), s
    assert "instnorm.hip" in lgu._build.SOURCES
    assert lgu.FeatureEncoder is lgu.features.FeatureEncoder and lgu.__version__ == "0.8.0"
    text = open(os.path.join(ROOT, "include", "lgu_corr.h")).read()
    assert "extractor.py" in text and "motion_filter.py:56-57" in text        # the reference citations
    limit = lgu._lib.load().lgu_instnorm_resident_limit
    assert limit(2) >= 192 * 256 and limit(4) >= 96 * 128 and limit(3) == 0    # the production planes qualify in half


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_stand_in_encoder_equals_the_reference_fixture_bit_for_bit(name):
    z, m, images = fixture(name)
    with torch.no_grad():
        st = m.stages(images)
    for k in R.STAGES:
        assert np.array_equal(st[k].numpy(), z[k]), k
    assert os.path.getsize(os.path.join(GOLD, name + ".npz")) < os.path.getsize(os.path.join(GOLD, "cvx_upsample_24x32.npz"))


@pytest.mark.skipif(not os.path.isdir(os.path.join(REFERENCE, "droid_slam")), reason="reference tree not present")
def test_fixture_regenerates_from_the_live_reference():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_features_golden.py"), "--reference", REFERENCE,
                        "--check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr


@pytest.mark.parametrize("mode", MODES)
def test_torch_composition_stays_within_the_fp32_bound(mode):
    """The allowance is not fitted to the kernels: torch's own fp32 ops hold it on every family."""
    worst = 0.0
    for family, (_, _, dts) in R.FAMILIES.items():
        for dt in dts:
            for hw in (2, 35, 3072):
                a, b = (t.float() for t in inputs(family, dt, 6, hw))        # the values as stored, composed in fp32
                ref, E = R.reference(mode, a, b)
                err = (R.torch_composition(mode, a, b).double() - ref).abs()
                ratio = float((err / E).max())
                worst = max(worst, ratio)
                assert ratio <= 1.0, (family, dt, hw, ratio)
    print("mode %d: torch fp32 composition reaches %.3f of the bound" % (mode, worst))


def test_half_bound_admits_one_rounding_and_no_more():
    a, b = inputs("unit", "h16", 6, 3072)
    ref, E = R.reference(1, a, b)
    once = ref.to(torch.float16).double()
    assert bool(((once - ref).abs() <= R.bound(ref, E, torch.float16)).all())
    twice = (ref + 0.75 * R.half_ulp(ref)).to(torch.float16).double()       # a result one more rounding away
    assert not bool(((twice - ref).abs() <= R.bound(ref, E, torch.float16)).all())


def test_install_and_uninstall_keep_the_state_dict_keys(lgu):
    m = R.set_weights(R.RefEncoder(), 3)
    keys = list(m.state_dict().keys())
    wr = lgu.features.install(m)
    assert isinstance(wr, lgu.features.FeatureEncoder) and m.forward is wr
    assert lgu.features.install(m) is wr
    assert list(m.state_dict().keys()) == keys and len(list(m.parameters())) == 2 * 16 and not list(m.buffers())
    m.load_state_dict(R.set_weights(R.RefEncoder(), 4).state_dict())
    lgu.features.uninstall(m)
    assert "forward" not in m.__dict__ and list(m.state_dict().keys()) == keys
    lgu.features.uninstall(m)


def test_construction_refuses_other_architectures(lgu):
    F = lgu.features
    F.FeatureEncoder(R.RefEncoder())
    F.FeatureEncoder(R.RefEncoder(output_dim=256))
    bad = R.RefEncoder()
    bad.layer2[1].norm2 = torch.nn.GroupNorm(8, 64)
    with pytest.raises(RuntimeError, match=r"layer2\.1\.norm2 must be InstanceNorm2d"):
        F.FeatureEncoder(bad)
    bad = R.RefEncoder()
    bad.norm1 = torch.nn.InstanceNorm2d(32, affine=True)
    with pytest.raises(RuntimeError, match="norm1 must be InstanceNorm2d"):
        F.FeatureEncoder(bad)
    bad = R.RefEncoder()
    bad.layer3[0].norm3 = torch.nn.InstanceNorm2d(128, track_running_stats=True)
    bad.layer3[0].downsample = torch.nn.Sequential(bad.layer3[0].downsample[0], bad.layer3[0].norm3)
    with pytest.raises(RuntimeError, match=r"layer3\.0\.downsample\.1 must be InstanceNorm2d"):
        F.FeatureEncoder(bad)
    bad = R.RefEncoder()
    del bad.layer3
    with pytest.raises(RuntimeError, match="layer3 must be"):
        F.FeatureEncoder(bad)
    with pytest.raises(RuntimeError, match="norm1 must be InstanceNorm2d"):
        F.FeatureEncoder(R.RefEncoder(norm_fn="none"))
    bad = R.RefEncoder()
    bad.layer1[0].conv2 = torch.nn.Conv2d(32, 32, 3, padding=2)
    with pytest.raises(RuntimeError, match=r"layer1\.0\.conv2 must be Conv2d"):
        F.FeatureEncoder(bad)
    with pytest.raises(RuntimeError, match="norm1"):
        F.install(R.RefEncoder(norm_fn="none"))


def test_cpu_inputs_reach_the_module_and_give_its_result(lgu):
    _, m, images = fixture("features_fnet_1x64x48")
    with torch.no_grad():
        want = m(images)
        wr = lgu.features.install(m)
        got = m(images)
    lgu.features.uninstall(m)
    assert wr.fused_calls == 0 and same_bits(got, want)


def test_argument_checks_raise_before_any_launch(lgu, monkeypatch):
    def boom():
        raise AssertionError("the library was touched before the argument check")
    monkeypatch.setattr(lgu._lib, "load", boom)
    F = lgu.features
    x = torch.zeros(2, 3, 4, 5)
    with pytest.raises(RuntimeError, match="HIP device tensor"):
        F.instance_norm_relu(x)
    with pytest.raises(RuntimeError, match="a must be contiguous"):
        F.instance_norm_relu(x.permute(0, 1, 3, 2))
    with pytest.raises(RuntimeError, match="residual must be contiguous"):
        F.instance_norm_relu(x, torch.zeros(2, 3, 5, 4).permute(0, 1, 3, 2))
    with pytest.raises(RuntimeError, match="out must be contiguous"):
        F.instance_norm_relu(x, out=torch.zeros(2, 3, 5, 4).permute(0, 1, 3, 2))
    with pytest.raises(RuntimeError, match=r"residual must be \(2, 3, 4, 5\)"):
        F.instance_norm_relu(x, torch.zeros(2, 3, 4, 6))
    with pytest.raises(RuntimeError, match="expected scalar type Float but found Half"):
        F.instance_norm_relu(x, x.half())
    with pytest.raises(RuntimeError, match="Float or Half"):
        F.instance_norm_relu(x.double())
    with pytest.raises(RuntimeError, match=r"a must be \(N,C,H,W\)"):
        F.instance_norm_relu(torch.zeros(3, 4, 5))
    with pytest.raises(ValueError, match="more than 1 spatial element"):
        F.instance_norm_relu(torch.zeros(2, 3, 1, 1))
    with pytest.raises(ValueError):
        F.instance_norm_relu(x, norm_residual=True)
    with pytest.raises(ValueError):
        F.instance_norm_relu(x, x, relu=False)
    with pytest.raises(RuntimeError, match="no autograd"):
        F.instance_norm_relu(x.clone().requires_grad_())
    with pytest.raises(RuntimeError, match=r"image must be \(N,3,H,W\)"):
        F.normalize_images(torch.zeros(2, 4, 5, 6, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="expected scalar type Byte"):
        F.normalize_images(torch.zeros(2, 3, 5, 6))


# ---- GPU ------------------------------------------------------------------------------------------------------------
def fused(lgu, mode, a, b, out=None):
    """instance_norm_relu on (planes, hw) device tensors, viewed as (1, planes, hw, 1)."""
    p, hw = a.shape
    v = (lambda t: None if t is None else t.view(1, p, hw, 1))
    res = lgu.features.instance_norm_relu(v(a), v(b) if mode in (1, 2) else None, norm_residual=mode == 2, relu=mode != 3,
                                          out=v(out))
    return res.view(p, hw)


def check_bound(lgu, mode, dt, family, planes, hw):
    a, b = inputs(family, dt, planes, hw)
    got = fused(lgu, mode, a.to(DEV), b.to(DEV)).cpu()
    ref, E = R.reference(mode, a, b)
    ratio = float(((got.double() - ref).abs() / R.bound(ref, E, a.dtype)).max())
    assert ratio <= 1.0, (mode, dt, family, planes, hw, ratio)
    return ratio


@pytest.mark.gpu
@pytest.mark.parametrize("dt", ["f32", "h16"])
@pytest.mark.parametrize("mode", MODES)
def test_kernels_within_the_bound(lgu, mode, dt):
    limit = lgu.features.resident_limit(R.DTYPES[dt])
    worst = 0.0
    for family, (_, _, dts) in R.FAMILIES.items():
        if dt not in dts:
            continue
        for planes in (1, 6, 70):
            for hw in (2, 35, 4095, limit):
                worst = max(worst, check_bound(lgu, mode, dt, family, planes, hw))
        for hw in (limit + 1, 2 * limit + 3):
            worst = max(worst, check_bound(lgu, mode, dt, family, 3, hw))
    print("mode %d %s: the kernels reach %.3f of the bound" % (mode, dt, worst))


@pytest.mark.gpu
@pytest.mark.parametrize("dt", ["f32", "h16"])
@pytest.mark.parametrize("planes,hw", [(32, 192 * 256), (64, 96 * 128), (128, 48 * 64)])
def test_production_planes_within_the_bound(lgu, planes, hw, dt):
    for mode in MODES:
        check_bound(lgu, mode, dt, "shift", planes, hw)


SENT = 12288.0      # exactly representable in half and float; no result of the cases below equals it


def banded(n, dtype, guard):
    big = torch.full((n + 2 * guard,), SENT, dtype=dtype, device=DEV)
    return big, big[guard:guard + n]


def bands_intact(big, guard, n):
    return bool((big[:guard] == SENT).all()) and bool((big[guard + n:] == SENT).all())


@pytest.mark.gpu
@pytest.mark.parametrize("dt", ["f32", "h16"])
def test_kernels_write_nothing_outside_their_tensors(lgu, dt):
    """Results written between sentinel bands equal those into fresh tensors, every element is written, the bands are
    untouched; guard 3 puts out at another offset within 16 bytes than a and b."""
    limit = lgu.features.resident_limit(R.DTYPES[dt])
    for planes, hw in ((6, 35), (70, 4095), (3, limit), (3, limit + 1)):
        a, b = (t.to(DEV) for t in inputs("unit", dt, planes, hw))
        for mode in MODES:
            want = fused(lgu, mode, a, b)
            for guard in (3, 64):
                big, out = banded(planes * hw, a.dtype, guard)
                fused(lgu, mode, a, b, out=out.view(planes, hw))
                assert same_bits(out.view(planes, hw), want), (mode, planes, hw, guard)
                assert not bool((out == SENT).any()) and bands_intact(big, guard, planes * hw), (mode, planes, hw, guard)


@pytest.mark.gpu
@pytest.mark.parametrize("dt", ["f32", "h16"])
def test_in_place_equals_out_of_place(lgu, dt):
    limit = lgu.features.resident_limit(R.DTYPES[dt])
    for planes, hw in ((6, 35), (70, 4095), (3, limit), (3, 2 * limit + 3)):
        a, b = (t.to(DEV) for t in inputs("shift", dt, planes, hw))
        for mode in MODES:
            want = fused(lgu, mode, a, b)
            a2 = a.clone()
            assert fused(lgu, mode, a2, b, out=a2).data_ptr() == a2.data_ptr()
            assert same_bits(a2, want), (mode, planes, hw, "out is a")
            if mode in (1, 2):
                b2 = b.clone()
                fused(lgu, mode, a, b2, out=b2)
                assert same_bits(b2, want), (mode, planes, hw, "out is b")
        assert same_bits(a.cpu(), inputs("shift", dt, planes, hw)[0])       # the inputs themselves were never written


@pytest.mark.gpu
def test_empty_calls_and_bad_arguments_launch_nothing(lgu):
    from lgu_slam_amd.ops import _ptr, _stream
    lib = lgu._lib.load()
    F = lgu.features
    x = torch.randn(2, 3, 4, 5, device=DEV)
    assert tuple(F.instance_norm_relu(x[:0]).shape) == (0, 3, 4, 5)
    assert tuple(F.instance_norm_relu(x[:, :0], x[:, :0]).shape) == (2, 0, 4, 5)
    out = torch.full_like(x, SENT)
    st = _stream(x)
    assert lib.lgu_instnorm_relu_f32(_ptr(x), None, _ptr(out), 0, 20, 1e-5, 0, st) == 0
    assert lib.lgu_instnorm_relu_f32(None, None, None, 0, 20, 1e-5, 0, st) == 0
    for planes, hw, mode in ((-1, 20, 0), (6, 0, 0), (6, -3, 0), (6, 20, 4), (6, 20, -1)):
        assert lib.lgu_instnorm_relu_f32(_ptr(x), _ptr(x), _ptr(out), planes, hw, 1e-5, mode, st) == BADARG
        assert lib.lgu_instnorm_relu_h16(_ptr(x), _ptr(x), _ptr(out), planes, hw, 1e-5, mode, st) == BADARG
    assert lib.lgu_instnorm_relu_f32(_ptr(x), None, _ptr(out), 6, 20, 1e-5, 1, st) == BADARG      # mode 1 without b
    assert lib.lgu_instnorm_relu_f32(None, None, _ptr(out), 6, 20, 1e-5, 0, st) == BADARG
    m3 = (ctypes.c_float * 3)(0, 0, 0)
    assert lib.lgu_image_normalize_u8(None, _ptr(out), -1, 4, m3, m3, st) == BADARG
    assert lib.lgu_image_normalize_u8(None, _ptr(out), 0, 4, m3, m3, st) == 0
    torch.cuda.synchronize()
    assert bool((out == SENT).all())
    with pytest.raises(RuntimeError, match="a must be contiguous"):
        F.instance_norm_relu(x.permute(0, 1, 3, 2))
    with pytest.raises(RuntimeError, match="residual must be contiguous"):
        F.instance_norm_relu(x, x.permute(0, 1, 3, 2).contiguous().permute(0, 1, 3, 2))
    with pytest.raises(ValueError, match="more than 1 spatial element"):
        F.instance_norm_relu(x[:, :, :1, :1].contiguous())
    with pytest.raises(RuntimeError, match="HIP device tensor"):
        F.instance_norm_relu(x, x.cpu())
    with pytest.raises(ValueError, match="more than 1 spatial element"):
        torch.nn.functional.instance_norm(x[:, :, :1, :1])             # the behaviour the ValueError mirrors


@pytest.mark.gpu
@pytest.mark.parametrize("dt", ["f32", "h16"])
def test_bits_do_not_depend_on_the_run_or_the_other_planes(lgu, dt):
    limit = lgu.features.resident_limit(R.DTYPES[dt])
    for planes, hw in ((70, 35), (70, 4095), (70, 3072), (3, limit + 1)):
        a, b = (t.to(DEV) for t in inputs("ill", dt, planes, hw))
        for mode in MODES:
            first = fused(lgu, mode, a, b)
            assert same_bits(fused(lgu, mode, a, b), first), (mode, hw)
            for p in (0, planes // 2 + 1, planes - 1):               # odd hw: the lone plane sits at another alignment
                alone = fused(lgu, mode, a[p:p + 1], b[p:p + 1])
                assert same_bits(alone, first[p:p + 1]), (mode, hw, p)
                moved = fused(lgu, mode, a[p:p + 1].clone(), b[p:p + 1].clone())
                assert same_bits(moved, alone), (mode, hw, p)


def torch_normalize(image):
    """motion_filter.py:56-57 on the device."""
    mean = torch.as_tensor([0.485, 0.456, 0.406], device=DEV)[:, None, None]
    std = torch.as_tensor([0.229, 0.224, 0.225], device=DEV)[:, None, None]
    x = image[None, :, [2, 1, 0]].to(DEV) / 255.0
    return x.sub_(mean).div_(std)


@pytest.mark.gpu
def test_image_normalisation_is_bit_identical_to_the_torch_ops(lgu):
    F = lgu.features
    every = torch.arange(256, dtype=torch.uint8).view(1, 1, 16, 16).expand(1, 3, 16, 16).contiguous()
    every[0, 1] = every[0, 1].flip(0)
    every[0, 2] = every[0, 2].t().clone()
    rs = np.random.RandomState(5)
    odd = torch.from_numpy(rs.randint(0, 256, (2, 3, 5, 7)).astype(np.uint8))
    for image in (every, odd):
        want = torch_normalize(image)
        got = F.normalize_images(image.to(DEV))
        assert got.dtype == torch.float32 and tuple(got.shape) == (1,) + tuple(image.shape)
        assert same_bits(got, want)
        assert same_bits(F.normalize_images(image), want)             # a CPU image is uploaded as uint8
    big, out = banded(2 * 3 * 35, torch.float32, 3)
    from lgu_slam_amd.ops import _ptr, _stream
    m = (ctypes.c_float * 3)(*F.IMAGENET_MEAN)
    s = (ctypes.c_float * 3)(*F.IMAGENET_STD)
    img = odd.to(DEV)
    assert lgu._lib.load().lgu_image_normalize_u8(_ptr(img), _ptr(out), 2, 35, m, s, _stream(img)) == 0
    assert same_bits(out.view(1, 2, 3, 5, 7), torch_normalize(odd)) and bands_intact(big, 3, 2 * 3 * 35)
    assert tuple(F.normalize_images(torch.zeros(0, 3, 4, 4, dtype=torch.uint8, device=DEV)).shape) == (1, 0, 3, 4, 4)


@functools.lru_cache(maxsize=None)
def encoder_case(name, seed_offset=0):
    """(device module, device images, float64 CPU forward of the same module); cached and never written."""
    m, images = R.make_case(name, seed_offset)
    m64 = R.RefEncoder().double()
    m64.load_state_dict(m.state_dict())
    with torch.no_grad():
        ref = m64.eval()(images.double())
    return m.to(DEV), images.to(DEV), ref


def rms(x, ref):
    return float(((x.double().cpu() - ref) ** 2).mean().sqrt())


@pytest.mark.gpu
@pytest.mark.parametrize("half", [False, True])
@pytest.mark.parametrize("name", sorted(R.CASES))
def test_installed_encoder_is_as_close_to_float64_as_the_module(lgu, name, half):
    m, images, ref = encoder_case(name)
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16, enabled=half):
        own = m(images)
        wr = lgu.features.install(m)
        try:
            before = wr.fused_calls
            got = m(images)
            assert wr.fused_calls == before + 1
            m(images)
            assert wr.fused_calls == before + 2
        finally:
            lgu.features.uninstall(m)
    assert got.dtype == own.dtype == (torch.float16 if half else torch.float32) and got.shape == own.shape
    r_got, r_own = rms(got, ref), rms(own, ref)
    print("%s %s: rms installed %.4g, module %.4g, ratio %.3f" % (name, "half" if half else "fp32", r_got, r_own, r_got / r_own))
    assert r_got <= 1.25 * r_own
    if not half:
        z = np.load(os.path.join(GOLD, name + ".npz"))
        assert rms(got, torch.from_numpy(z["conv2"]).double()) <= 1.25 * r_own + rms(torch.from_numpy(z["conv2"]), ref)


@pytest.mark.gpu
def test_other_modes_fall_back_to_the_module_bit_for_bit(lgu, monkeypatch):
    m, images, _ = encoder_case("features_fnet_1x64x48")
    wr = lgu.features.install(m)
    try:
        with torch.no_grad():
            with torch.autocast("cuda", dtype=torch.bfloat16):
                want = type(m).forward(m, images)
                got = m(images)
            assert wr.fused_calls == 0 and got.dtype == torch.bfloat16 and bool(torch.equal(got, want))
            assert same_bits(m(images), m(images)) and wr.fused_calls == 2
        x = images.clone().requires_grad_()
        assert m(x).requires_grad and wr.fused_calls == 2            # gradients are wanted: the module's own forward
    finally:
        lgu.features.uninstall(m)
    cl, _ = R.make_case("features_fnet_1x64x48")
    cl = cl.to(DEV).to(memory_format=torch.channels_last)
    # two runs of the module's own channels-last forward do not give the same bits on this device (the library's NHWC
    # convolutions), so "the module's own forward" is pinned by identity: the class's forward is called with the same
    # arguments and its result is returned as it is
    seen = []
    own = type(cl).forward

    def spy(self, x):
        seen.append((self, x))
        seen.append(own(self, x))
        return seen[-1]
    monkeypatch.setattr(type(cl), "forward", spy)
    with torch.no_grad():
        wr = lgu.features.install(cl)
        got = cl(images)
    assert wr.fused_calls == 0 and len(seen) == 2 and seen[0][0] is cl and seen[0][1] is images and got is seen[1]
    assert got.shape == (1, 1, 128, 8, 6) and bool(torch.isfinite(got).all())


@pytest.mark.gpu
def test_state_dict_loads_after_install(lgu):
    m, images, _ = encoder_case("features_fnet_1x64x48")
    other, _ = R.make_case("features_fnet_1x64x48", seed_offset=7)
    fresh = R.RefEncoder().to(DEV)
    wr = lgu.features.install(fresh)
    fresh.load_state_dict(other.state_dict())
    twin = other.to(DEV)
    lgu.features.install(twin)
    with torch.no_grad():
        got, want, base = fresh(images), twin(images), m(images)
    assert wr.fused_calls == 1 and same_bits(got, want) and not same_bits(got, base)
    assert list(fresh.state_dict().keys()) == list(other.state_dict().keys())
