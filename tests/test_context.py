"""The context encoder on the fused residual-stage convolutions (lgu_slam_amd.context, csrc/encconv.hip) and the feature
encoder's `convs=True` against the reference's own BasicEncoder(256, 'none') (fixtures tests/golden/context_cnet_*.npz,
written by tools/gen_context_golden.py from the live reference) and the float64 forward of the same module.

Contract:
- the stand-in RefEncoder(256, 'none') equals the reference fixture bit for bit, so the GPU tests need no reference tree;
- whole encoder under float16 autocast: rms(installed - ref64) <= 1.25 rms(module's own forward - ref64) on the same
  device, the project's whole-encoder contract of tests/test_features.py; the same for features.install(m, convs=True);
- every other mode is the module's own forward bit for bit, and features.install(m) keeps the bits it had.
Measured on an MI355X (ratios installed / module): see DESIGN.md §3.21.
The GPU tests read only the fixtures and the restatements, never the reference tree.
"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import context_restatement as C  # noqa: E402
from tests import features_restatement as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
REFERENCE = os.environ.get("LGU_REFERENCE", "/root/reference")
DEV = "cuda"


def same_bits(a, b):
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    iv = {torch.float16: torch.int16, torch.float32: torch.int32, torch.bfloat16: torch.int16}[a.dtype]
    return bool(torch.equal(a.view(iv), b.view(iv)))


def fixture(name):
    z = dict(np.load(os.path.join(GOLD, name + ".npz")))
    m, images = C.make_case(name)
    assert C.case_sha256(m, images) == str(z["sha256"]), "images or weights drifted from the fixture"
    return z, m, images


# ---- CPU ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(C.CASES))
def test_stand_in_encoder_equals_the_reference_fixture_bit_for_bit(name):
    z, m, images = fixture(name)
    with torch.no_grad():
        st = m.stages(images)
    for k in C.STAGES:
        assert np.array_equal(st[k].numpy(), z[k]), k
    assert z["conv2"].shape[2] == C.OUTPUT_DIM == 256
    assert os.path.getsize(os.path.join(GOLD, name + ".npz")) < os.path.getsize(os.path.join(GOLD, "cvx_upsample_24x32.npz"))


@pytest.mark.skipif(not os.path.isdir(os.path.join(REFERENCE, "droid_slam")), reason="reference tree not present")
def test_fixture_regenerates_from_the_live_reference():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_context_golden.py"), "--reference", REFERENCE,
                        "--check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr


def test_install_and_uninstall_keep_the_state_dict_keys(lgu):
    m = R.set_weights(R.RefEncoder(256, "none"), 3)
    keys = list(m.state_dict().keys())
    wr = lgu.context.install(m)
    assert isinstance(wr, lgu.context.ContextEncoder) and m.forward is wr and lgu.ContextEncoder is lgu.context.ContextEncoder
    assert lgu.context.install(m) is wr
    assert list(m.state_dict().keys()) == keys and len(list(m.parameters())) == 2 * 16 and not list(m.buffers())
    m.load_state_dict(R.set_weights(R.RefEncoder(256, "none"), 4).state_dict())
    lgu.context.uninstall(m)
    assert "forward" not in m.__dict__ and list(m.state_dict().keys()) == keys
    lgu.context.uninstall(m)
    # features.install takes convs and keeps its default
    f = R.RefEncoder()
    wf = lgu.features.install(f, convs=True)
    assert wf.convs is True and lgu.features.install(f) is wf
    lgu.features.uninstall(f)
    assert lgu.features.install(f).convs is False and lgu.features.FeatureEncoder(f).convs is False
    lgu.features.uninstall(f)


def test_construction_refuses_other_architectures(lgu):
    K = lgu.context
    nn = torch.nn

    def enc():
        return R.RefEncoder(256, "none")
    K.ContextEncoder(enc())
    K.ContextEncoder(R.RefEncoder(128, "none"))
    with pytest.raises(RuntimeError, match=r"norm1 is an InstanceNorm2d.*features\.install"):
        K.ContextEncoder(R.RefEncoder())
    with pytest.raises(RuntimeError, match=r"features\.install"):
        K.install(R.RefEncoder())
    bad = enc()
    bad.layer2[1].norm2 = nn.InstanceNorm2d(64)
    with pytest.raises(RuntimeError, match=r"layer2\.1\.norm2 is an InstanceNorm2d.*features\.install"):
        K.ContextEncoder(bad)
    bad = enc()
    bad.layer1[0].norm1 = nn.GroupNorm(4, 32)
    with pytest.raises(RuntimeError, match=r"layer1\.0\.norm1 must be an empty nn\.Sequential"):
        K.ContextEncoder(bad)
    bad = enc()
    bad.norm1 = nn.Sequential(nn.ReLU())
    with pytest.raises(RuntimeError, match=r"ContextEncoder: norm1 must be an empty"):
        K.ContextEncoder(bad)
    bad = enc()
    bad.layer3[0].downsample = nn.Sequential(bad.layer3[0].downsample[0], nn.BatchNorm2d(128))
    with pytest.raises(RuntimeError, match=r"layer3\.0\.downsample\.1 must be an empty"):
        K.ContextEncoder(bad)
    bad = enc()
    bad.layer3[0].downsample = nn.Sequential(nn.Conv2d(64, 128, 1, stride=1), nn.Sequential())
    with pytest.raises(RuntimeError, match=r"layer3\.0\.downsample\.0 must be Conv2d\(64, 128, 1, stride=2"):
        K.ContextEncoder(bad)
    bad = enc()
    bad.layer1[1].downsample = nn.Sequential(nn.Conv2d(32, 32, 1), nn.Sequential())
    with pytest.raises(RuntimeError, match=r"layer1\.1\.downsample must be None"):
        K.ContextEncoder(bad)
    bad = enc()
    del bad.layer3
    with pytest.raises(RuntimeError, match="layer3 must be"):
        K.ContextEncoder(bad)
    bad = enc()
    bad.layer2 = nn.Sequential(bad.layer2[0])
    with pytest.raises(RuntimeError, match="layer2 must be a Sequential of two"):
        K.ContextEncoder(bad)
    bad = enc()
    bad.layer1[0].conv2 = nn.Conv2d(32, 32, 3, padding=2)
    with pytest.raises(RuntimeError, match=r"layer1\.0\.conv2 must be Conv2d\(32, 32, 3, stride=1, padding=1\)"):
        K.ContextEncoder(bad)
    bad = enc()
    bad.layer2[0].conv1 = nn.Conv2d(32, 64, 3, stride=1, padding=1)
    with pytest.raises(RuntimeError, match=r"layer2\.0\.conv1 must be Conv2d\(32, 64, 3, stride=2"):
        K.ContextEncoder(bad)
    bad = enc()
    bad.layer3[1].conv1 = nn.Conv2d(128, 128, 3, padding=1, bias=False)
    with pytest.raises(RuntimeError, match=r"layer3\.1\.conv1 must be Conv2d"):
        K.ContextEncoder(bad)
    bad = enc()
    bad.conv1 = nn.Conv2d(3, 48, 7, stride=2, padding=3)
    with pytest.raises(RuntimeError, match=r"ContextEncoder: conv1 must be Conv2d\(3, 32, 7, stride=2, padding=3\)"):
        K.ContextEncoder(bad)
    bad = enc()
    bad.conv2 = nn.Conv2d(128, 256, 3, padding=1)
    with pytest.raises(RuntimeError, match=r"ContextEncoder: conv2 must be Conv2d\(128, 256, 1"):
        K.ContextEncoder(bad)
    other = nn.Linear(3, 3)
    with pytest.raises(RuntimeError, match="conv1 must be a Conv2d"):
        K.install(other)
    assert "forward" not in other.__dict__


def test_cpu_inputs_reach_the_module_and_give_its_result(lgu):
    _, m, images = fixture("context_cnet_1x64x48")
    with torch.no_grad():
        want = m(images)
        wr = lgu.context.install(m)
        got = m(images)
        with torch.autocast("cpu", dtype=torch.bfloat16):
            got_ac, want_ac = m(images), type(m).forward(m, images)
    assert m(images.clone().requires_grad_()).requires_grad
    lgu.context.uninstall(m)
    assert wr.fused_calls == 0 and same_bits(got, want) and same_bits(got_ac, want_ac)


# ---- GPU ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def encoder_case(name, seed_offset=0, kind="context"):
    """(device module, device images, float64 CPU forward of the same module); cached and never written."""
    if kind == "context":
        m, images = C.make_case(name, seed_offset)
        m64 = R.RefEncoder(C.OUTPUT_DIM, "none").double()
    else:
        m, images = R.make_case(name, seed_offset)
        m64 = R.RefEncoder().double()
    m64.load_state_dict(m.state_dict())
    with torch.no_grad():
        ref = m64.eval()(images.double())
    return m.to(DEV), images.to(DEV), ref


def rms(x, ref):
    return float(((x.double().cpu() - ref) ** 2).mean().sqrt())


# The library's convolutions do not repeat their bits from call to call at every configuration of these encoders (two
# calls of the module's own forward differ under autocast and at 2x40x56 in fp32; the fp32 forward at 1x64x48 repeats, which
# tests/test_features.py relies on too).  So "the module's own forward" and "the module's convolution" are pinned by
# identity where bits cannot be: which callables ran, on what, in which order; and by bits in fp32 at 1x64x48.
class Calls:
    """Records, in order, every Conv2d of `m` that runs (by name) and every instance-norm call of the library (mode)."""

    def __init__(self, lgu, m, monkeypatch):
        self.seq = []
        self._hooks = [mod.register_forward_hook(functools.partial(self._conv, name))
                       for name, mod in m.named_modules() if isinstance(mod, torch.nn.Conv2d)]
        own = lgu.features._instnorm

        def inorm(a, b, out, mode, eps):
            self.seq.append(("instnorm", mode, b is not None, out is a))
            return own(a, b, out, mode, eps)
        monkeypatch.setattr(lgu.features, "_instnorm", inorm)

    def _conv(self, name, mod, args, res):
        self.seq.append(("conv", name, tuple(args[0].shape)))

    def take(self):
        seq, self.seq = self.seq, []
        return seq

    def close(self):
        for h in self._hooks:
            h.remove()


@pytest.fixture
def no_threshold(lgu, monkeypatch):
    """The routing by size follows a measurement (MIN_FUSED_PIXELS); these tests are about the fused path."""
    monkeypatch.setattr(lgu.encconv, "MIN_FUSED_PIXELS", {s: 0 for s in lgu.encconv.SHAPES})


@pytest.fixture
def count_launches(lgu, monkeypatch):
    calls = []
    own = lgu.encconv.enc_conv3x3

    def spy(x, pack, stride=1, relu=False, residual=None, down=None):
        calls.append((x.shape[1], pack[1].shape[0], stride, relu, residual is not None, down is not None))
        return own(x, pack, stride=stride, relu=relu, residual=residual, down=down)
    monkeypatch.setattr(lgu.encconv, "enc_conv3x3", spy)
    return calls


def autocast_half():
    """A float16 autocast region of its own: autocast keeps the half copy of a parameter for the length of a region, so a
    load_state_dict inside one would not reach the module's own convolutions."""
    return torch.autocast("cuda", dtype=torch.float16)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(C.CASES))
def test_installed_context_encoder_is_as_close_to_float64_as_the_module(lgu, no_threshold, count_launches, name):
    m, images, ref = encoder_case(name)
    with torch.no_grad(), autocast_half():
        own = m(images)
        wr = lgu.context.install(m)
        try:
            before = wr.fused_calls
            got = m(images)
            assert wr.fused_calls == before + 1 and len(count_launches) == 12
            got_half_in = m(images.half())                                 # a half input is served too
            assert wr.fused_calls == before + 2
        finally:
            lgu.context.uninstall(m)
    # twelve launches: relu then residual per block, the two strided blocks with their branch
    assert count_launches[:12] == count_launches[12:] == [(32, 32, 1, True, False, False), (32, 32, 1, False, True, False)] * 2 + [
        (32, 64, 2, True, False, True), (64, 64, 1, False, True, False), (64, 64, 1, True, False, False),
        (64, 64, 1, False, True, False), (64, 128, 2, True, False, True), (128, 128, 1, False, True, False),
        (128, 128, 1, True, False, False), (128, 128, 1, False, True, False)]
    assert got.dtype == own.dtype == got_half_in.dtype == torch.float16 and got.shape == own.shape == got_half_in.shape == ref.shape
    r_got, r_own, r_half = rms(got, ref), rms(own, ref), rms(got_half_in, ref)
    print("%s: rms installed %.4g (half images %.4g), module %.4g, ratio %.3f" % (name, r_got, r_half, r_own, r_got / r_own))
    assert r_got <= 1.25 * r_own


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(R.CASES))
def test_feature_encoder_with_convs_is_as_close_to_float64_as_the_module(lgu, no_threshold, count_launches, name):
    m, images, ref = encoder_case(name, kind="features")
    with torch.no_grad(), autocast_half():
        own = m(images)
        wr = lgu.features.install(m, convs=True)
        try:
            got = m(images)
            assert wr.fused_calls == 1 and len(count_launches) == 12
        finally:
            lgu.features.uninstall(m)
    # identity epilogues only; the instance-norm calls take the outputs and the branch
    assert all(not relu and not res for _, _, _, relu, res, _ in count_launches)
    assert [c[5] for c in count_launches] == [False] * 4 + [True] + [False] * 3 + [True] + [False] * 3
    assert got.dtype == own.dtype == torch.float16 and got.shape == own.shape
    r_got, r_own = rms(got, ref), rms(own, ref)
    print("%s convs=True: rms installed %.4g, module %.4g, ratio %.3f" % (name, r_got, r_own, r_got / r_own))
    assert r_got <= 1.25 * r_own


def _parent_fused(lgu, m, x):
    """FeatureEncoder._fused as it stood before `convs`: the module's convolutions, one instance-norm call per site."""
    b, n, c1, h1, w1 = x.shape
    y = m.conv1(x.view(b * n, c1, h1, w1))
    y = lgu.features._instnorm(y, None, y, 0, m.norm1.eps)
    for layer in (m.layer1, m.layer2, m.layer3):
        for blk in layer:
            t = blk.conv1(y)
            t = blk.conv2(lgu.features._instnorm(t, None, t, 0, blk.norm1.eps))
            if blk.downsample is None:
                y = lgu.features._instnorm(t, y, t, 1, blk.norm2.eps)
            else:
                y = lgu.features._instnorm(t, blk.downsample[0](y), t, 2, blk.norm2.eps)
    y = m.conv2(y)
    return y.view(b, n, y.shape[1], y.shape[2], y.shape[3])


@pytest.mark.gpu
@pytest.mark.parametrize("half", [False, True])
def test_features_install_keeps_what_it_ran(lgu, monkeypatch, count_launches, half):
    """features.install(m) (convs=False) launches no encoder convolution of this library: it runs the module's 16
    convolutions and the 13 instance-norm calls of FeatureEncoder._fused as it stood, on the same shapes in the same
    order, and in fp32 (where the library repeats its bits) gives that forward's bits; convs=True leaves the fp32 path
    alone."""
    m, images, _ = encoder_case("features_fnet_1x64x48", kind="features")
    calls = Calls(lgu, m, monkeypatch)
    try:
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16, enabled=half):
            want = _parent_fused(lgu, m, images)
            seq = calls.take()
            assert len([c for c in seq if c[0] == "conv"]) == 16 and len([c for c in seq if c[0] == "instnorm"]) == 13
            for convs in (False,) if half else (False, True):
                wr = lgu.features.FeatureEncoder(m, convs=convs)
                got = wr(images)
                assert wr.fused_calls == 1 and wr.convs is convs and count_launches == []
                assert calls.take() == seq and got.dtype == want.dtype and got.shape == want.shape
                if not half:
                    assert same_bits(got, want)
                else:       # the library's half convolutions do not repeat their bits: a few half roundings apart
                    assert float((got.float() - want.float()).abs().max()) <= 2.0 ** -8 * float(want.float().abs().max())
    finally:
        calls.close()


@pytest.mark.gpu
def test_other_modes_are_the_modules_own_forward(lgu, no_threshold, count_launches, monkeypatch):
    m, images, _ = encoder_case("context_cnet_1x64x48")
    seen = []
    own = type(m).forward

    def spy(self, x):
        seen.append((self, x))
        seen.append(own(self, x))
        return seen[-1]
    with torch.no_grad():
        want32 = own(m, images)
    monkeypatch.setattr(type(m), "forward", spy)
    wr = lgu.context.install(m)

    def through_the_module(x):
        """m(x) calls the class's forward with m and x themselves and returns its result as it is."""
        del seen[:]
        got = m(x)
        assert len(seen) == 2 and seen[0][0] is m and seen[0][1] is x and got is seen[1]
        return got
    try:
        with torch.no_grad():
            got = through_the_module(images)                               # fp32, autocast off
            assert got.dtype == torch.float32 and same_bits(got, want32)   # the library repeats its bits here
            with torch.autocast("cuda", dtype=torch.bfloat16):
                assert through_the_module(images).dtype == torch.bfloat16
            with autocast_half():
                nc = images.transpose(3, 4).contiguous().transpose(3, 4)
                assert not nc.is_contiguous() and through_the_module(nc).dtype == torch.float16
                cl = images[0].contiguous(memory_format=torch.channels_last)[None]
                assert not cl.is_contiguous() and through_the_module(cl).dtype == torch.float16
                m.train()
                m.dropout = torch.nn.Dropout2d(p=0.5)
                assert through_the_module(images).dtype == torch.float16   # a dropout in training mode
                m.eval()
                m.dropout = None
        with autocast_half():
            assert through_the_module(images.clone().requires_grad_()).requires_grad    # gradients are wanted
        assert wr.fused_calls == 0 and count_launches == []
        del seen[:]
        with torch.no_grad(), autocast_half():
            m(images)
        assert wr.fused_calls == 1 and len(count_launches) == 12 and seen == []
    finally:
        m.eval()
        m.dropout = None
        lgu.context.uninstall(m)


@pytest.mark.gpu
def test_state_dict_loads_after_install(lgu, no_threshold):
    """The packs follow the parameters: after load_state_dict the installed encoder meets the whole-encoder contract for
    the NEW weights' float64 forward, which the old weights' result misses by far."""
    twin, images, ref = encoder_case("context_cnet_1x64x48", 7)
    fresh = R.RefEncoder(256, "none").to(DEV).eval()
    wr = lgu.context.install(fresh)
    with torch.no_grad():
        with autocast_half():
            first = fresh(images)                                          # packs made of the default initialisation
        fresh.load_state_dict(twin.state_dict())
        with autocast_half():
            got, own = fresh(images), twin(images)
    assert wr.fused_calls == 2 and "forward" not in twin.__dict__
    r_got, r_own, r_first = rms(got, ref), rms(own, ref), rms(first, ref)
    print("after load_state_dict: rms installed %.4g, module %.4g; with the old weights %.4g" % (r_got, r_own, r_first))
    assert r_got <= 1.25 * r_own and r_first > 20 * r_own
    assert list(fresh.state_dict().keys()) == list(twin.state_dict().keys())


@pytest.mark.gpu
def test_calls_below_the_threshold_take_the_modules_convolution(lgu, monkeypatch, count_launches):
    """With MIN_FUSED_PIXELS above the call's size no encoder convolution of this library is launched: the context
    encoder runs the module's 16 convolutions on the shapes of the module's own forward (with torch's tail, and still
    within the whole-encoder contract), the feature encoder with convs=True what features.install(m) runs.  A threshold on one
    shape routes that shape only."""
    E = lgu.encconv
    m, images, ref = encoder_case("context_cnet_2x40x56")
    f, fimages, _ = encoder_case("features_fnet_2x40x56", kind="features")
    monkeypatch.setattr(E, "MIN_FUSED_PIXELS", {s: 1 << 40 for s in E.SHAPES})
    calls, fcalls = Calls(lgu, m, monkeypatch), Calls(lgu, f, monkeypatch)
    try:
        with torch.no_grad(), autocast_half():
            own = type(m).forward(m, images)
            seq = calls.take()
            assert len(seq) == 16 and all(c[0] == "conv" for c in seq)
            wr = lgu.context.ContextEncoder(m)
            got = wr(images)
            # the branch's 1x1 runs right behind the block's first convolution here, behind the second in the module
            assert wr.fused_calls == 1 and count_launches == [] and sorted(calls.take()) == sorted(seq)
            assert rms(got, ref) <= 1.25 * rms(own, ref)
            _parent_fused(lgu, f, fimages)
            seq = fcalls.take()
            wf = lgu.features.FeatureEncoder(f, convs=True)
            wf(fimages)
            assert wf.fused_calls == 1 and count_launches == [] and fcalls.take() == seq
            # layer1 is 2 x 20 x 28 = 1120 output pixels here, layer2 280: a threshold between them on every shape
            monkeypatch.setattr(E, "MIN_FUSED_PIXELS", {s: 1000 for s in E.SHAPES})
            wf(fimages)
            assert [c[:3] for c in count_launches] == [(32, 32, 1)] * 4
            assert [c[1] for c in fcalls.take() if c[0] == "conv"] == [c[1] for c in seq if c[0] == "conv" and not c[1].startswith("layer1")]
            monkeypatch.setattr(E, "MIN_FUSED_PIXELS", {s: (1 << 40 if s == (32, 32, 1) else 0) for s in E.SHAPES})
            del count_launches[:]
            calls.take()
            wr(images)
            assert [c[:3] for c in count_launches] == [(32, 64, 2)] + [(64, 64, 1)] * 3 + [(64, 128, 2)] + [(128, 128, 1)] * 3
            assert [c[1] for c in calls.take()] == ["conv1", "layer1.0.conv1", "layer1.0.conv2", "layer1.1.conv1", "layer1.1.conv2", "conv2"]
    finally:
        calls.close()
        fcalls.close()
