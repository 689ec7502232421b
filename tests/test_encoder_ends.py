"""The two encoders with `ends=True`: the stem and the output layer on csrc/encends.hip (lgu_slam_amd.context,
lgu_slam_amd.features) on the seeded cases of tests/context_restatement.py and tests/features_restatement.py.

Contract:
- with ends=True the fused route of the context encoder, and of the feature encoder with convs=True, runs no Conv2d of the
  module: one stem launch, twelve residual-stage launches, one output launch;
- whole encoder under float16 autocast: rms(installed - ref64) <= 1.25 rms(module's own forward - ref64) on the same
  device, the project's whole-encoder contract of tests/test_context.py;
- net_inp is the output layer's SPLIT launch on the fused route and torch's split + tanh + relu on every other;
- every other mode is the module's own forward; the defaults launch neither new operator.
The GPU tests read only the restatements, never the reference tree.
"""
import functools

import pytest

torch = pytest.importorskip("torch")

from tests import context_restatement as C  # noqa: E402
from tests import encends_restatement as RE  # noqa: E402
from tests import features_restatement as R  # noqa: E402

DEV = "cuda"
TWELVE = [(32, 32, 1)] * 4 + [(32, 64, 2)] + [(64, 64, 1)] * 3 + [(64, 128, 2)] + [(128, 128, 1)] * 3


def same_bits(a, b):
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    iv = {torch.float16: torch.int16, torch.float32: torch.int32, torch.bfloat16: torch.int16}[a.dtype]
    return bool(torch.equal(a.view(iv), b.view(iv)))


# ---- CPU ------------------------------------------------------------------------------------------------------------
def test_ends_keeps_the_state_dict_keys_and_install_is_idempotent(lgu):
    m = R.set_weights(R.RefEncoder(256, "none"), 3)
    keys = list(m.state_dict().keys())
    wr = lgu.context.install(m, ends=True)
    assert isinstance(wr, lgu.context.ContextEncoder) and m.forward is wr and wr.ends is True
    assert lgu.context.install(m) is wr and lgu.context.install(m, ends=False) is wr and wr.ends is True
    assert list(m.state_dict().keys()) == keys and len(list(m.parameters())) == 2 * 16 and not list(m.buffers())
    m.load_state_dict(R.set_weights(R.RefEncoder(256, "none"), 4).state_dict())
    lgu.context.uninstall(m)
    assert "forward" not in m.__dict__ and list(m.state_dict().keys()) == keys
    assert lgu.context.install(m).ends is False and lgu.context.ContextEncoder(m).ends is False
    lgu.context.uninstall(m)
    f = R.RefEncoder()
    fkeys = list(f.state_dict().keys())
    wf = lgu.features.install(f, convs=True, ends=True)
    assert wf.convs is True and wf.ends is True and lgu.features.install(f) is wf and list(f.state_dict().keys()) == fkeys
    lgu.features.uninstall(f)
    wf = lgu.features.install(f, ends=True)
    assert wf.convs is False and wf.ends is True                     # independent of convs
    lgu.features.uninstall(f)
    assert lgu.features.install(f).ends is False and lgu.features.FeatureEncoder(f, convs=True).ends is False
    lgu.features.uninstall(f)


def test_cpu_inputs_reach_the_modules_own_forward_with_ends(lgu):
    for make, install, uninstall in ((lambda: C.make_case("context_cnet_1x64x48"), lgu.context.install, lgu.context.uninstall),
                                     (lambda: R.make_case("features_fnet_1x64x48"),
                                      functools.partial(lgu.features.install, convs=True), lgu.features.uninstall)):
        m, images = make()
        with torch.no_grad():
            want = m(images)
            wr = install(m, ends=True)
            got = m(images)
            with torch.autocast("cpu", dtype=torch.bfloat16):
                got_ac, want_ac = m(images), type(m).forward(m, images)
        assert m(images.clone().requires_grad_()).requires_grad
        uninstall(m)
        assert wr.ends is True and wr.fused_calls == 0 and same_bits(got, want) and same_bits(got_ac, want_ac)


@pytest.mark.parametrize("ends", [False, True])
def test_net_inp_on_the_cpu_is_split_tanh_relu_of_the_modules_output(lgu, ends):
    m, images = C.make_case("context_cnet_1x64x48")
    wr = lgu.context.ContextEncoder(m, ends=ends)
    with torch.no_grad():
        ctx = m(images)
        net, inp = wr.net_inp(images)
    want_net, want_inp = ctx.split([128, 128], dim=2)
    assert wr.fused_calls == 0 and net.is_contiguous() and inp.is_contiguous()
    assert tuple(net.shape) == tuple(inp.shape) == (1, 1, 128, 8, 6)
    assert same_bits(net, want_net.tanh()) and same_bits(inp, want_inp.relu())
    narrow = lgu.context.ContextEncoder(R.RefEncoder(128, "none"), ends=ends)
    with pytest.raises(RuntimeError, match=r"net_inp: output_dim must be 256 .*got 128"):
        narrow.net_inp(images)


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


def autocast_half():
    return torch.autocast("cuda", dtype=torch.float16)


class Calls:
    """Records, in order, every Conv2d of `m` that runs (by name) and every instance-norm call of the library (mode)."""

    def __init__(self, lgu, m, monkeypatch):
        self.seq = []
        self._hooks = [mod.register_forward_hook(functools.partial(self._conv, name))
                       for name, mod in m.named_modules() if isinstance(mod, torch.nn.Conv2d)]
        own = lgu.features._instnorm

        def inorm(a, b, out, mode, eps):
            self.seq.append(("instnorm", mode))
            return own(a, b, out, mode, eps)
        monkeypatch.setattr(lgu.features, "_instnorm", inorm)

    def _conv(self, name, mod, args, res):
        self.seq.append(("conv", name))

    def convs(self):
        return [c[1] for c in self.seq if c[0] == "conv"]

    def norms(self):
        return [c for c in self.seq if c[0] == "instnorm"]

    def take(self):
        seq, self.seq = self.seq, []
        return seq

    def close(self):
        for h in self._hooks:
            h.remove()


@pytest.fixture
def no_threshold(lgu, monkeypatch):
    """The routing by size follows a measurement; these tests are about the fused path."""
    monkeypatch.setattr(lgu.encconv, "MIN_FUSED_PIXELS", {s: 0 for s in lgu.encconv.SHAPES})
    monkeypatch.setattr(lgu.encconv, "MIN_STEM_PIXELS", 0)
    monkeypatch.setattr(lgu.encconv, "MIN_OUT_PIXELS", {c: 0 for c in lgu.encconv.OUT_COUTS})


@pytest.fixture
def spies(lgu, monkeypatch):
    """Every call of the three operator functions, in order: ("stem", relu), ("conv3", (Cin, Cout, stride)), ("out", Cout,
    split)."""
    calls = []
    E = lgu.encconv
    stem, conv3, out1 = E.enc_stem7x7, E.enc_conv3x3, E.enc_out1x1

    def spy_stem(x, pack, relu=False):
        calls.append(("stem", relu))
        return stem(x, pack, relu=relu)

    def spy_conv3(x, pack, stride=1, relu=False, residual=None, down=None):
        calls.append(("conv3", (x.shape[1], pack[1].shape[0], stride)))
        return conv3(x, pack, stride=stride, relu=relu, residual=residual, down=down)

    def spy_out(x, pack, split=False):
        calls.append(("out", pack[1].shape[0], split))
        return out1(x, pack, split=split)
    monkeypatch.setattr(E, "enc_stem7x7", spy_stem)
    monkeypatch.setattr(E, "enc_conv3x3", spy_conv3)
    monkeypatch.setattr(E, "enc_out1x1", spy_out)
    return calls


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(C.CASES))
def test_context_encoder_with_ends_runs_no_library_convolution_and_meets_the_contract(lgu, no_threshold, spies, monkeypatch, name):
    m, images, ref = encoder_case(name)
    calls = Calls(lgu, m, monkeypatch)
    try:
        with torch.no_grad(), autocast_half():
            own = m(images)
            assert len(calls.take()) == 16
            wr = lgu.context.install(m, ends=True)
            try:
                got = m(images)
                assert wr.fused_calls == 1 and calls.take() == []            # no Conv2d of the module ran
                assert spies == [("stem", True)] + [("conv3", s) for s in TWELVE] + [("out", 256, False)]
                got_half_in = m(images.half())                               # a half input is served too
                assert wr.fused_calls == 2 and calls.take() == [] and len(spies) == 28
            finally:
                lgu.context.uninstall(m)
    finally:
        calls.close()
    assert got.dtype == own.dtype == torch.float16 and got.shape == own.shape == got_half_in.shape == ref.shape
    assert got.is_contiguous()
    r_got, r_own, r_half = rms(got, ref), rms(own, ref), rms(got_half_in, ref)
    print("%s ends=True: rms installed %.4g (half images %.4g), module %.4g, ratio %.3f" % (name, r_got, r_half, r_own, r_got / r_own))
    assert r_got <= 1.25 * r_own and r_half <= 1.25 * r_own


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(R.CASES))
def test_feature_encoder_with_convs_and_ends_runs_no_library_convolution_and_meets_the_contract(lgu, no_threshold, spies, monkeypatch, name):
    m, images, ref = encoder_case(name, kind="features")
    calls = Calls(lgu, m, monkeypatch)
    try:
        with torch.no_grad(), autocast_half():
            own = m(images)
            calls.take()
            wr = lgu.features.install(m, convs=True, ends=True)
            try:
                got = m(images)
                assert wr.fused_calls == 1 and calls.convs() == [] and len(calls.norms()) == 13
            finally:
                lgu.features.uninstall(m)
    finally:
        calls.close()
    # the identity epilogue: norm1's call reads the stem
    assert spies == [("stem", False)] + [("conv3", s) for s in TWELVE] + [("out", 128, False)]
    assert got.dtype == own.dtype == torch.float16 and got.shape == own.shape == ref.shape
    r_got, r_own = rms(got, ref), rms(own, ref)
    print("%s convs=True, ends=True: rms installed %.4g, module %.4g, ratio %.3f" % (name, r_got, r_own, r_got / r_own))
    assert r_got <= 1.25 * r_own


@pytest.mark.gpu
def test_net_inp_is_the_split_launch_on_the_fused_route(lgu, no_threshold, spies, monkeypatch):
    m, images, _ = encoder_case("context_cnet_2x40x56")
    calls = Calls(lgu, m, monkeypatch)
    launched = []
    for fn in ("tanh", "relu", "split"):
        own = getattr(torch.Tensor, fn)
        monkeypatch.setattr(torch.Tensor, fn, (lambda own, fn: lambda self, *a, **k: (launched.append(fn), own(self, *a, **k))[1])(own, fn))
    try:
        wr = lgu.context.ContextEncoder(m, ends=True)
        with torch.no_grad(), autocast_half():
            plain = wr(images)
            del spies[:], launched[:]
            net, inp = wr.net_inp(images)
            assert spies[-1] == ("out", 256, True) and spies.count(("out", 256, True)) == 1 and len(spies) == 14
            assert launched == [] and calls.take() == [] and wr.fused_calls == 2   # nothing after the launch, no Conv2d
            assert net.is_contiguous() and inp.is_contiguous() and tuple(net.shape) == tuple(inp.shape) == (1, 2, 128, 5, 7)
            assert same_bits(inp, torch.relu(plain[:, :, 128:]))
            t, bound = RE.tanh_bound(plain[:, :, :128].cpu().double())
            err = (net.cpu().double() - t).abs()
            print("net_inp: tanh max err / bound %.3f" % float((err / bound).max()))
            assert bool((err <= bound).all())
            # every other route: the forward, then torch's split, tanh and relu
            for other, x in ((lgu.context.ContextEncoder(m), images), (wr, images.transpose(3, 4).contiguous().transpose(3, 4))):
                del spies[:], launched[:]
                ctx = other(x)
                del launched[:]
                net2, inp2 = other.net_inp(x)
                assert launched == ["split", "tanh", "relu"] and ("out", 256, True) not in spies
                assert net2.is_contiguous() and inp2.is_contiguous() and net2.shape == net.shape
                assert calls.convs()[-1] == "conv2"
                assert float((inp2.float() - torch.relu(ctx[:, :, 128:]).float()).abs().max()) <= 2.0 ** -8 * float(ctx.float().abs().max())
                calls.take()
    finally:
        calls.close()


@pytest.mark.gpu
def test_ends_without_convs_takes_only_conv1_and_conv2_from_the_module(lgu, no_threshold, spies, monkeypatch):
    m, images, ref = encoder_case("features_fnet_1x64x48", kind="features")
    calls = Calls(lgu, m, monkeypatch)
    try:
        with torch.no_grad(), autocast_half():
            own = m(images)
            calls.take()
            lgu.features.FeatureEncoder(m)(images)
            base = calls.take()
            wr = lgu.features.FeatureEncoder(m, ends=True)
            got = wr(images)
            assert wr.fused_calls == 1 and spies == [("stem", False), ("out", 128, False)]
            # the other 14 convolutions and the 13 instance-norm calls as before
            assert [c for c in base if c[0] == "conv"][0] == ("conv", "conv1") and [c for c in base if c[0] == "conv"][-1] == ("conv", "conv2")
            assert calls.seq == [c for c in base if c not in (("conv", "conv1"), ("conv", "conv2"))]
            assert len(calls.convs()) == 14 and len(calls.norms()) == 13
            assert rms(got, ref) <= 1.25 * rms(own, ref)
            # the fp32 path does not change
            calls.take()
            del spies[:]
    finally:
        calls.close()
    calls = Calls(lgu, m, monkeypatch)
    try:
        with torch.no_grad():
            want = lgu.features.FeatureEncoder(m)(images)
            seq = calls.take()
            got32 = lgu.features.FeatureEncoder(m, convs=True, ends=True)(images)
            assert spies == [] and calls.take() == seq and len([c for c in seq if c[0] == "conv"]) == 16 and same_bits(got32, want)
    finally:
        calls.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["context", "features"])
def test_other_modes_are_the_modules_own_forward_with_ends(lgu, no_threshold, spies, monkeypatch, kind):
    m, images, _ = encoder_case("context_cnet_1x64x48") if kind == "context" else encoder_case("features_fnet_1x64x48", kind="features")
    seen = []
    own = type(m).forward

    def spy(self, x):
        seen.append((self, x))
        seen.append(own(self, x))
        return seen[-1]
    monkeypatch.setattr(type(m), "forward", spy)
    if kind == "context":
        wr = lgu.context.install(m, ends=True)
    else:
        wr = lgu.features.install(m, convs=True, ends=True)

    def through_the_module(x):
        """m(x) calls the class's forward with m and x themselves and returns its result as it is."""
        del seen[:]
        got = m(x)
        assert len(seen) == 2 and seen[0][0] is m and seen[0][1] is x and got is seen[1]
        return got
    try:
        with torch.no_grad():
            if kind == "context":                                          # there is no fp32 kernel
                assert through_the_module(images).dtype == torch.float32
            else:                                                          # the fp32 instance-norm path, the module's convolutions
                assert m(images).dtype == torch.float32 and spies == []
            with torch.autocast("cuda", dtype=torch.bfloat16):
                assert through_the_module(images).dtype == torch.bfloat16
            with autocast_half():
                cl = images[0].contiguous(memory_format=torch.channels_last)[None]
                assert not cl.is_contiguous() and through_the_module(cl).dtype == torch.float16
                m.train()
                m.dropout = torch.nn.Dropout2d(p=0.5)
                assert through_the_module(images).dtype == torch.float16   # a dropout in training mode
                m.eval()
                m.dropout = None
        with autocast_half():
            assert through_the_module(images.clone().requires_grad_()).requires_grad    # gradients are wanted
        assert spies == []
        del seen[:]
        with torch.no_grad(), autocast_half():
            m(images)
        assert len(spies) == 14 and seen == []
    finally:
        m.eval()
        m.dropout = None
        (lgu.context if kind == "context" else lgu.features).uninstall(m)


@pytest.mark.gpu
def test_state_dict_loads_after_install_with_ends(lgu, no_threshold, spies):
    """The packs of the stem and the output layer follow the parameters: after load_state_dict the installed encoder meets
    the whole-encoder contract for the NEW weights' float64 forward, which the old weights' result misses by far."""
    twin, images, ref = encoder_case("context_cnet_1x64x48", 7)
    fresh = R.RefEncoder(256, "none").to(DEV).eval()
    wr = lgu.context.install(fresh, ends=True)
    with torch.no_grad():
        with autocast_half():
            first = fresh(images)                                          # packs made of the default initialisation
        fresh.load_state_dict(twin.state_dict())
        with autocast_half():
            got, own = fresh(images), twin(images)
            net, inp = wr.net_inp(images)
    assert wr.fused_calls == 3 and "forward" not in twin.__dict__ and len(spies) == 3 * 14
    r_got, r_own, r_first = rms(got, ref), rms(own, ref), rms(first, ref)
    print("ends=True after load_state_dict: rms installed %.4g, module %.4g; with the old weights %.4g" % (r_got, r_own, r_first))
    assert r_got <= 1.25 * r_own and r_first > 20 * r_own
    assert same_bits(inp, torch.relu(got[:, :, 128:]))
    assert list(fresh.state_dict().keys()) == list(twin.state_dict().keys())


@pytest.mark.gpu
def test_thresholds_route_exactly_their_layer_back_to_the_module(lgu, no_threshold, spies, monkeypatch):
    E = lgu.encconv
    m, images, ref = encoder_case("context_cnet_2x40x56")
    f, fimages, _ = encoder_case("features_fnet_2x40x56", kind="features")
    calls, fcalls = Calls(lgu, m, monkeypatch), Calls(lgu, f, monkeypatch)
    mid = [("conv3", s) for s in TWELVE]
    try:
        with torch.no_grad(), autocast_half():
            own = type(m).forward(m, images)
            calls.take()
            wr = lgu.context.ContextEncoder(m, ends=True)
            wf = lgu.features.FeatureEncoder(f, convs=True, ends=True)
            # the stem gives 2 x 20 x 28 = 1120 output pixels here, the output layer sees 2 x 5 x 7 = 70
            monkeypatch.setattr(E, "MIN_STEM_PIXELS", 1121)
            got = wr(images)
            assert spies == mid + [("out", 256, False)] and calls.convs() == ["conv1"]
            assert rms(got, ref) <= 1.25 * rms(own, ref)
            wf(fimages)
            assert spies[13:] == mid + [("out", 128, False)] and fcalls.convs() == ["conv1"]
            monkeypatch.setattr(E, "MIN_STEM_PIXELS", 1120)
            monkeypatch.setattr(E, "MIN_OUT_PIXELS", {128: 70, 256: 71})
            del spies[:]
            calls.take(), fcalls.take()
            got = wr(images)
            assert spies == [("stem", True)] + mid and calls.convs() == ["conv2"]
            assert rms(got, ref) <= 1.25 * rms(own, ref)
            net, inp = wr.net_inp(images)                                  # the output layer is the module's: torch's tail
            assert spies[13:] == [("stem", True)] + mid and calls.convs() == ["conv2", "conv2"] and net.is_contiguous()
            wf(fimages)
            assert spies[26:] == [("stem", False)] + mid + [("out", 128, False)] and fcalls.convs() == []
            monkeypatch.setattr(E, "MIN_OUT_PIXELS", {128: 71, 256: 0})
            del spies[:]
            wf(fimages)
            assert spies == [("stem", False)] + mid and fcalls.convs() == ["conv2"]
            # a stem of another width is the module's call
            wide = R.RefEncoder(256, "none")
            wide.conv1 = torch.nn.Conv2d(4, 32, 7, stride=2, padding=3)
            wide = wide.to(DEV).eval()
            wcalls = Calls(lgu, wide, monkeypatch)
            del spies[:]
            lgu.context.ContextEncoder(wide, ends=True)(torch.cat([images, images[:, :, :1]], dim=2).contiguous())
            assert spies == mid + [("out", 256, False)] and wcalls.convs() == ["conv1"]
            wcalls.close()
    finally:
        calls.close()
        fcalls.close()


@pytest.mark.gpu
def test_the_defaults_launch_neither_new_operator(lgu, no_threshold, spies, monkeypatch):
    m, images, _ = encoder_case("context_cnet_1x64x48")
    f, fimages, _ = encoder_case("features_fnet_1x64x48", kind="features")
    calls, fcalls = Calls(lgu, m, monkeypatch), Calls(lgu, f, monkeypatch)
    try:
        with torch.no_grad(), autocast_half():
            wr, wf = lgu.context.ContextEncoder(m), lgu.features.FeatureEncoder(f, convs=True)
            wr(images)
            wr.net_inp(images)
            wf(fimages)
        assert wr.ends is False and wf.ends is False and wr.fused_calls == 2 and wf.fused_calls == 1
        assert spies == [("conv3", s) for s in TWELVE] * 3
        assert calls.convs() == ["conv1", "conv2"] * 2 and fcalls.convs() == ["conv1", "conv2"]
    finally:
        calls.close()
        fcalls.close()
