"""The update operator's 1x1 convolution behind the correlation lookup (lgu_slam_amd.conv1, csrc/conv1.hip) against the
float64 restatement tests/conv1_restatement.py.

Numerics contract (include/lgu_corr.h):
- a single product is exact: impulses and the zero input are bit for bit act(half(b_h + x_h·w_h));
- every element of y = act(half(s)): |y - act(s64)| <= conv3_restatement.allowance(s64, S, terms=Cin + 2), S = Σ|x_h·w_h| +
  |b_h|: fp32 accumulation in any order, one half rounding, the half subnormal floor;
- fp32 x is rounded to half exactly once; a NaN reaches exactly its pixel's 128 outputs, through the ReLU as well; what
  lies behind the tensor's last channel is never read; a frame's bits do not depend on the batch.
The module's own autocast forward is not held to the single-layer bound; the test prints where it sits.
The GPU tests build their modules themselves and never read the reference tree.
"""
import ctypes
import os

import pytest

torch = pytest.importorskip("torch")

from tests import conv1_restatement as R1  # noqa: E402
from tests import conv3_restatement as R  # noqa: E402
from tests.test_upmask import same_bits  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = "lgu_conv1x1_o128_h16"
GROUP = 32          # pixels per staged group of csrc/conv1.hip
# the issue's shapes: the smallest at which a group of 32 pixels can go wrong (groups span frames and rows, the last one
# is partial), and (3,2,6), whose H * W % 4 == 0 puts a batch that spans frames on the 8-byte stores
SHAPES = [(1, 1, 1), (1, 2, 3), (2, 3, 17), (3, 5, 7), (1, 5, 33), (1, 6, 80), (3, 2, 6)]
# A workgroup takes a contiguous range of groups, one while there are at most 2 x 256 CUs of them, two up to twice that:
# 1031 groups are three per workgroup on an MI355X, so that both staging buffers are reused
BIG = (4, 67, 123)
assert (BIG[0] * BIG[1] * BIG[2] + GROUP - 1) // GROUP > 2 * 2 * 256
ALL_SHAPES = SHAPES + [BIG]
CASES = [(s, c) for s in ALL_SHAPES for c in (196, 98)] + [((2, 3, 17), c) for c in (147, 224, 33, 5)]
_CASES = {}
_NO_CPU = " must be a HIP device tensor: lgu_slam_amd has no CPU fallback"


def case(shape, cin):
    """(conv, x, s64, S) on the CPU for one shape and Cin, computed once and never changed."""
    key = (shape, cin)
    if key not in _CASES:
        m = R1.make_conv(50 + cin, cin)
        x = R.make_input(4000 + shape[1] * shape[2] + cin, *shape, C=cin)
        with torch.no_grad():
            _CASES[key] = (m, x) + R1.layer(x, m.weight, m.bias)
    return _CASES[key]


# ---- CPU ------------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_entry(lgu):
    from tests.test_abi import declared_symbols
    lib = ctypes.CDLL(lgu._lib._build.SO_PATH)
    L, M = lgu._lib, lgu.conv1
    assert ENTRY in declared_symbols() and hasattr(lib, ENTRY) and ENTRY in L.SIGNATURES
    sig = L.SIGNATURES[ENTRY]
    assert sig[0] is L.Conv1Args and issubclass(sig[0], ctypes.Structure) and sig[1] is ctypes.c_void_p
    assert [f[0] for f in sig[0]._fields_] == ["x", "wpack", "bias", "out", "N", "Cin", "H", "W", "flags"]
    assert ctypes.sizeof(sig[0]) == 4 * 8 + 5 * 4 + 4
    assert "conv1.hip" in lgu._build.SOURCES
    assert lgu.Conv1 is M.Conv1 and lgu.UpdateOperator is lgu.update.UpdateOperator
    text = open(os.path.join(ROOT, "include", "lgu_corr.h")).read()
    assert M.WPACK_HALVES == 7 * 8 * 64 * 8 == 28672 and M.COUT == 128 and M.MAX_CIN == 224
    assert "#define LGU_CONV1_WPACK_HALVES %d\n" % M.WPACK_HALVES in text
    assert "#define LGU_CONV1_COUT %d\n" % M.COUT in text
    assert "#define LGU_CONV1_MAX_CIN %d\n" % M.MAX_CIN in text
    assert "#define LGU_CONV1_X_HALF %d " % M.X_HALF in text and "#define LGU_CONV1_RELU %d " % M.RELU in text
    assert M.X_HALF & M.RELU == 0
    assert isinstance(M.MIN_FUSED_PIXELS, int) and M.MIN_FUSED_PIXELS >= 0


@pytest.mark.parametrize("cin", (196, 98, 224, 5))
def test_pack_puts_every_weight_in_its_documented_slot_and_zero_elsewhere(lgu, cin):
    g = torch.Generator().manual_seed(5 + cin)
    w = torch.randn((128, cin, 1, 1), generator=g)
    w[w == 0] = 1.0
    b = torch.randn((128,), generator=g)
    wpack, bias_h = lgu.conv1.pack_conv1(w, b)
    assert wpack.dtype == torch.float16 and wpack.is_contiguous() and wpack.numel() == lgu.conv1.WPACK_HALVES
    assert tuple(wpack.shape) == (7, 8, 64, 8) and same_bits(bias_h, b.half())
    kc, ct, lane, j = torch.meshgrid(torch.arange(7), torch.arange(8), torch.arange(64), torch.arange(8), indexing="ij")
    co, c = 16 * ct + (lane & 15), 32 * kc + 8 * (lane >> 4) + j
    live = c < cin
    # a weight tensor that names its own index: every (co, c < Cin) is named by exactly one live slot
    idx = torch.arange(128 * cin).view(128, cin)
    assert sorted(idx[co[live], c[live]].tolist()) == list(range(128 * cin))
    want = torch.zeros((7, 8, 64, 8), dtype=torch.float16)
    want[live] = w.half()[co[live], c[live], 0, 0]
    assert same_bits(wpack, want)
    assert bool((wpack[~live].view(torch.int16) == 0).all()) and bool((wpack[live] != 0).all())
    for bad_w, bad_b, what in ((torch.zeros(128, 225, 1, 1), b, "weight"), (w[:127], b[:127], "weight"), (w[:, :0], b, "weight"),
                               (torch.zeros(128, cin, 3, 3), b, "weight"), (w[:, :, 0, 0], b, "weight"), (w, torch.zeros(129), "bias")):
        with pytest.raises(RuntimeError, match=what + " must be"):
            lgu.conv1.pack_conv1(bad_w, bad_b)


@pytest.mark.parametrize("shape,cin", [((1, 1, 1), 196), ((2, 3, 17), 98), ((2, 3, 17), 5), ((1, 6, 80), 196)])
def test_restatement_equals_float64_conv2d_on_the_rounded_operands(shape, cin):
    m, x, s64, S = case(shape, cin)
    F = torch.nn.functional
    xh, wh, bh = R.h64(x), R.h64(m.weight), R.h64(m.bias)
    s = F.conv2d(xh, wh, bh)
    Sc = F.conv2d(xh.abs(), wh.abs(), bh.abs())
    # the operands are half values, so every product is exact in float64; the two sums differ in order only
    assert bool(((s - s64).abs() <= 2.0 ** -44 * S).all()) and bool(((Sc - S).abs() <= 2.0 ** -44 * S).all())
    assert bool((S >= s64.abs()).all()) and bool((R.allowance(s64, S, R1.terms(cin)) > 0).all())
    assert R1.terms(196) == 198 and R1.terms(cin) == cin + 2
    h = torch.tensor([-1.0, -0.0, 0.0, 2.0, float("nan")], dtype=torch.float16)
    y = R1.act(h, True)
    assert y[:4].tolist() == [0.0, -0.0, 0.0, 2.0] and bool(torch.isnan(y[4])) and R1.act(h, False) is h


def test_cpu_inputs_reach_the_module_and_install_keeps_the_state_dict(lgu):
    M = lgu.conv1
    for cin, relu in ((196, False), (98, True)):
        m, x = R1.make_conv(3, cin), R.make_input(1, 2, 5, 7, C=cin)
        keys = list(m.state_dict().keys())
        with torch.no_grad():
            want = m(x.clone())
            want = torch.relu(want) if relu else want
            direct = M.Conv1(m, relu=relu)
            assert same_bits(direct(x.clone()), want) and direct.fused_calls == 0
            wr = M.install(m, relu=relu)
            assert isinstance(wr, M.Conv1) and m.forward is wr and M.install(m) is wr
            assert list(m.state_dict().keys()) == keys and len(list(m.parameters())) == 2
            got = m(x.clone())
        want_grad = m(x.clone().requires_grad_())
        assert want_grad.requires_grad and same_bits(want_grad, want)
        M.uninstall(m)
        assert "forward" not in m.__dict__ and list(m.state_dict().keys()) == keys
        assert m.forward.__func__ is type(m).forward
        assert wr.fused_calls == 0 and same_bits(got, want) and tuple(got.shape) == (2, 128, 5, 7)
        # the cache follows the parameters
        p1 = wr.packed()
        assert wr.packed() is p1
        with torch.no_grad():
            m.weight.mul_(2.0)
        assert wr.packed() is not p1 and same_bits(wr.packed()[0], M.pack_conv1(m.weight, m.bias)[0])


def test_construction_and_install_refuse_other_layers(lgu):
    nn, M = torch.nn, lgu.conv1

    def conv(cin=196, cout=128, k=1, **kw):
        return nn.Conv2d(cin, cout, k, **kw)
    for ok in (conv(), conv(cin=1), conv(cin=224)):
        assert M.eligible(ok)
        M.Conv1(ok)
    bad = [conv(cin=225), conv(bias=False), conv(k=3, padding=1), conv(k=3), conv(cout=64), conv(padding=1), conv(stride=2),
           conv(groups=2), conv(dilation=2), nn.Sequential(conv()), nn.Linear(196, 128)]
    for m in bad:
        assert not M.eligible(m)
        with pytest.raises(RuntimeError, match="Conv1: the module must be"):
            M.Conv1(m)
        with pytest.raises(RuntimeError, match="Conv1: the module must be"):
            M.install(m)
        assert "forward" not in m.__dict__
    # a forward that carries another wrapper is refused, and nothing is bound
    m = conv()
    other = lgu.heads.Head(nn.Conv2d(128, 2, 3, padding=1))
    m.forward = other
    with pytest.raises(RuntimeError, match="conv1.install: forward already carries a Head"):
        M.install(m)
    assert m.forward is other
    M.uninstall(m)                      # a foreign wrapper is left alone
    assert m.forward is other


def test_a_stack_reaches_the_installed_layer_as_itself_on_cpu(lgu):
    """conv1.install on corr_encoder[0] and conv3.install on corr_encoder, in either order: both wrappers stay, the
    state_dict keys stay, and CPU inputs give the module's bits."""
    x = R.make_input(2, 1, 4, 5, C=R.COR_PLANES)
    for first in ("conv1", "conv3"):
        seq = R.make_stack(7, "corr_encoder")
        keys = list(seq.state_dict().keys())
        with torch.no_grad():
            want = seq(x.clone())
            if first == "conv1":
                w1, w3 = lgu.conv1.install(seq[0]), lgu.conv3.install(seq)
            else:
                w3, w1 = lgu.conv3.install(seq), lgu.conv1.install(seq[0])
            assert seq.forward is w3 and seq[0].forward is w1 and list(seq.state_dict().keys()) == keys
            assert same_bits(seq(x.clone()), want) and w1.fused_calls == 0 == w3.fused_calls
        lgu.conv3.uninstall(seq)
        assert seq[0].forward is w1
        lgu.conv1.uninstall(seq[0])
        assert "forward" not in seq[0].__dict__ and "forward" not in seq.__dict__


def test_operator_refusals_come_before_any_launch(lgu, monkeypatch):
    """Shape, Cin, pack size, bias shape, contiguity, dtypes, no-grad, device, the empty frame: each refusal's text, and
    which of two defects is reported.  None of them reaches the launch."""
    M = lgu.conv1
    H = torch.float16
    launched = []
    monkeypatch.setattr(M, "launch", lambda *a, **k: launched.append(a))

    def z(*shape, dtype=torch.float32):
        return torch.zeros(shape, dtype=dtype)

    def nc(t):
        return torch.zeros(tuple(t.shape) + (2,), dtype=t.dtype)[..., 0]

    x, wp, bh = z(2, 196, 2, 3), z(7, 8, 64, 8, dtype=H), z(128, dtype=H)
    no_grad = "conv1x1 has no autograd: its outputs would carry no gradient. Call it under torch.no_grad() or pass detached inputs"
    table = [
        ((x, wp, bh), {}, "x" + _NO_CPU),
        ((x.half(), wp, bh), {"relu": True}, "x" + _NO_CPU),
        ((z(196, 2, 2), wp, bh), {}, "x must be (N,Cin,H,W), got (196, 2, 2)"),
        ((z(1, 225, 2, 2), wp, bh), {}, "conv1x1: Cin must be in 1..224, got 225"),
        ((z(1, 0, 2, 2), wp, bh), {}, "conv1x1: Cin must be in 1..224, got 0"),
        ((x, wp, bh), {"cin": 225}, "conv1x1: Cin must be in 1..224, got 225"),
        ((x, wp, bh), {"cin": 98}, "x must be (N,98,H,W), got (2, 196, 2, 3)"),
        ((x, z(7, 8, 64, 7, dtype=H), bh), {}, "wpack must hold 28672 halves (pack_conv1), got (7, 8, 64, 7)"),
        ((x, wp, z(127, dtype=H)), {}, "bias_h must be (128,), got (127,)"),
        ((nc(x), wp, bh), {}, "x must be contiguous"),
        ((x, nc(wp), bh), {}, "wpack must be contiguous"),
        ((x, wp, nc(bh)), {}, "bias_h must be contiguous"),
        ((x.double(), wp, bh), {}, "expected scalar type Float or Half but found Double (x)"),
        ((x.bfloat16(), wp, bh), {}, "expected scalar type Float or Half but found BFloat16 (x)"),
        ((x, wp.float(), bh), {}, "expected scalar type Half but found Float (wpack)"),
        ((x, wp, bh.bfloat16()), {}, "expected scalar type Half but found BFloat16 (bias_h)"),
        ((x.clone().requires_grad_(), wp, bh), {}, no_grad),
        # two defects: the earlier check reports
        ((z(1, 225, 2, 2), z(5, dtype=H), bh), {}, "conv1x1: Cin must be in 1..224, got 225"),
        ((nc(x), z(5, dtype=H), bh), {}, "wpack must hold 28672 halves (pack_conv1), got (5,)"),
        ((x.double(), wp, nc(bh)), {}, "bias_h must be contiguous"),
        ((x.clone().requires_grad_(), wp, bh.float()), {}, "expected scalar type Half but found Float (bias_h)"),
        ((z(2, 196, 0, 3), wp, bh), {}, "x" + _NO_CPU),      # the empty frame is refused after the device
    ]
    for args, kw, message in table:
        with pytest.raises(RuntimeError) as info:
            M.conv1x1(*args, **kw)
        assert type(info.value) is RuntimeError and str(info.value) == message
    with torch.no_grad():      # grad mode off: the no-grad refusal does not apply, the device refusal is next
        with pytest.raises(RuntimeError) as info:
            M.conv1x1(x.clone().requires_grad_(), wp, bh)
        assert str(info.value) == "x" + _NO_CPU
    assert launched == []


# ---- GPU ------------------------------------------------------------------------------------------------------------
@pytest.fixture
def no_threshold(lgu, monkeypatch):
    """The wrapper's routing by size follows a measurement (MIN_FUSED_PIXELS); these tests are about the fused path."""
    monkeypatch.setattr(lgu.conv1, "MIN_FUSED_PIXELS", 0)
    monkeypatch.setattr(lgu.conv3, "MIN_FUSED_PIXELS", {64: 0, 128: 0})


def _need_gpu(lgu):
    assert torch.cuda.is_available(), "these tests need the MI355X"
    assert os.path.exists(lgu._lib.so_path()), "liblgu_corr.so missing — run __graft_entry__.build()"


def _packed(lgu, m):
    return lgu.conv1.pack_conv1(m.weight.detach().cuda(), m.bias.detach().cuda())


def _impulse_channels(cin):
    return [0, 7, 31, 32, cin // 2 + 3, cin - 1]


@pytest.mark.gpu
@pytest.mark.parametrize("cin", (196, 98))
def test_zero_input_and_impulses_are_bit_for_bit(lgu, cin):
    """Zero input: act(half(b_h)) everywhere.  One input element = v (each of six channels at each of three pixels of a 2x17
    image, v = 1 and v = -1.5): a single product is exact, so the pixel's outputs are act(half(b_h + v·w_h[:, c])) and every
    other pixel keeps act(half(b_h)).  The 36 frames are run as one batch (the groups of 32 pixels then fall anywhere
    across the 34-pixel frames) and each alone, where pixel (0,0) is the first of a group, (1,14) the last of one and
    (1,15) the first of the partial group."""
    _need_gpu(lgu)
    M = lgu.conv1
    m = R1.make_conv(43, cin)
    wpack, bias_h = _packed(lgu, m)
    bh = m.bias.detach().half()
    for relu in (False, True):
        for shape in SHAPES:
            x = torch.zeros((shape[0], cin) + shape[1:], device="cuda")
            want = R1.act(bh, relu).view(1, 128, 1, 1).expand(shape[0], 128, *shape[1:]).contiguous()
            assert same_bits(M.conv1x1(x, wpack, bias_h, relu=relu), want), shape
            assert same_bits(M.conv1x1(x.half(), wpack, bias_h, relu=relu), want), shape
    wh = m.weight.detach().half().view(128, cin)
    at = [(0, 0), (1, 14), (1, 15)]
    chans = _impulse_channels(cin)
    assert len(set(chans)) == 6 and {0, 31, 32, cin - 1} <= set(chans)
    x = torch.zeros((len(at) * len(chans) * 2, cin, 2, 17))
    want = {relu: R1.act(bh, relu).view(1, 128, 1, 1).expand(x.shape[0], 128, 2, 17).clone() for relu in (False, True)}
    n = 0
    for (y, xx) in at:
        for ch in chans:
            for v in (1.0, -1.5):
                x[n, ch, y, xx] = v
                for relu in (False, True):
                    want[relu][n, :, y, xx] = R1.single(bh, wh[:, ch].float() * v, relu)
                n += 1
    assert bool((want[True] != want[False]).any())
    xc = x.cuda()
    for relu in (False, True):
        got = M.conv1x1(xc, wpack, bias_h, relu=relu)
        got_h = M.conv1x1(xc.half(), wpack, bias_h, relu=relu)
        alone = torch.cat([M.conv1x1(xc[k:k + 1].contiguous(), wpack, bias_h, relu=relu) for k in range(x.shape[0])])
        torch.cuda.synchronize()
        assert same_bits(got, want[relu]), "max |diff| %g" % float((got.cpu().float() - want[relu].float()).abs().max())
        assert same_bits(got_h, want[relu]) and same_bits(alone, want[relu])


@pytest.mark.gpu
@pytest.mark.parametrize("shape,cin", CASES)
def test_every_element_is_within_the_derived_bound(lgu, shape, cin):
    """|y - act(s64)| <= allowance(s64, S, Cin + 2), relu on and off, for float32 and half input; prints where the library's
    own forward sits."""
    _need_gpu(lgu)
    m, x, s64, S = case(shape, cin)
    wpack, bias_h = _packed(lgu, m)
    bound = R.allowance(s64, S, R1.terms(cin))
    xc = x.cuda()
    mc = R1.make_conv(50 + cin, cin).cuda()
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        own = mc(xc)
    for relu in (False, True):
        ref = R.act(s64, relu)
        got = lgu.conv1.conv1x1(xc, wpack, bias_h, relu=relu)
        from_half = lgu.conv1.conv1x1(xc.half(), wpack, bias_h, relu=relu)
        rounded = lgu.conv1.conv1x1(xc.half().float(), wpack, bias_h, cin=cin, relu=relu)
        torch.cuda.synchronize()
        own_r = torch.relu(own) if relu else own
        err = (got.cpu().double() - ref).abs()
        err_own = (own_r.cpu().double() - ref).abs()
        print("conv1x1 %s Cin %d relu=%s: worst error %.3g of its bound; the module's own forward: worst %.3g of the bound, "
              "%.4f bit-identical to the kernel" % (shape, cin, relu, float((err / bound).max()), float((err_own / bound).max()),
                                                    float((own_r == got).double().mean())))
        assert got.dtype == torch.float16 == own.dtype and tuple(got.shape) == (shape[0], 128) + shape[1:] == tuple(own.shape)
        assert bool((err <= bound).all()), float((err / bound).max())
        assert same_bits(from_half, rounded) and same_bits(from_half, got)      # fp32 x is rounded to half exactly once
        if relu:
            assert bool((got >= 0).all())


@pytest.mark.gpu
@pytest.mark.parametrize("shape,cin,ats", [((2, 3, 17), 196, [(0, 5, 1, 14), (0, 195, 1, 15), (1, 64, 2, 16), (1, 0, 0, 0)]),
                                           ((2, 3, 17), 98, [(0, 97, 1, 14), (1, 31, 0, 13)]),
                                           ((1, 6, 80), 196, [(0, 9, 0, 31), (0, 195, 0, 32), (0, 33, 5, 79)])])
def test_nan_reaches_exactly_its_pixel(lgu, shape, cin, ats):
    """The pixel's 128 outputs, with and without the ReLU; every other element keeps its bits.  The places include the last
    channel and the pixels on either side of a group boundary (global pixel 31 and 32)."""
    _need_gpu(lgu)
    m, x, _, _ = case(shape, cin)
    wpack, bias_h = _packed(lgu, m)
    hw = shape[1] * shape[2]
    assert any(c == cin - 1 for _, c, _, _ in ats)
    assert {(n * hw + y * shape[2] + xx) % GROUP for n, _, y, xx in ats} & {0, GROUP - 1}
    for relu in (False, True):
        clean = lgu.conv1.conv1x1(x.cuda(), wpack, bias_h, relu=relu).cpu()
        assert not bool(torch.isnan(clean).any())
        for at in ats:
            xn = x.clone()
            xn[at] = float("nan")
            n, _, cy, cx = at
            for xin in (xn.cuda(), xn.cuda().half()):
                got = lgu.conv1.conv1x1(xin, wpack, bias_h, relu=relu).cpu()
                want = torch.zeros((shape[0], 1) + shape[1:], dtype=torch.bool)
                want[n, 0, cy, cx] = True
                want = want.expand_as(got)
                assert bool((torch.isnan(got) == want).all()), (at, relu)
                assert bool((got.view(torch.int16) == clean.view(torch.int16))[~want].all()), (at, relu)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(1, 3, 17), (1, 6, 80), (1, 1, 1)])
def test_garbage_behind_the_padded_channels_cannot_leak(lgu, shape):
    """Cin = 98: the kernel's K runs to 224.  x is the head of a buffer whose storage behind the tensor holds NaN (where
    channels 98.. of the one frame would lie), and a `shifted` carve, whose surroundings are poisoned: the bits of the
    clean call, and the guard bands intact."""
    from tests.alignment_cases import guards_intact, shifted
    _need_gpu(lgu)
    cin = 98
    m = R1.make_conv(50 + cin, cin)
    x = R.make_input(77, *shape, C=cin).cuda()
    wpack, bias_h = _packed(lgu, m)
    for xin in (x, x.half()):
        clean = lgu.conv1.conv1x1(xin, wpack, bias_h, relu=True)
        assert not bool(torch.isnan(clean).any())
        buf = torch.full((xin.numel() + (224 - cin + 8) * shape[1] * shape[2] + 64,), float("nan"), dtype=xin.dtype, device="cuda")
        head = buf[:xin.numel()].view(xin.shape)
        head.copy_(xin)
        assert same_bits(lgu.conv1.conv1x1(head, wpack, bias_h, relu=True), clean)
        assert bool(torch.isnan(buf[xin.numel():]).all())
        carve = shifted(xin, 0)
        assert same_bits(lgu.conv1.conv1x1(carve, wpack, bias_h, relu=True), clean) and guards_intact(carve)


@pytest.mark.gpu
@pytest.mark.parametrize("shape,cin", [((2, 3, 17), 196), ((3, 5, 7), 98), ((3, 2, 6), 196), (BIG, 196)])
def test_a_frame_does_not_depend_on_its_batch(lgu, shape, cin):
    """A frame alone, and the batch reversed, give the frame's bits."""
    _need_gpu(lgu)
    M = lgu.conv1
    m, x, _, _ = case(shape, cin)
    wpack, bias_h = _packed(lgu, m)
    xc = x.cuda()
    got = M.conv1x1(xc, wpack, bias_h, relu=True)
    back = torch.flip(xc, dims=(0,)).contiguous()
    assert same_bits(torch.flip(M.conv1x1(back, wpack, bias_h, relu=True), dims=(0,)), got)
    for k in range(shape[0]):
        assert same_bits(got[k:k + 1], M.conv1x1(xc[k:k + 1].contiguous(), wpack, bias_h, relu=True)), k


def _c_entry(lgu, x, wpack, bias_h, out, flags=0, n=None, cin=None):
    N, C, H, W = x.shape
    flags |= lgu.conv1.X_HALF if x.dtype == torch.float16 else 0
    args = lgu._lib.Conv1Args(x.data_ptr(), wpack.data_ptr(), bias_h.data_ptr(), out.data_ptr(), N if n is None else n,
                              C if cin is None else cin, H, W, flags)
    rc = getattr(lgu._lib.load(), ENTRY)(args, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc


@pytest.mark.gpu
@pytest.mark.parametrize("half_x", (False, True))
@pytest.mark.parametrize("shape", [(2, 3, 17), (1, 6, 80)])
def test_guard_bands_and_alignment(lgu, shape, half_x):
    """x, bias and out are served at element alignment with the aligned call's bits and no write outside out (at (1,6,80) the
    aligned call stores 8 bytes at a time and the shifted ones by element); a wpack that is not 16-byte aligned and a Cin
    outside 1..224 are refused with nothing written; N = 0 launches nothing."""
    from tests.alignment_cases import guards_intact, shifted
    _need_gpu(lgu)
    M, L = lgu.conv1, lgu._lib
    cin = 196
    m, x, _, _ = case(shape, cin)
    wpack, bias_h = _packed(lgu, m)
    xc = x.cuda().half() if half_x else x.cuda()
    want = M.conv1x1(xc, wpack, bias_h, relu=True)
    base = {"x": xc, "wpack": wpack, "bias": bias_h, "out": torch.empty_like(want)}
    xs = (2, 4, 8) if half_x else (4, 8)
    variants = [(k, s) for k, ss in (("x", xs), ("bias", (2, 4, 8)), ("out", (2, 4, 8)), ("wpack", (2, 4, 8))) for s in ss]
    for key, shift in variants + [("all but wpack", 0)]:
        keys = [key] if key in base else [k for k in base if k != "wpack"]
        args = dict(base)
        for k in keys:
            args[k] = shifted(base[k], shift if key in base else base[k].element_size())
        if "out" not in keys:
            args["out"] = shifted(base["out"], 0)      # always carved from a poisoned buffer
        before = {k: args[k].clone() for k in args}
        rc = _c_entry(lgu, args["x"], args["wpack"], args["bias"], args["out"], flags=M.RELU)
        if "wpack" in keys:
            assert rc == L.LGU_E_UNSUPPORTED, (key, shift, rc)
            assert same_bits(args["out"], before["out"]), "refused, but out changed"
        else:
            assert rc == 0, (key, shift, rc)
            assert same_bits(args["out"], want), "%s shifted by %d: differs from the aligned call" % (key, shift)
        for k in ("x", "wpack", "bias"):
            assert same_bits(args[k], before[k]), "read-only operand %s changed" % k
        for k in set(keys) | {"out"}:
            assert guards_intact(args[k]), "%s, %d: a guard band of %s was written" % (key, shift, k)
    with pytest.raises(L.UnsupportedShape):
        M.conv1x1(xc, shifted(wpack, 8), bias_h)
    # refusals and the empty case of the C entry: nothing written
    out = shifted(base["out"], 0)
    out.fill_(0.25)
    assert _c_entry(lgu, xc, wpack, bias_h, out, cin=0) == L.LGU_E_UNSUPPORTED
    assert _c_entry(lgu, xc, wpack, bias_h, out, cin=225) == L.LGU_E_UNSUPPORTED
    assert _c_entry(lgu, xc, wpack, bias_h, out, flags=4) == L.LGU_E_BADARG
    assert _c_entry(lgu, xc, wpack, bias_h, out, n=-1) == L.LGU_E_BADARG
    assert _c_entry(lgu, xc, wpack, bias_h, out, n=0) == 0
    assert bool((out == 0.25).all()) and guards_intact(out)
    assert tuple(M.conv1x1(xc[:0], wpack, bias_h).shape) == (0, 128) + shape[1:]
    with pytest.raises(RuntimeError, match="empty frame"):
        M.conv1x1(xc[:, :, :0], wpack, bias_h)


def _like(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and bool(((a.double() - b.double()).abs() <= 2.0 ** -6 * (1 + b.double().abs())).all())


def _spy(monkeypatch, module):
    """The list of what the class's own forward returns for `module`, call by call."""
    cls, seen = type(module), []
    orig = cls.forward

    def forward(self, *args, **kwargs):
        out = orig(self, *args, **kwargs)
        if self is module:
            seen.append(out)
        return out
    monkeypatch.setattr(cls, "forward", forward)
    return seen


@pytest.mark.gpu
def test_conv1_wrapper_under_autocast(lgu, no_threshold, monkeypatch):
    """Under float16 autocast Conv1(conv)(x) is one fused call with the bits of conv1x1; fp32 mode, a bfloat16 autocast,
    grad and a raised MIN_FUSED_PIXELS return what the module's own forward returns (the very tensor; its values are
    compared with a twin of the same weights to the precision of the coarsest mode, bfloat16) and the counter stays."""
    _need_gpu(lgu)
    M = lgu.conv1
    shape, cin = (2, 3, 17), 196
    _, x, s64, S = case(shape, cin)
    bound = R.allowance(s64, S, R1.terms(cin))
    mc = R1.make_conv(50 + cin, cin).cuda()
    wrapped = R1.make_conv(50 + cin, cin).cuda()
    xc = x.cuda()
    wr = M.Conv1(wrapped)
    seen = _spy(monkeypatch, wrapped)
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        own = mc(xc.clone())
        got = wr(xc)
        assert wr.fused_calls == 1
        assert same_bits(wr(xc.half()), got) and wr.fused_calls == 2      # a half input is used as it is
        assert same_bits(got, M.conv1x1(xc, *wr.packed()))
        with_relu = M.Conv1(wrapped, relu=True)
        assert same_bits(with_relu(xc), M.conv1x1(xc, *wr.packed(), relu=True)) and with_relu.fused_calls == 1
    assert seen == []
    with torch.no_grad():
        y = wr(xc)
        assert y is seen[-1] and _like(y, mc(xc))
        with torch.autocast("cuda", dtype=torch.bfloat16):
            y = wr(xc)
            assert y is seen[-1] and _like(y, mc(xc))
    with torch.autocast("cuda", dtype=torch.float16):
        grad = wr(xc.clone().requires_grad_())
        assert grad is seen[-1] and grad.requires_grad and _like(grad, mc(xc))
    assert wr.fused_calls == 2 and len(seen) == 3
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        assert M.install(wrapped) is wrapped.forward and wrapped.forward is not wr
        installed = wrapped(xc)
        assert wrapped.forward.fused_calls == 1
        M.uninstall(wrapped)
        monkeypatch.setattr(M, "MIN_FUSED_PIXELS", 1 << 40)      # below the threshold: the module
        y = wr(xc)
        assert y is seen[-1] and len(seen) == 4 and _like(y, own) and wr.fused_calls == 2
        yr = with_relu(xc)
        assert len(seen) == 5 and _like(yr, torch.relu(own)) and with_relu.fused_calls == 1
    torch.cuda.synchronize()
    assert got.dtype == own.dtype == torch.float16 and got.shape == own.shape == (2, 128, 3, 17)
    assert same_bits(installed, got)
    err = (got.cpu().double() - s64).abs()
    assert bool((err <= bound).all()), float((err / bound).max())


@pytest.mark.gpu
@pytest.mark.parametrize("first", ("conv1", "conv3"))
def test_installed_inside_a_stack_on_corr_encoder(lgu, no_threshold, first):
    """conv1.install on corr_encoder[0] under a Conv3Stack on corr_encoder, in either install order: the stack calls the
    layer as itself, one fused launch each, and the output is within conv3_restatement.stack's bound."""
    _need_gpu(lgu)
    seq = R.make_stack(7, "corr_encoder")
    x = R.make_input(9, 2, 5, 9, C=R.COR_PLANES)
    with torch.no_grad():
        ref, bound = R.stack(x, seq)
    sc = R.make_stack(7, "corr_encoder").cuda()
    if first == "conv1":
        w1, w3 = lgu.conv1.install(sc[0]), lgu.conv3.install(sc)
    else:
        w3, w1 = lgu.conv3.install(sc), lgu.conv1.install(sc[0])
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        got = sc(x.cuda())
    torch.cuda.synchronize()
    assert w3.fused_calls == 1 and w1.fused_calls == 1 and got.dtype == torch.float16
    err = (got.cpu().double() - ref).abs()
    print("corr_encoder through Conv3Stack + Conv1: worst error %.3g of the bound" % float((err / bound).max()))
    assert bool((err <= bound).all()), float((err / bound).max())
    lgu.conv3.uninstall(sc)
    lgu.conv1.uninstall(sc[0])
