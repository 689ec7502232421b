"""The KAN-bias GRU's fused 448-channel 3x3 convolutions (lgu_slam_amd.gru: pack_gruconv, gru_conv3x3, gru_conv_zr,
gru_conv_q, KanBiasGRU(convs=True); csrc/gruconv.hip) against the float64 restatement of their rounding model,
tests/gruconv_restatement.py.

Numerics contract (include/lgu_corr.h):
- a single product is exact: impulses and the zero input are bit for bit;
- every PLAIN element: |y - s64| <= 4034·2^-24·S + 2^-11·(|s64| + 4034·2^-24·S) + 2^-25 with S = Σ|x·w_h| + |b_h|;
- ZR and Q are bit for bit `kangru_gates_` and `kangru_blend` applied to the PLAIN output (those two kernels are pinned
  to the torch ops by tests/test_kangru.py::test_gates_and_blend_are_bit_identical_to_the_torch_ops);
- the segment split, the batch and the alignment of the operands do not change a bit; NaN reaches exactly its 3x3
  neighbourhood;
- the whole forward with convs=True is bit for bit the composition of the PLAIN calls with the kangru_* operators, and
  within the propagated bound of the float64 chain (gruconv_restatement.forward).
The GPU tests build their modules themselves and never read the reference tree.
"""
import ctypes
import os

import pytest

torch = pytest.importorskip("torch")

from tests import gruconv_restatement as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = "lgu_gruconv3x3_c448_h16"
COUTS = (128, 256)
# the issue's shapes.  The kernel's tiles are 64 x 4 or 32 x 8 pixels for Cout 128 and 64 x 2 or 32 x 4 for Cout 256, the
# one that pads the image less (ties: the wider).  1 x 17 x 130 straddles 64 x 4 and 64 x 2 in both directions, 1 x 5 x 65
# straddles 64 x 2; 1 x 13 x 65 is added because it selects 32 x 8 and 32 x 4 and straddles both in both directions
SHAPES = [(1, 1, 1), (1, 2, 3), (2, 9, 33), (1, 5, 65), (3, 16, 40), (1, 17, 130), (1, 13, 65)]
BITS_ONLY = [(1, 60, 80)]
FORWARD_SHAPES = [(3, 7, 13), (1, 12, 16), (2, 9, 33)]
_CASES = {}
_NO_CPU = " must be a HIP device tensor: lgu_slam_amd has no CPU fallback"
H16 = torch.float16


def same_bits(a, b):
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    iv = torch.int16 if a.dtype == torch.float16 else torch.int32
    return bool(torch.equal(a.view(iv), b.view(iv)))


def module():
    if "m" not in _CASES:
        _CASES["m"] = R.make_module(1061)
    return _CASES["m"]


def inputs(shape):
    """The half inputs (net, inp, corr, flow) and their concatenation x for one shape, made once and never changed."""
    if ("x", shape) not in _CASES:
        ins = R.make_inputs(2000 + shape[1] * shape[2], *shape)
        _CASES[("x", shape)] = (ins, torch.cat(ins, 1))
    return _CASES[("x", shape)]


def case(shape):
    """(x, s64, S) on the CPU: the sums of convz | convr | convq (384 outputs) on x, computed once and never changed."""
    if ("s", shape) not in _CASES:
        m = module()
        x = inputs(shape)[1]
        with torch.no_grad():
            _CASES[("s", shape)] = (x,) + R.conv(x, *R.stacked((m.convz, m.convr, m.convq)))
    return _CASES[("s", shape)]


def sums(shape, cout):
    """(x, s64, S) of the pack of `cout` outputs: 256 = (convz, convr), 128 = convq."""
    x, s, S = case(shape)
    sl = slice(0, 256) if cout == 256 else slice(256, 384)
    return x, s[:, sl], S[:, sl]


def convs_of(m, cout):
    return (m.convz, m.convr) if cout == 256 else m.convq


def gates_k(shape, seed=5):
    """kz, kr, kq (E,128) half with large and negative entries: sigmoid and tanh reach both of their flat ends."""
    g = torch.Generator().manual_seed(seed + shape[1])
    k = torch.randn((3, shape[0], 128), generator=g) * 2.0
    k[:, :, 0::17] = 30.0
    k[:, :, 5::17] = -30.0
    k[:, :, 9::17] = -0.0
    return k.half()


# ---- CPU ------------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_entry(lgu):
    from tests.test_abi import declared_symbols
    lib = ctypes.CDLL(lgu._lib._build.SO_PATH)
    assert ENTRY in declared_symbols() and hasattr(lib, ENTRY)
    sig = lgu._lib.SIGNATURES[ENTRY]
    assert sig[0] is lgu._lib.GruConvArgs and issubclass(sig[0], ctypes.Structure) and sig[1] is ctypes.c_void_p
    assert [f[0] for f in sig[0]._fields_] == ["seg", "wpack", "bias", "k0", "k1", "net", "z", "out0", "out1", "seg_ch", "nseg",
                                               "N", "H", "W", "Cout", "mode", "flags"]
    assert ctypes.sizeof(sig[0]) == 12 * 8 + 11 * 4 + 4
    assert "gruconv.hip" in lgu._build.SOURCES
    G = lgu.gru
    text = open(os.path.join(ROOT, "include", "lgu_corr.h")).read()
    for cout in COUTS:
        assert G.GRUCONV_WPACK_HALVES[cout] == 126 * (cout // 16) * 64 * 8
        assert "#define LGU_GRUCONV_WPACK_HALVES_%d %d\n" % (cout, G.GRUCONV_WPACK_HALVES[cout]) in text
    for name, value in (("PLAIN", G.PLAIN), ("ZR", G.ZR), ("Q", G.Q), ("STEPS", G.GRUCONV_STEPS), ("CIN", G.CIN),
                        ("MAX_SEGMENTS", G.MAX_SEGMENTS)):
        assert "#define LGU_GRUCONV_%s %d" % (name, value) in text
    assert lgu.gru_conv_zr is G.gru_conv_zr and lgu.gru_conv_q is G.gru_conv_q and lgu.gru_conv3x3 is G.gru_conv3x3
    assert lgu.pack_gruconv is G.pack_gruconv and isinstance(G.MIN_FUSED_CONV_PIXELS, int) and G.MIN_FUSED_CONV_PIXELS >= 0
    # kangru.hip and gruconv.hip share one definition of the gates' scalar arithmetic
    csrc = os.path.join(ROOT, "lgu-slam_amd", "csrc")
    for name in ("kangru.hip", "gruconv.hip"):
        src = open(os.path.join(csrc, name)).read()
        assert '#include "kangru_math.hpp"' in src and "float kg_sigmoid(" not in src
    assert "float kg_sigmoid(" in open(os.path.join(csrc, "kangru_math.hpp")).read()


@pytest.mark.parametrize("cout", COUTS)
def test_pack_puts_every_weight_in_its_documented_slot_and_nothing_else(lgu, cout):
    g = torch.Generator().manual_seed(5)
    convs = [torch.nn.Conv2d(448, 128, 3, padding=1) for _ in range(cout // 128)]
    with torch.no_grad():
        for m in convs:
            m.weight.copy_(torch.randn((128, 448, 3, 3), generator=g))
            m.bias.copy_(torch.randn((128,), generator=g))
    w, b = R.stacked(convs)
    wpack, bias_h = lgu.gru.pack_gruconv(convs[0] if cout == 128 else convs)
    assert wpack.dtype == H16 and wpack.is_contiguous() and wpack.numel() == lgu.gru.GRUCONV_WPACK_HALVES[cout]
    assert tuple(wpack.shape) == (126, cout // 16, 64, 8) and same_bits(bias_h, b.half())
    co, c, ky, kx = R.slot_source(cout)
    idx = torch.arange(cout * 448 * 9, dtype=torch.int32).view(cout, 448, 3, 3)
    assert sorted(idx[co, c, ky, kx].flatten().tolist()) == list(range(cout * 448 * 9))   # every weight once, nothing else
    assert same_bits(wpack, w.half()[co, c, ky, kx])
    with pytest.raises(RuntimeError, match="must be Conv2d\\(448, 128, 3, padding=1\\)"):
        lgu.gru.pack_gruconv(torch.nn.Conv2d(128, 128, 3, padding=1))
    with pytest.raises(RuntimeError, match="must be Conv2d\\(448, 128, 3, padding=1\\)"):
        lgu.gru.pack_gruconv([convs[0], torch.nn.Conv2d(448, 128, 3, padding=1, bias=False)])
    with pytest.raises(RuntimeError, match="one convolution or the pair"):
        lgu.gru.pack_gruconv([convs[0]] * 3)


@pytest.mark.parametrize("shape", [(1, 1, 1), (1, 2, 3), (2, 9, 33)])
def test_restatement_equals_float64_conv2d_on_the_rounded_operands(shape):
    m = module()
    x, s64, S = case(shape)
    w, b = R.stacked((m.convz, m.convr, m.convq))
    F = torch.nn.functional
    xh, wh, bh = R.h64(x), R.h64(w), R.h64(b)
    s = F.conv2d(xh, wh, bh, padding=1)
    Sc = F.conv2d(xh.abs(), wh.abs(), bh.abs(), padding=1)
    # the operands are half values, so every product is exact in float64; the two sums differ in order only
    assert bool(((s - s64).abs() <= 2.0 ** -42 * S).all()) and bool(((Sc - S).abs() <= 2.0 ** -42 * S).all())
    assert bool((S >= s64.abs()).all()) and bool((R.allowance(s64, S) > 0).all())
    assert R.TERMS == 448 * 9 + 2 == 4034 and x.dtype == H16 and tuple(x.shape) == (shape[0], 448) + shape[1:]
    assert [sum(c) for c in R.SPLITS] == [448] * 3


def test_operator_refusals_in_their_order(lgu):
    """Shapes, pack size, bias shape, contiguity, dtypes, no-grad, device: each refusal's text, and which of two defects
    is reported.  None of them touches a device."""
    G = lgu.gru

    def z(*shape, dtype=H16):
        return torch.zeros(shape, dtype=dtype)

    def nc(t):
        return torch.zeros(tuple(t.shape) + (2,), dtype=t.dtype)[..., 0]

    segs = [z(2, 128, 3, 4), z(2, 320, 3, 4)]
    wp, bh = {c: z(126, c // 16, 64, 8) for c in COUTS}, {c: z(c) for c in COUTS}
    k, fm = z(2, 128), z(2, 128, 3, 4)
    no_grad = " has no autograd: its outputs would carry no gradient. Call it under torch.no_grad() or pass detached inputs"
    calls = {
        "gru_conv3x3": lambda s=segs, w=wp[128], b=bh[128], **kw: G.gru_conv3x3(s, w, b),
        "gru_conv_zr": lambda s=segs, w=wp[256], b=bh[256], kz=k, kr=k, net=fm, **kw: G.gru_conv_zr(s, w, b, kz, kr, net),
        "gru_conv_q": lambda s=segs, w=wp[128], b=bh[128], kq=k, z=fm, net=fm, **kw: G.gru_conv_q(s, w, b, kq, z, net),
    }
    for what, f in calls.items():
        cases = [
            (dict(), "segments[0]" + _NO_CPU),
            (dict(s=[]), "%s: 1 to 4 segments, got 0" % what),
            (dict(s=[z(2, 64, 3, 4)] * 5), "%s: 1 to 4 segments, got 5" % what),
            (dict(s=[z(128, 3, 4)]), "segments[0] must be (E,ch,H,W), got (128, 3, 4)"),
            (dict(s=[segs[0], z(2, 320, 3, 5)]), "segments[1] must be (2,ch,3,4) with ch a multiple of 32, got (2, 320, 3, 5)"),
            (dict(s=[z(2, 120, 3, 4), z(2, 328, 3, 4)]), "segments[0] must be (2,ch,3,4) with ch a multiple of 32, got (2, 120, 3, 4)"),
            (dict(s=[segs[0], z(2, 288, 3, 4)]), "%s: the segments' channels must sum to 448, got [128, 288]" % what),
            (dict(w=z(5)), "wpack must hold %s halves (pack_gruconv), got (5,)"
             % {"gru_conv3x3": "516096 or 1032192", "gru_conv_zr": "1032192", "gru_conv_q": "516096"}[what]),
            (dict(b=z(64)), "bias_h must be (%d,), got (64,)" % (256 if what == "gru_conv_zr" else 128)),
            (dict(s=[nc(segs[0]), segs[1]]), "segments[0] must be contiguous"),
            (dict(w=nc(wp[256 if what == "gru_conv_zr" else 128])), "wpack must be contiguous"),
            (dict(s=[segs[0], segs[1].float()]), "expected scalar type Half but found Float (segments[1])"),
            (dict(b=bh[256 if what == "gru_conv_zr" else 128].bfloat16()), "expected scalar type Half but found BFloat16 (bias_h)"),
            (dict(s=[segs[0].clone().requires_grad_(), segs[1]]), what + no_grad),
            # two defects: the earlier check reports
            (dict(s=[segs[0], z(2, 288, 3, 4)], w=z(5)), "%s: the segments' channels must sum to 448, got [128, 288]" % what),
            (dict(s=[nc(segs[0]), segs[1]], b=z(64)), "bias_h must be (%d,), got (64,)" % (256 if what == "gru_conv_zr" else 128)),
            (dict(s=[segs[0].float(), nc(segs[1])]), "segments[1] must be contiguous"),
            (dict(s=[segs[0].float().requires_grad_(), segs[1]]), "expected scalar type Half but found Float (segments[0])"),
        ]
        if what == "gru_conv_zr":
            cases += [(dict(kr=z(2, 64)), "kr must be (2, 128), got (2, 64)"),
                      (dict(net=z(2, 128, 3, 5), w=z(5)), "net must be (2, 128, 3, 4), got (2, 128, 3, 5)"),
                      (dict(kz=nc(k)), "kz must be contiguous"), (dict(net=fm.float()), "expected scalar type Half but found Float (net)"),
                      (dict(w=wp[128]), "wpack must hold 1032192 halves (pack_gruconv), got (126, 8, 64, 8)")]
        if what == "gru_conv_q":
            cases += [(dict(kq=z(3, 128)), "kq must be (2, 128), got (3, 128)"), (dict(z=z(2, 128, 4, 4)), "z must be (2, 128, 3, 4), got (2, 128, 4, 4)"),
                      (dict(z=nc(fm)), "z must be contiguous"), (dict(net=fm.double()), "expected scalar type Half but found Double (net)"),
                      (dict(w=wp[256]), "wpack must hold 516096 halves (pack_gruconv), got (126, 16, 64, 8)")]
        for kw, message in cases:
            with pytest.raises(RuntimeError) as info:
                f(**kw)
            assert type(info.value) is RuntimeError and str(info.value) == message, (what, kw.keys())
        with torch.no_grad():      # grad mode off: the no-grad refusal does not apply, the device refusal is next
            with pytest.raises(RuntimeError) as info:
                f(s=[segs[0].clone().requires_grad_(), segs[1]])
            assert str(info.value) == "segments[0]" + _NO_CPU


def test_cpu_inputs_reach_the_module_and_install_keeps_the_state_dict(lgu):
    G = lgu.gru
    m = R.make_module(1062)
    keys, nparams = list(m.state_dict().keys()), len(list(m.parameters()))
    ins = [t.float() for t in R.make_inputs(7, 2, 4, 5)]
    with torch.no_grad():
        want = m(*ins)
        direct = G.KanBiasGRU(m, convs=True)
        assert direct.convs is True and G.KanBiasGRU(m).convs is False
        assert same_bits(direct(*ins), want) and direct.fused_calls == 0 and direct.fused_conv_calls == 0
        wr = G.install(m, convs=True)
        assert isinstance(wr, G.KanBiasGRU) and m.forward is wr and wr.convs is True
        assert list(m.state_dict().keys()) == keys and len(list(m.parameters())) == nparams
        assert same_bits(m(*ins), want) and wr.fused_conv_calls == 0
        assert G.install(m, convs=False) is wr and wr.convs is False        # a second install sets it on the wrapper
        assert G.install(m, convs=True) is wr and wr.convs is True
        assert G.install(m) is wr and wr.convs is False                     # the default stays False
    assert m(*[t.clone().requires_grad_() for t in ins]).requires_grad
    G.uninstall(m)
    assert "forward" not in m.__dict__ and list(m.state_dict().keys()) == keys


# ---- GPU ------------------------------------------------------------------------------------------------------------
def _need_gpu(lgu):
    assert torch.cuda.is_available(), "these tests need the MI355X"
    assert os.path.exists(lgu._lib.so_path()), "liblgu_corr.so missing — run __graft_entry__.build()"


def _packed(lgu, cout):
    """(wpack, bias_h) on the device of the module's (convz, convr) or convq, packed once."""
    key = ("pack", cout)
    if key not in _CASES:
        w, b = R.stacked(convs_of(module(), cout))
        convs = [torch.nn.Conv2d(448, 128, 3, padding=1) for _ in range(cout // 128)]
        with torch.no_grad():
            for i, c in enumerate(convs):
                c.weight.copy_(w[128 * i:128 * (i + 1)])
                c.bias.copy_(b[128 * i:128 * (i + 1)])
        _CASES[key] = lgu.gru.pack_gruconv([c.cuda() for c in convs] if cout == 256 else convs[0].cuda())
    return _CASES[key]


def _segs(x, chans=(128, 128, 128, 64)):
    return [t.cuda() for t in R.split(x, list(chans))]


IMPULSE_AT = [(2, 2), (0, 0), (0, 4), (4, 0), (4, 4)]
IMPULSE_SPLIT = [128, 128, 128, 64]


@pytest.mark.gpu
@pytest.mark.parametrize("cout", COUTS)
def test_impulses_give_the_weights_bit_for_bit(lgu, cout):
    """One input element = 1 (the first and the last channel of every 32-block of every segment; the centre and the four
    corners of a 5x5 image in turn), bias 0: a single product is exact, so every output is w_h[co, c, cy-y+1, cx-x+1] and
    0 outside the window.  A zero input with the bias gives b_h everywhere."""
    _need_gpu(lgu)
    w, b = R.stacked(convs_of(module(), cout))
    wh = w.half()
    convs = [torch.nn.Conv2d(448, 128, 3, padding=1) for _ in range(cout // 128)]
    with torch.no_grad():
        for i, c in enumerate(convs):
            c.weight.copy_(w[128 * i:128 * (i + 1)])
            c.bias.zero_()
    wpack, zero_bias = lgu.gru.pack_gruconv([c.cuda() for c in convs] if cout == 256 else convs[0].cuda())
    chans = [c for blk in range(14) for c in (32 * blk, 32 * blk + 31)]
    x = torch.zeros((len(chans), 448, 5, 5), dtype=H16)
    want = torch.zeros((len(chans), cout, 5, 5), dtype=H16)
    for n, c in enumerate(chans):
        cy, cx = IMPULSE_AT[n % len(IMPULSE_AT)]
        x[n, c, cy, cx] = 1.0
        for ky in range(3):
            for kx in range(3):
                y, xx = cy - ky + 1, cx - kx + 1
                if 0 <= y < 5 and 0 <= xx < 5:
                    want[n, :, y, xx] = wh[:, c, ky, kx]
    got = lgu.gru.gru_conv3x3(_segs(x, IMPULSE_SPLIT), wpack, zero_bias)
    torch.cuda.synchronize()
    assert int((want != 0).sum()) > 0.9 * len(chans) * 4 * cout
    assert same_bits(got, want), "max |diff| %g" % float((got.cpu().float() - want.float()).abs().max())
    _, bias_h = _packed(lgu, cout)
    for shape in SHAPES:
        zero = torch.zeros((shape[0], 448) + shape[1:], dtype=H16, device="cuda")
        got = lgu.gru.gru_conv3x3([zero], wpack, bias_h)
        assert same_bits(got, b.half().view(1, cout, 1, 1).expand(shape[0], cout, *shape[1:])), shape


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("cout", COUTS)
def test_every_element_is_within_the_derived_bound(lgu, cout, shape):
    _need_gpu(lgu)
    x, s64, S = sums(shape, cout)
    wpack, bias_h = _packed(lgu, cout)
    bound = R.allowance(s64, S)
    got = lgu.gru.gru_conv3x3(_segs(x), wpack, bias_h)
    w, b = R.stacked(convs_of(module(), cout))
    with torch.no_grad(), torch.autocast("cuda", dtype=H16):
        own = torch.nn.functional.conv2d(x.cuda(), w.cuda(), b.cuda(), padding=1)
    torch.cuda.synchronize()
    err = (got.cpu().double() - s64).abs()
    err_own = (own.cpu().double() - s64).abs()
    print("gru_conv3x3 Cout %d %s: worst error %.3g of its bound, %.4f of the elements are the restatement's bits; the "
          "library's autocast convolution: worst %.3g of the bound, %.4f bit-identical to the kernel"
          % (cout, shape, float((err / bound).max()), float((got.cpu() == s64.to(H16)).double().mean()),
             float((err_own / bound).max()), float((own == got).double().mean())))
    assert got.dtype == H16 and tuple(got.shape) == (shape[0], cout) + shape[1:]
    assert bool((err <= bound).all()), float((err / bound).max())


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES + BITS_ONLY)
def test_gate_modes_are_the_gates_and_the_blend_of_the_plain_output(lgu, shape):
    """gru_conv_zr = kangru_gates_ on the PLAIN-256 output and gru_conv_q = kangru_blend on the PLAIN-128 output, bit for
    bit, with k that drives sigmoid and tanh into both flat ends; one segment, [128,320] and [128,128,128,64] give the
    same bits in every mode."""
    _need_gpu(lgu)
    G = lgu.gru
    (net, _, _, _), x = inputs(shape)
    netc, xc = net.cuda(), x.cuda()
    kz, kr, kq = (t.cuda().contiguous() for t in gates_k(shape))
    wzr, bzr = _packed(lgu, 256)
    wq, bq = _packed(lgu, 128)
    c256, c128 = G.gru_conv3x3([xc], wzr, bzr), G.gru_conv3x3([xc], wq, bq)
    net_inp = xc.clone()
    z_want = G.kangru_gates_(net_inp, c256[:, :128].contiguous(), c256[:, 128:].contiguous(), kz, kr, netc)
    rnet_want = net_inp[:, :128].contiguous()
    out_want = G.kangru_blend(c128, kq, z_want, netc)
    for chans in R.SPLITS:
        segs = _segs(x, chans)
        z, rnet = G.gru_conv_zr(segs, wzr, bzr, kz, kr, netc)
        out = G.gru_conv_q(segs, wq, bq, kq, z_want, netc)
        torch.cuda.synchronize()
        assert same_bits(z, z_want) and same_bits(rnet, rnet_want), chans
        assert same_bits(out, out_want), chans
        assert same_bits(G.gru_conv3x3(segs, wzr, bzr), c256) and same_bits(G.gru_conv3x3(segs, wq, bq), c128), chans
        assert all(same_bits(s, t) for s, t in zip(segs, R.split(x, list(chans))))
    zc = z_want.cpu().float()
    assert float(zc.max()) == 1.0 and float(zc.min()) == 0.0 and not bool(torch.isnan(out_want).any())


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(3, 16, 40), (3, 9, 33), (2, 13, 65)])
def test_an_image_does_not_depend_on_its_batch(lgu, shape):
    _need_gpu(lgu)
    G = lgu.gru
    ins = R.make_inputs(77, *shape)
    x = torch.cat(ins, 1).cuda()
    net = ins[0].cuda()
    kz, kr, kq = (t.cuda().contiguous() for t in gates_k(shape, 9))
    wzr, bzr = _packed(lgu, 256)
    wq, bq = _packed(lgu, 128)
    z, rnet = G.gru_conv_zr([x], wzr, bzr, kz, kr, net)
    out = G.gru_conv_q([x], wq, bq, kq, z, net)
    c = G.gru_conv3x3([x], wzr, bzr)
    for i in range(shape[0]):
        one = slice(i, i + 1)
        zi, ri = G.gru_conv_zr([x[one].contiguous()], wzr, bzr, kz[one].contiguous(), kr[one].contiguous(), net[one].contiguous())
        oi = G.gru_conv_q([x[one].contiguous()], wq, bq, kq[one].contiguous(), z[one].contiguous(), net[one].contiguous())
        assert same_bits(zi, z[one]) and same_bits(ri, rnet[one]) and same_bits(oi, out[one]), i
        assert same_bits(G.gru_conv3x3([x[one].contiguous()], wzr, bzr), c[one]), i


# (image, channel, y, x): a border pixel, pixels on tile edges (x = 31 | 32 and 63 | 64; y = 1 | 2, 3 | 4 and 7 | 8), a channel
# on either side of every segment edge (127 | 128, 255 | 256, 383 | 384) and of a 64-channel chunk edge inside a segment
# (63 | 64, 319 | 320), one in each segment
NAN_AT = [((2, 9, 33), [(1, 5, 0, 32), (0, 64, 3, 31), (1, 127, 4, 16), (0, 128, 8, 0), (1, 447, 7, 32)]),
          ((1, 17, 130), [(0, 0, 16, 129), (0, 255, 4, 64), (0, 256, 3, 63), (0, 319, 8, 65), (0, 383, 1, 128), (0, 384, 2, 31)]),
          ((1, 13, 65), [(0, 63, 0, 0), (0, 320, 7, 31), (0, 200, 8, 32), (0, 440, 12, 64)])]


@pytest.mark.gpu
@pytest.mark.parametrize("shape,ats", NAN_AT)
@pytest.mark.parametrize("cout", COUTS)
def test_nan_reaches_exactly_its_3x3_neighbourhood(lgu, cout, shape, ats):
    _need_gpu(lgu)
    x = inputs(shape)[1]
    wpack, bias_h = _packed(lgu, cout)
    clean = lgu.gru.gru_conv3x3(_segs(x), wpack, bias_h).cpu()
    assert not bool(torch.isnan(clean).any())
    for at in ats:
        xn = x.clone()
        xn[at] = float("nan")
        got = lgu.gru.gru_conv3x3(_segs(xn), wpack, bias_h).cpu()
        n, _, cy, cx = at
        want = torch.zeros((shape[0], 1) + shape[1:], dtype=torch.bool)
        want[n, 0, max(cy - 1, 0):cy + 2, max(cx - 1, 0):cx + 2] = True
        assert bool((torch.isnan(got) == want.expand_as(got)).all()), at
        assert bool((got.view(torch.int16) == clean.view(torch.int16))[~want.expand_as(got)].all()), at


_OPERANDS = {"plain": ("seg0", "seg1", "seg2", "seg3", "bias", "out0", "wpack"),
             "zr": ("seg0", "seg1", "seg2", "seg3", "bias", "k0", "k1", "net", "out0", "out1", "wpack"),
             "q": ("seg0", "seg1", "seg2", "seg3", "bias", "k0", "net", "z", "out0", "wpack")}
_OUTPUTS = ("out0", "out1")


def _c_call(lgu, mode, a, N, H, W, cout, nseg=4, chans=(128, 128, 128, 64), flags=0, bias_offset=0):
    G = lgu._lib.GruConvArgs()
    for i in range(4):                                    # the block has four slots: nseg = 5 is only a count
        G.seg[i], G.seg_ch[i] = (a["seg%d" % i].data_ptr() if a.get("seg%d" % i) is not None else None), chans[i]
    for name in ("wpack", "bias", "k0", "k1", "net", "z", "out0", "out1"):
        setattr(G, name, a[name].data_ptr() if a.get(name) is not None else None)
    if bias_offset:
        G.bias = a["bias"].data_ptr() + bias_offset
    G.nseg, G.N, G.H, G.W, G.Cout, G.mode, G.flags = nseg, N, H, W, cout, mode, flags
    rc = lgu._lib.load().lgu_gruconv3x3_c448_h16(G, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(2, 9, 33), (3, 16, 40)])
@pytest.mark.parametrize("mode", ("plain", "zr", "q"))
def test_guard_bands_and_alignment(lgu, mode, shape):
    """The alignment audit of DESIGN.md §4.1 for lgu_gruconv3x3_c448_h16: the segments, bias, k, net, z and the outputs
    are served at element alignment with the aligned call's bits (16-byte stores and reads of net and z only where W
    and the addresses allow), a wpack that is not 16-byte aligned is refused with nothing launched, and so is every
    other refusal of the header; N == 0 launches nothing."""
    from tests.alignment_cases import guards_intact, shifted
    _need_gpu(lgu)
    G, L = lgu.gru, lgu._lib
    N, H, W = shape
    (net, _, _, _), x = inputs(shape)
    cout = 256 if mode == "zr" else 128
    code = {"plain": G.PLAIN, "zr": G.ZR, "q": G.Q}[mode]
    wpack, bias_h = _packed(lgu, cout)
    k = gates_k(shape, 3).cuda()
    zin = torch.rand((N, 128, H, W), generator=torch.Generator().manual_seed(1)).half().cuda()
    segs = _segs(x)
    base = {"seg0": segs[0], "seg1": segs[1], "seg2": segs[2], "seg3": segs[3], "wpack": wpack, "bias": bias_h,
            "k0": k[0].contiguous(), "k1": k[1].contiguous(), "net": net.cuda(), "z": zin,
            "out0": torch.zeros((N, cout if mode == "plain" else 128, H, W), dtype=H16, device="cuda"),
            "out1": torch.zeros((N, 128, H, W), dtype=H16, device="cuda")}
    base = {name: (t if name in _OPERANDS[mode] else None) for name, t in base.items()}
    assert all(t.data_ptr() % 16 == 0 for t in base.values() if t is not None)
    assert _c_call(lgu, code, base, N, H, W, cout) == 0
    outs = [o for o in _OUTPUTS if base[o] is not None]
    want = {o: base[o].clone() for o in outs}
    if mode == "plain":
        py = [G.gru_conv3x3(segs, wpack, bias_h)]
    elif mode == "zr":
        py = G.gru_conv_zr(segs, wpack, bias_h, base["k0"], base["k1"], base["net"])
    else:
        py = [G.gru_conv_q(segs, wpack, bias_h, base["k0"], base["z"], base["net"])]
    assert all(same_bits(p, want[o]) for p, o in zip(py, outs))
    variants = [(name, s) for name in _OPERANDS[mode] for s in (2, 4, 8)]
    for key, shift in variants + [("all", 0), ("all but wpack", 0)]:
        keys = [key] if key in base else [n for n in _OPERANDS[mode] if key == "all" or n != "wpack"]
        args = dict(base)
        for o in outs:
            args[o] = torch.full_like(base[o], 7.0)
        for n in keys:
            args[n] = shifted(args[n], shift if key in base else 2)
        before = {n: t.clone() for n, t in args.items() if t is not None}
        rc = _c_call(lgu, code, args, N, H, W, cout)
        if "wpack" in keys:
            assert rc == L.LGU_E_UNSUPPORTED, (key, shift, rc)
            assert all(same_bits(args[o], before[o]) for o in outs), "refused, but an output changed"
        else:
            assert rc == 0, (key, shift, rc)
            for o in outs:
                assert same_bits(args[o], want[o]), "%s shifted by %d: %s differs from the aligned call" % (key, shift, o)
        for n in _OPERANDS[mode]:
            if n not in outs:
                assert same_bits(args[n], before[n]), "read-only operand %s changed" % n
        for n in keys:
            assert guards_intact(args[n]), "%s, %d: a guard band of %s was written" % (key, shift, n)
    # the refusals of the header: nothing is written
    args = dict(base)
    for o in outs:
        args[o] = shifted(torch.full_like(base[o], 7.0), 0)
    before = {o: args[o].clone() for o in outs}
    bad, uns = L.LGU_E_BADARG, L.LGU_E_UNSUPPORTED
    other_cout = {"plain": 64, "zr": 128, "q": 256}[mode]
    null_of = {"plain": ("seg2", "bias", "out0"), "zr": ("k1", "net", "out1"), "q": ("k0", "z", "net")}[mode]
    refusals = [(dict(N=-1), bad), (dict(H=0), bad), (dict(W=0), bad), (dict(flags=1), bad), (dict(nseg=0), bad), (dict(nseg=5), bad),
                (dict(mode=3), bad), (dict(mode=-1), bad), (dict(cout=other_cout), uns), (dict(cout=96), uns),
                (dict(chans=(128, 128, 112, 80)), uns), (dict(chans=(128, 128, 128, 32)), uns), (dict(chans=(128, 128, 192, 0)), uns),
                (dict(nseg=3), uns)]
    refusals += [(dict(null=n), bad) for n in null_of] + [(dict(bias_offset=1), bad)]   # an odd address: below the element
    for kw, want_rc in refusals:
        a = dict(args)
        if "null" in kw:
            a[kw["null"]] = None
        rc = _c_call(lgu, kw.get("mode", code), a, kw.get("N", N), kw.get("H", H), kw.get("W", W), kw.get("cout", cout),
                     nseg=kw.get("nseg", 4), chans=kw.get("chans", (128, 128, 128, 64)), flags=kw.get("flags", 0),
                     bias_offset=kw.get("bias_offset", 0))
        assert rc == want_rc, (kw, rc)
        assert all(same_bits(args[o], before[o]) and guards_intact(args[o]) for o in outs), kw
    assert _c_call(lgu, code, args, 0, H, W, cout) == 0          # N == 0: nothing launched
    assert all(same_bits(args[o], before[o]) and guards_intact(args[o]) for o in outs)
    if mode == "plain":
        assert tuple(G.gru_conv3x3([s[:0] for s in segs], wpack, bias_h).shape) == (0, cout, H, W)
        with pytest.raises(RuntimeError, match=r"gru_conv3x3: empty frame \(H\*W = 0\)"):
            G.gru_conv3x3([s[:, :, :0] for s in segs], wpack, bias_h)


def _gpu_module(seed):
    return R.make_module(seed).cuda()


def _composition(lgu, wr, net, rest):
    """The convs=True forward spelled as PLAIN calls and the existing kangru_* operators; also returns the heads' k."""
    G = lgu.gru
    w, b, grid, wpack = wr.packed(H16)
    (wzr, bzr), (wq, bq) = wr.conv_packed()
    k = G.kan_heads(G.kangru_context(net, w, b), grid, wpack)
    net_inp = torch.cat([net] + list(rest), 1)
    c = G.gru_conv3x3([net_inp], wzr, bzr)
    z = G.kangru_gates_(net_inp, c[:, :128].contiguous(), c[:, 128:].contiguous(), k[0], k[1], net)
    cq = G.gru_conv3x3([net_inp], wq, bq)
    return G.kangru_blend(cq, k[2], z, net), k


@pytest.mark.gpu
@pytest.mark.parametrize("shape", FORWARD_SHAPES)
def test_whole_forward_with_fused_convolutions(lgu, monkeypatch, shape):
    """(a) bit for bit the composition of PLAIN calls with the kangru_* operators; (b) within the propagated bound of the
    float64 chain that takes the device's own kz, kr, kq as given (gruconv_restatement.forward)."""
    _need_gpu(lgu)
    G = lgu.gru
    monkeypatch.setattr(G, "MIN_FUSED_CONV_PIXELS", 0)
    m = R.make_module(1063)
    mc = _gpu_module(1063)
    ins = R.make_inputs(300 + shape[2], *shape)
    insc = [t.cuda() for t in ins]
    wr, parent = G.KanBiasGRU(mc, convs=True), G.KanBiasGRU(mc)
    with torch.no_grad(), torch.autocast("cuda", dtype=H16):
        got = wr(*insc)
        base = parent(*insc)
        own = mc(*insc)
        comp, k = _composition(lgu, wr, insc[0], insc[1:])
        # an input whose channel count is no multiple of 32, or a fourth input: one 320-channel segment, the same bits
        cut = wr(insc[0], insc[1][:, :100].contiguous(), torch.cat([insc[1][:, 100:], insc[2]], 1), insc[3])
        four = wr(insc[0], insc[1], insc[2][:, :64].contiguous(), insc[2][:, 64:].contiguous(), insc[3])
    torch.cuda.synchronize()
    assert wr.fused_calls == 3 and wr.fused_conv_calls == 3 and parent.fused_conv_calls == 0 and parent.fused_calls == 1
    assert got.dtype == H16 and tuple(got.shape) == (shape[0], 128) + shape[1:]
    assert same_bits(got, comp) and same_bits(cut, got) and same_bits(four, got)
    with torch.no_grad():
        ref, bound = R.forward(m, *ins, *(t.cpu() for t in k))
    err = {name: float(((t.cpu().double() - ref).abs() / bound).max()) for name, t in (("convs=True", got), ("convs=False", base),
                                                                                       ("the module's own forward", own))}
    print("KanBiasGRU %s: worst error as a fraction of the propagated bound: %s; %.4f of convs=True's elements are convs=False's bits"
          % (shape, ", ".join("%s %.3g" % kv for kv in err.items()), float((got == base).double().mean())))
    assert err["convs=True"] <= 1.0, err


@pytest.mark.gpu
def test_routes_and_weight_changes(lgu, monkeypatch):
    """Autocast off, a bfloat16 autocast, grad inputs and a call below MIN_FUSED_CONV_PIXELS do not count a
    fused-convolution call and return what convs=False returns (CPU tensors: the CPU test above); load_state_dict and
    in-place edits are followed."""
    _need_gpu(lgu)
    G = lgu.gru
    monkeypatch.setattr(G, "MIN_FUSED_CONV_PIXELS", 0)
    mc = _gpu_module(1064)
    shape = (2, 9, 33)
    ins = [t.cuda() for t in R.make_inputs(41, *shape)]
    wr = G.install(mc, convs=True)
    parent = G.KanBiasGRU(mc)
    with torch.no_grad():
        f32 = [t.float() for t in ins]
        assert same_bits(mc(*f32), parent(*f32))                                   # fp32 mode: the fused fp32 path of both
        with torch.autocast("cuda", dtype=torch.bfloat16):
            assert same_bits(mc(*ins), parent(*ins))
    assert wr.fused_conv_calls == 0 and wr.fused_calls == 1
    with torch.autocast("cuda", dtype=H16):
        grad = mc(ins[0].clone().requires_grad_(), *ins[1:])
        assert grad.requires_grad and wr.fused_conv_calls == 0
        with torch.no_grad():
            monkeypatch.setattr(G, "MIN_FUSED_CONV_PIXELS", 1 << 40)
            routed = mc(*ins)
            assert wr.fused_conv_calls == 0 and wr.fused_calls == 2 and same_bits(routed, parent(*ins))
            monkeypatch.setattr(G, "MIN_FUSED_CONV_PIXELS", 0)
            first = mc(*ins)
            assert wr.fused_conv_calls == 1 and same_bits(first, _composition(lgu, wr, ins[0], ins[1:])[0])
            other = R.make_module(999)
            mc.load_state_dict(other.state_dict())
            second = mc(*ins)
            assert same_bits(second, _composition(lgu, wr, ins[0], ins[1:])[0]) and not same_bits(second, first)
            twin = G.KanBiasGRU(_gpu_module(999), convs=True)
            assert same_bits(twin(*ins), second)
            mc.convq.weight.mul_(0.5)
            mc.convz.bias.add_(0.25)
            third = mc(*ins)
            assert same_bits(third, _composition(lgu, wr, ins[0], ins[1:])[0]) and not same_bits(third, second)
            assert wr.fused_conv_calls == 3
            assert G.install(mc) is wr and wr.convs is False and same_bits(mc(*ins), parent(*ins)) and wr.fused_conv_calls == 3
    G.uninstall(mc)
    assert "forward" not in mc.__dict__


@pytest.mark.gpu
def test_graph_capture_and_side_stream_equal_eager(lgu, monkeypatch):
    _need_gpu(lgu)
    G = lgu.gru
    monkeypatch.setattr(G, "MIN_FUSED_CONV_PIXELS", 0)
    mc = _gpu_module(1065)
    ins = [t.cuda() for t in R.make_inputs(47, 4, 24, 32)]
    wr = G.KanBiasGRU(mc, convs=True)

    def run():
        with torch.no_grad(), torch.autocast("cuda", dtype=H16):
            return wr(*ins)
    eager = run()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        side = run()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    assert same_bits(side, eager)
    g = torch.cuda.CUDAGraph()
    s2 = torch.cuda.Stream()
    s2.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s2):
        run()                                            # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(s2)
    with torch.cuda.graph(g):
        cap = run()
    g.replay()
    torch.cuda.synchronize()
    assert same_bits(cap, eager) and wr.fused_conv_calls == 4
