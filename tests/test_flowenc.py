"""The fused first layer of the motion encoder (lgu_slam_amd.flow, csrc/flowenc.hip) against the float64 restatement of
its rounding model, tests/flowenc_restatement.py.

Numerics contract (include/lgu_corr.h):
- a single product is exact: impulses and the zero input are bit for bit;
- every element: |y - relu(s64)| <= 198·2^-24·S + 2^-11·(|s64| + 198·2^-24·S) + 2^-25 with S = Σ|x_h·w_h| + |b_h|: fp32
  accumulation in any order, one half rounding, the half subnormal floor;
- NaN reaches exactly the pixels whose window covers it; an image's bits do not depend on the batch;
- the whole encoder: the first layer's allowance pushed through |w2_h| plus the second layer's own (1154 terms); the
  module's own autocast forward is held to the same bound.
The alignment audit of lgu_flow_conv7_relu_h16 (its operands travel in a parameter block, so the registry of
tests/alignment_cases.py does not see it) is test_guard_bands_and_alignment here.
The GPU tests build the Sequential themselves and never read the reference tree.
"""
import ctypes
import os

import pytest

torch = pytest.importorskip("torch")

from tests import flowenc_restatement as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = "lgu_flow_conv7_relu_h16"
SHAPES = [(1, 1, 1), (1, 3, 5), (2, 9, 33), (3, 16, 40), (1, 60, 80), (2, 48, 64)]
_CASES = {}


def same_bits(a, b):
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    iv = torch.int16 if a.dtype == torch.float16 else torch.int32
    return bool(torch.equal(a.view(iv), b.view(iv)))


def case(shape):
    """(module, x, s64, S, want) on the CPU for one shape, computed once and never changed."""
    if shape not in _CASES:
        m = R.make_module(41)
        x = R.make_input(1000 + shape[1] * shape[2], *shape)
        with torch.no_grad():
            _CASES[shape] = (m, x) + R.conv7_relu(x, m[0].weight, m[0].bias)
    return _CASES[shape]


# ---- CPU ------------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_entry(lgu):
    from tests.test_abi import declared_symbols
    lib = ctypes.CDLL(lgu._lib._build.SO_PATH)
    assert ENTRY in declared_symbols() and hasattr(lib, ENTRY)
    sig = lgu._lib.SIGNATURES[ENTRY]
    assert issubclass(sig[0], ctypes.Structure) and sig[1] is ctypes.c_void_p
    assert [f[0] for f in sig[0]._fields_] == ["x", "wpack", "bias", "out", "N", "H", "W"]
    assert ctypes.sizeof(sig[0]) == 4 * 8 + 3 * 4 + 4
    assert "flowenc.hip" in lgu._build.SOURCES
    assert lgu.FlowEncoder is lgu.flow.FlowEncoder
    text = open(os.path.join(ROOT, "include", "lgu_corr.h")).read()
    assert "#define LGU_FLOW_CONV7_WPACK_HALVES %d" % lgu.flow.WPACK_HALVES in text and "droid_net.py:82-84" in text


def test_pack_puts_every_weight_in_its_documented_slot_and_zero_elsewhere(lgu):
    g = torch.Generator().manual_seed(5)
    w = torch.randn((128, 4, 7, 7), generator=g)
    b = torch.randn((128,), generator=g)
    wpack, bias_h = lgu.flow.pack_conv7(w, b)
    assert wpack.dtype == torch.float16 and wpack.is_contiguous() and wpack.numel() == lgu.flow.WPACK_HALVES == 28672
    assert tuple(wpack.shape) == (7, 8, 64, 8) and same_bits(bias_h, b.half())
    wh = w.half()
    seen = torch.zeros((128, 4, 7, 7), dtype=torch.bool)
    for ky in range(7):
        for ct in range(8):
            for lane in range(64):
                for j in range(8):
                    k = 8 * (lane >> 4) + j
                    kx, c, co = k // 4, k % 4, 16 * ct + (lane & 15)
                    v = wpack[ky, ct, lane, j]
                    if kx == 7:
                        assert v.view(torch.int16).item() == 0
                    else:
                        assert v.view(torch.int16).item() == wh[co, c, ky, kx].view(torch.int16).item()
                        seen[co, c, ky, kx] = True
    assert bool(seen.all())
    with pytest.raises(RuntimeError, match="weight must be"):
        lgu.flow.pack_conv7(w[:, :3], b)
    with pytest.raises(RuntimeError, match="bias must be"):
        lgu.flow.pack_conv7(w, b[:64])


@pytest.mark.parametrize("shape", [(1, 1, 1), (2, 9, 33)])
def test_restatement_equals_float64_conv2d_on_the_rounded_operands(shape):
    m, x, s64, S, want = case(shape)
    F = torch.nn.functional
    xh, wh, bh = R.h64(x), R.h64(m[0].weight), R.h64(m[0].bias)
    s = F.conv2d(xh, wh, bh, padding=3)
    Sc = F.conv2d(xh.abs(), wh.abs(), bh.abs(), padding=3)
    # the operands are half values, so every product is exact in float64; the two sums differ in order only
    assert bool(((s - s64).abs() <= 2.0 ** -44 * S).all()) and bool(((Sc - S).abs() <= 2.0 ** -44 * S).all())
    assert want.dtype == torch.float16 and bool((want >= 0).all())
    assert float(x.max()) == 64.0 and float(x.min()) == -64.0
    assert bool((S >= s64.abs()).all()) and bool((R.allowance(s64, S, R.TERMS1) > 0).all())


def test_cpu_inputs_reach_the_module_and_install_keeps_the_state_dict(lgu):
    m, x, _, _, _ = case((2, 9, 33))
    keys = list(m.state_dict().keys())
    with torch.no_grad():
        want = m(x.clone())
        direct = lgu.flow.FlowEncoder(m)
        assert same_bits(direct(x.clone()), want) and direct.fused_calls == 0
        wr = lgu.flow.install(m)
        assert isinstance(wr, lgu.flow.FlowEncoder) and m.forward is wr and lgu.flow.install(m) is wr
        assert list(m.state_dict().keys()) == keys and len(list(m.parameters())) == 4
        got = m(x.clone())
    want_grad = m(x.clone().requires_grad_())
    assert want_grad.requires_grad and same_bits(want_grad, want)
    lgu.flow.uninstall(m)
    assert "forward" not in m.__dict__ and list(m.state_dict().keys()) == keys
    assert wr.fused_calls == 0 and same_bits(got, want)


def test_construction_refuses_other_architectures(lgu):
    nn = torch.nn
    lgu.flow.FlowEncoder(R.make_module(1))
    bad = [nn.Sequential(nn.Conv2d(4, 128, 7, padding=3), nn.ReLU(), nn.Conv2d(128, 64, 3, padding=1)),
           nn.Sequential(nn.Conv2d(4, 128, 7, padding=2), nn.ReLU(), nn.Conv2d(128, 64, 3, padding=1), nn.ReLU()),
           nn.Sequential(nn.Conv2d(4, 128, 7, padding=3, bias=False), nn.ReLU(), nn.Conv2d(128, 64, 3, padding=1), nn.ReLU()),
           nn.Sequential(nn.Conv2d(4, 128, 7, padding=3), nn.Tanh(), nn.Conv2d(128, 64, 3, padding=1), nn.ReLU()),
           nn.Sequential(nn.Conv2d(4, 128, 7, padding=3), nn.ReLU(), nn.Conv2d(128, 128, 3, padding=1), nn.ReLU()),
           nn.Sequential(nn.Conv2d(2, 128, 7, padding=3), nn.ReLU(), nn.Conv2d(128, 64, 3, padding=1), nn.ReLU()),
           nn.Conv2d(4, 128, 7, padding=3)]
    for m in bad:
        with pytest.raises(RuntimeError, match="FlowEncoder: the module must be"):
            lgu.flow.FlowEncoder(m)
        with pytest.raises(RuntimeError, match="FlowEncoder: the module must be"):
            lgu.flow.install(m)
        assert "forward" not in m.__dict__


def test_operator_argument_errors_are_raised_before_anything_is_launched(lgu):
    F = lgu.flow
    m, x, _, _, _ = case((2, 9, 33))
    wpack, bias_h = F.pack_conv7(m[0].weight, m[0].bias)
    with pytest.raises(RuntimeError, match="x must be contiguous"):
        F.flow_conv7_relu(x.permute(0, 1, 3, 2).contiguous().permute(0, 1, 3, 2), wpack, bias_h)
    with pytest.raises(RuntimeError, match="wpack must be contiguous"):
        F.flow_conv7_relu(x, torch.zeros((7, 8, 64, 16), dtype=torch.float16)[..., ::2], bias_h)
    with pytest.raises(RuntimeError, match="bias_h must be contiguous"):
        F.flow_conv7_relu(x, wpack, torch.zeros(256, dtype=torch.float16)[::2])
    with pytest.raises(RuntimeError, match=r"x must be \(N,4,H,W\)"):
        F.flow_conv7_relu(x[:, :3].contiguous(), wpack, bias_h)
    with pytest.raises(RuntimeError, match="expected scalar type Float or Half but found Double"):
        F.flow_conv7_relu(x.double(), wpack, bias_h)
    with pytest.raises(RuntimeError, match="expected scalar type Half but found Float"):
        F.flow_conv7_relu(x, wpack.float(), bias_h)
    with pytest.raises(RuntimeError, match="has no autograd"):
        F.flow_conv7_relu(x.clone().requires_grad_(), wpack, bias_h)
    with pytest.raises(RuntimeError, match="must be a HIP device tensor"):
        F.flow_conv7_relu(x, wpack, bias_h)


# ---- GPU ------------------------------------------------------------------------------------------------------------
def _need_gpu(lgu):
    assert torch.cuda.is_available(), "these tests need the MI355X"
    assert os.path.exists(lgu._lib.so_path()), "liblgu_corr.so missing — run __graft_entry__.build()"


def _packed(lgu, m):
    return lgu.flow.pack_conv7(m[0].weight.detach().cuda(), m[0].bias.detach().cuda())


IMPULSE_AT = [(6, 6), (0, 0), (0, 12), (12, 0), (12, 12)]


@pytest.mark.gpu
def test_impulses_give_the_weights_bit_for_bit(lgu):
    """One input element = 1 (centre and the four corners of a 13x13 image, each of the 4 channels), bias 0: a single
    product is exact, so every output is relu(w_h[co, c, cy-y+3, cx-x+3]) and 0 outside the window."""
    _need_gpu(lgu)
    m = R.make_module(43)
    with torch.no_grad():
        m[0].bias.zero_()
    wh = m[0].weight.detach().half()
    x = torch.zeros((4 * len(IMPULSE_AT), 4, 13, 13))
    want = torch.zeros((x.shape[0], 128, 13, 13), dtype=torch.float16)
    for i, (cy, cx) in enumerate(IMPULSE_AT):
        for c in range(4):
            n = 4 * i + c
            x[n, c, cy, cx] = 1.0
            for ky in range(7):
                for kx in range(7):
                    y, xx = cy - ky + 3, cx - kx + 3
                    if 0 <= y < 13 and 0 <= xx < 13:
                        want[n, :, y, xx] = torch.relu(wh[:, c, ky, kx])
    wpack, bias_h = _packed(lgu, m)
    got = lgu.flow.flow_conv7_relu(x.cuda(), wpack, bias_h)
    torch.cuda.synchronize()
    assert int((want != 0).sum()) > 0.4 * 20 * 128 * 25       # about half the weights are positive
    assert same_bits(got, want), "max |diff| %g" % float((got.cpu().float() - want.float()).abs().max())


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES)
def test_zero_input_gives_relu_of_the_bias_everywhere(lgu, shape):
    _need_gpu(lgu)
    m = R.make_module(41)
    wpack, bias_h = _packed(lgu, m)
    got = lgu.flow.flow_conv7_relu(torch.zeros((shape[0], 4) + shape[1:], device="cuda"), wpack, bias_h)
    torch.cuda.synchronize()
    want = torch.relu(m[0].bias.detach().half()).view(1, 128, 1, 1).expand(shape[0], 128, *shape[1:])
    assert same_bits(got, want)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES)
def test_every_element_is_within_the_derived_bound(lgu, shape):
    _need_gpu(lgu)
    m, x, s64, S, want = case(shape)
    wpack, bias_h = _packed(lgu, m)
    got = lgu.flow.flow_conv7_relu(x.cuda(), wpack, bias_h)
    from_half = lgu.flow.flow_conv7_relu(x.half().cuda(), wpack, bias_h)
    mc = R.make_module(41).cuda()
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        own = mc[1](mc[0](x.cuda()))
    torch.cuda.synchronize()
    bound = R.allowance(s64, S, R.TERMS1)
    ref = torch.relu(s64)
    err = (got.cpu().double() - ref).abs()
    err_own = (own.cpu().double() - ref).abs()
    print("flow_conv7_relu %s: worst error %.3g of its bound, %.4f of the elements are the restatement's bits; the module's "
          "own forward: worst %.3g of the bound, %.4f bit-identical to the kernel"
          % (shape, float((err / bound).max()), float((got.cpu() == want).double().mean()), float((err_own / bound).max()),
             float((own == got).double().mean())))
    assert got.dtype == torch.float16 and tuple(got.shape) == (shape[0], 128) + shape[1:]
    assert bool((err <= bound).all()), float((err / bound).max())
    assert same_bits(from_half, lgu.flow.flow_conv7_relu(x.half().float().cuda(), wpack, bias_h))


@pytest.mark.gpu
@pytest.mark.parametrize("shape,at", [((2, 9, 33), (1, 2, 0, 32)), ((3, 16, 40), (2, 0, 15, 17)), ((1, 60, 80), (0, 3, 8, 64))])
def test_nan_reaches_exactly_the_pixels_whose_window_covers_it(lgu, shape, at):
    _need_gpu(lgu)
    m, x, _, _, _ = case(shape)
    wpack, bias_h = _packed(lgu, m)
    xn = x.clone()
    xn[at] = float("nan")
    got = lgu.flow.flow_conv7_relu(xn.cuda(), wpack, bias_h).cpu()
    clean = lgu.flow.flow_conv7_relu(x.cuda(), wpack, bias_h).cpu()
    n, _, cy, cx = at
    want = torch.zeros((shape[0], 1) + shape[1:], dtype=torch.bool)
    want[n, 0, max(cy - 3, 0):cy + 4, max(cx - 3, 0):cx + 4] = True
    assert bool((torch.isnan(got) == want.expand_as(got)).all())
    assert bool((got.view(torch.int16) == clean.view(torch.int16))[~want.expand_as(got)].all())


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(3, 16, 40), (3, 9, 33)])
def test_an_image_does_not_depend_on_its_batch(lgu, shape):
    _need_gpu(lgu)
    m = R.make_module(41)
    x = R.make_input(77, *shape).cuda()
    wpack, bias_h = _packed(lgu, m)
    got = lgu.flow.flow_conv7_relu(x, wpack, bias_h)
    for k in range(shape[0]):
        assert same_bits(got[k:k + 1], lgu.flow.flow_conv7_relu(x[k:k + 1].contiguous(), wpack, bias_h)), k


def _c_call(lgu, x, wpack, bias_h, out):
    N, _, H, W = x.shape
    args = lgu._lib.FlowConv7Args(x.data_ptr(), wpack.data_ptr(), bias_h.data_ptr(), out.data_ptr(), N, H, W)
    rc = lgu._lib.load().lgu_flow_conv7_relu_h16(args, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(2, 9, 33), (3, 16, 40)])
def test_guard_bands_and_alignment(lgu, shape):
    """The alignment audit of DESIGN.md §4.1 for lgu_flow_conv7_relu_h16: x, bias and out are served at element
    alignment with the aligned call's bits (out by element stores when it is not 8-byte aligned or W % 4 != 0), a wpack
    that is not 16-byte aligned is refused with nothing launched."""
    from tests.alignment_cases import guards_intact, shifted
    _need_gpu(lgu)
    m, x, _, _, _ = case(shape)
    wpack, bias_h = _packed(lgu, m)
    base = {"x": x.cuda(), "wpack": wpack, "bias": bias_h,
            "out": torch.empty((shape[0], 128) + shape[1:], dtype=torch.float16, device="cuda")}
    assert all(t.data_ptr() % 16 == 0 for t in base.values())
    assert _c_call(lgu, base["x"], base["wpack"], base["bias"], base["out"]) == 0
    want = base["out"].clone()
    variants = [(k, s) for k, ss in (("x", (4, 8)), ("bias", (2, 4, 8)), ("out", (2, 4, 8)), ("wpack", (2, 4, 8))) for s in ss]
    for key, shift in variants + [("all", 0), ("all but wpack", 0)]:
        keys = [key] if key in base else [k for k in base if key == "all" or k != "wpack"]
        args = dict(base)
        for k in keys:
            args[k] = shifted(base[k], shift if key in base else base[k].element_size())
        before = {k: args[k].clone() for k in args}
        rc = _c_call(lgu, args["x"], args["wpack"], args["bias"], args["out"])
        if "wpack" in keys:
            assert rc == lgu._lib.LGU_E_UNSUPPORTED, (key, shift, rc)
            assert same_bits(args["out"], before["out"]), "refused, but out changed"
        else:
            assert rc == 0, (key, shift, rc)
            assert same_bits(args["out"], want), "%s shifted by %d: differs from the aligned call" % (key, shift)
        for k in ("x", "wpack", "bias"):
            assert same_bits(args[k], before[k]), "read-only operand %s changed" % k
        for k in keys:
            assert guards_intact(args[k]), "%s, %d: a guard band of %s was written" % (key, shift, k)
    # the class serves every contiguous input
    mc = R.make_module(41).cuda()
    wr = lgu.flow.FlowEncoder(mc)
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        first = wr(base["x"])
        for shift in (4, 8):
            xs = shifted(base["x"], shift)
            assert same_bits(wr(xs), first) and same_bits(xs, base["x"]) and guards_intact(xs)
    assert wr.fused_calls == 3


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(2, 9, 33), (1, 60, 80), (2, 48, 64)])
def test_whole_encoder_is_within_the_propagated_bound(lgu, shape):
    _need_gpu(lgu)
    m, x, _, _, _ = case(shape)
    with torch.no_grad():
        s2, bound = R.encoder(x, m)
    ref = torch.relu(s2)
    mc = R.make_module(41).cuda()
    xc = x.cuda()
    wr = lgu.flow.FlowEncoder(mc)
    with torch.no_grad():
        with torch.autocast("cuda", dtype=torch.float16):
            own = mc(xc.clone())
            got = wr(xc)
            assert wr.fused_calls == 1
            assert same_bits(wr(xc.half()), wr(xc.half().float()))      # a half input is widened, which is exact
            assert wr.fused_calls == 3
        plain = wr(xc)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            bf = wr(xc)
    with torch.autocast("cuda", dtype=torch.float16):
        grad = wr(xc.clone().requires_grad_())
        with torch.no_grad():
            lgu.flow.install(mc)
            installed = mc(xc)
            lgu.flow.uninstall(mc)
    torch.cuda.synchronize()
    assert wr.fused_calls == 3 and plain.dtype == torch.float32 and bf.dtype == torch.bfloat16 and grad.requires_grad
    assert got.dtype == own.dtype == torch.float16 and got.shape == own.shape == (shape[0], 64) + shape[1:]
    assert same_bits(installed, got)
    err, err_own = (got.cpu().double() - ref).abs(), (own.cpu().double() - ref).abs()
    print("FlowEncoder %s: worst error %.3g of the bound; the module's own forward %.3g; %.4f of the elements bit-identical"
          % (shape, float((err / bound).max()), float((err_own / bound).max()), float((got == own).double().mean())))
    assert bool((err <= bound).all()), float((err / bound).max())
    assert bool((err_own <= bound).all()), float((err_own / bound).max())
