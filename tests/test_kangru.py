"""The KAN-bias GRU of the update operator (lgu_slam_amd.gru, csrc/kangru.hip) against the op-for-op restatement
tests/kangru_restatement.py and the reference's own forward (tests/golden/kangru_*.npz, tools/gen_kangru_golden.py).

Numerics contract:
- bases (one-hot spline weights, zero base weight): bit-identical to the restatement in fp32;
- gates and blend, given the same conv outputs and biases: bit-identical to torch's element-wise ops in both modes;
- context glo: fp32 within a bound derived from the 128-term conv sum and the mean over H*W terms (vs fp64); half
  within 1 half ulp of glo plus 2 half ulps of the mean pixel term of the restatement under autocast;
- KAN heads: fp32 within (n+2)·2^-24·Σ|terms| per GEMM (vs fp64 of the same features); half within 2 half ulps of the
  restatement and no farther from fp64 than the library composition;
- whole forward: a bound derived from the rows above (σ' <= 1/4, tanh' <= 1); in half never above 2^-8.
The GPU tests read only the fixtures and the restatement, never the reference tree.
"""
import ctypes
import os
import subprocess
import sys
import types

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import kangru_restatement as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
REFERENCE = os.environ.get("LGU_REFERENCE", "/root/reference")
ENTRIES = ("lgu_kangru_context_f32", "lgu_kangru_context_h16", "lgu_kan_heads_f32", "lgu_kan_heads_h16",
           "lgu_kangru_gates_f32", "lgu_kangru_gates_h16", "lgu_kangru_blend_f32", "lgu_kangru_blend_h16")
U24 = 2.0 ** -24
HALF_ABS_CAP = 2.0 ** -8
# half glo: the library's 1x1 convolution sums in another order, so a conv output can round to the neighbouring half;
# through the sigmoid (σ' <= 1/4) and the product each pixel's term moves by at most 2 of its half ulps, and the mean of
# those moves is added to the 1 ulp of glo itself.  glo is a cancelling sum: a single ulp of glo is not a bound.
CTX_HALF_TERM_ULPS = 2


def same_bits(a, b):
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    iv = torch.int16 if a.dtype == torch.float16 else torch.int32
    return bool(torch.equal(a.view(iv), b.view(iv)))


def half_ulp(x):
    """Spacing of float16 at |x| (float64 tensor)."""
    ax = x.abs().double().clamp_min(2.0 ** -14)
    return torch.exp2(torch.floor(torch.log2(ax)) - 10)


def fixture(name):
    z = dict(np.load(os.path.join(GOLD, name + ".npz")))
    m, ins = R.make_case(name, grid=z["grid"])
    assert R.case_sha256(m, ins) == str(z["sha256"]), "inputs or weights drifted from the fixture"
    return z, m, ins


# ---- CPU ------------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_kangru_entries(lgu):
    from tests.test_abi import declared_symbols
    syms = declared_symbols()
    lib = ctypes.CDLL(lgu._lib._build.SO_PATH)
    for s in ENTRIES:
        assert s in syms and s in lgu._lib.SIGNATURES and hasattr(lib, s), s
    assert "kangru.hip" in lgu._build.SOURCES
    assert lgu.KanBiasGRU is lgu.gru.KanBiasGRU


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_restatement_equals_the_reference_fixture_bit_for_bit(name):
    z, m, ins = fixture(name)
    assert np.array_equal(z["grid"], torch.stack([getattr(m, n).grid for n in R.HEADS]).numpy())
    with torch.no_grad():
        out, p = R.forward(m, *ins, parts=True)
    for k in ("glo", "kz", "kr", "kq"):
        assert np.array_equal(p[k].numpy(), z[k]), k
    assert np.array_equal(out.numpy(), z["out"])


def test_nonuniform_fixture_has_knots_on_inputs_and_inputs_outside_the_knots():
    z, m, _ = fixture("kangru_nonuniform")
    glo, grid = z["glo"], z["grid"]
    on = sum(int(np.any(grid[h, i] == glo[i % 3, i])) for h in range(3) for i in range(0, 128, 5))
    assert on == 3 * 26
    b = R.bases(torch.from_numpy(glo), torch.from_numpy(grid[0]))
    assert (b[:, 1::5] == 0).all() and (b[:, 2::5] == 0).all() and (b[:, 0::5] != 0).any()


@pytest.mark.skipif(not os.path.isdir(os.path.join(REFERENCE, "droid_slam")), reason="reference tree not present")
def test_fixture_regenerates_from_the_live_reference():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_kangru_golden.py"), "--reference", REFERENCE,
                        "--check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr


def test_construction_refuses_other_architectures(lgu):
    G = lgu.gru
    G.KanBiasGRU(R.RefGRU())
    bad = R.RefGRU()
    bad.kanr_glo.grid_size = 5
    with pytest.raises(RuntimeError, match="kanr_glo must be KANLinear"):
        G.KanBiasGRU(bad)
    bad = R.RefGRU()
    bad.kanq_glo.enable_standalone_scale_spline = False
    with pytest.raises(RuntimeError, match="kanq_glo"):
        G.KanBiasGRU(bad)
    bad = R.RefGRU()
    bad.kanz_glo.base_activation = torch.nn.ReLU()
    with pytest.raises(RuntimeError, match="kanz_glo"):
        G.KanBiasGRU(bad)
    bad = R.RefGRU()
    bad.kanz_glo.spline_weight = torch.nn.Parameter(torch.zeros(128, 128, 8))
    with pytest.raises(RuntimeError, match="kanz_glo"):
        G.KanBiasGRU(bad)
    bad = R.RefGRU()
    bad.convr = torch.nn.Conv2d(448, 128, 3, padding=2)
    with pytest.raises(RuntimeError, match="convr must be"):
        G.KanBiasGRU(bad)
    bad = R.RefGRU()
    bad.w = torch.nn.Conv2d(128, 128, 1, bias=False)
    with pytest.raises(RuntimeError, match="w must be"):
        G.KanBiasGRU(bad)


def test_install_and_uninstall_keep_the_state_dict_keys(lgu):
    m = R.set_weights(R.RefGRU(), 3)
    keys = list(m.state_dict().keys())
    wr = lgu.gru.install(m)
    assert isinstance(wr, lgu.gru.KanBiasGRU) and m.forward is wr
    assert lgu.gru.install(m) is wr
    assert list(m.state_dict().keys()) == keys and len(list(m.parameters())) == 3 * 2 + 3 * 3 + 2
    lgu.gru.uninstall(m)
    assert "forward" not in m.__dict__ and list(m.state_dict().keys()) == keys


def test_cpu_inputs_reach_the_module_and_give_its_result(lgu):
    _, m, ins = fixture("kangru_uniform")
    with torch.no_grad():
        want = R.forward(m, *ins)
        wr = lgu.gru.install(m)
        got = m(*ins)
    lgu.gru.uninstall(m)
    assert wr.fused_calls == 0 and same_bits(got, want)


def _no_lib(monkeypatch, lgu):
    def boom():
        raise AssertionError("the library was touched before the argument check")
    monkeypatch.setattr(lgu._lib, "load", boom)


def test_argument_checks_raise_before_any_launch(lgu, monkeypatch):
    _no_lib(monkeypatch, lgu)
    G = lgu.gru
    net, w, b = torch.zeros(2, 128, 3, 4), torch.zeros(128, 128, 1, 1), torch.zeros(128)
    with pytest.raises(RuntimeError, match="net must be"):
        G.kangru_context(torch.zeros(2, 64, 3, 4), w, b)
    with pytest.raises(RuntimeError, match="weight must be"):
        G.kangru_context(net, torch.zeros(128, 64), b)
    with pytest.raises(RuntimeError, match="net must be contiguous"):
        G.kangru_context(torch.zeros(2, 128, 4, 3).transpose(2, 3), w, b)
    with pytest.raises(RuntimeError, match="Float but found Half"):
        G.kangru_context(net, w.half(), b)
    with pytest.raises(RuntimeError, match="Float or Half but found Double"):
        G.kangru_context(net.double(), w.double(), b.double())
    with pytest.raises(RuntimeError, match="no autograd"):
        G.kangru_context(net, w.clone().requires_grad_(), b)
    with pytest.raises(RuntimeError, match="HIP device tensor"):
        G.kangru_context(net, w, b)
    glo, grid, wp = torch.zeros(2, 128), torch.zeros(3, 128, 10), torch.zeros(384, 896)
    with pytest.raises(RuntimeError, match="grid must be"):
        G.kan_heads(glo, torch.zeros(128, 10), wp)
    with pytest.raises(RuntimeError, match="wpack must be"):
        G.kan_heads(glo, grid, torch.zeros(384, 895))
    with pytest.raises(RuntimeError, match="Float but found Half"):
        G.kan_heads(glo, grid.half(), wp)
    with pytest.raises(RuntimeError, match="Half but found Float"):
        G.kan_heads(glo.half(), grid, wp)
    with pytest.raises(RuntimeError, match="HIP device tensor"):
        G.kan_heads(glo, grid, wp)
    ni, f, k = torch.zeros(2, 448, 3, 4), torch.zeros(2, 128, 3, 4), torch.zeros(2, 128)
    with pytest.raises(RuntimeError, match="net_inp must be"):
        G.kangru_gates_(torch.zeros(2, 320, 3, 4), f, f, k, k, f)
    with pytest.raises(RuntimeError, match="cr must be"):
        G.kangru_gates_(ni, f, torch.zeros(2, 128, 3, 5), k, k, f)
    with pytest.raises(RuntimeError, match="kr must be"):
        G.kangru_gates_(ni, f, f, k, torch.zeros(2, 127), f)
    with pytest.raises(RuntimeError, match="kz must be contiguous"):
        G.kangru_gates_(ni, f, f, torch.zeros(128, 2).t(), k, f)
    with pytest.raises(RuntimeError, match="HIP device tensor"):
        G.kangru_gates_(ni, f, f, k, k, f)
    with pytest.raises(RuntimeError, match="kq must be"):
        G.kangru_blend(f, torch.zeros(3, 128), f, f)
    with pytest.raises(RuntimeError, match="Float but found Half"):
        G.kangru_blend(f, k, f.half(), f)
    with pytest.raises(RuntimeError, match="HIP device tensor"):
        G.kangru_blend(f, k, f, f)


def test_torch_ops_registration(lgu):
    import lgu_slam_amd.torch_ops  # noqa: F401
    for name in ("kangru_context", "kan_heads", "kangru_gates_", "kangru_blend"):
        assert hasattr(torch.ops.lgu, name), name
    assert "Tensor(a0!) net_inp" in str(torch.ops.lgu.kangru_gates_.default._schema)


# ---- GPU ------------------------------------------------------------------------------------------------------------
DEV = "cuda"


def gpu_case(name_or_seed, E=None, H=None, W=None, half=False):
    if isinstance(name_or_seed, str):
        _, m, ins = fixture(name_or_seed)
    else:
        m, ins = R.set_weights(R.RefGRU(), name_or_seed + 1000), R.make_inputs(name_or_seed, E, H, W)
    m = m.to(DEV)
    ins = [t.to(DEV) for t in ins]
    if half:
        ins = [t.half() for t in ins]
    return m, ins


def restated(m, ins, half):
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16, enabled=half):
        return R.forward(m, *ins, parts=True)


def fused(lgu, m, ins, half, wrapper=None):
    wr = wrapper or lgu.gru.KanBiasGRU(m)
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16, enabled=half):
        out = wr(*ins)
    return out, wr


def conv_row_norm(conv, cols=slice(0, 128)):
    """max over output channels of sum |W[o, cols]|: the gain of a conv input change of 1 in every channel."""
    return float(conv.weight.detach()[:, cols].abs().sum(dim=(1, 2, 3)).max())


def forward_bound(m, p, dk, half):
    """|Δout| from head-output differences dk = (dz, dr, dq) (max abs): Δz <= dz/4, Δ(r*net) <= dr/4 * max|net|
    (|net| < 1), Δcq <= that times the conv_q gain over its first 128 channels, Δq <= dq + Δcq (tanh' <= 1),
    Δout <= |q - net| Δz + max|z| Δq with |q - net| <= 2, plus the rounding of the blend (a few fp32 or half ulps)."""
    dz, dr, dq = dk
    dcq = dr / 4 * conv_row_norm(m.convq)
    return dz / 4 * 2.0 + (dq + dcq) * float(p["z"].float().abs().max()) + (4 * 2.0 ** -11 if half else 16 * U24)


@pytest.mark.gpu
@pytest.mark.parametrize("half", [False, True])
def test_gates_and_blend_are_bit_identical_to_the_torch_ops(lgu, half):
    g = torch.Generator(device=DEV).manual_seed(5)
    dt = torch.float16 if half else torch.float32
    E = 5
    for H, W in ((7, 13), (8, 16)):          # scalar and 16-byte vector forms
        cz, cr, cq = [(4 * torch.randn(E, 128, H, W, device=DEV, generator=g)).to(dt) for _ in range(3)]
        kz, kr, kq = [(2 * torch.randn(E, 128, device=DEV, generator=g)).to(dt) for _ in range(3)]
        net = torch.tanh(torch.randn(E, 128, H, W, device=DEV, generator=g)).to(dt)
        rest = torch.randn(E, 320, H, W, device=DEV, generator=g).to(dt)
        net_inp = torch.cat([torch.zeros_like(net), rest], 1)
        z = lgu.gru.kangru_gates_(net_inp, cz, cr, kz, kr, net)
        wz, wrn = R.gates(cz, cr, kz, kr, net)
        assert same_bits(z, wz), "z"
        assert same_bits(net_inp[:, :128], wrn), "r*net"
        assert same_bits(net_inp[:, 128:], rest), "channels 128.. touched"
        out = lgu.gru.kangru_blend(cq, kq, z, net)
        assert same_bits(out, R.blend(cq, kq, wz, net)), "blend"


@pytest.mark.gpu
def test_bases_are_bit_identical_to_the_restatement(lgu):
    """One-hot spline weights, zero base weight: every head output is one basis value, in fp32 exactly."""
    _, m, _ = fixture("kangru_nonuniform")
    z = dict(np.load(os.path.join(GOLD, "kangru_nonuniform.npz")))
    grid = torch.from_numpy(z["grid"]).to(DEV)
    glo = torch.from_numpy(z["glo"]).to(DEV)
    g = torch.Generator(device=DEV).manual_seed(9)
    extra = torch.stack([grid[0, :, 5], grid[1, :, 0], grid[2, :, 9], grid[0, :, 9] + 1.0, grid[1, :, 0] - 1e-3,
                         (grid[0, :, 4] + grid[0, :, 5]) / 2, 0.5 * torch.randn(128, device=DEV, generator=g)])
    x = torch.cat([glo, extra])
    x[4, 7] = float("nan")
    x[5, 9] = float("inf")
    finite = torch.isfinite(x).all(1)
    for shift in range(6):
        wp = torch.zeros(384, 896, device=DEV)
        o = torch.arange(128, device=DEV)
        for h in range(3):
            wp[h * 128 + o, 128 + o * 6 + (o + shift + h) % 6] = 1.0
        got = lgu.gru.kan_heads(x.contiguous(), grid, wp)
        for h in range(3):
            want = R.bases(x, grid[h])[:, o, (o + shift + h) % 6]
            assert same_bits(got[h][finite], want[finite].contiguous()), (shift, h)
            # a non-finite x: silu(x) * 0 and B(x) * 0 are NaN, so the whole row is NaN, as in the composition
            head = types.SimpleNamespace(grid=grid[h], out_features=128, base_weight=wp[h * 128:(h + 1) * 128, :128],
                                         spline_weight=wp[h * 128:(h + 1) * 128, 128:].reshape(128, 128, 6),
                                         spline_scaler=torch.ones(128, 128, device=DEV))
            assert torch.equal(torch.isnan(got[h]), torch.isnan(R.kan(x, head))), (shift, h)
    assert torch.isnan(got[:, 4]).all() and torch.isnan(got[:, 5]).all()


@pytest.mark.gpu
def test_dtypes_of_the_autocast_composition(lgu, capsys):
    """The rounding points the half kernels assume, as autocast produces them on the device."""
    m, ins = gpu_case(11, 2, 12, 16, half=True)
    out, p = restated(m, ins, True)
    for k in ("gate", "glo", "kz", "kr", "kq", "cz", "cr", "cq", "z", "r", "q"):
        assert p[k].dtype == torch.float16, k
    assert out.dtype == torch.float16
    net = ins[0]
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        fusedb = m.w(net)
        sep = torch.nn.functional.conv2d(net, m.w.weight.half()) + m.w.bias.half().view(1, -1, 1, 1)
        b = R.bases(p["glo"], m.kanz_glo.grid)
    assert b.dtype == torch.float32
    with capsys.disabled():
        print("\n[kangru] autocast 1x1 conv: bias %s" % ("added in a separate pass (bit-equal)" if same_bits(fusedb, sep)
                                                       else "fused: differs from conv + bias in %.4f of outputs"
                                                       % float((fusedb != sep).float().mean())))


def glo_bound_f32(m, net):
    """fp32 |Δglo| from the 128-term conv sum (γ = 130·2^-24 times Σ|w·net| + |b|), through σ' <= 1/4 and the product
    (one more rounding each), then the mean over H*W terms (γ_HW times the mean of |terms|)."""
    E, _, H, W = net.shape
    n64 = net.double().reshape(E, 128, H * W)
    w = m.w.weight.double().reshape(128, 128)
    a = torch.einsum("ck,ekp->ecp", w.abs(), n64.abs()) + m.w.bias.double().abs()[None, :, None]
    y = torch.einsum("ck,ekp->ecp", w, n64) + m.w.bias.double()[None, :, None]
    s = torch.sigmoid(y)
    term = (0.25 * 130 * U24 * a + 2 * U24) * n64.abs() + 2 * U24 * (s * n64).abs()
    ref = (s * n64).mean(-1)
    return ref, term.mean(-1) + (H * W + 2) * U24 * (s * n64).abs().mean(-1) + U24 * ref.abs()


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["kangru_uniform", "kangru_nonuniform", "frontend"])
def test_context_within_its_bound(lgu, case, capsys):
    args = (case,) if case != "frontend" else (3, 48, 48, 64)
    for half in (False, True):
        m, ins = gpu_case(*args, half=half)
        wr = lgu.gru.KanBiasGRU(m)
        w, b, _, _ = wr.packed(torch.float16 if half else torch.float32)
        with torch.no_grad():
            got = lgu.gru.kangru_context(ins[0], w, b)
        _, p = restated(m, ins, half)
        if not half:
            ref64, bound = glo_bound_f32(m, ins[0])
            assert ((got.double() - ref64).abs() <= bound).all()
            assert ((p["glo"].double() - ref64).abs() <= bound).all()      # the library composition, same bound
        else:
            d = (got.double() - p["glo"].double()).abs()
            ulp = half_ulp(torch.maximum(got.abs(), p["glo"].abs()))
            terms = half_ulp(p["gate"]).flatten(2).mean(-1)     # mean over the pixels of one ulp of each product
            assert (d <= ulp + CTX_HALF_TERM_ULPS * terms).all(), float(d.max())
            ulps = d / ulp
            with capsys.disabled():
                print("\n[kangru] context %s half: %.4f of glo differ from the restatement, %.4f by more than 1 ulp"
                      % (case, float((d > 0).float().mean()), float((ulps > 1).float().mean())))


def heads_f64(glo, grid, m, half):
    """fp64 heads of the features the composition feeds the GEMMs (silu and bases as torch computes them, rounded to
    half in half mode, weights likewise), and Σ|terms| of each GEMM."""
    dt = torch.float16 if half else torch.float32
    outs, tb, ts = [], [], []
    m = {n: getattr(m, n) for n in R.HEADS}
    for h, name in enumerate(R.HEADS):
        hd = m[name]
        s = torch.nn.functional.silu(glo).to(dt).double()
        bs = R.bases(glo, grid[h]).to(dt).double().reshape(glo.shape[0], -1)
        wb = hd.base_weight.to(dt).double()
        ws = (hd.spline_weight * hd.spline_scaler.unsqueeze(-1)).reshape(128, -1).to(dt).double()
        outs.append((s @ wb.t(), bs @ ws.t()))
        tb.append(s.abs() @ wb.abs().t())
        ts.append(bs.abs() @ ws.abs().t())
    return outs, tb, ts


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["kangru_uniform", "kangru_nonuniform", "frontend"])
def test_heads_within_their_bound(lgu, case, capsys):
    args = (case,) if case != "frontend" else (3, 48, 48, 64)
    for half in (False, True):
        m, ins = gpu_case(*args, half=half)
        _, p = restated(m, ins, half)
        glo = p["glo"]
        wr = lgu.gru.KanBiasGRU(m)
        _, _, grid, wpack = wr.packed(glo.dtype)
        with torch.no_grad():
            got = lgu.gru.kan_heads(glo.contiguous(), grid, wpack)
        with torch.no_grad():
            outs, tb, ts = heads_f64(glo, grid, m, half)
        for h, key in enumerate(("kz", "kr", "kq")):
            lib = p[key]
            if not half:
                ref = outs[h][0] + outs[h][1]
                bound = 130 * U24 * tb[h] + 770 * U24 * ts[h] + 2 * U24 * tb[h] + U24 * ref.abs()
                assert ((got[h].double() - ref).abs() <= bound).all(), key
                assert ((lib.double() - ref).abs() <= bound).all(), key
            else:
                d = (got[h].double() - lib.double()).abs()
                assert (d <= 2 * half_ulp(lib)).all(), (key, float(d.max()))
                ref = outs[h][0] + outs[h][1]
                e_got, e_lib = (got[h].double() - ref).abs(), (lib.double() - ref).abs()
                assert float(e_got.mean()) <= 1.01 * float(e_lib.mean()), (key, float(e_got.mean()), float(e_lib.mean()))
                assert float(e_got.max()) <= float(e_lib.max()) + float(half_ulp(ref.abs().max())), key
                with capsys.disabled():
                    print("\n[kangru] heads %s %s half: %.4f differ from the restatement; max |Δ| vs fp64 %.3g (library "
                          "%.3g), mean %.3g (library %.3g)" % (case, key, float((d > 0).float().mean()),
                                                               float(e_got.max()), float(e_lib.max()),
                                                               float(e_got.mean()), float(e_lib.mean())))


def check_forward(lgu, m, ins, half, tag, capsys, ref_out=None, ref_k=None):
    out, wr = fused(lgu, m, ins, half)
    assert wr.fused_calls == 1
    want, p = restated(m, ins, half)
    if ref_out is not None:
        want = ref_out
    assert out.dtype == want.dtype and out.shape == want.shape and out.is_contiguous()
    # the heads' own differences, each within its row's bound (tests above), propagated
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16, enabled=half):
        w, b, grid, wpack = wr.packed(torch.float16 if half else torch.float32)
        k = lgu.gru.kan_heads(lgu.gru.kangru_context(ins[0].contiguous(), w, b), grid, wpack)
    kref = ref_k if ref_k is not None else [p[x] for x in ("kz", "kr", "kq")]
    dk = [float((k[h].double() - kref[h].double()).abs().max()) for h in range(3)]
    bound = forward_bound(m, p, dk, half)
    if half:
        bound = min(bound, HALF_ABS_CAP)
    d = (out.double() - want.double()).abs()
    assert float(d.max()) <= bound, (tag, float(d.max()), bound, dk)
    with capsys.disabled():
        print("\n[kangru] forward %s %s: max |Δ| %.3g (bound %.3g), %.4f not bit-identical"
              % (tag, "half" if half else "fp32", float(d.max()), bound, float((d > 0).float().mean())))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(R.CASES))
def test_fp32_fused_path_against_the_reference_fixture(lgu, name, capsys):
    z, _, _ = fixture(name)
    m, ins = gpu_case(name)
    ref_k = [torch.from_numpy(z[k]).to(DEV) for k in ("kz", "kr", "kq")]
    check_forward(lgu, m, ins, False, name, capsys, ref_out=torch.from_numpy(z["out"]).to(DEV), ref_k=ref_k)


@pytest.mark.gpu
@pytest.mark.parametrize("half", [False, True])
@pytest.mark.parametrize("size", [(48, 48, 64), (8, 60, 80), (3, 7, 13), (1, 12, 16)])
def test_whole_forward_within_its_bound(lgu, size, half, capsys):
    E, H, W = size
    m, ins = gpu_case(20 + E, E, H, W, half=half)
    check_forward(lgu, m, ins, half, "%dx%dx%d" % size, capsys)


@pytest.mark.gpu
def test_no_edges_launch_nothing_and_return_empty(lgu):
    for half in (False, True):
        m, ins = gpu_case(3, 0, 12, 16, half=half)
        out, wr = fused(lgu, m, ins, half)
        assert out.shape == (0, 128, 12, 16) and out.dtype == (torch.float16 if half else torch.float32)
        w, b, grid, wpack = wr.packed(out.dtype)
        with torch.no_grad():
            assert lgu.gru.kangru_context(ins[0], w, b).shape == (0, 128)
            assert lgu.gru.kan_heads(torch.zeros(0, 128, device=DEV, dtype=out.dtype), grid, wpack).shape == (3, 0, 128)


@pytest.mark.gpu
@pytest.mark.parametrize("half", [False, True])
def test_context_and_heads_do_not_depend_on_the_other_edges(lgu, half):
    m, ins = gpu_case(31, 6, 60, 80, half=half)
    wr = lgu.gru.KanBiasGRU(m)
    w, b, grid, wpack = wr.packed(ins[0].dtype)
    with torch.no_grad():
        glo = lgu.gru.kangru_context(ins[0], w, b)
        k = lgu.gru.kan_heads(glo, grid, wpack)
        for e in range(6):
            g1 = lgu.gru.kangru_context(ins[0][e:e + 1].contiguous(), w, b)
            assert same_bits(g1, glo[e:e + 1])
            assert same_bits(lgu.gru.kan_heads(g1, grid, wpack), k[:, e:e + 1])
        again = lgu.gru.kangru_context(ins[0], w, b)
    assert same_bits(again, glo)


@pytest.mark.gpu
@pytest.mark.parametrize("half", [False, True])
def test_nan_in_one_edge_stays_in_that_edge(lgu, half):
    m, ins = gpu_case(33, 4, 12, 16, half=half)
    ins[0][2, 5, 3, 4] = float("nan")
    out, _ = fused(lgu, m, ins, half)
    want, _ = restated(m, ins, half)
    assert torch.equal(torch.isnan(out), torch.isnan(want))
    assert not torch.isnan(out[[0, 1, 3]]).any() and torch.isnan(out[2]).any()


class UpdateLike(torch.nn.Module):
    """The reference UpdateModule's data flow around its GRU (droid_net.py:100-122), without the encoders."""

    def __init__(self):
        super().__init__()
        self.gru = R.RefGRU()
        self.delta = torch.nn.Conv2d(128, 2, 3, padding=1)

    def forward(self, net, inp, corr, flow):
        batch, num, ch, ht, wd = net.shape
        net = net.view(batch * num, -1, ht, wd)
        inp, corr, flow = (t.view(batch * num, -1, ht, wd) for t in (inp, corr, flow))
        net = self.gru(net, inp, corr, flow)
        return net.view(batch, num, -1, ht, wd), self.delta(net)


@pytest.mark.gpu
def test_installed_update_module_reaches_the_fused_path(lgu, capsys):
    um = UpdateLike()
    R.set_weights(um.gru, 1044)
    um = um.to(DEV)
    ins = [t.to(DEV).half().unsqueeze(0) for t in R.make_inputs(44, 5, 24, 32)]
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        want, _ = um(*ins)
        wr = lgu.gru.install(um.gru)
        got, _ = um(*ins)
    assert wr.fused_calls == 1 and got.shape == want.shape
    assert float((got.double() - want.double()).abs().max()) <= HALF_ABS_CAP
    lgu.gru.uninstall(um.gru)
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        um(*ins)
    assert wr.fused_calls == 1


@pytest.mark.gpu
def test_grad_mode_with_trainable_parameters_takes_the_module_path(lgu):
    m, ins = gpu_case(45, 2, 12, 16)
    wr = lgu.gru.install(m)
    out = m(*ins)
    assert wr.fused_calls == 0 and out.requires_grad
    out.sum().backward()
    assert m.kanz_glo.spline_weight.grad is not None and m.convz.weight.grad is not None
    with torch.autocast("cuda", dtype=torch.bfloat16), torch.no_grad():
        m(*ins)
    assert wr.fused_calls == 0
    with torch.no_grad():
        m(*ins)
    assert wr.fused_calls == 1
    lgu.gru.uninstall(m)


@pytest.mark.gpu
def test_load_state_dict_and_in_place_grid_changes_are_followed(lgu):
    m, ins = gpu_case(46, 3, 12, 16)
    wr = lgu.gru.install(m)
    with torch.no_grad():
        first = m(*ins)
        other = R.set_weights(R.RefGRU(), 999)
        m.load_state_dict(other.state_dict())
        second = m(*ins)
        want2 = R.forward(m, *ins)
        m.kanq_glo.grid.mul_(0.8)
        third = m(*ins)
        want3 = R.forward(m, *ins)
    assert wr.fused_calls == 3
    assert not torch.equal(first, second) and not torch.equal(second, third)
    assert float((second - want2).abs().max()) < 1e-4 and float((third - want3).abs().max()) < 1e-4
    lgu.gru.uninstall(m)


@pytest.mark.gpu
def test_graph_capture_and_side_stream_equal_eager(lgu):
    m, ins = gpu_case(47, 4, 24, 32, half=True)
    wr = lgu.gru.KanBiasGRU(m)
    eager, _ = fused(lgu, m, ins, True, wr)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        side, _ = fused(lgu, m, ins, True, wr)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    assert same_bits(side, eager)
    g = torch.cuda.CUDAGraph()
    s2 = torch.cuda.Stream()
    s2.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s2):
        fused(lgu, m, ins, True, wr)                     # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(s2)
    with torch.cuda.graph(g):
        cap, _ = fused(lgu, m, ins, True, wr)
    g.replay()
    torch.cuda.synchronize()
    assert same_bits(cap, eager)
