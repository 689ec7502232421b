"""The four backward operators (defCorr_index_backward, corr_index_backward, gaussianMask_backward, altcorr_backward)
against the float64 restatements of tests/backward_restatement.py, element by element, at the shapes where a scatter
kernel goes wrong: targets that differ from the source grid, odd widths, a 1x1 slice, tap boxes that leave LDS for
global atomics, radii whose taps need several passes of the wave, every channel-count dispatch of the altcorr kernel,
windows that straddle or miss the slice.

Bounds: |got - ref64| <= K * 2^-24 * A per element, K and A as derived in the restatement module's docstring; exactly 0
where the reference is structurally 0.  The first half of the file runs on the CPU: it holds the sequential fp32 C
oracle to the same bounds on every input set the GPU tests use (so the restatement restates the reference's formulas
and a correct fp32 implementation fits), and counts which code path of the kernel every input set takes.  Every check
prints `RATIO <side> <output> <largest err / (2^-24 A)> / <K>` (run with -s).
"""
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import backward_restatement as R  # noqa: E402

gpu = pytest.mark.gpu
U = R.U


# ---------------------------------------------------------------------------------------------------------------------
# shared checks: the same function judges the C oracle (CPU) and the HIP kernels (GPU)
# ---------------------------------------------------------------------------------------------------------------------
def within(side, what, got, ref, bound, A, K, ctx=""):
    got = np.asarray(got, np.float64).reshape(np.shape(ref))
    err = np.abs(got - ref)
    print("RATIO %s %s %.3f / %s %s" % (side, what, R.ratio(got, ref, A), K, ctx))
    bad = ~(err <= bound)      # NaN counts as bad
    if bad.any():
        k = np.unravel_index(np.argmax(np.where(bad, err - bound, -np.inf)), err.shape)
        pytest.fail("%s %s %s: %d of %d elements beyond their bound; worst at %s: got %r want %r bound %.3e (%d structural "
                    "zeros violated)" % (side, what, ctx, bad.sum(), bad.size, k, got[k], ref[k], bound[k],
                                         int((bad & (np.asarray(A) == 0)).sum())))


def check_sampler(side, case, refs, vg, og, pvg, ctx=""):
    ra, rp = refs
    K = R.k_vol(case["radius"])
    within(side, "volume_grad", vg, ra["volume_grad"], K * U * ra["A_vol"], ra["A_vol"], K, ctx)
    within(side, "offset_grad", og, ra["offset_grad"], R.K_OFF * U * ra["A_off"], ra["A_off"], R.K_OFF, ctx)
    within(side, "plain_volume_grad", pvg, rp["volume_grad"], K * U * rp["A_vol"], rp["A_vol"], K, ctx)


def check_gauss(side, refs, mg, cg, nt, ctx=""):
    within(side, "means_grad", mg, refs["means_grad"], refs["bound_means"], refs["A_means"], "(12+%d)+5|f|" % nt, ctx)
    within(side, "covs_grad", cg, refs["covs_grad"], refs["bound_covs"], refs["A_covs"], "(12+%d)+5|f|" % nt, ctx)


def check_altcorr(side, case, refs, f1g, f2g, ctx=""):
    S = case["coords"].shape[1]
    within(side, "fmap1_grad", f1g, refs["fmap1_grad"], refs["bound_f1"], refs["A_f1"], R.k_f1(S, case["radius"]), ctx)
    within(side, "fmap2_grad", f2g, refs["fmap2_grad"], refs["bound_f2"], refs["A_f2"], "N+8<=%d" % (refs["N"].max() + 8), ctx)


def zeroed_centre(case):
    want = case["offset"].copy()
    want[:, :, :, case["radius"], case["radius"], :] = 0.0
    return want


def oracle_sampler(oracle, case):
    off = case["offset"].copy()
    vg, og = oracle.defCorr_index_backward(case["volume"], case["coords"], off, case["corr_grad"], case["radius"])
    pvg, = oracle.corr_index_backward(case["volume"], case["coords"], case["corr_grad"], case["radius"])
    return vg, og, pvg, off


BATCH_SAMPLER = (150, 3, 5, 7, 9, 11, 3, 2.0, 3.0)     # seed, E, H1, W1, H2, W2, radius, sigma, offset scale
BATCH_GAUSS = ((3, 5, 7, 9, 10), 4)
BATCH_ALTCORR = (160, 3, 2, 5, 7, 6, 8, 96, 3, 3.0)    # seed, B, S, H1, W1, H2, W2, C, radius, sigma


def batch_sampler_case():
    return R.make_sampler_inputs(np.random.default_rng(BATCH_SAMPLER[0]), *BATCH_SAMPLER[1:])


def batch_gauss_case():
    c = R.make_gauss_inputs(np.random.default_rng(151), BATCH_GAUSS[0], BATCH_GAUSS[1] + 1.0)
    c["radius"] = BATCH_GAUSS[1]
    return c


def batch_altcorr_case():
    return R.make_altcorr_inputs(np.random.default_rng(BATCH_ALTCORR[0]), *BATCH_ALTCORR[1:])


def edge_of(case, e):
    return {k: (np.ascontiguousarray(v[e:e + 1]) if isinstance(v, np.ndarray) else v) for k, v in case.items()}


GAUSS_PARAMS = [(s, r, False) for s in R.GAUSS_SHAPES for r in R.GAUSS_RADII] + [(R.GAUSS_SHAPES[1], 4, True)]
GAUSS_IDS = ["%dx%d_r%d%s" % (s[3], s[4], r, "_outside" if o else "") for s, r, o in GAUSS_PARAMS]


# ---------------------------------------------------------------------------------------------------------------------
# CPU: the restatements restate the reference, and the sequential fp32 oracle fits the bounds
# ---------------------------------------------------------------------------------------------------------------------
def _oracle_vs_sampler_refs(oracle, case, refs, ctx=""):
    vg, og, pvg, off = oracle_sampler(oracle, case)
    check_sampler("oracle", case, refs, vg, og.reshape(refs[0]["offset_grad"].shape), pvg, ctx)
    assert np.array_equal(vg != 0, refs[0]["volume_grad"] != 0), "zero pattern of volume_grad"
    assert np.array_equal(pvg != 0, refs[1]["volume_grad"] != 0), "zero pattern of the plain volume_grad"
    assert np.array_equal(refs[0]["volume_grad"] != 0, refs[0]["A_vol"] != 0)
    assert np.array_equal(off, zeroed_centre(case))
    fwd, = oracle.defCorr_index_forward(case["volume"], case["coords"], case["offset"].copy(), case["radius"])
    within("oracle", "sampler_forward", fwd, refs[0]["fwd"], R.K_FWD * U * refs[0]["A_fwd"], refs[0]["A_fwd"], R.K_FWD, ctx)


@pytest.mark.parametrize("name", list(R.SAMPLER_CASES))
def test_sampler_restatement_and_oracle_agree(oracle, name):
    _oracle_vs_sampler_refs(oracle, R.sampler_case(name), R.sampler_case_refs(name), name)


@pytest.mark.parametrize("seed", list(range(8)))
def test_sampler_restatement_and_oracle_agree_on_the_random_inputs(oracle, seed):
    desc, case = R.random_sampler_case(seed)
    _oracle_vs_sampler_refs(oracle, case, R.sampler_refs(case), str(desc))


def test_sampler_restatement_and_oracle_agree_on_the_batch_inputs(oracle):
    case = batch_sampler_case()
    _oracle_vs_sampler_refs(oracle, case, R.sampler_refs(case), "batch")


def _oracle_vs_gauss_refs(oracle, case, refs, ctx=""):
    mg, cg = oracle.gaussianMask_backward(case["means"], case["covs"], case["volume"], case["grad"], case["radius"])
    check_gauss("oracle", refs, mg, cg, (2 * case["radius"] + 1) ** 2, ctx)
    fwd, = oracle.gaussianMask(case["means"], case["covs"], case["volume"], case["radius"])
    want = R.gaussmask_forward64(*(torch.from_numpy(case[k]).double() for k in ("means", "covs", "volume")), case["radius"]).numpy()
    assert np.abs(fwd - want).max() <= 1e-5     # the forward restatement is the reference's window, too


@pytest.mark.parametrize("shape,radius,outside", GAUSS_PARAMS, ids=GAUSS_IDS)
def test_gauss_restatement_and_oracle_agree(oracle, shape, radius, outside):
    case, refs = R.gauss_case(shape, radius, outside), R.gauss_case_refs(shape, radius, outside)
    _oracle_vs_gauss_refs(oracle, case, refs, GAUSS_IDS[GAUSS_PARAMS.index((shape, radius, outside))])
    if outside:
        assert not refs["means_grad"].any() and not refs["covs_grad"].any() and not refs["bound_means"].any()
    else:   # windows straddle every border of the slice, and some lie inside it
        cx, cy = np.floor(case["means"][..., 0]), np.floor(case["means"][..., 1])
        H2, W2 = shape[3:]
        assert (cx - radius < 0).any() and (cx + radius >= W2).any() and (cy - radius < 0).any() and (cy + radius >= H2).any()
        assert refs["A_means"].any() and refs["A_covs"].any()


def test_gauss_restatement_and_oracle_agree_on_the_batch_inputs(oracle):
    case = batch_gauss_case()
    refs = R.gaussmask_backward64(case["means"], case["covs"], case["volume"], case["grad"], case["radius"])
    _oracle_vs_gauss_refs(oracle, case, refs, "batch")


def _oracle_vs_altcorr_refs(oracle, case, refs, ctx=""):
    f1g, f2g, cg = oracle.altcorr_backward(case["fmap1"], case["fmap2"], case["coords"], case["corr_grad"], case["radius"])
    check_altcorr("oracle", case, refs, f1g, f2g, ctx)
    assert np.array_equal(f2g != 0, refs["fmap2_grad"] != 0) and not cg.any()
    fwd, = oracle.altcorr_forward(case["fmap1"], case["fmap2"], case["coords"], case["radius"])
    within("oracle", "altcorr_forward", fwd, refs["fwd"], refs["bound_fwd"], refs["A_fwd"], R.k_afwd(case["fmap1"].shape[-1]), ctx)


@pytest.mark.parametrize("name", list(R.ALTCORR_CASES))
def test_altcorr_restatement_and_oracle_agree(oracle, name):
    refs = R.altcorr_case_refs(name)
    _oracle_vs_altcorr_refs(oracle, R.altcorr_case(name), refs, name)
    if name == "far_outside":
        assert not refs["fmap1_grad"].any() and not refs["fmap2_grad"].any() and not refs["N"].any()
    else:   # lattice points fall outside fmap2 on some pixels and inside on others
        B, H2, W2, _ = R.altcorr_case(name)["fmap2"].shape
        S, rl = R.altcorr_case(name)["coords"].shape[1], 2 * R.altcorr_case(name)["radius"] + 2
        n_in = refs["N"].sum()
        assert 0 < n_in < R.altcorr_case(name)["fmap1"][..., 0].size * S * rl * rl


@pytest.mark.parametrize("seed", list(range(8)))
def test_altcorr_restatement_and_oracle_agree_on_the_random_inputs(oracle, seed):
    desc, case = R.random_altcorr_case(seed)
    _oracle_vs_altcorr_refs(oracle, case, R.altcorr_refs(case), str(desc))


def test_altcorr_restatement_and_oracle_agree_on_the_batch_inputs(oracle):
    case = batch_altcorr_case()
    _oracle_vs_altcorr_refs(oracle, case, R.altcorr_refs(case), "batch")


# ---------------------------------------------------------------------------------------------------------------------
# CPU: which path of defcorr_bwd_kernel every input set takes, so that no GPU test passes vacuously
# ---------------------------------------------------------------------------------------------------------------------
def _paths(name):
    case = R.sampler_case(name)
    H2, W2 = case["volume"].shape[3:]
    return R.tap_paths(case["coords"], case["offset"], case["radius"], H2, W2)


@pytest.mark.parametrize("name", R.LARGE_BOX_CASES)
def test_large_box_cases_reach_the_global_atomics_branch(name):
    p = _paths(name)
    live = (p["nvalid"] > 0).any(1)
    large = (p["box"] > R.BW_BOX_FLOATS).any(1)
    print(name, "pixels with a valid tap:", int(live.sum()), "through a box > 1024:", int(large.sum()))
    assert large.sum() * 4 >= live.sum() > 0


@pytest.mark.parametrize("name", [n for n in R.SAMPLER_CASES if n not in R.LARGE_BOX_CASES])
def test_ordinary_cases_stay_in_the_lds_box(name):
    p = _paths(name)
    assert not (p["box"] > R.BW_BOX_FLOATS).any()
    if name == "far_outside":
        assert not p["nvalid"].any()
    else:
        assert p["nvalid"].any()


@pytest.mark.parametrize("name", R.BORDER_CASES)
def test_border_cases_touch_and_cross_every_border(name):
    p = _paths(name)
    for k in ("last_col", "last_row", "rej_left", "rej_right", "rej_top", "rej_bottom"):
        assert p[k] > 0, (name, k)


def test_multi_pass_cases_have_valid_taps_in_every_pass_and_mix_the_two_branches():
    for name, passes in (("radius4", 2), ("radius7", 4), ("radius5_large_box", 2)):
        p = _paths(name)
        assert p["nvalid"].shape[1] == passes and (p["nvalid"] > 0).any(0).all(), name
        # later passes revisit elements that an earlier pass of the same pixel wrote: some pixel is live in all passes
        assert (p["nvalid"] > 0).all(1).any(), name
    p = _paths("radius5_large_box")
    in_box = (p["nvalid"] > 0) & (p["box"] <= R.BW_BOX_FLOATS)
    in_atomics = p["box"] > R.BW_BOX_FLOATS
    assert (in_box.any(1) & in_atomics.any(1)).any(), "no pixel sends one pass through the box and another through atomics"
    assert (in_box[:, 0] & in_atomics[:, 1]).any() or (in_atomics[:, 0] & in_box[:, 1]).any()


def test_offset_scale_decides_the_branch_at_the_large_box_shape():
    """5x7 source pixels in the middle of a 40x48 slice: offsets 20*tanh put a good part of the pixels through the
    large box, offsets 4*tanh none."""
    for osc, expect in ((20.0, True), (4.0, False)):
        case = R.make_sampler_inputs(np.random.default_rng(104), 1, 5, 7, 40, 48, 3, 3.0, osc, 1.0, 16.0)
        p = R.tap_paths(case["coords"], case["offset"], 3, 40, 48)
        assert bool((p["box"] > R.BW_BOX_FLOATS).any()) == expect


def test_random_inputs_cover_both_branches_and_several_passes():
    large = passes = boxed = 0
    for seed in range(8):
        desc, case = R.random_sampler_case(seed)
        p = R.tap_paths(case["coords"], case["offset"], desc["radius"], desc["H2"], desc["W2"])
        large += int((p["box"] > R.BW_BOX_FLOATS).any())
        boxed += int(((p["nvalid"] > 0) & (p["box"] <= R.BW_BOX_FLOATS)).any())
        passes += int(p["nvalid"].shape[1] > 1 and (p["nvalid"][:, 1:] > 0).any())
    assert boxed and passes, (large, boxed, passes)


# ---------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------
def dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()


def host(t):
    return t.detach().cpu().numpy()


@pytest.fixture
def native(lgu):
    assert torch.cuda.is_available(), "these tests need the MI355X"
    assert os.path.exists(lgu._lib.so_path()), "liblgu_corr.so missing — run __graft_entry__.build()"
    lgu._lib.load()
    return lgu


def gpu_sampler(lgu, case):
    v, c, g, r = dev(case["volume"]), dev(case["coords"]), dev(case["corr_grad"]), case["radius"]
    o = dev(case["offset"])
    vg, og = lgu.ops.defCorr_index_backward(v, c, o, g, r)
    pvg, = lgu.ops.corr_index_backward(v, c, g, r)
    torch.cuda.synchronize()
    return host(vg), host(og).reshape(case["offset"].shape), host(pvg), host(o)


def _sampler_adjoint(lgu, case, refs, vg, pvg):
    """<forward(v), g> == <v, volume_grad> with the project's own forward kernels, in float64, within the sum of the
    per-element bounds of the two sides."""
    v, c, g, r = dev(case["volume"]), dev(case["coords"]), dev(case["corr_grad"]), case["radius"]
    fwd, = lgu.ops.defCorr_index_forward(v, c, dev(case["offset"]), r)
    pfwd, = lgu.ops.corr_index_forward(v, c, r)
    v64, g64 = case["volume"].astype(np.float64), case["corr_grad"].astype(np.float64)
    K = R.k_vol(r)
    for what, f, grad, ref in (("defCorr", fwd, vg, refs[0]), ("plain", pfwd, pvg, refs[1])):
        lhs = float((host(f).astype(np.float64) * g64).sum())
        rhs = float((v64 * grad.astype(np.float64)).sum())
        tol = float((np.abs(g64) * R.K_FWD * U * ref["A_fwd"]).sum() + (np.abs(v64) * K * U * ref["A_vol"]).sum())
        print("ADJOINT %s |lhs - rhs| = %.3e, allowed %.3e, scale %.3e" % (what, abs(lhs - rhs), tol, abs(lhs)))
        assert abs(lhs - rhs) <= tol, (what, lhs, rhs, tol)


@gpu
@pytest.mark.parametrize("name", list(R.SAMPLER_CASES))
def test_sampler_backward_against_float64(native, name):
    case, refs = R.sampler_case(name), R.sampler_case_refs(name)
    vg, og, pvg, off = gpu_sampler(native, case)
    check_sampler("HIP", case, refs, vg, og, pvg, name)
    assert not vg[refs[0]["volume_grad"] == 0].any() and not pvg[refs[1]["volume_grad"] == 0].any()
    assert np.array_equal(off, zeroed_centre(case)), "the caller's offsets: centre zeroed, the rest untouched"
    if name == "far_outside":
        assert not vg.any() and not og.any() and not pvg.any()
    _sampler_adjoint(native, case, refs, vg, pvg)


@gpu
@pytest.mark.parametrize("shape,radius,outside", GAUSS_PARAMS, ids=GAUSS_IDS)
def test_gaussian_mask_backward_against_float64(native, shape, radius, outside):
    case, refs = R.gauss_case(shape, radius, outside), R.gauss_case_refs(shape, radius, outside)
    mg, cg = native.ops.gaussianMask_backward(dev(case["means"]), dev(case["covs"]), dev(case["volume"]), dev(case["grad"]), radius)
    check_gauss("HIP", refs, host(mg), host(cg), (2 * radius + 1) ** 2, GAUSS_IDS[GAUSS_PARAMS.index((shape, radius, outside))])
    if outside:
        assert not host(mg).any() and not host(cg).any()


def gpu_altcorr(lgu, case):
    f1, f2, c, g = (dev(case[k]) for k in ("fmap1", "fmap2", "coords", "corr_grad"))
    f1g, f2g, cg = lgu.ops.altcorr_backward(f1, f2, c, g, case["radius"])
    torch.cuda.synchronize()
    return host(f1g), host(f2g), host(cg)


@gpu
@pytest.mark.parametrize("name", list(R.ALTCORR_CASES))
def test_altcorr_backward_against_float64(native, name):
    case, refs = R.altcorr_case(name), R.altcorr_case_refs(name)
    f1g, f2g, cg = gpu_altcorr(native, case)
    check_altcorr("HIP", case, refs, f1g, f2g, name)
    assert not cg.any() and cg.shape == case["coords"].shape
    if name == "far_outside":
        assert not f1g.any() and not f2g.any()
    # adjoint identity against the project's forward kernels: the forward is linear in each feature map
    f1_64, f2_64, g64 = (case[k].astype(np.float64) for k in ("fmap1", "fmap2", "corr_grad"))
    for variant in (0, 2):
        os.environ["LGU_LOWMEM_VARIANT"] = str(variant)
        try:
            fwd, = native.ops.altcorr_forward(dev(case["fmap1"]), dev(case["fmap2"]), dev(case["coords"]), case["radius"])
            lhs = float((host(fwd).astype(np.float64) * g64).sum())
        finally:
            os.environ.pop("LGU_LOWMEM_VARIANT", None)
        ftol = float((np.abs(g64) * refs["bound_fwd"]).sum())
        for what, rhs, tol in (("fmap1", float((f1_64 * f1g).sum()), float((np.abs(f1_64) * refs["bound_f1"]).sum())),
                               ("fmap2", float((f2_64 * f2g).sum()), float((np.abs(f2_64) * refs["bound_f2"]).sum()))):
            print("ADJOINT altcorr variant %d %s |lhs - rhs| = %.3e, allowed %.3e" % (variant, what, abs(lhs - rhs), ftol + tol))
            assert abs(lhs - rhs) <= ftol + tol, (variant, what, lhs, rhs)


# ---- outputs fully written, nothing outside them -------------------------------------------------------------------
_SENT = 1234.5


def _banded(shape, guard=4096):
    n = int(np.prod(shape))
    big = torch.full((n + 2 * guard,), _SENT, dtype=torch.float32, device="cuda")
    return big, big[guard:guard + n].view(shape), guard


def _bands_intact(big, guard):
    return bool((big[:guard] == _SENT).all()) and bool((big[-guard:] == _SENT).all())


@gpu
@pytest.mark.parametrize("name", ["odd_target", "large_box", "radius4"])
def test_sampler_backward_entry_points_write_all_of_their_outputs_and_nothing_else(native, name):
    """The C entry points called as ops.py calls them, with offset_grad in sentinel-filled memory (the operator hands
    the kernel torch.empty: every element, out-of-bounds taps included, must be written) and the caller-zeroed
    volume_grad between sentinel bands."""
    case, refs = R.sampler_case(name), R.sampler_case_refs(name)
    L, P = native._lib.load(), native.ops._ptr
    v, c, g, r = dev(case["volume"]), dev(case["coords"]), dev(case["corr_grad"]), case["radius"]
    E, H1, W1, H2, W2 = v.shape
    obig, o, og_ = _banded(case["offset"].shape)
    o.copy_(dev(case["offset"]))
    gbig, og, gg = _banded(case["offset"].shape)
    vbig, vg, vgd = _banded(v.shape)
    pbig, pvg, pgd = _banded(v.shape)
    vg.zero_()
    pvg.zero_()
    st = native.ops._stream(v)
    native._lib.check(L.lgu_defcorr_bwd_f32(P(v), P(c), P(o), P(g), P(vg), P(og), E, H1, W1, H2, W2, r, st), "defcorr_bwd")
    native._lib.check(L.lgu_corridx_bwd_f32(P(v), P(c), P(g), P(pvg), E, H1, W1, H2, W2, r, st), "corridx_bwd")
    torch.cuda.synchronize()
    assert not bool((og == _SENT).any()), "offset_grad has elements the kernel never wrote"
    assert not bool((vg == _SENT).any()) and not bool((pvg == _SENT).any())
    for big, gd in ((obig, og_), (gbig, gg), (vbig, vgd), (pbig, pgd)):
        assert _bands_intact(big, gd), "a kernel wrote outside the tensor it was given"
    check_sampler("HIP", case, refs, host(vg), host(og), host(pvg), name + " banded")
    assert np.array_equal(host(o), zeroed_centre(case))


@gpu
@pytest.mark.parametrize("name", ["c32_r3", "c96_r3", "c160_r1"])
def test_altcorr_backward_entry_point_writes_all_of_fmap1_grad_and_nothing_else(native, name):
    case, refs = R.altcorr_case(name), R.altcorr_case_refs(name)
    L, P = native._lib.load(), native.ops._ptr
    f1, f2, c, g = (dev(case[k]) for k in ("fmap1", "fmap2", "coords", "corr_grad"))
    B, S, H1, W1, _ = c.shape
    _, H2, W2, C = f2.shape
    big1, f1g, g1 = _banded(f1.shape)
    big2, f2g, g2 = _banded(f2.shape)
    f2g.zero_()
    rc = L.lgu_altcorr_bwd_f32(P(f1), P(f2), P(c), P(g), P(f1g), P(f2g), B, S, H1, W1, H2, W2, C, case["radius"],
                               native.ops._stream(f1))
    native._lib.check(rc, "altcorr_bwd")
    torch.cuda.synchronize()
    assert not bool((f1g == _SENT).any()), "fmap1_grad has elements the kernel never wrote"
    assert not bool((f2g == _SENT).any())
    assert _bands_intact(big1, g1) and _bands_intact(big2, g2), "the kernel wrote outside the tensor it was given"
    check_altcorr("HIP", case, refs, host(f1g), host(f2g), name + " banded")


@gpu
def test_gaussian_mask_backward_entry_point_writes_all_of_its_outputs_and_nothing_else(native):
    shape, radius = R.GAUSS_SHAPES[1], 5
    case, refs = R.gauss_case(shape, radius), R.gauss_case_refs(shape, radius)
    L, P = native._lib.load(), native.ops._ptr
    m, c, v, g = (dev(case[k]) for k in ("means", "covs", "volume", "grad"))
    E, H1, W1, H2, W2 = shape
    mbig, mg, gm = _banded(m.shape)
    cbig, cg, gc = _banded(c.shape)
    rc = L.lgu_gaussmask_bwd_f32(P(m), P(c), P(v), P(g), P(mg), P(cg), E, H1, W1, H2, W2, radius, native.ops._stream(v))
    native._lib.check(rc, "gaussmask_bwd")
    torch.cuda.synchronize()
    assert not bool((mg == _SENT).any()) and not bool((cg == _SENT).any())
    assert _bands_intact(mbig, gm) and _bands_intact(cbig, gc)
    check_gauss("HIP", refs, host(mg), host(cg), (2 * radius + 1) ** 2, "banded")


# ---- batch independence ---------------------------------------------------------------------------------------------
def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@gpu
def test_sampler_backward_edges_are_independent(native):
    case = batch_sampler_case()
    refs = R.sampler_refs(case)
    vg, og, pvg, _ = gpu_sampler(native, case)
    check_sampler("HIP", case, refs, vg, og, pvg, "batch")
    K = R.k_vol(case["radius"])
    for e in range(case["volume"].shape[0]):
        vg1, og1, pvg1, _ = gpu_sampler(native, edge_of(case, e))
        assert np.array_equal(_bits(og1[0]), _bits(og[e])), "offset_grad of edge %d depends on the batch" % e
        for got, ref in ((vg1, refs[0]), (pvg1, refs[1])):
            within("HIP", "volume_grad", got[0], ref["volume_grad"][e], K * U * ref["A_vol"][e], ref["A_vol"][e], K, "edge %d alone" % e)


@gpu
def test_gaussian_mask_backward_edges_are_independent(native):
    case = batch_gauss_case()
    run = lambda c: [host(t) for t in native.ops.gaussianMask_backward(dev(c["means"]), dev(c["covs"]), dev(c["volume"]),
                                                                       dev(c["grad"]), c["radius"])]
    mg, cg = run(case)
    refs = R.gaussmask_backward64(case["means"], case["covs"], case["volume"], case["grad"], case["radius"])
    check_gauss("HIP", refs, mg, cg, (2 * case["radius"] + 1) ** 2, "batch")
    for e in range(case["volume"].shape[0]):
        mg1, cg1 = run(edge_of(case, e))
        assert np.array_equal(_bits(mg1[0]), _bits(mg[e])) and np.array_equal(_bits(cg1[0]), _bits(cg[e])), e


@gpu
def test_altcorr_backward_batch_items_are_independent(native):
    case = batch_altcorr_case()
    refs = R.altcorr_refs(case)
    f1g, f2g, _ = gpu_altcorr(native, case)
    check_altcorr("HIP", case, refs, f1g, f2g, "batch")
    for b in range(case["fmap1"].shape[0]):
        f1g1, f2g1, _ = gpu_altcorr(native, edge_of(case, b))
        assert np.array_equal(_bits(f1g1[0]), _bits(f1g[b])), "fmap1_grad of batch item %d depends on the batch" % b
        within("HIP", "fmap2_grad", f2g1[0], refs["fmap2_grad"][b], refs["bound_f2"][b], refs["A_f2"][b], "N+8", "item %d alone" % b)


# ---- randomized differential ----------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("seed", list(range(8)))
def test_randomized_differential_sampler_backward(native, seed):
    desc, case = R.random_sampler_case(seed)
    vg, og, pvg, off = gpu_sampler(native, case)
    check_sampler("HIP", case, R.sampler_refs(case), vg, og, pvg, "seed %d %s" % (seed, desc))
    assert np.array_equal(off, zeroed_centre(case)), desc


@gpu
@pytest.mark.parametrize("seed", list(range(8)))
def test_randomized_differential_altcorr_backward(native, seed):
    desc, case = R.random_altcorr_case(seed)
    f1g, f2g, cg = gpu_altcorr(native, case)
    check_altcorr("HIP", case, R.altcorr_refs(case), f1g, f2g, "seed %d %s" % (seed, desc))
    assert not cg.any(), desc
