"""CorrBlock in the mode the reference runs it in: built and called inside float16 autocast on half feature maps
(factor_graph.py decorates add_factors / rm_factors / update with autocast(enabled=True); video.fmaps is half).

`tests/golden/glue_corrblock_autocast_16x16_*.npz` hold what the reference's unchanged corr.py / gaussianMask_cuda.py
produced on the inputs of glue_corrblock_16x16 inside `cuda_autocast_on_cpu()` of oracle/gen_glue_golden.py: CPU float16
autocast with the GPU's policy emulated for the one operator of the glue whose policy differs between the two devices
(nearest upsampling: fp32 on the GPU, left half on the CPU).  `glue_autocast_policy.json` is the audit behind "the one":
every aten operator the scenario executed, with whether the dispatcher holds an AutocastCPU / AutocastCUDA kernel for it.

CPU tests: the installed torch still shows that split; this build's torch compositions under the same emulation equal the
fixture (half tensors bit for bit, float tensors to fp32 round-off, dtypes from the fixture's table); the half
denominator of the Gaussian head is visible in the stored pyramid; the fixture is what the generator produces.

GPU tests (-m gpu): the fused builder and the fused offset post-processing given the reference's own half inputs, the raw
offset heads against the reference's raw half convolutions, and the whole life under torch.autocast("cuda") for both pyramid layouts and both builders, held to the YARDSTICK
    e_ref[k] = max |autocast fixture[k] - fp32 fixture[k]|
— the movement the reference's own half roundings cause, computed here from the two committed fixtures.  A correct half
run and the fixture both sit within that noise of the exact value, so they are within 2 * e_ref[k] of each other
(triangle inequality).  Lookups: q = the (1 - 1e-4)-quantile of |out_autocast - out_fp32|, tolerance 2 q with at most
2e-4 of the entries outside (whole-tap border flips, the cap tests/test_glue_reference.py uses).
Every measured distance is printed next to its bound (`pytest -s`)."""
import functools
import json
import math
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests.test_glue_reference import GOLD, REF, T, _gen, _require_gpu, _rowmajor_levels, build_heads, gold

needs_ref = pytest.mark.skipif(not os.path.isdir(REF), reason="reference checkout not present on this machine")
NAME = "glue_corrblock_autocast_16x16"


@functools.lru_cache(maxsize=None)
def auto():
    """The autocast fixture: its parts (stored apart to keep every committed file small) merged into one dict."""
    z = {}
    for part in _gen().AUTOCAST_PARTS:
        p = np.load(os.path.join(GOLD, "%s_%s.npz" % (NAME, part)), allow_pickle=False)
        assert not set(p.files) & set(z)
        z.update({k: p[k] for k in p.files})
    return z


@functools.lru_cache(maxsize=None)
def policy():
    with open(os.path.join(GOLD, "glue_autocast_policy.json")) as fh:
        return json.load(fh)


def dtype_table():
    return dict(e.split("=") for e in auto()["dtypes"])


def name_of(dtype):
    return str(dtype).replace("torch.", "")


def half_maps(z, device="cpu"):
    """(fmap1, fmap2) of the fp32 fixture as the half tensors they are stored as, (1,E,128,h,w)."""
    assert z["fmap1"].dtype == np.float16 and z["fmap2"].dtype == np.float16
    return T(z["fmap1"], device), T(z["fmap2"], device)


def half_ulp(scale):
    return 2.0 ** (math.floor(math.log2(max(scale, 2.0 ** -14))) - 10)


def same(got, key, what=None):
    """got == fixture[key] under the rule of its dtype: half bit for bit when the fixture was made by the installed torch
    (one half ulp at the tensor's scale otherwise), float to 1e-6 * scale; the dtype is the fixture's."""
    za, what = auto(), what or key
    want = T(za[key])
    assert name_of(got.dtype) == dtype_table()[key] == name_of(want.dtype), "%s: dtype %s, fixture %s" % (what, got.dtype, want.dtype)
    got = got.detach().reshape(want.shape)
    scale = float(want.float().abs().max())
    err = float((got.float() - want.float()).abs().max())
    if want.dtype == torch.float16:
        if policy()["torch"] == torch.__version__:
            assert torch.equal(got, want), "%s: not bit-equal, max err %.3g (scale %.3g)" % (what, err, scale)
        else:
            assert err <= half_ulp(scale), "%s: max err %.3g > one half ulp %.3g" % (what, err, half_ulp(scale))
    else:
        assert err <= 1e-6 * scale, "%s: max err %.3g > %.3g" % (what, err, 1e-6 * scale)


# ------------------------------------------------------------------------------------------------ CPU: policy
def test_the_installed_torch_has_the_recorded_autocast_policy_split():
    """The fixture stands for a GPU run only while CPU and GPU autocast cast the same operators of the glue, the emulated
    one (and those recorded as inert: cast on one device only, but only ever met with operands the cast leaves alone)
    excepted.  Read again from the installed torch's dispatcher, operator by operator."""
    gen, pol = _gen(), policy()
    allowed = set(pol["emulated"]) | set(pol["inert"])
    assert pol["emulated"] == ["aten::upsample_nearest2d"] == list(gen.EMULATED_OPS) and set(pol["inert"]) == set(gen.INERT_OPS)
    assert set(gen.COMPOSITE_ENTRY_POINTS) <= set(pol["ops"])
    for name, rec in sorted(pol["ops"].items()):
        cpu, cuda = gen.autocast_kernels(name)
        assert (cpu, cuda) == (rec["AutocastCPU"], rec["AutocastCUDA"]), \
            "%s: AutocastCPU %s / AutocastCUDA %s here, recorded %s" % (name, cpu, cuda, rec)
        assert cpu == cuda or name in allowed, "%s is cast on one device only and is not emulated" % name
    for name in pol["emulated"]:
        assert pol["ops"][name] == {"AutocastCPU": False, "AutocastCUDA": True}, name


def test_cuda_autocast_on_cpu_restores_interpolate_and_promotes_only_half_inputs():
    gen = _gen()
    import torch.nn.functional as F
    real = F.interpolate
    x = torch.arange(8.0).view(1, 2, 2, 2)
    with gen.cuda_autocast_on_cpu():
        assert F.interpolate is not real and torch.is_autocast_enabled("cpu")
        up = F.interpolate(x.half(), (4, 4))
        assert up.dtype == torch.float32 and torch.equal(up, real(x, (4, 4)))
        assert F.interpolate(x.double(), (4, 4)).dtype == torch.float64
    assert F.interpolate is real and not torch.is_autocast_enabled("cpu")
    with pytest.raises(ZeroDivisionError):
        with gen.cuda_autocast_on_cpu():
            1 / 0
    assert F.interpolate is real


# ------------------------------------------------------------------------------------------------ CPU: compositions
@pytest.mark.parametrize("blk", ["A", "B"])
def test_offset_heads_torch_composition_under_autocast_matches_the_reference(lgu, blk):
    """generate_offsets / finish_offsets == CorrBlock.fpn_offset_generate of the reference (corr.py:117-135) in half
    autocast: half convolutions, level 0 half at every step, level 1 fp32 from the promoted upsampling on."""
    gen, z, za = _gen(), gold("glue_corrblock_16x16"), auto()
    h, w, Ea = int(z["h"]), int(z["w"]), int(z["E_a"])
    f1, f2 = half_maps(z)
    sl = slice(0, Ea) if blk == "A" else slice(Ea, None)
    feats = torch.cat((f1[0, sl], f2[0, sl]), dim=1)
    ofsMap, ofs_residual, _ = build_heads(lgu, h, w)
    with torch.no_grad(), gen.cuda_autocast_on_cpu():
        same(ofsMap(feats), blk + "_raw_o0")
        same(ofs_residual(torch.nn.functional.avg_pool2d(feats, kernel_size=2, stride=2)), blk + "_raw_o1_low")
        offs, zero = lgu.corr.finish_offsets(T(za[blk + "_raw_o0"]), T(za[blk + "_raw_o1_low"]), 4)
        assert zero == [False, False, True, True]
        same(offs[0], blk + "_offset0_init", "level 0 from the reference's head outputs")
        same(offs[1], blk + "_offset1_init", "level 1 from the reference's head outputs")
        table = dtype_table()
        for l in (2, 3):
            assert float(offs[l].abs().max()) == 0.0 and name_of(offs[l].dtype) == table["%s built:offset[%d]" % (blk, l)]
        offs, _ = lgu.corr.generate_offsets(ofsMap, ofs_residual, feats, 4)
        same(offs[0], blk + "_offset0_init", "level 0 end to end")
        same(offs[1], blk + "_offset1_init", "level 1 end to end")


@pytest.mark.parametrize("blk", ["A", "B"])
def test_gaussian_head_torch_composition_under_autocast_matches_the_reference(lgu, blk):
    """GaussianMask.gaussian_parameters == the reference's GaussianMask.forward up to its kernel call in half autocast:
    half linear heads, half PCN / sigmoid / det, fp32 cov and mean (the grid is fp32, the learned shift half)."""
    gen, z, za = _gen(), gold("glue_corrblock_16x16"), auto()
    h, w, Ea = int(z["h"]), int(z["w"]), int(z["E_a"])
    f1, f2 = half_maps(z)
    sl = slice(0, Ea) if blk == "A" else slice(Ea, None)
    t = torch.cat((f1[0, sl], f2[0, sl]), dim=1).permute(0, 2, 3, 1).contiguous()
    _, _, GA = build_heads(lgu, h, w)
    with torch.no_grad(), gen.cuda_autocast_on_cpu():
        same(GA.map(t), blk + "_raw_map")
        tt = GA.mapA(t)
        same(GA.meanMap(tt), blk + "_raw_mean_ofs")
        same(GA.covMap(tt), blk + "_raw_cov")
        mean, cov, det = GA.gaussian_parameters(t)
        same(mean, blk + "_means", "mean handed to gaussianMask")
        same(cov, blk + "_covs", "cov handed to gaussianMask")
        same(det, blk + "_det")
        same(mean.view(1, -1, h, w, 2), blk + "_mean_n")
        same(2 * det.view(1, -1, h, w), blk + "_theta")
    table = dtype_table()
    assert name_of(mean.dtype) == table[blk + " built:mean_n"] and name_of((2 * det).dtype) == table[blk + " built:theta"]
    assert name_of(t.dtype) == table[blk + " built:t"]


def test_all_pairs_product_under_autocast_matches_the_reference(lgu):
    gen, z = _gen(), gold("glue_corrblock_16x16")
    Ea = int(z["E_a"])
    f1, f2 = half_maps(z)
    with torch.no_grad(), gen.cuda_autocast_on_cpu():
        same(lgu.CorrBlock.corr(f1[:, :Ea].contiguous(), f2[:, :Ea].contiguous()), "A_raw_product")
        same(lgu.CorrBlock.corr(f1[:, Ea:].contiguous(), f2[:, Ea:].contiguous()), "B_raw_product")


def test_the_half_denominator_is_visible_in_the_fixture(oracle):
    """level 0 = gaussianMask(means, covs, raw) / (6.28 * sqrt(det)) + raw (gaussianMask_cuda.py:84-86) with det HALF:
    the square root and the product are each rounded to half.  Formed from the stored means, covs, raw product and det
    with those two roundings it reproduces the stored level 0 to 1e-5 * scale; with the denominator evaluated in fp32
    it does not — so a builder that skipped the roundings would miss the 1e-5 bound of the GPU test below."""
    za = auto()
    E, h, w = za["A_means"].shape[:3]
    raw = za["A_raw_product"].reshape(E, h, w, h, w).astype(np.float32)
    g, = oracle.gaussianMask(np.ascontiguousarray(za["A_means"]), np.ascontiguousarray(za["A_covs"]), raw, 4)
    det = T(za["A_det"])
    assert det.dtype == torch.float16
    den_half = 6.28 * torch.sqrt(det)
    assert den_half.dtype == torch.float16
    want = za["A_pyr0"]
    scale = float(np.abs(want).max())
    with_roundings = (T(g) / den_half.view(E, h, w, 1, 1) + T(raw)).numpy()
    in_fp32 = (T(g) / (6.28 * torch.sqrt(det.float())).view(E, h, w, 1, 1) + T(raw)).numpy()
    assert with_roundings.dtype == np.float32
    e_half, e_f32 = float(np.abs(with_roundings - want).max()), float(np.abs(in_fp32 - want).max())
    print("AUTOCAST_PIN half denominator: with both roundings %.3g, in fp32 %.3g, bound %.3g" % (e_half, e_f32, 1e-5 * scale))
    assert e_half <= 1e-5 * scale, (e_half, scale)
    assert e_f32 > 1e-5 * scale, (e_f32, scale)


@needs_ref
def test_committed_autocast_fixture_is_what_the_generator_produces():
    gen = _gen()
    executed = set()
    fresh = gen.corrblock_autocast_scenario(16, 16, 2, 1, seed=101, inputs_of=gold("glue_corrblock_16x16"), executed=executed)
    z = auto()
    assert set(fresh) == set(z)
    for k in z:
        a, b = np.asarray(fresh[k]), z[k]
        assert a.shape == b.shape and a.dtype == b.dtype, k
        if a.dtype.kind == "f":
            assert np.abs(a.astype(np.float64) - b).max() <= 2e-5 * max(1.0, float(np.abs(b.astype(np.float64)).max())), k
        else:
            assert np.array_equal(a, b), k
    assert {k: gen.autocast_part_of(k) for k in z} == {k: part for part in gen.AUTOCAST_PARTS
                                                       for k in np.load(os.path.join(GOLD, "%s_%s.npz" % (NAME, part))).files}
    assert gen.autocast_policy(executed) == policy()


# ------------------------------------------------------------------------------------------------ GPU
def _no_centre(a):
    a = np.array(a, dtype=np.float32).reshape(a.shape[:-1] + (7, 7, 2))
    a[..., 3, 3, :] = 0
    return a.reshape(a.shape[:-3] + (98,))


def _np(t):
    return t.detach().float().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t, dtype=np.float32)


@functools.lru_cache(maxsize=None)
def yardstick():
    """e_ref[k] = max |autocast fixture[k] - fp32 fixture[k]| (offsets: centre tap zeroed on both sides, no operator reads
    it); q[k] for the lookups."""
    z, za = gold("glue_corrblock_16x16"), auto()
    e = {}
    for k in za:
        if k in z.files and za[k].dtype.kind == "f" and not k.startswith("out"):
            a, b = za[k].astype(np.float32), z[k].astype(np.float32)
            if "_offset" in k:
                a, b = _no_centre(a), _no_centre(b)
            e[k] = float(np.abs(a - b).max())
    q = {k: float(np.quantile(np.abs(za[k] - z[k]), 1 - 1e-4)) for k in ("out1", "out2", "out3")}
    return e, q


def held(got, key, what=None, offsets=False):
    """|got - autocast fixture[key]| <= 2 * e_ref[key], printed before it is asserted."""
    e, _ = yardstick()
    want, got = auto()[key].astype(np.float32), _np(got)
    assert got.shape == want.shape, "%s: shape %s != %s" % (key, got.shape, want.shape)
    if offsets:
        got, want = _no_centre(got), _no_centre(want)
    d = float(np.abs(got - want).max())
    print("AUTOCAST_PIN %-34s distance %.4g  e_ref %.4g  (%.2f e_ref, bound 2)" % (what or key, d, e[key], d / e[key]))
    assert d <= 2 * e[key], "%s: %.4g > 2 * e_ref = %.4g" % (what or key, d, 2 * e[key])


def held_lookup(got, key, what):
    _, q = yardstick()
    d = np.abs(_np(got) - auto()[key])
    frac = float((d > 2 * q[key]).mean())
    print("AUTOCAST_PIN %-34s outside 2q = %.4g: %.3g of the entries (cap 2e-4); 0.9999-quantile %.4g, max %.4g" % (
        what, 2 * q[key], frac, float(np.quantile(d, 1 - 1e-4)), float(d.max())))
    assert frac <= 2e-4, "%s: %.3g of the entries beyond 2q = %.4g" % (what, frac, 2 * q[key])


def half_representable(t):
    return torch.equal(t.float().half().float(), t.float())


@pytest.mark.gpu
@pytest.mark.parametrize("tiled", [True, False])
def test_fused_builder_given_the_reference_half_inputs(lgu, tiled):
    """ops.volume_pyramid on the reference's raw half product, means, covs and half det: everything behind those inputs
    is fp32 except the two elementwise, correctly rounded half steps of the denominator — 1e-5 * scale per level."""
    _require_gpu(lgu)
    za, d = auto(), "cuda"
    E, h, w = za["A_means"].shape[:3]
    raw = T(za["A_raw_product"], d).view(E, h, w, h, w).contiguous()
    det = T(za["A_det"], d).contiguous()
    assert raw.dtype == torch.float16 and det.dtype == torch.float16
    levels = lgu.ops.volume_pyramid(T(za["A_means"], d), T(za["A_covs"], d), raw, 4, 4, inplace=False, tiled=tiled, det=det)
    for l, lv in enumerate(levels):
        if tiled:
            lv = lgu.ops.volume_retile(lv.contiguous(), to_tiled=False, hw=(h >> l, w >> l))
        want = za["A_pyr%d" % l]
        scale = float(np.abs(want).max())
        err = float(np.abs(_np(lv) - want).max())
        print("AUTOCAST_PIN builder level %d (%s): max err %.3g, bound %.3g" % (l, "tiled" if tiled else "row-major", err, 1e-5 * scale))
        assert lv.dtype == torch.float32 and err <= 1e-5 * scale, (l, err, scale)


@pytest.mark.gpu
@pytest.mark.parametrize("blk", ["A", "B"])
def test_fused_half_offset_post_processing_given_the_reference_head_outputs(lgu, blk, monkeypatch):
    """lgu_offsets_finalize in its autocast mode on the reference's raw half convolution outputs against the reference's
    initial offsets, within the kernel's own bound (max <= 2^-7, mean <= 1e-4: bit-equal unless a statistic lands across
    a half rounding boundary); level 0 holds half values, level 1 is fp32."""
    _require_gpu(lgu)
    za, d = auto(), "cuda"
    ran = []
    real = lgu.ops.offsets_finalize
    monkeypatch.setattr(lgu.ops, "offsets_finalize", lambda *a, **k: (ran.append(1), real(*a, **k))[1])
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        offs, zero = lgu.corr.finish_offsets(T(za[blk + "_raw_o0"], d), T(za[blk + "_raw_o1_low"], d), 4)
    assert ran == [1] and zero == [False, False, True, True], "the fused post-processing must be what runs here"
    assert half_representable(offs[0]) and offs[1].dtype == torch.float32
    for l in range(2):
        dist = np.abs(_np(offs[l]) - auto()["%s_offset%d_init" % (blk, l)].astype(np.float32))
        print("AUTOCAST_PIN fused finish_offsets %s level %d: max %.4g (bound %.4g), mean %.3g (bound 1e-4)" % (
            blk, l, float(dist.max()), 2.0 ** -7, float(dist.mean())))
        assert float(dist.max()) <= 2.0 ** -7 and float(dist.mean()) <= 1e-4, (l, float(dist.max()), float(dist.mean()))


@pytest.mark.gpu
@pytest.mark.parametrize("blk", ["A", "B"])
def test_offset_heads_under_autocast_round_once_like_the_reference_half_convolution(lgu, blk, monkeypatch):
    """The two offset heads on half maps inside autocast (corr.py's matrix-core route, which must be what runs) against the
    reference's raw half convolution outputs.  Both are ONE rounding of an fp32 sum of the same exact products (half maps x
    weights rounded to half), the sums differing by their order only, so an entry either agrees or sits on the other side
    of one rounding boundary: at most one half ulp apart (taken at max(|x|, 2^-6): below that the fp32 summation error
    of the 2304 products is itself a half ulp), and at few entries — capped at the 2 % the project allows its half volume
    build against the library GEMM (test_gpu_parity.py::test_half_volume_build_...)."""
    _require_gpu(lgu)
    z, za, d = gold("glue_corrblock_16x16"), auto(), "cuda"
    h, w, Ea = int(z["h"]), int(z["w"]), int(z["E_a"])
    f1, f2 = half_maps(z, d)
    sl = slice(0, Ea) if blk == "A" else slice(Ea, None)
    feats = torch.cat((f1[0, sl], f2[0, sl]), dim=1)
    ofsMap, ofs_residual, _ = build_heads(lgu, h, w, d)
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        heads = lgu.corr._autocast_heads_on_matrix_cores(ofsMap, ofs_residual, feats)
    assert heads is not None, "the matrix-core heads must serve the production case"
    for got, key in zip(heads, (blk + "_raw_o0", blk + "_raw_o1_low")):
        want = T(za[key], d)
        assert got.dtype == torch.float16 and got.shape == want.shape
        ulp = torch.exp2(torch.floor(torch.log2(want.float().abs().clamp_min(2.0 ** -6))) - 10.0)
        dist = (got.float() - want.float()).abs()
        frac = float((dist > 0).float().mean())
        print("AUTOCAST_PIN heads %s: max %.3f half ulp (bound 1), differing %.4f of the entries (cap 0.02)" % (
            key, float((dist / ulp).max()), frac))
        assert bool((dist <= ulp).all()) and frac <= 0.02, (key, float((dist / ulp).max()), frac)


@pytest.mark.gpu
@pytest.mark.parametrize("inject", ["end_to_end", "reference_offsets"])
@pytest.mark.parametrize("fused_half", [False, True])
@pytest.mark.parametrize("tiled", [True, False])
def test_corrblock_life_under_autocast_against_the_reference_under_autocast(lgu, tiled, fused_half, inject, monkeypatch):
    """build A -> call -> build B -> cat -> call -> drop the middle edge -> call on the half maps inside
    torch.autocast("cuda", float16), as factor_graph.py drives the block, for both pyramid layouts and both builders
    (library half GEMM + fused post-processing; FUSED_BUILD_HALF: the matrix-core build, tiled layout only).
    reference_offsets: the reference's autocast offsets are injected after each build, which isolates the lookups."""
    _require_gpu(lgu)
    monkeypatch.setattr(lgu.CorrBlock, "TILED_PYRAMID", tiled)
    monkeypatch.setattr(lgu.CorrBlock, "FUSED_BUILD_HALF", fused_half)
    builders = []
    for fn in ("volume_build_pyramid", "volume_pyramid", "offset_conv_frames"):
        real = getattr(lgu.ops, fn)
        monkeypatch.setattr(lgu.ops, fn, lambda *a, _real=real, _fn=fn, **k: (builders.append(_fn), _real(*a, **k))[1])
    intended = "volume_build_pyramid" if (tiled and fused_half) else "volume_pyramid"
    z, za, table, d = gold("glue_corrblock_16x16"), auto(), dtype_table(), "cuda"
    h, w, Ea = int(z["h"]), int(z["w"]), int(z["E_a"])
    f1, f2 = half_maps(z, d)
    ofsMap, ofs_residual, GA = build_heads(lgu, h, w, d)
    exact = inject == "reference_offsets"

    def built(blk, tag):
        # both offset heads on the matrix cores, then the intended volume builder
        assert builders == ["offset_conv_frames"] * 2 + [intended] and blk._store is not None and blk._tiled == tiled, (builders, intended)
        del builders[:]
        assert name_of(blk.mean_n.dtype) == table[tag + " built:mean_n"] and name_of(blk.theta.dtype) == table[tag + " built:theta"]
        assert name_of(blk.offset[1].dtype) == table[tag + " built:offset[1]"] and half_representable(blk.offset[0])
        held(blk.mean_n, tag + "_mean_n")
        held(blk.theta, tag + "_theta")
        if not exact:
            held(blk.offset[0], tag + "_offset0_init", offsets=True)
            held(blk.offset[1], tag + "_offset1_init", offsets=True)
        else:
            blk.offset[0] = T(za[tag + "_offset0_init"], d).float()
            blk.offset[1] = T(za[tag + "_offset1_init"], d).clone()
        assert float(blk.offset[2].abs().max()) == 0.0 and float(blk.offset[3].abs().max()) == 0.0

    def called(blk, r, step, n, out_key, offset_keys):
        assert name_of(r.dtype) == table[step + ":out"] and r.shape == (1, n, 196, h, w) and r.is_contiguous()
        assert name_of(blk.offset[1].dtype) == table[step + ":offset[1]"] and half_representable(blk.offset[0])
        held_lookup(r, out_key, "%s (%s)" % (out_key, inject))
        for l, key in offset_keys:
            held(blk.offset[l], key, offsets=True)

    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        A = lgu.CorrBlock(ofsMap, ofs_residual, GA, f1[:, :Ea].contiguous(), f2[:, :Ea].contiguous(), num_levels=4, radius=3)
        built(A, "A")
        for l, lv in enumerate(_rowmajor_levels(lgu, A)):
            held(lv, "A_pyr%d" % l)
        r1, mean_n, theta = A(T(z["coords1"], d)[:, :Ea])
        assert mean_n is A.mean_n and theta is A.theta
        called(A, r1, "A called", Ea, "out1", [(0, "A_offset0_after1"), (1, "A_offset1_after1")])

        B = lgu.CorrBlock(ofsMap, ofs_residual, GA, f1[:, Ea:].contiguous(), f2[:, Ea:].contiguous(), num_levels=4, radius=3)
        built(B, "B")
        A = A.cat(B)
        r2, _, _ = A(T(z["coords2"], d))
        called(A, r2, "AB called", Ea + int(z["E_b"]), "out2", [(0, "AB_offset0_after2"), (1, "AB_offset1_after2")])

        keep = T(za["keep"], d)
        assert np.array_equal(za["keep"], z["keep"])
        A = A[keep]
        r3, _, _ = A(T(z["coords3"], d)[:, keep])
        called(A, r3, "AB[keep] called", Ea + int(z["E_b"]) - 1, "out3", [(1, "AB_offset1_after3")])
        assert A.offset[2].shape[0] == Ea + int(z["E_b"]) - 1 and float(A.offset[2].abs().max()) == 0.0
