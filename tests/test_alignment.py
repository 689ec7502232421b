"""Every operator on contiguous operands that are aligned to their element only.

The host entries of csrc/ choose their kernels by the addresses of their operands; fresh allocations are 512-byte aligned,
so those branches stay dark unless a test hands over `poses[t0:]`, `ii[k:]`, a half tensor cut at an odd element or a
tensor carved out of an arena.  tests/alignment_cases.py holds the helper and the registry (one entry per operator, with
what DESIGN.md section 4.1 says each operand's misalignment leads to); here every operand of every entry is replaced by
its shifted twin for each shift of the issue's table, then all operands together, and the call is held to exactly the
outcome the audit states:

  served, same arithmetic   bit for bit the aligned call
  served by a fallback      both results within the bound the operator's own parity test uses, against the same oracle
  refused                   UnsupportedShape / RuntimeError with nothing launched: outputs and in-place operands unchanged

and in every case: in-place operands end as in the aligned call, read-only operands are untouched, both guard bands of
every shifted tensor are intact.  Reference-named operators (the names the drop-in modules export) must serve.
"""
import os
import re

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import alignment_cases as AC            # noqa: E402  (it needs torch at import)
from tests.test_abi import declared_symbols        # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BY_NAME = {c.name: c for c in AC.CASES}


# ---- CPU: the helper, and the registry against the header --------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.int64, torch.uint8, torch.int32, torch.float64])
def test_shifted_is_contiguous_equal_and_at_the_requested_address(dtype):
    src = (torch.arange(3 * 5 * 7) % 120).reshape(3, 5, 7).to(dtype)
    for nbytes in AC.shifts_for(dtype) + (0,):
        t = AC.shifted(src, nbytes)
        assert t.is_contiguous() and t.dtype == dtype and t.shape == src.shape
        assert t.data_ptr() % 16 == nbytes
        assert torch.equal(t, src) and AC.guards_intact(t)
        raw, start, nb = t._lgu_guard
        assert start >= AC.GUARD and raw.numel() - (start + nb) >= AC.GUARD and nb == src.numel() * src.element_size()
        t.view(-1)[0] = 1                       # writes inside leave the bands alone ...
        assert AC.guards_intact(t)
        raw[start - 1] = 0                      # ... one byte before or after does not
        assert not AC.guards_intact(t)
        raw[start - 1] = AC.SENTINEL
        raw[start + nb] = 0
        assert not AC.guards_intact(t)


def test_shift_table_is_the_issues():
    assert AC.shifts_for(torch.float32) == (4, 8) and AC.shifts_for(torch.float16) == (2, 4, 8)
    assert AC.shifts_for(torch.int64) == (8,) and AC.shifts_for(torch.uint8) == (1,)


def pointer_entries():
    """The lgu_* functions of include/lgu_corr.h that take at least one pointer other than the stream: as a parameter, or
    as a field (a pointer, or an array of pointers) of an argument struct they take by value."""
    text = open(os.path.join(ROOT, "include", "lgu_corr.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    last = r"([A-Za-z_0-9]+)\s*(?:\[\d*\])?\s*$"
    structs = {}
    for body, name in re.findall(r"typedef\s+struct\s*\{([^}]*)\}\s*(lgu_[a-z0-9_]+)\s*;", text):
        structs[name] = [re.findall(last, d.strip())[0] for d in body.split(";") if "*" in d]
    out = {}
    for name, params in re.findall(r"\b(lgu_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", text):
        names = []
        for p in (q.strip() for q in params.split(",")):
            by_value = re.match(r"(lgu_[a-z0-9_]+)\s+[A-Za-z_0-9]+$", p)
            if by_value and by_value.group(1) in structs:
                names += structs[by_value.group(1)]
            elif ("*" in p or "[" in p) and not re.search(r"void\s*\*\s*stream\s*$", p):
                names.append(re.findall(last, p)[0])
        if names:
            out[name] = names
    return out


STRUCT_ARGS = ("lgu_flow_conv7_relu_h16", "lgu_conv3x3_c128_h16", "lgu_conv3x3_fanout_c128_h16", "lgu_head3x3_c128_h16",
               "lgu_head3x3_pair_c128_h16", "lgu_gruconv3x3_c448_h16", "lgu_upmask1x1_c128_h16", "lgu_upmask_upsample_f32",
               "lgu_conv1x1_o128_h16", "lgu_encconv3x3_h16", "lgu_encstem7x7_h16", "lgu_encout1x1_c128_h16", "lgu_encconv3x3_norm_h16",
               "lgu_encstats_finalize", "lgu_gaussian_head", "lgu_cloud_decide_f32", "lgu_cloud_write_f32", "lgu_intake_frame_u8",
               "lgu_intake_depth_f32", "lgu_render_view")


def test_pointer_entries_parse_the_header():
    ents = pointer_entries()
    assert set(ents) <= set(declared_symbols())
    assert ents["lgu_corridx_fwd_f32"] == ["volume", "coords", "corr"]
    assert ents["lgu_image_normalize_u8"] == ["img", "out", "mean", "std"]
    # entries that take a parameter block by value: its pointer fields, arrays of pointers and pointers to tables included
    assert set(STRUCT_ARGS) <= set(ents) and len(STRUCT_ARGS) == 20
    assert ents["lgu_conv3x3_c128_h16"] == ["x", "wpack", "bias", "out"]
    assert ents["lgu_conv3x3_fanout_c128_h16"] == ["x", "wpack", "bias", "out"]
    assert ents["lgu_head3x3_pair_c128_h16"] == ["x", "wpack", "bias", "out", "coords"]
    assert ents["lgu_intake_frame_u8"] == ["raw", "image", "inputs", "cam_table"]
    assert ents["lgu_encstats_finalize"] == ["acc", "mean_rstd"]
    assert ents["lgu_render_view"] == ["points", "colors", "view", "intrinsics", "cameras", "scratch", "image", "depth"]
    for pure in ("lgu_version", "lgu_ba_build_slices", "lgu_offsets_finalize_scratch_bytes", "lgu_proximity_capacity",
                 "lgu_instnorm_resident_limit", "lgu_error_string"):
        assert pure not in ents


def test_every_pointer_entry_is_reached_or_excluded_with_a_reason():
    """A function added to the header later fails here until it has a registry entry or a stated exclusion."""
    reached = {s for c in AC.CASES for s in c.symbols}
    ents = pointer_entries()
    assert reached <= set(ents), sorted(reached - set(ents))
    assert not (reached & set(AC.EXCLUDED)), sorted(reached & set(AC.EXCLUDED))
    missing = sorted(set(ents) - reached - set(AC.EXCLUDED))
    assert not missing, "no alignment case and no exclusion for: %s" % ", ".join(missing)
    assert set(AC.EXCLUDED) <= set(ents)
    assert all(len(r.strip()) > 10 and "\n" not in r for r in AC.EXCLUDED.values())


def test_the_audit_table_names_every_pointer_operand():
    """DESIGN.md section 4.1 has a row for every pointer operand of every entry of the header."""
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    m = re.search(r"^### 4\.1 .*?(?=^## 5\. )", text, flags=re.S | re.M)
    assert m, "DESIGN.md has no section 4.1"
    rows = {}
    for line in m.group(0).splitlines():
        cells = [c.strip() for c in line.split("|")]
        if len(cells) >= 6 and cells[1].startswith("`lgu_"):
            for fn in re.findall(r"lgu_[a-z0-9_]+", cells[1]):
                rows.setdefault(fn, set()).update(re.findall(r"[A-Za-z_0-9]+", cells[2]))
    for fn, operands in pointer_entries().items():
        assert fn in rows, "no audit row for %s" % fn
        assert set(operands) <= rows[fn], "%s: no audit row for %s" % (fn, sorted(set(operands) - rows[fn]))


def test_registry_is_consistent():
    assert len(BY_NAME) == len(AC.CASES)
    for c in AC.CASES:
        assert c.kind in ("reference", "own") and c.symbols and c.operands
        for key, op in c.operands.items():
            assert op.miss in AC.RANK and (op.need is None or op.need in (2, 4, 8, 16))
            # the names the drop-in modules export must serve every contiguous tensor, as the reference's extensions do
            assert not (c.kind == "reference" and op.miss in ("unsupported", "badarg")), (c.name, key)
            # a fallback with another summation order needs the bound it is held to
            assert op.miss != "fallback" or c.bound is not None, (c.name, key)
        assert set(c.inplace) <= set(c.operands), c.name


def test_dropin_exports_are_registered_as_reference_named(lgu):
    ref = {c.name for c in AC.CASES if c.kind == "reference"}
    for n in ("defCorr_index_forward", "defCorr_index_backward", "corr_index_forward", "corr_index_backward", "gaussianMask",
              "gaussianMask_backward", "altcorr_forward", "altcorr_backward"):
        assert "ops." + n in ref
    assert {"ops.lowMem_defSample[A]", "ops.lowMem_defSample[B]", "geom.frame_distance", "geom.projmap", "geom.depth_filter", "geom.iproj",
            "aggregate.scatter_mean[f32]", "aggregate.scatter_mean[h16]", "lie.SE3", "lie.SO3", "ba.ba"} <= ref


# ---- GPU ------------------------------------------------------------------------------------------------------------------
PARAMS = [(c.name, key) for c in AC.CASES for key in list(c.operands) + ["all"]]
_REF = {}
_STOP = []     # set after an error that did not come from an argument check: nothing more is started on the device


def _status(lgu, c, args):
    try:
        outs = c.call(lgu, args)
        torch.cuda.synchronize()
        return "served", outs
    except lgu._lib.UnsupportedShape:
        return "unsupported", None
    except RuntimeError as exc:
        msg = str(exc)
        if "(code 100001)" in msg:           # LGU_E_BADARG through _lib.check
            return "badarg", None
        if " failed: " in msg or "HIP error" in msg or "CUDA error" in msg:   # a launch or device error
            _STOP.append(msg)
        raise


def _within_bound(c, oracle, host_args, outs, what):
    ref_fn, tol = c.bound
    if c.name not in _REF:
        _REF[c.name] = ref_fn(oracle, host_args)
    for i, (g, w) in enumerate(zip(outs, _REF[c.name])):
        err = float(np.abs(g.detach().cpu().numpy().reshape(w.shape) - w).max())
        print("%s %s output %d: max abs err %.3g (bound %.3g)" % (c.name, what, i, err, tol(w)))
        assert err <= tol(w), (c.name, what, i, err, tol(w))


def _same(a, b):
    if a is None or b is None:
        return a is None and b is None
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b)


@pytest.mark.gpu
@pytest.mark.parametrize("name,key", PARAMS)
def test_operand_at_element_alignment(lgu, oracle, name, key):
    assert not _STOP, "an earlier case ended in a device error: %s" % _STOP[0]
    assert torch.cuda.is_available(), "these tests need the MI355X"
    assert os.path.exists(lgu._lib.so_path()), "liblgu_corr.so missing — run __graft_entry__.build()"
    c = BY_NAME[name]
    dev = torch.device("cuda:0")
    base = c.build(dev)
    assert all(base[k].is_contiguous() and base[k].data_ptr() % 16 == 0 for k in c.operands)
    host_args = {k: v.detach().cpu().numpy() for k, v in base.items() if isinstance(v, torch.Tensor) and v.dtype != torch.float16} \
        if c.bound else None
    status0, outs0 = _status(lgu, c, base)
    assert status0 == "served", "%s refuses its aligned operands" % name
    if c.bound:
        _within_bound(c, oracle, host_args, outs0, "aligned")
    keys = list(c.operands) if key == "all" else [key]
    shifts = (0,) if key == "all" else AC.shifts_for(base[key].dtype)
    for shift in shifts:
        args = c.build(dev)
        before = {k: args[k].clone() for k in c.operands}
        for k in keys:
            args[k] = AC.shifted(args[k], args[k].element_size() if key == "all" else shift)
            assert args[k].data_ptr() % 16 == (args[k].element_size() if key == "all" else shift)
        want = AC.expected(c, args, key, shift)
        tag = "%s shifted by %s" % (key, "one element each" if key == "all" else "%d bytes" % shift)
        status, outs = _status(lgu, c, args)
        assert status == ("served" if want in ("same", "fallback") else want), (name, tag, "audit says " + want, "call was " + status)
        if status == "served":
            assert len(outs) == len(outs0)
            if c.bound is None:
                for i, (a, b) in enumerate(zip(outs, outs0)):
                    assert _same(a, b), "%s, %s: output %d differs from the aligned call" % (name, tag, i)
            else:
                _within_bound(c, oracle, host_args, outs, tag)
                if want == "same" and c.bound[1] is AC.ABS_1E5:   # deterministic kernels: the same kernel gives the same bits
                    for i, (a, b) in enumerate(zip(outs, outs0)):
                        assert _same(a, b), "%s, %s: output %d differs from the aligned call" % (name, tag, i)
            for k in c.inplace:      # mutated exactly as in the aligned call
                assert torch.equal(args[k], base[k]), "%s, %s: in-place operand %s differs from the aligned call" % (name, tag, k)
        else:
            for k in c.inplace:      # nothing launched
                assert torch.equal(args[k], before[k]), "%s, %s: refused, but %s changed" % (name, tag, k)
        for k in c.operands:
            if k not in c.inplace:
                assert torch.equal(args[k], before[k]), "%s, %s: read-only operand %s changed" % (name, tag, k)
        for k in keys:
            assert AC.guards_intact(args[k]), "%s, %s: a guard band of %s was written" % (name, tag, k)


# ---- GPU: the glue classes.  Whatever their fused entries refuse, the classes serve, within the bound and against the
# reference their own tests use -------------------------------------------------------------------------------------------
def _variants(tensors):
    """(index or "all", shift) over a list of tensors, as for the registry entries."""
    out = [(i, s) for i, t in enumerate(tensors) for s in AC.shifts_for(t.dtype)]
    return out + [("all", 0)]


def _shift_some(tensors, which, shift):
    ts = list(tensors)
    for i in (range(len(ts)) if which == "all" else [which]):
        ts[i] = AC.shifted(ts[i], ts[i].element_size() if which == "all" else shift)
    return ts, [ts[i] for i in (range(len(ts)) if which == "all" else [which])]


def _corrblock_want(lgu, oracle, blk, offs, coords1, tiled):
    """The reference-shaped composition of tests/test_gpu_parity.py::test_corrblock_matches_reference_shaped_composition:
    probe + mask + four per-level oracle calls + cat on the block's own pyramid and offsets."""
    E, h, w = coords1.shape[1:4]
    rowmajor = [lgu.ops.volume_retile(v.contiguous(), to_tiled=False, hw=blk._level_hw[i]) if tiled else v
                for i, v in enumerate(blk.corr_pyramid)]
    pyr = [v.cpu().numpy() for v in rowmajor]
    c = coords1.permute(0, 1, 4, 2, 3).contiguous().view(E, 2, h, w).cpu().numpy()
    probe, = oracle.corr_index_forward(pyr[1], (c / 2).astype(np.float32), 1)
    var = torch.var(torch.from_numpy(probe).permute(0, 3, 4, 1, 2), dim=[3, 4])
    offs[1] = (offs[1] * torch.sigmoid(var).numpy().reshape(E, h, w, 1, 1, 1)).astype(np.float32)
    return oracle.defcorr_pyramid_forward(pyr, c, [offs[0], offs[1], None, None], 3)


@pytest.mark.gpu
@pytest.mark.parametrize("tiled", [True, False])
def test_corrblock_serves_shifted_operands(lgu, oracle, tiled, monkeypatch):
    """CorrBlock on shifted fmap1 / fmap2 / coords: lgu_volume_build_pyramid_f32 and the fused lookup refuse them, the
    class takes the library GEMM + fused builder and the separate probe instead.  Bound and reference of
    test_corrblock_matches_reference_shaped_composition: 2e-5 against the oracle's composition."""
    monkeypatch.setattr(lgu.CorrBlock, "TILED_PYRAMID", tiled)
    E, h, w = 2, 16, 16
    g = AC._gen(3)
    dev = "cuda"
    torch.manual_seed(3)
    ofsMap = torch.nn.Conv2d(256, 98, 3, padding=1).to(dev)
    ofsRes = torch.nn.Conv2d(256, 98, 3, padding=1).to(dev)
    GA = lgu.GaussianMask(h, w).to(dev)
    torch.nn.init.normal_(GA.meanMap.weight, 0, 0.3)
    ys, xs = torch.meshgrid(torch.arange(h).float(), torch.arange(w).float(), indexing="ij")
    base = [AC._randn(g, (1, E, 128, h, w), dev, 0.5), AC._randn(g, (1, E, 128, h, w), dev, 0.5),
            (torch.stack([xs, ys], -1)[None, None] + 2 * torch.randn((1, E, h, w, 2), generator=g)).to(dev).contiguous()]
    for which, shift in [(None, 0)] + _variants(base):
        ts, sh = (base, []) if which is None else _shift_some(base, which, shift)
        with torch.no_grad():
            blk = lgu.CorrBlock(ofsMap, ofsRes, GA, ts[0], ts[1])
            offs = [o.contiguous().cpu().numpy().reshape(E, h, w, 7, 7, 2).copy() for o in blk.offset[:2]]
            got, mean_n, theta = blk(ts[2])
            torch.cuda.synchronize()
            want = _corrblock_want(lgu, oracle, blk, offs, ts[2], blk._tiled)
        err = float(np.abs(got.cpu().numpy()[0] - want).max())
        print("CorrBlock tiled=%s operand %s shift %s: max abs err %.3g (bound 2e-5)" % (tiled, which, shift, err))
        assert got.shape == (1, E, 196, h, w) and err <= 2e-5, (which, shift, err)
        assert all(torch.equal(a, b) for a, b in zip(ts, base)) and all(AC.guards_intact(t) for t in sh)


@pytest.mark.gpu
def test_altcorrblock_serves_shifted_operands(lgu, oracle):
    """AltCorrBlock on shifted fmaps / coords / ii / jj.  Bound and reference of test_altcorrblock_matches_oracle_composition:
    2e-5 against the per-level oracle composition on the block's own pyramid and offsets."""
    N, C, H, W = 4, 128, 16, 16
    dev = "cuda"
    torch.manual_seed(5)
    ofsMap = torch.nn.Conv2d(256, 98, 3, padding=1).to(dev)
    ofsRes = torch.nn.Conv2d(256, 98, 3, padding=1).to(dev)
    g = AC._gen(5)
    ys, xs = torch.meshgrid(torch.arange(H).float(), torch.arange(W).float(), indexing="ij")
    E = 5
    base = [AC._randn(g, (1, N, C, H, W), dev, 0.5),
            (torch.stack([xs, ys], -1)[None, None] + 2 * torch.randn((1, E, H, W, 2), generator=g)).to(dev).contiguous(),
            torch.tensor([0, 0, 1, 2, 3], device=dev), torch.tensor([1, 2, 3, 0, 2], device=dev)]
    for which, shift in [(None, 0)] + _variants(base):
        ts, sh = (base, []) if which is None else _shift_some(base, which, shift)
        fmaps, coords, ii, jj = ts
        with torch.no_grad():
            blk = lgu.AltCorrBlock(ofsMap, ofsRes, None, fmaps)
            got = blk(coords, ii, jj)
            torch.cuda.synchronize()
            f1 = blk.pyramid[0][0, ii].float().contiguous().cpu().numpy()
            feats = torch.cat(((blk.pyramid[0][0, ii] * 4.0).permute(0, 3, 1, 2), (blk.pyramid[0][0, jj] * 4.0).permute(0, 3, 1, 2)), 1).float()
            offs, _ = lgu.corr.generate_offsets(ofsMap, ofsRes, feats, 4)
            offs = [o.contiguous().cpu().numpy().reshape(E, H, W, 7, 7, 2).copy() for o in offs]
            c = coords[0].cpu().numpy()
            outs = []
            for l in range(4):
                f2 = blk.pyramid[l][0, jj].float().contiguous().cpu().numpy()
                cl = (c / 2 ** l).astype(np.float32).reshape(E, 1, H, W, 2)
                if l == 1:
                    probe, = oracle.altcorr_forward(f1, f2, cl, 1)
                    pr = torch.from_numpy(probe).permute(0, 1, 3, 4, 2).contiguous().view(E, H, W, 3, 3)
                    offs[1] = (offs[1] * torch.sigmoid(torch.var(pr, dim=[3, 4])).numpy().reshape(E, H, W, 1, 1, 1)).astype(np.float32)
                corr, = oracle.lowMem_defSample(f1, f2, cl, offs[l], 3)
                outs.append(corr.reshape(E, 49, H, W))
            want = np.concatenate(outs, 1)
        err = float(np.abs(got.cpu().numpy()[0] - want).max())
        print("AltCorrBlock operand %s shift %s: max abs err %.3g (bound 2e-5)" % (which, shift, err))
        assert got.shape == (1, E, 196, H, W) and err <= 2e-5, (which, shift, err)
        assert all(torch.equal(a, b) for a, b in zip(ts, base)) and all(AC.guards_intact(t) for t in sh)


def _gaussmask_forward_bound(m0, c0, corr, dm, dc, radius=4):
    """|v1 - v0| allowed per element when the parameters moved by at most dm (mean) and dc (cov): v = corr (1 + g),
    g = 3 exp(-(dx^2 / c1 + dy^2 / c2) / 2) / (6.28 sqrt(c1 c2)) inside the window.  First-order terms in float64 from the
    aligned parameters, doubled for the second order, plus 8 fp32 roundings of the value.  Pixels whose window moved
    (floor(mean) changed) are the caller's to exclude."""
    E, h, w = m0.shape[:3]
    m, c, v = m0.double(), c0.double(), corr.double()
    ys, xs = torch.meshgrid(torch.arange(h, device=m.device, dtype=torch.float64), torch.arange(w, device=m.device, dtype=torch.float64),
                            indexing="ij")
    dx = xs.view(1, 1, 1, h, w) - m[..., 0].view(E, h, w, 1, 1)
    dy = ys.view(1, 1, 1, h, w) - m[..., 1].view(E, h, w, 1, 1)
    c1, c2 = c[..., 0].view(E, h, w, 1, 1), c[..., 1].view(E, h, w, 1, 1)
    cx, cy = torch.floor(m[..., 0]).view(E, h, w, 1, 1), torch.floor(m[..., 1]).view(E, h, w, 1, 1)
    inside = ((xs.view(1, 1, 1, h, w) - cx).abs() <= radius) & ((ys.view(1, 1, 1, h, w) - cy).abs() <= radius)
    g = 3 * torch.exp(-0.5 * (dx * dx / c1 + dy * dy / c2)) / (6.28 * torch.sqrt(c1 * c2)) * inside
    dg = g * ((dx.abs() / c1 + dy.abs() / c2) * dm + (0.5 * dx * dx / (c1 * c1) + 0.5 / c1 + 0.5 * dy * dy / (c2 * c2) + 0.5 / c2) * dc)
    return v.abs() * (2 * dg + 8 * 2.0 ** -24 * (1 + g))


@pytest.mark.gpu
def test_gaussianmask_serves_shifted_operands(lgu):
    """GaussianMask on a shifted feature pair and a shifted volume.  Parameters: the bound and reference of
    test_fused_gaussian_parameters_equal_the_torch_composition (mean 1e-5, cov 2e-5 against the torch composition of the
    same module).  The re-weighted volume: bit for bit the aligned call where the parameters are (a shifted volume alone
    changes no arithmetic), otherwise within what the parameters' own differences allow (_gaussmask_forward_bound)."""
    import lgu_slam_amd.gaussian_mask as gm
    E, h, w = 2, 7, 9
    g = AC._gen(11)
    torch.manual_seed(11)
    GA = lgu.GaussianMask(h, w).cuda()
    torch.nn.init.normal_(GA.meanMap.weight, 0, 0.3)
    base = [AC._randn(g, (E, h, w, 256), "cuda"), AC._randn(g, (E, h, w, h, w), "cuda")]
    gm.FUSED_PARAMS = False
    try:
        with torch.no_grad():
            m2, c2, _ = GA.gaussian_parameters(base[0])
    finally:
        gm.FUSED_PARAMS = True
    with torch.no_grad():
        m0, c0, _ = GA.gaussian_parameters(base[0])
        v0, _, _ = GA(base[0], base[1])
    for which, shift in _variants(base):
        ts, sh = _shift_some(base, which, shift)
        with torch.no_grad():
            m1, c1, _ = GA.gaussian_parameters(ts[0])
            v1, _, _ = GA(ts[0], ts[1])
        torch.cuda.synchronize()
        assert float((m1 - m2).abs().max()) <= 1e-5 and float((c1 - c2).abs().max()) <= 2e-5, (which, shift)
        assert v1.shape == v0.shape and v1.dtype == v0.dtype
        if which == 1 or (torch.equal(m1, m0) and torch.equal(c1, c0)):
            assert torch.equal(v1, v0), (which, shift)
        else:
            dm, dc = float((m1 - m0).abs().max()), float((c1 - c0).abs().max())
            same_window = (torch.floor(m1) == torch.floor(m0)).all(dim=-1).view(E, h, w, 1, 1)
            bound = _gaussmask_forward_bound(m0, c0, base[1], dm, dc)
            d = (v1.double() - v0.double()).abs()
            print("GaussianMask operand %s shift %s: dm %.3g dc %.3g, max |dv| %.3g" % (which, shift, dm, dc, float(d.max())))
            assert bool(((d <= bound) | ~same_window).all()), (which, shift, float((d - bound).max()))
            assert float(same_window.float().mean()) >= 0.99
        assert all(torch.equal(a, b) for a, b in zip(ts, base)) and all(AC.guards_intact(t) for t in sh)


@pytest.mark.gpu
@pytest.mark.parametrize("half", [False, True])
def test_kanbiasgru_serves_shifted_operands(lgu, half, capsys):
    """KanBiasGRU on shifted net / inputs, held to the propagated bound of tests/test_kangru.py (check_forward) against the
    restated module."""
    from tests import test_kangru as TK
    m, base = TK.gpu_case(23, 3, 7, 13, half=half)
    base = [t.contiguous() for t in base]
    for which, shift in [(None, 0)] + _variants(base):
        ts, sh = (base, []) if which is None else _shift_some(base, which, shift)
        TK.check_forward(lgu, m, ts, half, "operand %s shift %s" % (which, shift), capsys)
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(ts, base)) and all(AC.guards_intact(t) for t in sh)


@pytest.mark.gpu
@pytest.mark.parametrize("half", [False, True])
def test_feature_encoder_serves_shifted_images(lgu, half):
    """The installed FeatureEncoder on a shifted image batch: as close to the float64 forward as the module itself, the
    bound of tests/test_features.py::test_installed_encoder_is_as_close_to_float64_as_the_module."""
    from tests import test_features as TF
    m, images, ref = TF.encoder_case("features_fnet_1x64x48")
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16, enabled=half):
        own = m(images)
        wr = lgu.features.install(m)
        try:
            for shift in (0, 4, 8):
                x = AC.shifted(images.contiguous(), shift)
                before = wr.fused_calls
                got = m(x)
                torch.cuda.synchronize()
                assert wr.fused_calls == before + 1
                r_got, r_own = TF.rms(got, ref), TF.rms(own, ref)
                print("FeatureEncoder %s shift %d: rms %.4g, module %.4g" % ("half" if half else "fp32", shift, r_got, r_own))
                assert got.dtype == own.dtype and got.shape == own.shape and r_got <= 1.25 * r_own
                assert torch.equal(x, images) and AC.guards_intact(x)
        finally:
            lgu.features.uninstall(m)
