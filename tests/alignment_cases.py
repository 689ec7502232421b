"""Contiguous operands at element alignment: the helper and the registry behind tests/test_alignment.py.

`shifted(t, nbytes)` hands back a contiguous copy of `t` whose address is `nbytes` past a 16-byte boundary, cut out of a
sentinel-filled buffer whose two guard bands `guards_intact` inspects afterwards.

`CASES` has one entry per operator of the Python layer (every function of ops, geom, aggregate, gru, features, lie,
graph and ba that reaches a kernel, and the two plan classes in each of their forms) plus, where the Python layer
allocates the output itself, one entry that calls the C entry through ctypes with an output of the caller's.  An entry
names the `lgu_*` symbols it reaches, builds seeded inputs at the smallest shape that still reaches the production
kernel, and states for every tensor operand what DESIGN.md section 4.1 states: the alignment below which the host
leaves the kernel it would otherwise take (`need`, bytes; None = the operand is only ever accessed by element) and what
the call then does (`miss`):

    "same"         served with the same arithmetic (the same kernel, or its element-wise twin): bit for bit the aligned call
    "fallback"     served by a kernel that sums in another order: both results within the operator's parity bound
    "unsupported"  LGU_E_UNSUPPORTED -> _lib.UnsupportedShape, nothing launched
    "badarg"       LGU_E_BADARG -> RuntimeError, nothing launched

Operators whose aligned call is itself not bit-reproducible (float atomics) are compared through their parity bound in
every outcome (`bound`).  The bounds are the ones the operators' own parity tests use; each is quoted where it is set.
"""
import ctypes

import numpy as np

from tests import inputs

import torch

GUARD = 256          # bytes of sentinel on either side of a shifted tensor
SENTINEL = 0xA5


def shifts_for(dtype):
    """Byte shifts of the issue's table: one element and 8 for fp32, 2 / 4 / 8 for half, 8 for int64, 1 for uint8
    (int32 and fp64 operands, which the table does not list, take one element and 8)."""
    return {torch.float32: (4, 8), torch.float16: (2, 4, 8), torch.int64: (8,), torch.uint8: (1,),
            torch.int32: (4, 8), torch.float64: (8,)}[dtype]


def shifted(t, nbytes, guard=GUARD):
    """A contiguous tensor equal to `t` with data_ptr() % 16 == nbytes, inside a sentinel-filled buffer."""
    assert t.is_contiguous() and 0 <= nbytes < 16 and nbytes % t.element_size() == 0
    nb = t.numel() * t.element_size()
    raw = torch.full((guard + 16 + nb + guard,), SENTINEL, dtype=torch.uint8, device=t.device)
    start = guard + (nbytes - (raw.data_ptr() + guard)) % 16
    view = raw[start:start + nb].view(t.dtype).view(t.shape)
    view.copy_(t)
    view._lgu_guard = (raw, start, nb)
    return view


def guards_intact(t):
    raw, start, nb = t._lgu_guard
    return bool((raw[:start] == SENTINEL).all()) and bool((raw[start + nb:] == SENTINEL).all())


class Op:
    def __init__(self, need=None, miss="same"):
        self.need, self.miss = need, miss

    def outcome(self, shift):
        return "same" if self.need is None or shift % self.need == 0 else self.miss


SAME = Op()
RANK = {"same": 0, "fallback": 1, "unsupported": 2, "badarg": 3}


class Case:
    """name; symbols reached; kind "reference" (must serve every call) or "own" (may refuse); build(dev) -> dict of
    arguments; call(lgu, args) -> tuple of output tensors; operands {key: Op}; inplace: keys whose contents the call may
    change (compared with the aligned call when served, with their values before the call when refused);
    bound = (ref(oracle, host_args) -> list of arrays like the outputs, tol(want) -> float) or None for bit equality."""

    def __init__(self, name, symbols, kind, build, call, operands, inplace=(), bound=None):
        self.name, self.symbols, self.kind = name, tuple(symbols), kind
        self.build, self.call, self.operands, self.inplace, self.bound = build, call, dict(operands), tuple(inplace), bound

    def variants(self, args):
        """(operand key or "all", shift) for every shift of every operand, then all operands by one element each."""
        out = []
        for key in self.operands:
            out += [(key, s) for s in shifts_for(args[key].dtype)]
        out.append(("all", 0))
        return out


def expected(case, args, key, shift):
    if key != "all":
        return case.operands[key].outcome(shift)
    worst = "same"
    for k, op in case.operands.items():
        o = op.outcome(args[k].element_size())
        worst = o if RANK[o] > RANK[worst] else worst
    return worst


CASES = []


def case(*a, **kw):
    CASES.append(Case(*a, **kw))


def _d(x, dev):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dev)


def _randn(gen, shape, dev, scale=1.0, dtype=None):
    t = torch.randn(shape, generator=gen) * scale
    return (t if dtype is None else t.to(dtype)).to(dev)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _check(lgu, rc, what):
    lgu._lib.check(rc, what)


def _st(t):
    return ctypes.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


A16 = lambda miss: Op(16, miss)   # noqa: E731
A8 = lambda miss: Op(8, miss)     # noqa: E731

# ---- bounds quoted from the operators' parity tests (tests/test_gpu_parity.py) ---------------------------------------
ABS_1E5 = lambda w: 1e-5                                    # noqa: E731  test_lowmem_defsample, test_altcorr_forward_backward
REL_1E5 = lambda w: 1e-5 * max(1.0, float(np.abs(w).max()))  # noqa: E731  test_defcorr_backward, test_altcorr_forward_backward


# ======================================================================================================================
# ops: the volume-path samplers (E 2, 12 x 16, r 3)
# ======================================================================================================================
def _sampler_inputs(dev, radius=3, seed=101):
    rng = np.random.default_rng(seed)
    E, H1, W1, H2, W2 = 2, 12, 16, 12, 16
    rd = 2 * radius + 1
    return dict(volume=_d(rng.standard_normal((E, H1, W1, H2, W2)).astype(np.float32), dev),
                coords=_d(inputs.grid_coords(rng, E, H1, W1, 3.0), dev),
                offset=_d((4 * np.tanh(rng.standard_normal((E, H1, W1, rd, rd, 2)))).astype(np.float32), dev),
                corr_grad=_d(rng.standard_normal((E, rd, rd, H1, W1)).astype(np.float32), dev))


def _pick(build, *keys):
    return lambda dev: {k: v for k, v in build(dev).items() if k in keys}


# fast gather kernel <-> defcorr_generic_kernel, "same arithmetic" (csrc/defcorr.hip)
case("ops.defCorr_index_forward", ["lgu_defcorr_fwd_f32"], "reference", _pick(_sampler_inputs, "volume", "coords", "offset"),
     lambda lgu, a: tuple(lgu.ops.defCorr_index_forward(a["volume"], a["coords"], a["offset"], 3)),
     dict(volume=A16("same"), coords=A16("same"), offset=A16("same")), inplace=("offset",))
case("ops.corr_index_forward", ["lgu_corridx_fwd_f32"], "reference", _pick(_sampler_inputs, "volume", "coords"),
     lambda lgu, a: tuple(lgu.ops.corr_index_forward(a["volume"], a["coords"], 3)),
     dict(volume=A16("same"), coords=A16("same")))
# backward: one kernel, element accesses, LDS / global float atomics -> the bound of test_defcorr_backward
case("ops.defCorr_index_backward", ["lgu_defcorr_bwd_f32"], "reference", _sampler_inputs,
     lambda lgu, a: tuple(lgu.ops.defCorr_index_backward(a["volume"], a["coords"], a["offset"], a["corr_grad"], 3)),
     dict(volume=SAME, coords=SAME, offset=SAME, corr_grad=SAME), inplace=("offset",),
     bound=(lambda O, h: list(O.defCorr_index_backward(h["volume"], h["coords"], h["offset"].copy(), h["corr_grad"], 3)), REL_1E5))
case("ops.corr_index_backward", ["lgu_corridx_bwd_f32"], "reference", _pick(_sampler_inputs, "volume", "coords", "corr_grad"),
     lambda lgu, a: tuple(lgu.ops.corr_index_backward(a["volume"], a["coords"], a["corr_grad"], 3)),
     dict(volume=SAME, coords=SAME, corr_grad=SAME),
     bound=(lambda O, h: list(O.corr_index_backward(h["volume"], h["coords"], h["corr_grad"], 3)), REL_1E5))


# ---- Gaussian mask and volume_pyramid: (2, 12, 16, 12, 16), L 3 ------------------------------------------------------
def _gauss_inputs(dev, half_volume=False, seed=131):
    rng = np.random.default_rng(seed)
    E, H1, W1, H2, W2 = 2, 12, 16, 12, 16
    ys, xs = np.meshgrid(np.arange(H1, dtype=np.float32), np.arange(W1, dtype=np.float32), indexing="ij")
    means = (np.stack([xs, ys], -1)[None].repeat(E, 0) + rng.standard_normal((E, H1, W1, 2)) * 2).astype(np.float32)
    covs = rng.uniform(0.05, 5.05, (E, H1, W1, 2)).astype(np.float32)
    vol = _d(rng.standard_normal((E, H1, W1, H2, W2)).astype(np.float32), dev)
    a = dict(means=_d(means, dev), covs=_d(covs, dev), volume=vol.half() if half_volume else vol,
             volume_grad=_d(rng.standard_normal((E, H1, W1, H2, W2)).astype(np.float32), dev))
    a["det"] = (a["covs"][..., 0] * a["covs"][..., 1]).reshape(E, H1 * W1).contiguous()
    return a


# float4 kernel <-> gaussmask_fwd_generic_kernel (same expression per element); the backward reads by element and
# reduces with a fixed wave butterfly
case("ops.gaussianMask", ["lgu_gaussmask_fwd_f32"], "reference", _pick(_gauss_inputs, "means", "covs", "volume"),
     lambda lgu, a: tuple(lgu.ops.gaussianMask(a["means"], a["covs"], a["volume"], 4)),
     dict(means=SAME, covs=SAME, volume=A16("same")))
case("ops.gaussianMask_backward", ["lgu_gaussmask_bwd_f32"], "reference", _pick(_gauss_inputs, "means", "covs", "volume", "volume_grad"),
     lambda lgu, a: tuple(lgu.ops.gaussianMask_backward(a["means"], a["covs"], a["volume"], a["volume_grad"], 4)),
     dict(means=SAME, covs=SAME, volume=SAME, volume_grad=SAME))


def _ctypes_gaussmask(lgu, a):
    E, H1, W1, H2, W2 = a["volume"].shape
    _check(lgu, lgu._lib.load().lgu_gaussmask_fwd_f32(_p(a["means"]), _p(a["covs"]), _p(a["volume"]), _p(a["out"]), E, H1, W1, H2, W2, 4,
                                                      _st(a["out"])), "gaussmask")
    return (a["out"],)


def _with_out(build, shape_of, dtype=None, keys=None):
    def b(dev):
        a = build(dev)
        if keys is not None:
            a = {k: v for k, v in a.items() if k in keys}
        a["out"] = torch.full(shape_of(a), 7.0, dtype=dtype or torch.float32, device=dev)
        return a
    return b


case("c.lgu_gaussmask_fwd_f32[out]", ["lgu_gaussmask_fwd_f32"], "reference",
     _with_out(_gauss_inputs, lambda a: tuple(a["volume"].shape), keys=("means", "covs", "volume")), _ctypes_gaussmask,
     dict(out=A16("same")), inplace=("out",))


def _vp_case(name, syms, tiled=False, half=False, det=None):
    def build(dev):
        a = _gauss_inputs(dev, half_volume=half)
        keep = ["means", "covs", "volume"] + (["det"] if det else [])
        a = {k: a[k] for k in keep}
        if det == "half":
            a["det"] = a["det"].half()
        return a
    ops = dict(means=SAME, covs=SAME, volume=A16("unsupported"))
    if det:
        ops["det"] = SAME
    case(name, syms, "own", build,
         lambda lgu, a: tuple(lgu.ops.volume_pyramid(a["means"], a["covs"], a["volume"], 3, radius=4, tiled=tiled, det=a.get("det"))),
         ops)


_vp_case("ops.volume_pyramid[f32]", ["lgu_volume_pyramid_f32"])
_vp_case("ops.volume_pyramid[tiled]", ["lgu_volume_pyramid_tiled_f32"], tiled=True)
_vp_case("ops.volume_pyramid[h16]", ["lgu_volume_pyramid_h16"], half=True)
_vp_case("ops.volume_pyramid[h16,tiled]", ["lgu_volume_pyramid_h16"], tiled=True, half=True)
_vp_case("ops.volume_pyramid[det]", ["lgu_volume_pyramid_det"], det="f32")
_vp_case("ops.volume_pyramid[det half,tiled]", ["lgu_volume_pyramid_det"], tiled=True, det="half")


def _ctypes_volume_pyramid(tiled, form="f32"):
    def call(lgu, a):
        E, H1, W1, H2, W2 = a["volume"].shape
        lv = [a["out"], a["l1"], a["l2"]]
        lp = (ctypes.c_void_p * 3)(*[t.data_ptr() for t in lv])
        lib = lgu._lib.load()
        if form == "h16":
            rc = lib.lgu_volume_pyramid_h16(_p(a["means"]), _p(a["covs"]), _p(a["volume"]), lp, 3, E, H1, W1, H2, W2, 4, int(tiled),
                                            _st(a["out"]))
        elif form == "det":
            rc = lib.lgu_volume_pyramid_det(_p(a["means"]), _p(a["covs"]), _p(a["det"]), 0, _p(a["volume"]), 0, lp, 3, E, H1, W1, H2, W2, 4,
                                            int(tiled), _st(a["out"]))
        else:
            fn = lib.lgu_volume_pyramid_tiled_f32 if tiled else lib.lgu_volume_pyramid_f32
            rc = fn(_p(a["means"]), _p(a["covs"]), _p(a["volume"]), lp, 3, E, H1, W1, H2, W2, 4, _st(a["out"]))
        _check(lgu, rc, "volume_pyramid")
        return tuple(lv)

    def build(dev):
        a = {k: v for k, v in _gauss_inputs(dev, half_volume=(form == "h16")).items()
             if k in ("means", "covs", "volume") + (("det",) if form == "det" else ())}
        E, H1, W1, H2, W2 = a["volume"].shape
        shp = (lambda h, w: (E, H1, W1, -(-h // 4), -(-w // 8), 4, 8)) if tiled else (lambda h, w: (E, H1, W1, h, w))
        a["out"] = torch.full(shp(H2, W2), 7.0, device=dev)
        a["l1"] = torch.full(shp(H2 >> 1, W2 >> 1), 7.0, device=dev)
        a["l2"] = torch.full(shp(H2 >> 2, W2 >> 2), 7.0, device=dev)
        return a
    return build, call


for _t in (False, True):
    _b, _c = _ctypes_volume_pyramid(_t)
    # levels[0] is written as float4; the coarser levels by element
    case("c.lgu_volume_pyramid%s_f32[levels]" % ("_tiled" if _t else ""), ["lgu_volume_pyramid_tiled_f32" if _t else "lgu_volume_pyramid_f32"],
         "own", _b, _c, dict(out=A16("unsupported"), l1=SAME, l2=SAME), inplace=("out", "l1", "l2"))
    for _f in ("h16", "det"):     # their own entry code in front of the shared host function
        _b, _c = _ctypes_volume_pyramid(_t, _f)
        case("c.lgu_volume_pyramid_%s[levels%s]" % (_f, ",tiled" if _t else ""), ["lgu_volume_pyramid_" + _f], "own", _b, _c,
             dict(out=A16("unsupported"), l1=SAME, l2=SAME), inplace=("out", "l1", "l2"))


def _retile_inputs(dev):
    return dict(volume=_randn(_gen(5), (2, 3, 4, 6, 10), dev))


case("ops.volume_retile", ["lgu_volume_retile_f32"], "own", _retile_inputs,
     lambda lgu, a: (lgu.ops.volume_retile(lgu.ops.volume_retile(a["volume"]), to_tiled=False, hw=(6, 10)),
                     lgu.ops.volume_retile(a["volume"])), dict(volume=SAME))


# ---- volume_build_pyramid: (3, 16, 8, 16) fp32; the half kernel needs C % 32 == 0, so (3, 32, 8, 16) ------------------
def _vb_inputs(half):
    def build(dev):
        g = _gen(17)
        E, C, H, W = (3, 32, 8, 16) if half else (3, 16, 8, 16)
        ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
        means = (torch.stack([xs, ys], -1)[None] + torch.randn((E, H, W, 2), generator=g) * 2).to(dev).contiguous()
        covs = (torch.rand((E, H, W, 2), generator=g) * 5 + 0.05).to(dev)
        a = dict(means=means, covs=covs, det=(covs[..., 0] * covs[..., 1]).reshape(E, H * W).contiguous())
        if half:
            a["feats"] = _randn(g, (E, H, W, 2 * C), dev, 0.5, torch.float16)
        else:
            a["fmap1"], a["fmap2"] = _randn(g, (E, C, H, W), dev, 0.5), _randn(g, (E, C, H, W), dev, 0.5)
        return a
    return build


case("ops.volume_build_pyramid[f32]", ["lgu_volume_build_pyramid_f32"], "own", _vb_inputs(False),
     lambda lgu, a: tuple(lgu.ops.volume_build_pyramid(a["fmap1"], a["fmap2"], a["means"], a["covs"], det=a["det"])),
     dict(fmap1=A16("unsupported"), fmap2=A16("unsupported"), means=SAME, covs=SAME, det=SAME))
case("ops.volume_build_pyramid[h16]", ["lgu_volume_build_pyramid_h16"], "own", _vb_inputs(True),
     lambda lgu, a: tuple(lgu.ops.volume_build_pyramid(a["feats"], None, a["means"], a["covs"], det=a["det"])),
     dict(feats=A16("unsupported"), means=SAME, covs=SAME, det=SAME))


def _ctypes_volume_build(half):
    def build(dev):
        a = _vb_inputs(half)(dev)
        E, H, W = a["means"].shape[:3]
        for l in range(4):
            a["lv%d" % l] = torch.full((E, H, W, -(-(H >> l) // 4), -(-(W >> l) // 8), 4, 8), 7.0, device=dev)
        if half:
            a["work"] = torch.zeros_like(a["feats"])
        return a

    def call(lgu, a):
        E, H, W = a["means"].shape[:3]
        lv = [a["lv%d" % l] for l in range(4)]
        lp = (ctypes.c_void_p * 4)(*[t.data_ptr() for t in lv])
        lib = lgu._lib.load()
        if half:
            rc = lib.lgu_volume_build_pyramid_h16(_p(a["feats"]), _p(a["work"]), _p(a["means"]), _p(a["covs"]), _p(a["det"]), 0, lp, 4,
                                                  E, a["feats"].shape[3] // 2, H, W, 4, _st(lv[0]))
        else:
            rc = lib.lgu_volume_build_pyramid_f32(_p(a["fmap1"]), _p(a["fmap2"]), _p(a["means"]), _p(a["covs"]), _p(a["det"]), 0, lp, 4,
                                                  E, a["fmap1"].shape[1], H, W, 4, _st(lv[0]))
        _check(lgu, rc, "volume_build_pyramid")
        return tuple(lv)
    return build, call


for _h in (False, True):
    _b, _c = _ctypes_volume_build(_h)
    _ops = {"lv%d" % l: A16("unsupported") for l in range(4)}
    if _h:
        _ops["work"] = A16("unsupported")
    case("c.lgu_volume_build_pyramid_%s[levels]" % ("h16" if _h else "f32"), ["lgu_volume_build_pyramid_%s" % ("h16" if _h else "f32")],
         "own", _b, _c, _ops, inplace=tuple(k for k in _ops if k != "work"))


# ======================================================================================================================
# ops: the fused pyramid sampler and DefcorrPyramidPlan — (E 2, 12 x 16, L 3, r 3), LEAN one_tile_wide, TILED w2_not_mult4
# ======================================================================================================================
def _pyr_inputs(kind):
    def build(dev):
        if kind == "lean":        # LEAN_CASES["one_tile_wide"]: four levels, offsets on 0-1, 24 x 32 target slices
            E, H1, W1, H2, W2, L = 3, 5, 9, 24, 32, 4
            rng = np.random.default_rng(701)
            vols = inputs.volume_pyramid(rng, E, H1, W1, 4, H2, W2)
            coords = (inputs.grid_coords(rng, E, H1, W1, 3.0) * np.array([W2 / W1, H2 / H1], np.float32).reshape(1, 2, 1, 1)).astype(np.float32)
            offs = inputs.canonical_offsets(rng, E, H1, W1, 4)
        elif kind == "w2_not_mult4":   # TILED_CASES["w2_not_mult4"]: level 2 is 5 x 6
            c = inputs.pyramid_case(36, 1, 20, 24, 3, 3, 3.0, 4.0, False)
            vols, coords, offs = c["volumes"], c["coords"], c["offsets"]
        elif kind == "mixed_nulls":    # offsets on levels 0 and 2 only: three launches, one per run of equal kind
            c = inputs.pyramid_case(1, 2, 12, 16, 3, 3, 3.0, 4.0, True)
            vols, coords, offs = c["volumes"], c["coords"], [c["offsets"][0], None, c["offsets"][2]]
        else:
            c = inputs.pyramid_case(1, 2, 12, 16, 3, 3, 3.0, 4.0, False)
            vols, coords, offs = c["volumes"], c["coords"], c["offsets"]
        a = {"coords": _d(coords, dev)}
        for l, v in enumerate(vols):
            a["vol%d" % l] = _d(v, dev)
        for l, o in enumerate(offs):
            if o is not None:
                a["off%d" % l] = _d(o, dev)
        return a
    return build


def _pyr_call(L, probe=False, tiled=False, mode="plain", fmt="planar", enc=False, plan=True, with_out=True):
    def call(lgu, a):
        vols = [a["vol%d" % l] for l in range(L)]
        hw = [tuple(v.shape[3:]) for v in vols]
        offs = [a.get("off%d" % l) for l in range(L)]
        E, H1, W1 = vols[0].shape[:3]
        slots = a.get("slots")
        if tiled:
            vols = [a["tvol%d" % l] for l in range(L)]
        coords = a["coords"]
        out = a.get("out") if with_out else None
        if out is not None and (fmt != "planar" or enc):
            out = out.permute(0, 3, 1, 2)
        if not plan:
            return (lgu.ops.defcorr_pyramid_forward(vols, coords, offs, 3, probe=probe, tiled=tiled, level_hw=hw if tiled else None,
                                                    coords_last=(mode == "coords_last"), out=out, out_format=fmt),)
        encoder = (a["enc_w"], a["enc_b"]) if enc else None
        pl = lgu.ops.DefcorrPyramidPlan(vols, offs, 3, probe=probe, tiled=tiled, level_hw=hw if tiled else None,
                                        coords_last=(mode == "coords_last"), slots=slots, out_format=fmt, encoder=encoder)
        return (pl(coords, out=out),)
    return call


def _pyr_build(kind, L, tiled=False, mode="plain", fmt="planar", enc=False):
    base = _pyr_inputs(kind)

    def build(dev):
        import lgu_slam_amd as lgu
        a = base(dev)
        E, H1, W1 = a["vol0"].shape[:3]
        if mode == "slots":   # the volumes live in larger buffers at permuted slots
            perm = torch.randperm(E + 2, generator=_gen(3))[:E]
            for l in range(L):
                big = _randn(_gen(40 + l), (E + 2,) + tuple(a["vol%d" % l].shape[1:]), dev)
                big[perm.to(dev)] = a["vol%d" % l]
                a["vol%d" % l] = big
            a["slots"] = perm.to(torch.int32).to(dev)
        if tiled:
            for l in range(L):
                a["tvol%d" % l] = lgu.ops.volume_retile(a["vol%d" % l])
        if mode == "coords_last":
            a["coords"] = a["coords"].permute(0, 2, 3, 1).contiguous()
        C = L * 49
        if enc:
            g = _gen(9)
            a["enc_w"], a["enc_b"] = lgu.ops.pack_encoder_layer(_randn(g, (128, C, 1, 1), dev, 0.1), _randn(g, (128,), dev, 0.1))
            a["out"] = torch.full((E, H1, W1, 128), 7.0, dtype=torch.float16, device=dev)
        elif fmt == "planar":
            a["out"] = torch.full((E, C, H1, W1), 7.0, device=dev)
        else:
            a["out"] = torch.full((E, H1, W1, C), 7.0, dtype=torch.float16 if fmt == "nhwc_f16" else torch.float32, device=dev)
        return a
    return build


def _pyr_case(name, syms, kind, L, miss, out=SAME, offs=(0, 1), **kw):
    tiled = kw.get("tiled", False)
    ops = {"coords": A16(miss)}
    for l in range(L):
        ops[("tvol%d" if tiled else "vol%d") % l] = A16(miss)
    for l in offs:
        ops["off%d" % l] = A16(miss)
    ops["out"] = out
    if kw.get("mode") == "slots":
        ops["slots"] = SAME
    if kw.get("enc"):
        ops["enc_w"], ops["enc_b"] = A16("unsupported"), A8("unsupported")
    bkw = {k: v for k, v in kw.items() if k in ("tiled", "mode", "fmt", "enc")}
    case(name, syms, "own", _pyr_build(kind, L, **bkw), _pyr_call(L, **kw), ops,
         inplace=tuple("off%d" % l for l in offs) + ("out",))


_PF, _PS, _PE = ["lgu_defcorr_pyramid_fwd_f32"], ["lgu_defcorr_pyramid_slots_fwd_f32"], ["lgu_defcorr_pyramid_enc_fwd_f32"]
# row-major, no probe: the generic kernel serves any address with the same arithmetic; `out` is stored by element
_pyr_case("DefcorrPyramidPlan[row-major]", _PF, "tiny", 3, "same")
_pyr_case("ops.defcorr_pyramid_forward[row-major]", _PF, "tiny", 3, "same", plan=False)
_pyr_case("DefcorrPyramidPlan[row-major,lean shape]", _PF, "lean", 4, "same")
# everything else exists in the fast kernels only
_pyr_case("DefcorrPyramidPlan[row-major,probe]", _PF, "tiny", 3, "unsupported", probe=True)
_pyr_case("DefcorrPyramidPlan[tiled]", _PF, "tiny", 3, "unsupported", tiled=True)
_pyr_case("DefcorrPyramidPlan[tiled,probe,lean shape]", _PF, "lean", 4, "unsupported", tiled=True, probe=True)
_pyr_case("ops.defcorr_pyramid_forward[tiled,w2_not_mult4]", _PF, "w2_not_mult4", 3, "unsupported", tiled=True, plan=False)
# a refusal for the last of several launches must come before the first one
_pyr_case("DefcorrPyramidPlan[tiled,mixed nulls]", _PF, "mixed_nulls", 3, "unsupported", offs=(0, 2), tiled=True)
_pyr_case("DefcorrPyramidPlan[row-major,mixed nulls]", _PF, "mixed_nulls", 3, "same", offs=(0, 2))
_pyr_case("DefcorrPyramidPlan[slots]", _PS, "tiny", 3, "unsupported", mode="slots")
_pyr_case("DefcorrPyramidPlan[tiled,slots,lean shape]", _PS, "lean", 4, "unsupported", tiled=True, mode="slots")
_pyr_case("DefcorrPyramidPlan[coords_last]", _PF, "tiny", 3, "unsupported", mode="coords_last")
_pyr_case("DefcorrPyramidPlan[tiled,nhwc]", _PF, "tiny", 3, "unsupported", tiled=True, fmt="nhwc")
_pyr_case("DefcorrPyramidPlan[tiled,nhwc_f16]", _PF, "tiny", 3, "unsupported", tiled=True, fmt="nhwc_f16")
_pyr_case("DefcorrPyramidPlan[tiled,encoder]", _PE, "tiny", 3, "unsupported", out=A16("unsupported"), tiled=True, enc=True)


# ======================================================================================================================
# ops: the low-memory samplers — (2, 1, 12x16 onto 6x8, C 128, r 3), (1, 2, 8x16, C 32, r 1); altcorr (3, 1, .., r 1)
# ======================================================================================================================
def _fmap_inputs(cfg, half=False, grad=False):
    B, S, H1, W1, H2, W2, C, radius, sigma, scale = cfg

    def build(dev):
        c = inputs.fmap_case(40 + H2, B, S, H1, W1, H2, W2, C, radius, sigma, scale)
        a = {k: _d(v, dev) for k, v in c.items()}
        if half:
            a["fmap1"], a["fmap2"] = a["fmap1"].half(), a["fmap2"].half()
        if grad:
            rd = 2 * radius + 1
            a["corr_grad"] = _d(np.random.default_rng(60).standard_normal((B, S, rd * rd, H1, W1)).astype(np.float32), dev)
        return a
    return build


_LM_A = (2, 1, 12, 16, 6, 8, 128, 3, 3.0, 0.5)
_LM_B = (1, 2, 8, 16, 8, 16, 32, 1, 3.0, 1.0)
_ALT = (3, 1, 12, 16, 6, 8, 128, 1, 3.0, 0.5)

for _tag, _cfg in (("A", _LM_A), ("B", _LM_B)):
    _r = _cfg[7]
    # matrix-core kernel -> tile kernel -> wave-per-pixel kernel (element accesses): another channel summation order,
    # held to the 1e-5 of test_lowmem_defsample against the oracle
    case("ops.lowMem_defSample[%s]" % _tag, ["lgu_lowmem_defsample_fwd_f32"], "reference", _fmap_inputs(_cfg),
         (lambda r: lambda lgu, a: tuple(lgu.ops.lowMem_defSample(a["fmap1"], a["fmap2"], a["coords"], a["offset"], r)))(_r),
         dict(fmap1=A16("fallback"), fmap2=A16("fallback"), coords=A8("fallback"), offset=A8("fallback")), inplace=("offset",),
         bound=((lambda r: lambda O, h: list(O.lowMem_defSample(h["fmap1"], h["fmap2"], h["coords"], h["offset"].copy(), r)))(_r), ABS_1E5))
    # half maps: matrix-core kernels and the tile kernel only
    case("ops.lowMem_defSample_mixed[%s]" % _tag, ["lgu_lowmem_defsample_fwd_h16"], "own", _fmap_inputs(_cfg, half=True),
         (lambda r: lambda lgu, a: tuple(lgu.ops.lowMem_defSample_mixed(a["fmap1"], a["fmap2"], a["coords"], a["offset"], r)))(_r),
         dict(fmap1=A16("unsupported"), fmap2=A16("unsupported"), coords=A8("unsupported"), offset=A8("unsupported")),
         inplace=("offset",))

case("ops.altcorr_forward", ["lgu_altcorr_fwd_f32"], "reference", _pick(_fmap_inputs(_ALT), "fmap1", "fmap2", "coords"),
     lambda lgu, a: tuple(lgu.ops.altcorr_forward(a["fmap1"], a["fmap2"], a["coords"], 1)),
     dict(fmap1=A16("fallback"), fmap2=A16("fallback"), coords=A8("fallback")),
     bound=(lambda O, h: list(O.altcorr_forward(h["fmap1"], h["fmap2"], h["coords"], 1)), ABS_1E5))
case("ops.altcorr_forward_mixed", ["lgu_altcorr_fwd_h16"], "own", _pick(_fmap_inputs(_ALT, half=True), "fmap1", "fmap2", "coords"),
     lambda lgu, a: tuple(lgu.ops.altcorr_forward_mixed(a["fmap1"], a["fmap2"], a["coords"], 1)),
     dict(fmap1=A16("unsupported"), fmap2=A16("unsupported"), coords=A8("unsupported")))
# one kernel, element accesses, global float atomics into fmap2_grad: the bound of test_altcorr_forward_backward
case("ops.altcorr_backward", ["lgu_altcorr_bwd_f32"], "reference", _pick(_fmap_inputs(_ALT, grad=True), "fmap1", "fmap2", "coords", "corr_grad"),
     lambda lgu, a: tuple(lgu.ops.altcorr_backward(a["fmap1"], a["fmap2"], a["coords"], a["corr_grad"], 1)[:2]),
     dict(fmap1=SAME, fmap2=SAME, coords=SAME, corr_grad=SAME),
     bound=(lambda O, h: list(O.altcorr_backward(h["fmap1"], h["fmap2"], h["coords"], h["corr_grad"], 1)[:2]), REL_1E5))


def _ctypes_lowmem(which):
    """corr of the caller's: vec_out of the matrix-core kernels (16-byte stores <-> element stores of the same values)."""
    cfg = _LM_A if which != "altcorr" else _ALT
    B, S, H1, W1, H2, W2, C, radius = cfg[:8]
    rd = 2 * radius + 1

    def build(dev):
        a = _fmap_inputs(cfg, half=which.endswith("h16"))(dev)
        if which.startswith("altcorr"):
            del a["offset"]
        a["out"] = torch.full((B, S, rd * rd, H1, W1), 7.0, device=dev)
        return a

    def call(lgu, a):
        lib = lgu._lib.load()
        if which.startswith("altcorr"):
            fn = lib.lgu_altcorr_fwd_h16 if which.endswith("h16") else lib.lgu_altcorr_fwd_f32
            rc = fn(_p(a["fmap1"]), _p(a["fmap2"]), _p(a["coords"]), _p(a["out"]), B, S, H1, W1, H2, W2, C, radius, _st(a["out"]))
        else:
            fn = lib.lgu_lowmem_defsample_fwd_h16 if which.endswith("h16") else lib.lgu_lowmem_defsample_fwd_f32
            rc = fn(_p(a["fmap1"]), _p(a["fmap2"]), _p(a["coords"]), _p(a["offset"]), _p(a["out"]), B, S, H1, W1, H2, W2, C, B, radius,
                    _st(a["out"]))
        _check(lgu, rc, which)
        return (a["out"],)
    return build, call


for _w, _sym in (("lowmem_f32", "lgu_lowmem_defsample_fwd_f32"), ("lowmem_h16", "lgu_lowmem_defsample_fwd_h16"),
                 ("altcorr_f32", "lgu_altcorr_fwd_f32"), ("altcorr_h16", "lgu_altcorr_fwd_h16")):
    _b, _c = _ctypes_lowmem(_w)
    case("c.%s[corr]" % _sym, [_sym], "reference" if _w.endswith("f32") else "own", _b, _c, dict(out=A16("same")), inplace=("out",))


# ---- LowmemPyramidPlan: row-major, chunked, ii / jj, several calls ----------------------------------------------------
def _lmp_inputs(form, half, small=False):
    def build(dev):
        import lgu_slam_amd as lgu
        g = _gen(71)
        if small:      # (1, 2, 8x16, C 32, r 1): two samples per pixel, one level
            B, S, H, W, C, radius, L, noffs = 1, 2, 8, 16, 32, 1, 1, 1
        else:          # (2, 1, 12x16 onto 12x16 / 6x8 / 3x4, C 128, r 3): offsets on levels 0-1 as AltCorrBlock has them
            B, S, H, W, C, radius, L, noffs = 2, 1, 12, 16, 128, 3, 3, 2
        rd = 2 * radius + 1
        F = 3 if form in ("iijj", "calls") else B
        dt = torch.float16 if half else torch.float32
        a = {"fmap1": _randn(g, (F, H, W, C), dev, 0.125, dt)}
        for l in range(L):
            f2 = _randn(g, (F, max(H >> l, 1), max(W >> l, 1), C), dev, 0.125, dt)
            a["f2_%d" % l] = lgu.ops.lowmem_chunked(f2) if form in ("chunked", "calls") else f2
        ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
        a["coords"] = (torch.stack([xs, ys], -1)[None, None] + torch.randn((B, S, H, W, 2), generator=g) * 3).to(dev).contiguous()
        NO = 2 if form == "calls" else max(B, 2)
        for l in range(noffs):
            a["off%d" % l] = (4 * torch.tanh(torch.randn((NO, H, W, rd, rd, 2), generator=g))).to(dev)
        if form in ("iijj", "calls"):
            a["ii"] = torch.tensor([2, 0][:B], dtype=torch.int64, device=dev)
            a["jj"] = torch.tensor([1, 2][:B], dtype=torch.int64, device=dev)
        if form == "calls":
            a["off_row"] = torch.tensor([1, 0][:B], dtype=torch.int32, device=dev)
        a["out"] = torch.full((B, S, L * rd * rd, H, W), 7.0, device=dev)
        return a
    L, noffs, radius = (1, 1, 1) if small else (3, 2, 3)

    def call(lgu, a):
        offs = [a.get("off%d" % l) for l in range(L)]
        pl = lgu.ops.LowmemPyramidPlan(a["fmap1"], [a["f2_%d" % l] for l in range(L)], offs, radius, ii=a.get("ii"), jj=a.get("jj"),
                                       chunked=form in ("chunked", "calls"), off_row=a.get("off_row"))
        return (pl(a["coords"], out=a["out"]),)
    ops = {"fmap1": A16("unsupported"), "coords": A8("unsupported"), "out": A16("same")}
    for l in range(L):
        ops["f2_%d" % l] = A16("unsupported")
    for l in range(noffs):
        ops["off%d" % l] = A8("unsupported")
    if form in ("iijj", "calls"):
        ops["ii"], ops["jj"] = SAME, SAME
    if form == "calls":
        ops["off_row"] = SAME
    return build, call, ops, tuple("off%d" % l for l in range(noffs)) + ("out",)


for _form, _half, _small, _sym in (("rowmajor", True, False, "lgu_lowmem_pyramid_fwd_h16"), ("rowmajor", False, False, "lgu_lowmem_pyramid_fwd_f32"),
                                   ("rowmajor", True, True, "lgu_lowmem_pyramid_fwd_h16"), ("rowmajor", False, True, "lgu_lowmem_pyramid_fwd_f32"),
                                   ("chunked", True, False, "lgu_lowmem_pyramid_chunked_fwd_h16"),
                                   ("chunked", False, False, "lgu_lowmem_pyramid_chunked_fwd_f32"),
                                   ("iijj", True, False, "lgu_lowmem_pyramid_fwd_h16"), ("iijj", False, False, "lgu_lowmem_pyramid_fwd_f32"),
                                   ("calls", True, False, "lgu_lowmem_pyramid_calls_fwd_h16")):
    _b, _c, _o, _i = _lmp_inputs(_form, _half, _small)
    case("LowmemPyramidPlan[%s,%s%s]" % (_form, "h16" if _half else "f32", ",S2 r1" if _small else ""), [_sym], "own", _b, _c, _o, inplace=_i)


_b, _c, _o, _i = _lmp_inputs("rowmajor", True, False)
case("ops.lowmem_pyramid_forward_mixed", ["lgu_lowmem_pyramid_fwd_h16"], "own", _b,
     lambda lgu, a: (lgu.ops.lowmem_pyramid_forward_mixed(a["fmap1"], [a["f2_%d" % l] for l in range(3)], a["coords"],
                                                          [a["off0"], a["off1"], None], 3, out=a["out"]),), _o, inplace=_i)


# ======================================================================================================================
# ops: the offset heads and their post-processing
# ======================================================================================================================
def _gp_inputs(half):
    def build(dev):
        g = _gen(23)
        dt = torch.float16 if half else torch.float32
        return dict(mean_ofs=_randn(g, (2, 63, 2), dev, 2.0, dt), cov_raw=_randn(g, (2, 63, 2), dev, 1.0, dt))
    return build


for _h in (False, True):
    case("ops.gaussian_params[%s]" % ("h16" if _h else "f32"), ["lgu_gaussian_params"], "own", _gp_inputs(_h),
         lambda lgu, a: tuple(lgu.ops.gaussian_params(a["mean_ofs"], a["cov_raw"], 7, 9)), dict(mean_ofs=SAME, cov_raw=SAME))


def _pms_inputs(dev):
    g = _gen(29)
    return dict(probe=_randn(g, (2, 9, 7, 9), dev), offset=_randn(g, (2, 7, 9, 98), dev, 2.0))


case("ops.probe_mask_scale_", ["lgu_probe_mask_scale_f32"], "own", _pms_inputs,
     lambda lgu, a: (lgu.ops.probe_mask_scale_(a["probe"], a["offset"]).clone(),), dict(probe=SAME, offset=SAME), inplace=("offset",))


def _of_inputs(half, probe):
    def build(dev):
        g = _gen(31)
        dt = torch.float16 if half else torch.float32
        a = dict(o0=_randn(g, (2, 98, 25, 37), dev, 1.0, dt), o1=_randn(g, (2, 98, 12, 18), dev, 1.0, dt))
        if probe:
            a["probe"] = _randn(g, (2, 9, 25, 37), dev)
        return a
    return build


for _h in (False, True):
    case("ops.offsets_finalize[%s]" % ("h16" if _h else "f32"), ["lgu_offsets_finalize"], "own", _of_inputs(_h, False),
         lambda lgu, a: tuple(lgu.ops.offsets_finalize(a["o0"], a["o1"], autocast=False)), dict(o0=SAME, o1=SAME))
case("ops.offsets_finalize[masked]", ["lgu_offsets_finalize_masked"], "own", _of_inputs(False, True),
     lambda lgu, a: tuple(lgu.ops.offsets_finalize(a["o0"], a["o1"], autocast=False, probe=a["probe"])), dict(o0=SAME, o1=SAME, probe=SAME))


def _oc_inputs(cfg, lo, parts=False):
    E, NF, H, W = cfg

    def build(dev):
        import lgu_slam_amd as lgu
        g = _gen(E * 100 + H)
        weight, bias = _randn(g, (98, 256, 3, 3), dev, 0.02), _randn(g, (98,), dev, 0.1)
        a = dict(frames=_randn(g, (NF, H, W, 128), dev, 0.125, torch.float16),
                 ii=torch.randint(0, NF, (E,), generator=g).to(dev), jj=torch.randint(0, NF, (E,), generator=g).to(dev))
        if lo:
            a["frames_lo"] = _randn(g, (NF, H, W, 128), dev, 1e-4, torch.float16)
        if parts:
            a["wpack_a"], a["wpack_b"], a["bias"], _, _ = lgu.ops.pack_offset_conv_parts(weight, bias)
        else:
            a["wpack"], a["bias"], _, _ = lgu.ops.pack_offset_conv(weight, bias)
        return a
    return build


for _cfg in ((1, 2, 7, 9), (3, 4, 13, 21)):
    for _lo in (False, True):
        _ops = dict(frames=A16("unsupported"), ii=SAME, jj=SAME, wpack=A16("unsupported"), bias=SAME)
        if _lo:
            _ops["frames_lo"] = A16("unsupported")
        case("ops.offset_conv_frames[%s%s]" % ("x".join(map(str, _cfg)), ",lo" if _lo else ""), ["lgu_offset_conv_frames_h16"], "own",
             _oc_inputs(_cfg, _lo),
             lambda lgu, a: (lgu.ops.offset_conv_frames(a["frames"], a["ii"], a["jj"], (a["wpack"], a["bias"], 98, 128),
                                                        frames_lo=a.get("frames_lo")),), _ops)


def _ctypes_offset_conv(lgu, a):
    NF, H, W, C = a["frames"].shape
    E = a["ii"].shape[0]
    _check(lgu, lgu._lib.load().lgu_offset_conv_frames_h16(_p(a["frames"]), None, _p(a["ii"]), _p(a["jj"]), _p(a["wpack"]), _p(a["bias"]),
                                                           _p(a["out"]), E, H, W, C, 98, _st(a["out"])), "offset_conv_frames")
    return (a["out"],)


case("c.lgu_offset_conv_frames_h16[out]", ["lgu_offset_conv_frames_h16"], "own",
     _with_out(_oc_inputs((3, 4, 13, 21), False), lambda a: (a["ii"].shape[0], 98) + tuple(a["frames"].shape[1:3])), _ctypes_offset_conv,
     dict(out=A16("unsupported")), inplace=("out",))


def _wl_inputs(dev):
    a = _oc_inputs((3, 4, 12, 20), True, parts=True)(dev)
    a["worklist"] = torch.tensor([0, 3, 5], dtype=torch.int32, device=dev)     # frame 0 as source, frames 1 and 2 as target
    a["count"] = torch.tensor([3], dtype=torch.int32, device=dev)
    a["PA"] = torch.full((4, 98, 12, 20), 7.0, device=dev)
    a["PB"] = torch.full((4, 98, 12, 20), 7.0, device=dev)
    return a


def _c_worklist(lgu, a):
    NF, H, W, C = a["frames"].shape
    _check(lgu, lgu._lib.load().lgu_offset_conv_worklist_h16(_p(a["frames"]), _p(a["frames_lo"]), _p(a["worklist"]), _p(a["count"]), 3,
                                                             _p(a["wpack_a"]), _p(a["wpack_b"]), _p(a["bias"]), _p(a["PA"]), _p(a["PB"]), H, W,
                                                             C, 98, _st(a["PA"])), "offset_conv_worklist")
    return (a["PA"], a["PB"])


case("c.lgu_offset_conv_worklist_h16[PA,PB]", ["lgu_offset_conv_worklist_h16"], "own", _wl_inputs, _c_worklist,
     dict(PA=A16("unsupported"), PB=A16("unsupported"), worklist=SAME, count=SAME), inplace=("PA", "PB"))


def _cmb_inputs(dev):
    g = _gen(37)
    return dict(PA=_randn(g, (4, 24), dev), PB=_randn(g, (4, 24), dev), ii=torch.tensor([3, 0, 1], dtype=torch.int64, device=dev),
                jj=torch.tensor([1, 2, 2], dtype=torch.int64, device=dev), out=torch.full((3, 24), 7.0, device=dev))


def _c_combine(lgu, a):
    _check(lgu, lgu._lib.load().lgu_offset_heads_combine_f32(_p(a["PA"]), _p(a["PB"]), _p(a["ii"]), _p(a["jj"]), _p(a["out"]), 3, 24, None,
                                                             _st(a["out"])), "offset_heads_combine")
    return (a["out"],)


case("c.lgu_offset_heads_combine_f32[PA,PB,out]", ["lgu_offset_heads_combine_f32"], "own", _cmb_inputs, _c_combine,
     dict(PA=A16("unsupported"), PB=A16("unsupported"), out=A16("unsupported"), ii=SAME, jj=SAME), inplace=("out",))


def _fin_inputs(dev):
    import lgu_slam_amd as lgu
    a = _of_inputs(False, False)(dev)
    a["out0"], a["out1"] = torch.full((2, 25, 37, 98), 7.0, device=dev), torch.full((2, 25, 37, 98), 7.0, device=dev)
    a["scratch"] = torch.zeros(int(lgu._lib.load().lgu_offsets_finalize_scratch_bytes(2)), dtype=torch.uint8, device=dev)
    return a


def _c_finalize(lgu, a):
    _check(lgu, lgu._lib.load().lgu_offsets_finalize(_p(a["o0"]), _p(a["o1"]), _p(a["out0"]), _p(a["out1"]), _p(a["scratch"]), 2, 98, 25, 37,
                                                     12, 18, 0, 1e-5, _st(a["out0"])), "offsets_finalize")
    return (a["out0"], a["out1"])


# scratch holds doubles in an untyped buffer: LGU_E_BADARG below 8 bytes
case("c.lgu_offsets_finalize[scratch]", ["lgu_offsets_finalize"], "own", _fin_inputs, _c_finalize,
     dict(scratch=Op(8, "badarg"), out0=SAME, out1=SAME), inplace=("out0", "out1", "scratch"))   # partial sums: no atomics, fixed order


def _ohc_call(lgu, a):
    cache = lgu.ops.OffsetHeadCache(a["frames"], (a["wpack_a"], a["wpack_b"], a["bias"], 98, 128), frames_lo=a.get("frames_lo"))
    return (cache(a["ii"], a["jj"]),)


# the cache's partial planes PA / PB, its flags, worklist and count are its own allocations
case("ops.OffsetHeadCache", ["lgu_offset_heads_mark", "lgu_offset_conv_worklist_h16", "lgu_offset_heads_combine_f32"], "own",
     _oc_inputs((3, 4, 12, 20), True, parts=True), _ohc_call,
     dict(frames=A16("unsupported"), frames_lo=A16("unsupported"), ii=SAME, jj=SAME, wpack_a=A16("unsupported"),
          wpack_b=A16("unsupported"), bias=SAME))


# ======================================================================================================================
# geom: element accesses throughout, except the pair / quad stores of the reprojection outputs (allocated inside) and
# the 8-byte loads of motion_features' target
# ======================================================================================================================
def _geom_inputs(batched=False, target=False):
    def build(dev):
        g = _gen(41)
        N, ht, wd = 6, 12, 16
        poses = torch.zeros((N, 7))
        poses[:, :3] = torch.randn((N, 3), generator=g) * 0.2
        q = torch.randn((N, 4), generator=g) * 0.1 + torch.tensor([0.0, 0.0, 0.0, 1.0])
        poses[:, 3:] = q / q.norm(dim=1, keepdim=True)
        a = dict(poses=poses.to(dev), disps=(torch.rand((N, ht, wd), generator=g) * 0.7 + 0.3).to(dev),
                 intrinsics=torch.tensor([20.0, 20.0, wd / 2, ht / 2]).to(dev),
                 ii=torch.tensor([0, 1, 2, 3, 5, 2], dtype=torch.int64).to(dev), jj=torch.tensor([1, 0, 4, 3, 2, 5], dtype=torch.int64).to(dev))
        if batched:
            a["poses"], a["disps"] = a["poses"][None].contiguous(), a["disps"][None].contiguous()
            a["intrinsics"] = a["intrinsics"][None, None].repeat(1, N, 1).contiguous()
        if target:
            a["target"] = _randn(g, (1, 6, ht, wd, 2), dev, 8.0)
        return a
    return build


_G5 = dict(poses=SAME, disps=SAME, intrinsics=SAME, ii=SAME, jj=SAME)
case("geom.frame_distance", ["lgu_frame_distance_f32"], "reference", _geom_inputs(),
     lambda lgu, a: (lgu.geom.frame_distance(a["poses"], a["disps"], a["intrinsics"], a["ii"], a["jj"], 0.25),), _G5)
case("geom.projmap", ["lgu_projmap_f32"], "reference", _geom_inputs(),
     lambda lgu, a: tuple(lgu.geom.projmap(a["poses"], a["disps"], a["intrinsics"], a["ii"], a["jj"])), _G5)


def _df_inputs(dev):
    a = _geom_inputs()(dev)
    return dict(poses=a["poses"], disps=a["disps"], intrinsics=a["intrinsics"], ix=torch.tensor([0, 2, 3, 5], dtype=torch.int64).to(dev),
                thresh=torch.tensor([0.1, 0.2, 0.05, 0.3]).to(dev))


case("geom.depth_filter", ["lgu_depth_filter_f32"], "reference", _df_inputs,
     lambda lgu, a: (lgu.geom.depth_filter(a["poses"], a["disps"], a["intrinsics"], a["ix"], a["thresh"]),),
     dict(poses=SAME, disps=SAME, intrinsics=SAME, ix=SAME, thresh=SAME))
case("geom.iproj", ["lgu_iproj_f32"], "reference", _pick(_geom_inputs(), "poses", "disps", "intrinsics"),
     lambda lgu, a: (lgu.geom.iproj(a["poses"], a["disps"], a["intrinsics"]),), dict(poses=SAME, disps=SAME, intrinsics=SAME))
for _jac, _dep in ((False, False), (True, False), (False, True)):
    case("geom.projective_transform[%s]" % ("jacobian" if _jac else "depth" if _dep else "plain"), ["lgu_projective_transform_f32"], "own",
         _geom_inputs(batched=True),
         (lambda j, d: lambda lgu, a: (lambda r: tuple(r[:2]) + (tuple(r[2]) if j else ()))(
             lgu.geom.projective_transform(a["poses"], a["disps"], a["intrinsics"], a["ii"], a["jj"], jacobian=j, return_depth=d)))(_jac, _dep),
         _G5)


def _reproject_inputs(dev):
    a = _geom_inputs(batched=True)(dev)
    return dict(poses=a["poses"][0].contiguous(), disps=a["disps"][0].contiguous(), intrinsics=a["intrinsics"][0].contiguous(),
                ii=a["ii"], jj=a["jj"])


case("geom.reproject", ["lgu_projective_transform_f32"], "own", _reproject_inputs,
     lambda lgu, a: tuple(lgu.geom.reproject(a["poses"], a["disps"], a["intrinsics"], a["ii"], a["jj"])), _G5)
case("geom.motion_features", ["lgu_motion_features_f32"], "own", _geom_inputs(batched=True, target=True),
     lambda lgu, a: tuple(lgu.geom.motion_features(a["poses"], a["disps"], a["intrinsics"], a["ii"], a["jj"], a["target"])),
     dict(_G5, target=A8("unsupported")))


# ======================================================================================================================
# aggregate
# ======================================================================================================================
def _sm_inputs(half):
    def build(dev):
        g = _gen(43)
        return dict(src=_randn(g, (2, 11, 24), dev, 1.0, torch.float16 if half else torch.float32),
                    index=torch.tensor([0, 2, 2, 1, 0, 4, 4, 4, 1, 0, 2], dtype=torch.int64).to(dev))
    return build


for _h in (False, True):
    _sym = "lgu_scatter_mean_%s" % ("h16" if _h else "f32")
    # 16-byte loads <-> element loads; sums in ascending j either way ("the bits do not depend on the launch geometry")
    case("aggregate.scatter_mean[%s]" % ("h16" if _h else "f32"), [_sym], "reference", _sm_inputs(_h),
         lambda lgu, a: (lgu.aggregate.scatter_mean(a["src"], a["index"], dim=1, dim_size=5),), dict(src=A16("same"), index=SAME))

    def _c_sm(lgu, a, _sym=_sym):
        _check(lgu, getattr(lgu._lib.load(), _sym)(_p(a["src"]), _p(a["index"]), 2, 11, 24, 5, _p(a["out"]), _st(a["out"])), "scatter_mean")
        return (a["out"],)
    case("c.%s[out]" % _sym, [_sym], "reference",
         _with_out(_sm_inputs(_h), lambda a: (2, 5, 24), dtype=torch.float16 if _h else torch.float32), _c_sm, dict(out=A16("same")),
         inplace=("out",))


def _ups_inputs(half, indexed):
    def build(dev):
        g = _gen(47)
        N, ht, wd = 3, 6, 8
        a = dict(mask=_randn(g, (2 if indexed else N, 576, ht, wd), dev, 1.0, torch.float16 if half else torch.float32))
        if indexed:
            a.update(disps=_randn(g, (N, ht, wd), dev).abs() + 0.1, ix=torch.tensor([2, 0], dtype=torch.int64).to(dev),
                     disps_up=_randn(g, (N, 8 * ht, 8 * wd), dev))
        else:
            a["data"] = _randn(g, (N, ht, wd, 1), dev)
        return a
    return build


for _h in (False, True):
    # the default build reads the mask one coarse pixel at a time (LGU_CVX_XV = 1): element accesses
    case("aggregate.cvx_upsample[%s mask]" % ("h16" if _h else "f32"), ["lgu_cvx_upsample_f32"], "own", _ups_inputs(_h, False),
         lambda lgu, a: (lgu.aggregate.cvx_upsample(a["data"], a["mask"]),), dict(data=SAME, mask=SAME))
    # disps_up is written as 16-byte quads: no element-store twin
    case("aggregate.upsample_disps_[%s mask]" % ("h16" if _h else "f32"), ["lgu_upsample_disps_f32"], "own", _ups_inputs(_h, True),
         lambda lgu, a: (lgu.aggregate.upsample_disps_(a["disps_up"], a["disps"], a["ix"], a["mask"]).clone(),),
         dict(disps_up=A16("unsupported"), disps=SAME, ix=SAME, mask=SAME), inplace=("disps_up",))


def _upd_inputs(dev):
    g = _gen(49)
    return dict(disp=_randn(g, (1, 3, 6, 8), dev), mask=_randn(g, (1, 3, 576, 6, 8), dev))


case("aggregate.upsample_disp", ["lgu_cvx_upsample_f32"], "own", _upd_inputs,
     lambda lgu, a: (lgu.aggregate.upsample_disp(a["disp"], a["mask"]),), dict(disp=SAME, mask=SAME))


def _c_cvx(lgu, a):
    N, ht, wd, _ = a["data"].shape
    _check(lgu, lgu._lib.load().lgu_cvx_upsample_f32(_p(a["data"]), _p(a["mask"]), N, ht, wd, 0, _p(a["out"]), _st(a["out"])), "cvx_upsample")
    return (a["out"],)


case("c.lgu_cvx_upsample_f32[out]", ["lgu_cvx_upsample_f32"], "own", _with_out(_ups_inputs(False, False), lambda a: (3, 48, 64)), _c_cvx,
     dict(out=A16("unsupported")), inplace=("out",))


# ======================================================================================================================
# gru: the KAN-bias GRU entries (E 2, 6 x 8)
# ======================================================================================================================
def _gru_inputs(half, which):
    def build(dev):
        g = _gen(53)
        dt = torch.float16 if half else torch.float32
        E, H, W = 2, 6, 8
        r = lambda *s, sc=0.5: _randn(g, s, dev, sc, dt)   # noqa: E731
        if which == "context":
            return dict(net=r(E, 128, H, W), weight=r(128, 128, sc=0.05), bias=r(128, sc=0.1))
        if which == "heads":
            knots = torch.linspace(-2.2, 2.2, 10).repeat(3, 128, 1).contiguous().to(dev)
            return dict(glo=r(E, 128), grid=knots, wpack=r(384, 896, sc=0.05))
        if which == "gates":
            return dict(net_inp=r(E, 448, H, W), cz=r(E, 128, H, W), cr=r(E, 128, H, W), kz=r(E, 128), kr=r(E, 128), net=r(E, 128, H, W))
        return dict(cq=r(E, 128, H, W), kq=r(E, 128), z=torch.sigmoid(r(E, 128, H, W).float()).to(dt), net=r(E, 128, H, W))
    return build


for _h in (False, True):
    _s = "h16" if _h else "f32"
    case("gru.kangru_context[%s]" % _s, ["lgu_kangru_context_" + _s], "own", _gru_inputs(_h, "context"),
         lambda lgu, a: (lgu.gru.kangru_context(a["net"], a["weight"], a["bias"]),),
         dict(net=A16("same"), weight=A16("unsupported"), bias=SAME))
    case("gru.kan_heads[%s]" % _s, ["lgu_kan_heads_" + _s], "own", _gru_inputs(_h, "heads"),
         lambda lgu, a: (lgu.gru.kan_heads(a["glo"], a["grid"], a["wpack"]),), dict(glo=SAME, grid=SAME, wpack=A16("unsupported")))
    case("gru.kangru_gates_[%s]" % _s, ["lgu_kangru_gates_" + _s], "own", _gru_inputs(_h, "gates"),
         lambda lgu, a: (lgu.gru.kangru_gates_(a["net_inp"], a["cz"], a["cr"], a["kz"], a["kr"], a["net"]),),
         dict(net_inp=A16("same"), cz=A16("same"), cr=A16("same"), kz=SAME, kr=SAME, net=A16("same")), inplace=("net_inp",))
    case("gru.kangru_blend[%s]" % _s, ["lgu_kangru_blend_" + _s], "own", _gru_inputs(_h, "blend"),
         lambda lgu, a: (lgu.gru.kangru_blend(a["cq"], a["kq"], a["z"], a["net"]),), dict(cq=A16("same"), kq=SAME, z=A16("same"), net=A16("same")))


# ======================================================================================================================
# features: instance norm (operands at element alignment by contract: "the bits do not depend on the address") and the
# frame normalisation
# ======================================================================================================================
def _in_inputs(half, mode):
    def build(dev):
        g = _gen(59)
        dt = torch.float16 if half else torch.float32
        a = dict(a=_randn(g, (2, 3, 7, 9), dev, 1.0, dt), out=torch.full((2, 3, 7, 9), 7.0, dtype=dt, device=dev))
        if mode in (1, 2):
            a["residual"] = _randn(g, (2, 3, 7, 9), dev, 1.0, dt)
        return a
    return build


for _h in (False, True):
    for _m in (0, 1, 2, 3):
        _ops = dict(a=SAME, out=SAME)
        if _m in (1, 2):
            _ops["residual"] = SAME
        case("features.instance_norm_relu[%s,mode %d]" % ("h16" if _h else "f32", _m), ["lgu_instnorm_relu_%s" % ("h16" if _h else "f32")], "own",
             _in_inputs(_h, _m),
             (lambda m: lambda lgu, a: (lgu.features.instance_norm_relu(a["a"], a.get("residual"), norm_residual=(m == 2), relu=(m != 3),
                                                                        out=a["out"]),))(_m), _ops, inplace=("out",))


def _img_inputs(dev):
    return dict(image=torch.randint(0, 256, (2, 3, 6, 8), generator=_gen(61), dtype=torch.uint8).to(dev))


# uchar4 loads / float4 stores when img is 4-byte aligned, by element otherwise: the same three fp32 operations
case("features.normalize_images", ["lgu_image_normalize_u8"], "own", _img_inputs,
     lambda lgu, a: (lgu.features.normalize_images(a["image"]),), dict(image=Op(4, "same")))


# ======================================================================================================================
# lie: the group operations (the drop-in lietorch exports SO3 / SE3)
# ======================================================================================================================
def _lie_inputs(K):
    def build(dev):
        g = _gen(67)
        n = 5
        G = torch.randn((n, K), generator=g) * 0.3
        q = torch.randn((n, 4), generator=g)
        G[:, K - 4:] = q / q.norm(dim=1, keepdim=True)
        H = G.flip(0).contiguous()
        T = 6 if K == 7 else 3
        return dict(G=G.to(dev), H=H.to(dev), a=_randn(g, (n, T), dev, 0.3), p3=_randn(g, (n, 3), dev), p4=_randn(g, (n, 4), dev))
    return build


def _lie_call(K):
    def call(lgu, a):
        cls = lgu.lie.SE3 if K == 7 else lgu.lie.SO3
        X = cls(a["G"])
        return (X.inv().data, X.log(), X.matrix(), X.mul(cls(a["H"])).data, X.retr(a["a"]).data, cls.exp(a["a"]).data, X.act(a["p3"]),
                X.act(a["p4"]), X.adj(a["a"]), X.adjT(a["a"]))
    return call


_LIE = ["lgu_lie_inv_f32", "lgu_lie_log_f32", "lgu_lie_matrix_f32", "lgu_lie_mul_f32", "lgu_lie_retr_f32", "lgu_lie_exp_f32",
        "lgu_lie_act_f32", "lgu_lie_adj_f32"]
for _K in (7, 4):
    # act / adj stream their operand with 16-byte accesses when it is aligned, by element otherwise
    case("lie.%s" % ("SE3" if _K == 7 else "SO3"), _LIE, "reference", _lie_inputs(_K), _lie_call(_K),
         dict(G=SAME, H=SAME, a=A16("same"), p3=A16("same"), p4=A16("same")))


# ======================================================================================================================
# graph: proximity edges, both forms
# ======================================================================================================================
def _prox_inputs(dev):
    a = _geom_inputs()(dev)
    return dict(poses=a["poses"], disps=a["disps"], intrinsics=a["intrinsics"], ii_known=torch.tensor([0, 1, 3], dtype=torch.int64).to(dev),
                jj_known=torch.tensor([1, 0, 5], dtype=torch.int64).to(dev))


for _form, _syms in (("small", ["lgu_proximity_select_small"]), ("sorted", ["lgu_proximity_keys", "lgu_proximity_select_sorted"])):
    case("graph.proximity_edges[%s]" % _form, _syms + ["lgu_frame_distance_f32"], "own", _prox_inputs,
         (lambda f: lambda lgu, a: tuple(lgu.graph.proximity_edges(a["poses"], a["disps"], a["intrinsics"], 6, a["ii_known"], a["jj_known"], t0=1,
                                                                   rad=1, nms=1, thresh=100.0, form=f)))(_form),
         dict(poses=SAME, disps=SAME, intrinsics=SAME, ii_known=SAME, jj_known=SAME))


_PX = dict(t=6, t0=1, t1=0, rad=1, nms=1)      # 30 cells: one 32-bit word of bitmap


def _pkeys_inputs(dev):
    g = _gen(73)
    return dict(dist=(torch.rand((30,), generator=g) * 20).to(dev), keys=torch.full((30,), -7, dtype=torch.int64, device=dev),
                work=torch.full((4,), 9, dtype=torch.uint8, device=dev))


def _c_pkeys(lgu, a):
    _check(lgu, lgu._lib.load().lgu_proximity_keys(_p(a["dist"]), None, None, 0, _PX["t"], _PX["t0"], _PX["t1"], _PX["rad"], _PX["nms"], 16.0, 0,
                                                   _p(a["keys"]), _p(a["work"]), _st(a["keys"])), "proximity_keys")
    return (a["keys"], a["work"])


# work is a bitmap of 32-bit words that are or-ed atomically, handed over as void*: LGU_E_BADARG below 4 bytes
case("c.lgu_proximity_keys[work]", ["lgu_proximity_keys"], "own", _pkeys_inputs, _c_pkeys,
     dict(work=Op(4, "badarg"), keys=SAME, dist=SAME), inplace=("work", "keys"))


def _psorted_inputs(dev):
    import lgu_slam_amd as lgu
    a = _pkeys_inputs(dev)
    _c_pkeys(lgu, a)
    cap = int(lgu.graph.capacity(_PX["t"], _PX["t0"], _PX["t1"], _PX["rad"], False, -1))
    return dict(sorted_keys=torch.sort(a["keys"]).values.contiguous(), work=a["work"],
                e_ii=torch.full((cap,), -7, dtype=torch.int64, device=dev), e_jj=torch.full((cap,), -7, dtype=torch.int64, device=dev),
                count=torch.full((1,), -7, dtype=torch.int32, device=dev))


def _c_psorted(lgu, a):
    _check(lgu, lgu._lib.load().lgu_proximity_select_sorted(_p(a["sorted_keys"]), _p(a["work"]), _PX["t"], _PX["t0"], _PX["t1"], _PX["rad"],
                                                            _PX["nms"], -1, 0, _p(a["e_ii"]), _p(a["e_jj"]), a["e_ii"].numel(), _p(a["count"]),
                                                            _st(a["count"])), "proximity_select_sorted")
    return (a["e_ii"], a["e_jj"], a["count"])


case("c.lgu_proximity_select_sorted[work]", ["lgu_proximity_select_sorted"], "own", _psorted_inputs, _c_psorted,
     dict(work=Op(4, "badarg"), sorted_keys=SAME, e_ii=SAME, e_jj=SAME, count=SAME), inplace=("work", "e_ii", "e_jj", "count"))


def _chol_inputs(dev):
    import lgu_slam_amd as lgu
    g = _gen(79)
    P = 33      # the smallest window tests/test_ba.py solves this way
    M = torch.randn((6 * P, 6 * P), generator=g, dtype=torch.float64)
    return dict(A=(M @ M.t() + 6 * P * torch.eye(6 * P, dtype=torch.float64)).to(dev), b=torch.randn((6 * P,), generator=g, dtype=torch.float64).to(dev),
                x=torch.full((P, 6), 7.0, device=dev),
                work=torch.zeros(int(lgu._lib.load().lgu_ba_solve_blocked_work_doubles(P)), dtype=torch.float64, device=dev))


def _c_chol(lgu, a):
    _check(lgu, lgu._lib.load().lgu_ba_solve_blocked_f64(_p(a["A"]), _p(a["b"]), _p(a["x"]), _p(a["work"]), 33, 1e-4, 0.1, _st(a["x"])),
           "ba blocked solve")
    return (a["x"],)


# the one entry of the BA that loads 16 bytes at a time (A and work): LGU_E_BADARG, as tests/test_ba.py calls it
case("c.lgu_ba_solve_blocked_f64[A,work]", ["lgu_ba_solve_blocked_f64"], "own", _chol_inputs, _c_chol,
     dict(A=Op(16, "badarg"), work=Op(16, "badarg"), b=SAME, x=SAME), inplace=("A", "work", "x"))


# ======================================================================================================================
# ba: scene(N=5, H=12, W=16) of tests/test_ba.py
# ======================================================================================================================
def _ba_inputs(dev):
    from tests import test_ba as T
    rng, intr, poses, disps, ii, jj, targets = T.scene(4, N=5, H=12, W=16)
    p, d = T.perturb(rng, poses, disps, 2)
    weights = (0.5 + rng.random(targets.shape)).astype(np.float32)
    sens = (d * (rng.random(d.shape) > 0.5)).astype(np.float32)
    eta = np.full(d.shape, 1e-3, np.float32)
    return dict(poses=_d(p, dev), disps=_d(d, dev), intrinsics=_d(intr, dev), disps_sens=_d(sens, dev), targets=_d(targets, dev),
                weights=_d(weights, dev), eta=_d(eta, dev), ii=_d(ii.astype(np.int64), dev), jj=_d(jj.astype(np.int64), dev))


def _ba_call(lgu, a):
    dx, dz = lgu.ba.ba(a["poses"], a["disps"], a["intrinsics"], a["disps_sens"], a["targets"], a["weights"], a["eta"], a["ii"], a["jj"], 2, 5, 2,
                       1e-4, 0.1, False)
    return (dx, dz)


# every kernel of csrc/ba.hip reads and writes by element and sums in a fixed order
case("ba.ba", ["lgu_ba_build_f32", "lgu_ba_accum_f32", "lgu_ba_depth_system_f32", "lgu_ba_depth_update_f32", "lgu_ba_eet_f32", "lgu_ba_ev_f32",
               "lgu_ba_evt_f32", "lgu_ba_assemble_f64", "lgu_ba_solve_f64", "lgu_ba_pose_retr_f32"], "reference", _ba_inputs, _ba_call,
     dict(poses=SAME, disps=SAME, intrinsics=SAME, disps_sens=SAME, targets=SAME, weights=SAME, eta=SAME, ii=SAME, jj=SAME),
     inplace=("poses", "disps"))


# ======================================================================================================================
# The entries that take a parameter block by value (DESIGN.md sections 3.14-3.27), through their operator functions at
# (2, 9, 33): an odd width, two images, more than one tile.  Their operands at element alignment are served with the
# aligned call's bits; a pack (wpack, dpack) below 16 bytes is LGU_E_UNSUPPORTED.  The outputs these functions allocate
# themselves are shifted by the per-file tests (test_guard_bands_and_alignment of each operator's own file).
# ======================================================================================================================
PACK = A16("unsupported")
_N, _H, _W = 2, 9, 33


def _conv_w(g, cout, cin, k, dev, bias_scale=0.1):
    return _randn(g, (cout, cin, k, k), dev, (cin * k * k) ** -0.5), _randn(g, (cout,), dev, bias_scale)


def _layer_inputs(seed, cin, pack, x_half, extra=None):
    """x (2,cin,9,33) float32 or half, (wpack, bias) of pack(lgu)(weight, bias)."""
    def build(dev):
        import lgu_slam_amd as lgu
        g = _gen(seed)
        a = dict(x=_randn(g, (_N, cin, _H, _W), dev, 1.0, torch.float16 if x_half else torch.float32))
        a["wpack"], a["bias"] = pack(lgu, g, dev)
        if extra:
            extra(lgu, g, dev, a)
        return a
    return build


_XWB = dict(x=SAME, wpack=PACK, bias=SAME)

case("flow.flow_conv7_relu", ["lgu_flow_conv7_relu_h16"], "own",
     _layer_inputs(201, 4, lambda lgu, g, dev: lgu.flow.pack_conv7(*_conv_w(g, 128, 4, 7, dev)), False),
     lambda lgu, a: (lgu.flow.flow_conv7_relu(a["x"], a["wpack"], a["bias"]),), _XWB)
for _h, _co in ((False, 64), (True, 128)):
    case("conv3.conv3x3[%s x, Cout %d]" % ("h16" if _h else "f32", _co), ["lgu_conv3x3_c128_h16"], "own",
         _layer_inputs(203 + _co, 128, (lambda co: lambda lgu, g, dev: lgu.conv3.pack_conv3(*_conv_w(g, co, 128, 3, dev)))(_co), _h),
         lambda lgu, a: (lgu.conv3.conv3x3(a["x"], a["wpack"], a["bias"], relu=True),), _XWB)


def _fanout_inputs(x_half):
    def build(dev):
        import lgu_slam_amd as lgu
        g = _gen(207)
        a = dict(x=_randn(g, (_N, 128, _H, _W), dev, 1.0, torch.float16 if x_half else torch.float32))
        for i in range(3):
            a["w%d" % i], a["b%d" % i] = lgu.conv3.pack_conv3(*_conv_w(g, 128, 128, 3, dev))
        return a
    return build


for _h in (False, True):
    case("conv3.conv3x3_fanout[%s x]" % ("h16" if _h else "f32"), ["lgu_conv3x3_fanout_c128_h16"], "own", _fanout_inputs(_h),
         lambda lgu, a: tuple(lgu.conv3.conv3x3_fanout(a["x"], [(a["w%d" % i], a["b%d" % i]) for i in range(3)], relu=True)),
         dict(x=SAME, w0=PACK, w1=PACK, w2=PACK, b0=SAME, b1=SAME, b2=SAME))
for _h, _co, _act in ((False, 2, "none"), (True, 2, "sigmoid"), (False, 1, "softplus")):
    case("heads.head_conv3x3[%s x, Cout %d, %s]" % ("h16" if _h else "f32", _co, _act), ["lgu_head3x3_c128_h16"], "own",
         _layer_inputs(211 + _co, 128, (lambda co: lambda lgu, g, dev: lgu.heads.pack_head(*_conv_w(g, co, 128, 3, dev)))(_co), _h),
         (lambda act: lambda lgu, a: (lgu.heads.head_conv3x3(a["x"], a["wpack"], a["bias"], act=act),))(_act), _XWB)


def _pair_inputs(x_half, f32):
    def build(dev):
        import lgu_slam_amd as lgu
        g = _gen(217)
        dt = torch.float16 if x_half else torch.float32
        a = dict(d=_randn(g, (_N, 128, _H, _W), dev, 1.0, dt), w=_randn(g, (_N, 128, _H, _W), dev, 1.0, dt))
        a["wd"], a["bd"] = lgu.heads.pack_head(*_conv_w(g, 2, 128, 3, dev))
        a["ww"], a["bw"] = lgu.heads.pack_head(*_conv_w(g, 2, 128, 3, dev))
        if f32:
            a["coords"] = _randn(g, (1, _N, _H, _W, 2), dev, 8.0)
        return a
    return build


for _h, _f in ((False, False), (True, True)):
    _ops = dict(d=SAME, w=SAME, wd=PACK, ww=PACK, bd=SAME, bw=SAME)
    if _f:
        _ops["coords"] = A8("unsupported")      # a whole (x, y) pair per access
    case("heads.head_pair[%s x%s]" % ("h16" if _h else "f32", ", coords" if _f else ""), ["lgu_head3x3_pair_c128_h16"], "own",
         _pair_inputs(_h, _f),
         lambda lgu, a: tuple(lgu.heads.head_pair(a["d"], a["w"], (a["wd"], a["bd"]), (a["ww"], a["bw"]), coords=a.get("coords"))), _ops)


def _gruconv_inputs(mode):
    def build(dev):
        import lgu_slam_amd as lgu
        g = _gen(223)
        h16 = torch.float16
        convs = []
        for _ in range(2 if mode == "zr" else 1):
            c = torch.nn.Conv2d(448, 128, 3, padding=1)
            with torch.no_grad():
                w, b = _conv_w(g, 128, 448, 3, "cpu")
                c.weight.copy_(w)
                c.bias.copy_(b)
            convs.append(c.to(dev))
        a = {"seg%d" % i: _randn(g, (_N, ch, _H, _W), dev, 1.0, h16) for i, ch in enumerate((128, 128, 128, 64))}
        a["wpack"], a["bias"] = lgu.gru.pack_gruconv(convs if mode == "zr" else convs[0])
        if mode != "plain":
            a["k0"], a["net"] = _randn(g, (_N, 128), dev, 1.0, h16), _randn(g, (_N, 128, _H, _W), dev, 1.0, h16)
        if mode == "zr":
            a["k1"] = _randn(g, (_N, 128), dev, 1.0, h16)
        if mode == "q":
            a["z"] = torch.rand((_N, 128, _H, _W), generator=g).to(h16).to(dev)
        return a
    return build


def _gruconv_call(mode):
    def call(lgu, a):
        segs = [a["seg%d" % i] for i in range(4)]
        if mode == "plain":
            return (lgu.gru.gru_conv3x3(segs, a["wpack"], a["bias"]),)
        if mode == "zr":
            return tuple(lgu.gru.gru_conv_zr(segs, a["wpack"], a["bias"], a["k0"], a["k1"], a["net"]))
        return (lgu.gru.gru_conv_q(segs, a["wpack"], a["bias"], a["k0"], a["z"], a["net"]),)
    return call


for _m, _more in (("plain", ()), ("zr", ("k0", "k1", "net")), ("q", ("k0", "z", "net"))):
    _ops = dict({"seg%d" % i: SAME for i in range(4)}, wpack=PACK, bias=SAME)
    _ops.update({k: SAME for k in _more})
    case("gru.gru_conv[%s]" % _m, ["lgu_gruconv3x3_c448_h16"], "own", _gruconv_inputs(_m), _gruconv_call(_m), _ops)

for _h in (False, True):
    case("upmask.upmask_conv1x1[%s x]" % ("h16" if _h else "f32"), ["lgu_upmask1x1_c128_h16"], "own",
         _layer_inputs(227, 128, lambda lgu, g, dev: lgu.upmask.pack_upmask(*_conv_w(g, 576, 128, 1, dev)), _h),
         lambda lgu, a: (lgu.upmask.upmask_conv1x1(a["x"], a["wpack"], a["bias"]),), _XWB)


def _ups_net_inputs(x_half):
    def build(dev):
        import lgu_slam_amd as lgu
        g = _gen(229)
        U, N, ht, wd = 2, 4, 5, 7
        a = dict(x=_randn(g, (U, 128, ht, wd), dev, 1.0, torch.float16 if x_half else torch.float32))
        a["wpack"], a["bias"] = lgu.upmask.pack_upmask(*_conv_w(g, 576, 128, 1, dev))
        a.update(disps=_randn(g, (N, ht, wd), dev).abs() + 0.1, ix=torch.tensor([3, 1], dtype=torch.int64).to(dev),
                 disps_up=torch.full((N, 8 * ht, 8 * wd), -3.0, device=dev))
        return a
    return build


for _h in (False, True):
    # disps_up is written as 16-byte quads, like aggregate.upsample_disps_
    case("upmask.upsample_from_net_[%s x]" % ("h16" if _h else "f32"), ["lgu_upmask_upsample_f32"], "own", _ups_net_inputs(_h),
         lambda lgu, a: (lgu.upmask.upsample_from_net_(a["disps_up"], a["disps"], a["ix"], a["x"], a["wpack"], a["bias"],
                                                       half_weights=True).clone(),),
         dict(x=SAME, wpack=PACK, bias=SAME, disps=SAME, ix=SAME, disps_up=A16("unsupported")), inplace=("disps_up",))

for _h, _ci in ((False, 196), (True, 98)):
    case("conv1.conv1x1[%s x, Cin %d]" % ("h16" if _h else "f32", _ci), ["lgu_conv1x1_o128_h16"], "own",
         _layer_inputs(233 + _ci, _ci, (lambda ci: lambda lgu, g, dev: lgu.conv1.pack_conv1(*_conv_w(g, 128, ci, 1, dev)))(_ci), _h),
         (lambda ci: lambda lgu, a: (lgu.conv1.conv1x1(a["x"], a["wpack"], a["bias"], cin=ci, relu=True),))(_ci), _XWB)


# ---- the encoders' convolutions: (32, 64, stride 2) with the downsample branch, (64, 64, 1) with a residual -----------
def _enc_inputs(cin, cout, stride, residual=False):
    def build(dev):
        import lgu_slam_amd as lgu
        g = _gen(239 + cout + stride)
        a = dict(x=_randn(g, (_N, cin, _H, _W), dev, 1.0, torch.float16))
        a["wpack"], a["bias"] = lgu.encconv.pack_enc3(*_conv_w(g, cout, cin, 3, dev))
        if stride == 2:
            a["dpack"], a["dbias"] = lgu.encconv.pack_enc1(*_conv_w(g, cout, cin, 1, dev))
        if residual:
            a["res"] = _randn(g, (_N, cout) + tuple(lgu.encconv.out_size(_H, _W, stride)), dev, 1.0, torch.float16)
        return a
    return build


def _enc_call(lgu, a):
    stride = 2 if "dpack" in a else 1
    got = lgu.encconv.enc_conv3x3(a["x"], (a["wpack"], a["bias"]), stride=stride, relu="res" not in a, residual=a.get("res"),
                                  down=(a["dpack"], a["dbias"]) if stride == 2 else None)
    return tuple(got) if stride == 2 else (got,)


case("encconv.enc_conv3x3[32-64-s2, down]", ["lgu_encconv3x3_h16"], "own", _enc_inputs(32, 64, 2), _enc_call,
     dict(x=SAME, wpack=PACK, bias=SAME, dpack=PACK, dbias=SAME))
case("encconv.enc_conv3x3[64-64-s1, residual]", ["lgu_encconv3x3_h16"], "own", _enc_inputs(64, 64, 1, residual=True), _enc_call,
     dict(x=SAME, wpack=PACK, bias=SAME, res=SAME))

for _h in (False, True):
    case("encconv.enc_stem7x7[%s x]" % ("h16" if _h else "f32"), ["lgu_encstem7x7_h16"], "own",
         _layer_inputs(241, 3, lambda lgu, g, dev: lgu.encconv.pack_stem(*_conv_w(g, 32, 3, 7, dev)), _h),
         lambda lgu, a: (lgu.encconv.enc_stem7x7(a["x"], (a["wpack"], a["bias"]), relu=True),), _XWB)
for _co, _split in ((128, False), (256, True)):
    case("encconv.enc_out1x1[Cout %d%s]" % (_co, ", split" if _split else ""), ["lgu_encout1x1_c128_h16"], "own",
         _layer_inputs(243 + _co, 128, (lambda co: lambda lgu, g, dev: lgu.encconv.pack_out1(*_conv_w(g, co, 128, 1, dev)))(_co), True),
         (lambda sp: lambda lgu, a: (lambda r: tuple(r) if sp else (r,))(lgu.encconv.enc_out1x1(a["x"], (a["wpack"], a["bias"]), split=sp)))(
             _split), _XWB)


def _encnorm_inputs(dev):
    """x and y with the exact sums of their planes (made by two emitting launches), and the (32, 64, 2) layer with its
    branch that reads them: RES_NORM with keep and emit, every pointer of the block in use."""
    import lgu_slam_amd as lgu
    E = lgu.encconv
    g = _gen(251)
    x0 = _randn(g, (_N, 32, _H, _W), dev, 1.0, torch.float16)
    a = {}
    for k, s in (("x", "stats_x"), ("y", "stats_y")):
        a[k], _, _, a[s], _ = E.enc_conv3x3_norm(x0, E.pack_enc3(*_conv_w(g, 32, 32, 3, dev)), emit=True)
    a["wpack"], a["bias"] = E.pack_enc3(*_conv_w(g, 64, 32, 3, dev))
    a["dpack"], a["dbias"] = E.pack_enc1(*_conv_w(g, 64, 32, 1, dev))
    return a


def _encnorm_call(lgu, a):
    out, r, kept, so, sr = lgu.encconv.enc_conv3x3_norm(a["x"], (a["wpack"], a["bias"]), stride=2, down=(a["dpack"], a["dbias"]),
                                                        pre=("res_norm", a["stats_x"], a["y"], a["stats_y"]), keep=True, emit=True)
    return out, r, kept, so.sum(2), sr.sum(2)     # which replica slot a block adds to is not fixed; the sums are exact


case("encconv.enc_conv3x3_norm[res_norm, keep, emit]", ["lgu_encconv3x3_norm_h16"], "own", _encnorm_inputs, _encnorm_call,
     dict(x=SAME, y=SAME, stats_x=SAME, stats_y=SAME, wpack=PACK, bias=SAME, dpack=PACK, dbias=SAME))
case("encconv.stats_mean_rstd", ["lgu_encstats_finalize"], "own", _pick(_encnorm_inputs, "stats_x"),
     lambda lgu, a: (lgu.encconv.stats_mean_rstd(a["stats_x"], _H * _W),), dict(stats_x=SAME))


# ---- the Gaussian head: x is read with 16-byte loads, there is no element-wise twin -----------------------------------
def _gh_inputs(half, x_half):
    def build(dev):
        import lgu_slam_amd as lgu
        g = _gen(257)
        with torch.random.fork_rng(devices=[]):      # the module draws its initial weights from torch's global generator
            torch.manual_seed(257)
            ga = lgu.GaussianMask(3, 7)
        with torch.no_grad():
            ga.meanMap.weight.copy_(torch.randn((2, 16), generator=g) * 0.3)
        ga = ga.to(dev)
        a = dict(x=_randn(g, (2, 3, 7, 256), dev, 0.5, torch.float16 if x_half else torch.float32))
        a["wpack"], a["bias"] = lgu.gaussian_mask.pack_gaussian_head(ga.map, ga.meanMap, ga.covMap, half)
        return a
    return build


for _half, _xh in ((False, False), (True, False), (True, True)):
    case("gaussian_mask.gaussian_head[%s, %s x]" % ("half" if _half else "fp32", "h16" if _xh else "f32"), ["lgu_gaussian_head"], "own",
         _gh_inputs(_half, _xh),
         (lambda hf: lambda lgu, a: tuple(lgu.gaussian_mask.gaussian_head(a["x"], a["wpack"], a["bias"], half=hf, hidden=True)))(_half),
         dict(x=A16("unsupported"), wpack=PACK, bias=SAME))


# ---- the map export, the intake and the view: element accesses on every operand ---------------------------------------
def _cloud_inputs(dev):
    from tests import test_cloud as T
    N, ht, wd = 8, 9, 13
    poses, disps, intr, images = T.make_scene(100 * N + ht, N, ht, wd)
    ix, th = T.entries(N)
    a = dict(poses=_d(poses, dev), disps=_d(disps, dev), intrinsics=_d(intr, dev), ix=_d(ix, dev), thresh=_d(th, dev), images=_d(images, dev))
    a["floor"] = (0.5 * a["disps"][a["ix"].clamp(0, N - 1)].mean(dim=[1, 2])).contiguous()
    a["points"] = torch.full((ix.shape[0] * ht * wd, 3), 7.0, device=dev)        # room for every pixel: nothing is cut off
    a["colors"] = torch.full((ix.shape[0] * ht * wd, 3), 7, dtype=torch.uint8, device=dev)
    return a


def _cloud_call(lgu, a):
    p, c, o = lgu.cloud.point_cloud(a["poses"], a["disps"], a["intrinsics"], a["ix"], a["thresh"], a["images"], disp_floor=a["floor"],
                                    color_dtype=torch.uint8, out=(a["points"], a["colors"]))
    return p, c, o


case("cloud.point_cloud[out]", ["lgu_cloud_decide_f32", "lgu_cloud_write_f32"], "own", _cloud_inputs, _cloud_call,
     dict(poses=SAME, disps=SAME, intrinsics=SAME, ix=SAME, thresh=SAME, images=SAME, floor=SAME, points=SAME, colors=SAME),
     inplace=("points", "colors"))


def _intake_inputs(name):
    def build(dev):
        from tests import test_intake as T
        seed, shape, _, _ = T.CASES[name]
        import lgu_slam_amd as lgu
        raw = torch.from_numpy(np.random.default_rng(seed).integers(0, 256, size=shape, dtype=np.uint8)).to(dev)
        return dict(raw=raw, plan=T.make_plan(lgu, name))      # the plan keeps its camera table on the device once it was used
    return build


def _intake_call(name):
    def call(lgu, a):
        from tests import test_intake as T
        return tuple(lgu.intake.frame(a["raw"], a["plan"], **T.CASES[name][3]))
    return call


for _name in ("tum5", "stereo", "table3"):      # one camera; two, in the block; three, in a device table
    case("intake.frame[%s]" % _name, ["lgu_intake_frame_u8"], "own", _intake_inputs(_name), _intake_call(_name), dict(raw=SAME))


def _depth_inputs(dev):
    g = _gen(263)
    raw = torch.rand((72, 104), generator=g) * 4000.0
    raw[torch.rand((72, 104), generator=g) < 0.15] = 0.0
    return dict(raw=raw.to(dev))


def _depth_call(lgu, a):
    from tests import test_intake as T
    return (lgu.intake.sensor_disparity(a["raw"], lgu.intake.plan((72, 104), T._cam(72, 104), resize=(51, 75), crop=(0, 0, 48, 72))),)


case("intake.sensor_disparity[f32]", ["lgu_intake_depth_f32"], "own", _depth_inputs, _depth_call, dict(raw=SAME))


def _render_inputs(color_u8):
    def build(dev):
        g = _gen(269)
        P = 300
        pts = torch.randn((P, 3), generator=g) * 0.5 + torch.tensor([0.0, 0.0, 2.0])
        col = torch.rand((P, 3), generator=g)
        cams = torch.zeros((3, 7))
        cams[:, :3] = torch.randn((3, 3), generator=g) * 0.2 + torch.tensor([0.0, 0.0, -1.0])
        cams[:, 6] = 1.0
        return dict(points=pts.to(dev), colors=((col * 255).to(torch.uint8) if color_u8 else col).to(dev),
                    view=torch.tensor([0.05, -0.02, 0.3, 0.0, 0.0, 0.0, 1.0]).to(dev), intrinsics=torch.tensor([24.0, 24.0, 19.5, 14.5]).to(dev),
                    cameras=cams.to(dev), image=torch.full((30, 40, 3), 7, dtype=torch.uint8, device=dev),
                    depth=torch.full((30, 40), 7.0, device=dev))
    return build


for _u8 in (False, True):
    case("render.render_view[%s colours]" % ("u8" if _u8 else "f32"), ["lgu_render_view"], "own", _render_inputs(_u8),
         lambda lgu, a: tuple(lgu.render.render_view(a["points"], a["colors"], a["view"], a["intrinsics"], (30, 40), cameras=a["cameras"],
                                                     camera_scale=0.2, out=(a["image"], a["depth"]))),
         dict(points=SAME, colors=SAME, view=SAME, intrinsics=SAME, cameras=SAME, image=SAME, depth=SAME), inplace=("image", "depth"))


# ======================================================================================================================
# Entries with a pointer parameter that no case reaches, each with its reason
# ======================================================================================================================
EXCLUDED = {
    "lgu_ba_scatter_sum_f64": "ba.ba assembles with lgu_ba_assemble_f64; kept as the cross-check of tests/test_ba.py; element accesses only",
    "lgu_ba_disp_retr_f32": "not called by the Python layer (lgu_ba_depth_update_f32 applies the update); element accesses only",
}
