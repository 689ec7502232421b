"""The rows behind tests/test_capture.py: what is launched on a stream and recorded into a graph, and what is not.

A row is a `Case` of tests/alignment_cases.py: the `lgu_*` symbols it reaches, `build(dev)` -> a dict of arguments,
`call(lgu, args)` -> a tuple of output tensors, the keys the call changes in place, and for rows whose aligned call is not
bit-reproducible (float atomics) the bound of their parity test.  `ROWS` is every case of the alignment registry (every
operator function and most C entries at the smallest shape that reaches the production kernel), the C entries that only a
host-reading operator reaches, and the module-level rows: what production captures (the wrappers, the GRU, the update
operator, the encoders, the Gaussian mask, both correlation blocks).  A module row builds its module in `build` and hands
it over in the dict under a non-tensor key; the tensors a block keeps and changes in place (the offsets whose centre the
sampler zeroes) are listed as in-place keys, so the harness can put them back.

    HOST_READS     row -> the line that reads the host.  Such a row must raise under torch's sync debug mode and is never
                   captured.
    NOT_CAPTURED   row -> why its capture is not attempted; the probe and the side stream still run.
    COLD           row -> cold(lgu, dev): a fresh wrapper whose first call ever is recorded.
"""
import contextlib

from tests import alignment_cases as AC

import torch

Case = AC.Case
EXTRA = []


def row(name, symbols, build, call, inplace=(), bound=None):
    EXTRA.append(Case(name, symbols, "own", build, call, {}, inplace=inplace, bound=bound))


@contextlib.contextmanager
def fused_route(lgu, half=True):
    """No grad, float16 autocast, and every size threshold of the package at 0: the rows are about the fused routes."""
    saved = []
    for mod, attr in ((lgu.conv3, "MIN_FANOUT_PIXELS"), (lgu.heads, "MIN_PAIR_PIXELS"), (lgu.gru, "MIN_FUSED_CONV_PIXELS")):
        saved.append((mod, attr, getattr(mod, attr)))
        setattr(mod, attr, 0)
    try:
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16, enabled=half):
            yield
    finally:
        for mod, attr, v in saved:
            setattr(mod, attr, v)


# ======================================================================================================================
# C entries that the Python layer reaches only from an operator that reads the host
# ======================================================================================================================
def _small_inputs(dev):
    import lgu_slam_amd as lgu
    a = AC._pkeys_inputs(dev)
    cap = int(lgu.graph.capacity(AC._PX["t"], AC._PX["t0"], AC._PX["t1"], AC._PX["rad"], False, -1))
    return dict(dist=a["dist"], known_ii=torch.tensor([1, 3], dtype=torch.int64, device=dev), known_jj=torch.tensor([4, 5], dtype=torch.int64, device=dev),
                e_ii=torch.full((cap,), -7, dtype=torch.int64, device=dev), e_jj=torch.full((cap,), -7, dtype=torch.int64, device=dev),
                count=torch.full((1,), -7, dtype=torch.int32, device=dev))


def _c_small(lgu, a):
    P = AC._PX
    AC._check(lgu, lgu._lib.load().lgu_proximity_select_small(AC._p(a["dist"]), AC._p(a["known_ii"]), AC._p(a["known_jj"]), 2, P["t"], P["t0"],
                                                              P["t1"], P["rad"], P["nms"], 16.0, -1, 0, AC._p(a["e_ii"]), AC._p(a["e_jj"]),
                                                              a["e_ii"].numel(), AC._p(a["count"]), AC._st(a["count"])), "proximity_select_small")
    return (a["e_ii"], a["e_jj"], a["count"])


row("c.lgu_proximity_select_small", ["lgu_proximity_select_small"], _small_inputs, _c_small, inplace=("e_ii", "e_jj", "count"))


# ======================================================================================================================
# Operators that read the host (each on the line HOST_READS names)
# ======================================================================================================================
row("aggregate.scatter_mean[no dim_size]", ["lgu_scatter_mean_f32"], AC._sm_inputs(False),
    lambda lgu, a: (lgu.aggregate.scatter_mean(a["src"], a["index"], dim=1),))
row("cloud.point_cloud[no out]", ["lgu_cloud_decide_f32", "lgu_cloud_write_f32"], AC._pick(AC._cloud_inputs, "poses", "disps", "intrinsics", "ix", "thresh"),
    lambda lgu, a: tuple(t for t in lgu.cloud.point_cloud(a["poses"], a["disps"], a["intrinsics"], a["ix"], a["thresh"]) if t is not None))


def _update_inputs(with_ii):
    def build(dev):
        import lgu_slam_amd as lgu
        from tests import update_restatement as RU
        u = RU.make_update(21).to(dev)
        net, inp, corr, flow = RU.make_inputs(22, 5, 5, 7)
        a = dict(net=net.to(dev).half(), inp=inp.to(dev).half(), corr=corr.to(dev), flow=flow.to(dev), wr=lgu.update.UpdateOperator(u, gru_convs=True))
        if with_ii:
            a["ii"] = torch.tensor([4, 4, 7, 2, 7], device=dev)
        return a
    return build


def _update_call(lgu, a):
    with fused_route(lgu):
        before = a["wr"].fused_calls
        out = a["wr"](a["net"], a["inp"], a["corr"], a["flow"], a.get("ii"))
        assert a["wr"].fused_calls == before + 1
    return tuple(out)


_UPDATE_SYMS = ["lgu_conv1x1_o128_h16", "lgu_conv3x3_c128_h16", "lgu_flow_conv7_relu_h16", "lgu_kangru_context_h16", "lgu_kan_heads_h16",
                "lgu_gruconv3x3_c448_h16", "lgu_conv3x3_fanout_c128_h16", "lgu_head3x3_pair_c128_h16"]
row("update.UpdateOperator[ii]", _UPDATE_SYMS + ["lgu_scatter_mean_h16", "lgu_head3x3_c128_h16", "lgu_upmask1x1_c128_h16"], _update_inputs(True),
    _update_call)


def _corrblock_inputs(tiled):
    def build(dev):
        import lgu_slam_amd as lgu
        E, h, w = 2, 32, 32      # level 3 is 4 x 4: the fused lookup serves both layouts (W2 % 4 == 0)
        g = AC._gen(3)
        with torch.random.fork_rng(devices=[]):
            torch.manual_seed(3)
            ofsMap = torch.nn.Conv2d(256, 98, 3, padding=1).to(dev)
            ofsRes = torch.nn.Conv2d(256, 98, 3, padding=1).to(dev)
            GA = lgu.GaussianMask(h, w)
            torch.nn.init.normal_(GA.meanMap.weight, 0, 0.3)
        GA = GA.to(dev)
        ys, xs = torch.meshgrid(torch.arange(h).float(), torch.arange(w).float(), indexing="ij")
        fmap1, fmap2 = AC._randn(g, (1, E, 128, h, w), dev, 0.5), AC._randn(g, (1, E, 128, h, w), dev, 0.5)
        coords = (torch.stack([xs, ys], -1)[None, None] + 2 * torch.randn((1, E, h, w, 2), generator=g)).to(dev).contiguous()
        saved = lgu.CorrBlock.TILED_PYRAMID
        lgu.CorrBlock.TILED_PYRAMID = tiled
        try:
            with torch.no_grad():
                blk = lgu.CorrBlock(ofsMap, ofsRes, GA, fmap1, fmap2)
        finally:
            lgu.CorrBlock.TILED_PYRAMID = saved
        assert blk._store is not None and blk._tiled == tiled
        a = dict(coords=coords, blk=blk)
        for i in range(2):      # the offsets the lookup zeroes the centre of and, on level 1, scales by the probe's mask
            blk.offset[i] = blk.offset[i].float().contiguous()
            a["off%d" % i] = blk.offset[i]
        for l, v in enumerate(blk._store):
            a["lvl%d" % l] = v
        return a
    return build


def _corrblock_call(lgu, a):
    with torch.no_grad():
        out, mean_n, theta = a["blk"](a["coords"])
    assert a["blk"]._store is not None and a["blk"].offset[1] is a["off1"]      # the fused lookup served the call
    return out, a["off0"].clone(), a["off1"].clone()


_CB_SYMS = ["lgu_defcorr_pyramid_slots_fwd_f32"]
for _tiled in (True, False):
    row("CorrBlock.__call__[%s]" % ("tiled" if _tiled else "row-major"), _CB_SYMS, _corrblock_inputs(_tiled), _corrblock_call, inplace=("off0", "off1"))


def _corrblock_encoder_cold(lgu, dev):
    """CorrBlock with CorrBlock.ENCODER set: the lookup launch applies the encoder's first layer, whose packed weights
    CorrEncoder.fused_operands makes at its first call — here while the stream records.  The block itself is warm (its slot
    table is uploaded by an eager call without the encoder); every run starts from the same offsets."""
    a = _corrblock_inputs(True)(dev)
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(13)
        module = torch.nn.Sequential(torch.nn.Conv2d(196, 128, 1), torch.nn.ReLU(), torch.nn.Conv2d(128, 128, 3, padding=1), torch.nn.ReLU())
    module = module.to(dev)
    offs = [a["off0"].clone(), a["off1"].clone()]

    def run_with(enc):
        saved = lgu.CorrBlock.ENCODER
        lgu.CorrBlock.ENCODER = enc
        try:
            with torch.no_grad():
                a["off0"].copy_(offs[0])
                a["off1"].copy_(offs[1])
                out = a["blk"](a["coords"])[0]
        finally:
            lgu.CorrBlock.ENCODER = saved
        assert a["blk"]._store is not None and (enc is None or (out.dtype == torch.float16 and out.shape[2] == 128))
        return (out,)
    run_with(None)
    enc = lgu.CorrEncoder(module)

    def change():
        with torch.no_grad():
            module[0].weight.mul_(0.5)
    return a, lambda: run_with(enc), lambda: run_with(lgu.CorrEncoder(module)), change


def _getitem_call(lgu, a):
    with torch.no_grad():
        blk = a["blk"][torch.ones(len(a["blk"]._slot_list), dtype=torch.bool, device=a["coords"].device)]
        return (blk(a["coords"])[0],)


row("CorrBlock.__getitem__", _CB_SYMS, _corrblock_inputs(True), _getitem_call, inplace=("off0", "off1"))

HOST_READS = {
    "graph.proximity_edges[small]": "graph.py:156 count.item(), the number of edges selected",
    "graph.proximity_edges[sorted]": "graph.py:156 count.item(), the number of edges selected",
    "ba.ba": "ba.py:164 ii.cpu() / jj.cpu(), the edge set the plan tables are built from on the host",
    "CorrBlock.__getitem__": "corr.py:502 .tolist(), the kept positions edit the host's slot list",
    "update.UpdateOperator[ii]": "update.py:183 torch.unique(ii), whose result's size is read on the host",
    "aggregate.scatter_mean[no dim_size]": "aggregate.py:56 int(index.max()), the number of segments when dim_size is not given",
    "cloud.point_cloud[no out]": "cloud.py:182 int(offsets[-1]), the size of the exact results",
}


# ======================================================================================================================
# What production captures
# ======================================================================================================================
def _wrapper_inputs(name):
    def build(dev):
        import lgu_slam_amd as lgu
        from tests import test_wrapper_routes as W
        r = W.row(lgu, name)
        m = W.module(r).to(dev)
        a = dict(x=AC._randn(AC._gen(11), (2, r.cin, 5, 9), dev), wr=r.cls(m, **r.kw), m=m, r=r)
        if r.home is lgu.flow:      # torch's own convolution behind the fused layer: what the fused layer hands it is the result
            a["fed"] = []
            m[2].register_forward_pre_hook(lambda _, args: a["fed"].append(args[0].clone()))
        return a
    return build


def _wrapper_call(lgu, a):
    with fused_route(lgu):
        before = a["wr"].fused_calls
        y = a["wr"](a["x"])
        assert a["wr"].fused_calls == before + 1
    return (a["fed"][-1],) if "fed" in a else (y,)


def _wrapper_cold(name):
    def cold(lgu, dev):
        a = _wrapper_inputs(name)(dev)
        r, m = a["r"], a["m"]
        conv = r.conv(m)

        def want():
            with fused_route(lgu):
                return (r.op(a["x"], r.pack(conv.weight, conv.bias)),)

        def change():
            with torch.no_grad():
                conv.weight.mul_(2.0)
        return a, lambda: _wrapper_call(lgu, a), want, change
    return cold


_WRAPPER_SYMS = {"conv1-relu": "lgu_conv1x1_o128_h16", "conv3-64": "lgu_conv3x3_c128_h16", "conv3-128-relu": "lgu_conv3x3_c128_h16",
                 "stack": "lgu_conv3x3_c128_h16", "head-conv": "lgu_head3x3_c128_h16", "head-tail": "lgu_head3x3_c128_h16",
                 "upmask": "lgu_upmask1x1_c128_h16", "flow": "lgu_flow_conv7_relu_h16"}
COLD = {"CorrBlock.__call__[tiled]": _corrblock_encoder_cold}
for _name, _sym in _WRAPPER_SYMS.items():
    row("wrapper[%s]" % _name, [_sym], _wrapper_inputs(_name), _wrapper_call)
    COLD["wrapper[%s]" % _name] = _wrapper_cold(_name)


def _gru_inputs(convs):
    def build(dev):
        import lgu_slam_amd as lgu
        from tests import test_kangru as TK
        m, ins = TK.gpu_case(47, 4, 24, 32, half=True)      # the case tests/test_kangru.py and tests/test_gruconv.py capture
        a = dict(wr=lgu.gru.KanBiasGRU(m, convs=convs), m=m)
        for i, t in enumerate(ins):
            a["in%d" % i] = t.contiguous()
        a["n"] = len(ins)
        return a
    return build


def _gru_call(lgu, a):
    with fused_route(lgu):
        before = a["wr"].fused_calls
        out = a["wr"](*[a["in%d" % i] for i in range(a["n"])])
        assert a["wr"].fused_calls == before + 1
    return (out,)


def _gru_cold(convs):
    def cold(lgu, dev):
        a = _gru_inputs(convs)(dev)

        def want():      # a second wrapper of the same module, warm: the same kernels on packs made eagerly
            other = dict(a, wr=lgu.gru.KanBiasGRU(a["m"], convs=convs))
            return _gru_call(lgu, other)

        def change():
            with torch.no_grad():
                a["m"].w.weight.mul_(0.5)
                a["m"].kanq_glo.grid.mul_(0.8)
                if convs:
                    a["m"].convq.weight.mul_(0.5)
        return a, lambda: _gru_call(lgu, a), want, change
    return cold


for _convs in (False, True):
    _n = "gru.KanBiasGRU[convs=%s]" % _convs
    row(_n, ["lgu_kangru_context_h16", "lgu_kan_heads_h16"] + (["lgu_gruconv3x3_c448_h16"] if _convs else ["lgu_kangru_gates_h16", "lgu_kangru_blend_h16"]),
        _gru_inputs(_convs), _gru_call)
    COLD[_n] = _gru_cold(_convs)

row("update.UpdateOperator[ii=None]", _UPDATE_SYMS, _update_inputs(False), _update_call)


def _update_cold(lgu, dev):
    a = _update_inputs(False)(dev)
    u = a["wr"].module

    def want():
        other = dict(a, wr=lgu.update.UpdateOperator(u, gru_convs=True))
        return _update_call(lgu, other)

    def change():
        with torch.no_grad():
            u.corr_encoder[0].weight.mul_(0.5)
            u.delta[2].weight.mul_(2.0)
            u.gru.convq.weight.mul_(0.5)
    return a, lambda: _update_call(lgu, a), want, change


COLD["update.UpdateOperator[ii=None]"] = _update_cold


def _encoder_inputs(kind):
    def build(dev):
        import lgu_slam_amd as lgu
        from tests import context_restatement as C, features_restatement as R
        name = "features_fnet_1x64x48" if kind == "features" else "context_cnet_1x64x48"
        m, images = (R if kind == "features" else C).make_case(name)
        m = m.to(dev)
        # the planes behind the stem are 32 x 24: the single-launch instance norm serves them (NOT_CAPTURED has the other path)
        assert 32 * 24 <= lgu.features.resident_limit(torch.float16)
        wr = lgu.features.install(m, convs=True, ends=True) if kind == "features" else lgu.context.install(m, ends=True)
        return dict(images=images.to(dev), m=m, wr=wr)
    return build


def _encoder_call(lgu, a):
    with fused_route(lgu):
        before = a["wr"].fused_calls
        out = a["m"](a["images"])
        assert a["wr"].fused_calls == before + 1
    return tuple(out) if isinstance(out, (tuple, list)) else (out,)


def _encoder_cold(kind):
    def cold(lgu, dev):
        a = _encoder_inputs(kind)(dev)
        home = lgu.features if kind == "features" else lgu.context

        def want():      # the same module under a new wrapper, warm
            home.uninstall(a["m"])
            fresh = home.install(a["m"], convs=True, ends=True) if kind == "features" else home.install(a["m"], ends=True)
            try:
                return _encoder_call(lgu, dict(a, wr=fresh))
            finally:
                home.uninstall(a["m"])
                a["m"].forward = a["wr"]

        def change():
            with torch.no_grad():
                a["m"].conv1.weight.mul_(0.5)
                a["m"].conv2.weight.mul_(2.0)
        return a, lambda: _encoder_call(lgu, a), want, change
    return cold


_ENC_SYMS = ["lgu_encstem7x7_h16", "lgu_encconv3x3_h16", "lgu_encout1x1_c128_h16"]
row("features.FeatureEncoder[convs, ends]", _ENC_SYMS + ["lgu_instnorm_relu_h16"], _encoder_inputs("features"), _encoder_call)
row("context.ContextEncoder[ends]", _ENC_SYMS, _encoder_inputs("context"), _encoder_call)
COLD["features.FeatureEncoder[convs, ends]"] = _encoder_cold("features")
COLD["context.ContextEncoder[ends]"] = _encoder_cold("context")


def _ga_inputs(dev):
    import lgu_slam_amd as lgu
    E, h, w = 2, 7, 9
    g = AC._gen(11)
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(11)
        GA = lgu.GaussianMask(h, w)
        torch.nn.init.normal_(GA.meanMap.weight, 0, 0.3)
    GA = GA.to(dev)
    return dict(feats=AC._randn(g, (E, h, w, 256), dev), volume=AC._randn(g, (E, h, w, h, w), dev), GA=GA, wr=lgu.gaussian_mask.install(GA))


def _ga_call(lgu, a):
    with torch.no_grad():
        before = a["wr"].fused_calls
        v, mean, det = a["GA"](a["feats"], a["volume"])
        assert a["wr"].fused_calls == before + 1
    return v, mean, det


def _ga_cold(lgu, dev):
    a = _ga_inputs(dev)
    GA = a["GA"]

    def want():
        lgu.gaussian_mask.uninstall(GA)
        fresh = lgu.gaussian_mask.install(GA)
        try:
            return _ga_call(lgu, dict(a, wr=fresh))
        finally:
            lgu.gaussian_mask.uninstall(GA)
            GA.gaussian_parameters = a["wr"]

    def change():
        with torch.no_grad():
            GA.map.weight.mul_(0.5)
    return a, lambda: _ga_call(lgu, a), want, change


row("gaussian_mask.GaussianMask[fused head]", ["lgu_gaussian_head", "lgu_gaussian_params", "lgu_gaussmask_fwd_f32"], _ga_inputs, _ga_call)
COLD["gaussian_mask.GaussianMask[fused head]"] = _ga_cold


def _alt_inputs(many):
    def build(dev):
        import lgu_slam_amd as lgu
        N, C, H, W, E = 4, 128, 16, 16, 5
        with torch.random.fork_rng(devices=[]):
            torch.manual_seed(5)
            ofsMap = torch.nn.Conv2d(256, 98, 3, padding=1).to(dev)
            ofsRes = torch.nn.Conv2d(256, 98, 3, padding=1).to(dev)
        g = AC._gen(5)
        ys, xs = torch.meshgrid(torch.arange(H).float(), torch.arange(W).float(), indexing="ij")
        fmaps = AC._randn(g, (1, N, C, H, W), dev, 0.5, torch.float16)      # half maps: the fused launches of update_lowmem
        coords = (torch.stack([xs, ys], -1)[None, None] + 2 * torch.randn((1, E, H, W, 2), generator=g)).to(dev).contiguous()
        with torch.no_grad():
            blk = lgu.AltCorrBlock(ofsMap, ofsRes, None, fmaps)
        a = dict(coords=coords, ii=torch.tensor([0, 0, 1, 2, 3], device=dev), jj=torch.tensor([1, 2, 3, 0, 2], device=dev), blk=blk,
                 ofsMap=ofsMap, fmaps=fmaps)
        for l, p in enumerate(blk.pyramid):
            a["pyr%d" % l] = p
        return a
    return build


def _alt_call(many):
    def call(lgu, a):
        with torch.no_grad():
            if many:
                before = getattr(a["blk"], "one_launch_calls", 0)
                out = a["blk"].call_many(a["coords"], a["ii"], a["jj"], [2, 3])
                assert a["blk"].one_launch_calls == before + 1
            else:
                out = a["blk"](a["coords"], a["ii"], a["jj"])
        return (out,)
    return call


def _alt_cold(lgu, dev):
    """The first lookup of a fresh block: the chunk-planar maps, the pooled frames and the packed heads are all made by it."""
    a = _alt_inputs(False)(dev)

    def want():
        with torch.no_grad():
            other = lgu.AltCorrBlock(a["blk"].ofsMap, a["blk"].ofs_residual, None, a["fmaps"])
        return _alt_call(False)(lgu, dict(a, blk=other))

    def change():
        with torch.no_grad():
            a["ofsMap"].weight.mul_(0.5)
    return a, lambda: _alt_call(False)(lgu, a), want, change


_ALT_SYMS = ["lgu_lowmem_pyramid_chunked_fwd_h16", "lgu_offset_conv_frames_h16", "lgu_offsets_finalize_masked"]
row("AltCorrBlock.__call__", _ALT_SYMS, _alt_inputs(False), _alt_call(False))
row("AltCorrBlock.call_many", _ALT_SYMS + ["lgu_lowmem_pyramid_calls_fwd_h16"], _alt_inputs(True), _alt_call(True))
COLD["AltCorrBlock.__call__"] = _alt_cold


def _ohc_cold(lgu, dev):
    """ops.OffsetHeadCache, built eagerly, whose first call (the one that makes its work list) is recorded.  The mark pass
    writes the work list before anything reads it, so this row passes without the guard too: it shows that not keeping the
    list does no harm, not that the guard is needed.  No weights of its own to change."""
    a = AC._oc_inputs((3, 4, 12, 20), True, parts=True)(dev)
    a["cache"] = lgu.ops.OffsetHeadCache(a["frames"], (a["wpack_a"], a["wpack_b"], a["bias"], 98, 128), frames_lo=a["frames_lo"])
    return a, lambda: (a["cache"](a["ii"], a["jj"]),), lambda: AC._ohc_call(lgu, a), None


COLD["ops.OffsetHeadCache"] = _ohc_cold


# ======================================================================================================================
# Not captured, by decision
# ======================================================================================================================
def _two_launch_inputs(dev):
    import lgu_slam_amd as lgu
    limit = lgu.features.resident_limit(torch.float32)
    H = limit // 64 + 1
    return dict(a=AC._randn(AC._gen(59), (1, 2, H, 64), dev), out=torch.full((1, 2, H, 64), 7.0, device=dev))


row("features.instance_norm_relu[two launches]", ["lgu_instnorm_relu_f32"], _two_launch_inputs,
    lambda lgu, a: (lgu.features.instance_norm_relu(a["a"], out=a["out"]),), inplace=("out",))

NOT_CAPTURED = {
    "features.instance_norm_relu[two launches]": "planes above lgu_instnorm_resident_limit take their statistics buffer from hipMallocAsync / "
                                                 "hipFreeAsync: allocation nodes, whose capture depends on the runtime (include/lgu_corr.h)",
}

# ---- the two BA entries the Python layer does not call (tests/test_ba.py keeps the first as a cross-check) -------------
def _scatter_sum_inputs(dev):
    g = AC._gen(83)
    return dict(inp=AC._randn(g, (6, 4), dev), ptrs=torch.tensor([0, 2, 3, 6], dtype=torch.int64, device=dev),
                idxs=torch.tensor([0, 3, 1, 2, 4, 5], dtype=torch.int64, device=dev), dst=torch.tensor([2, 0, 1], dtype=torch.int64, device=dev),
                out=AC._randn(g, (3, 4), dev).double())


def _c_scatter_sum(lgu, a):      # out[dst[j]] += sign * sum of the rows idxs[ptrs[j]:ptrs[j + 1]] of inp, in double
    AC._check(lgu, lgu._lib.load().lgu_ba_scatter_sum_f64(AC._p(a["inp"]), AC._p(a["ptrs"]), AC._p(a["idxs"]), AC._p(a["dst"]), AC._p(a["out"]), 3, 4,
                                                          -1.0, AC._st(a["out"])), "ba scatter sum")
    return (a["out"],)


row("c.lgu_ba_scatter_sum_f64", ["lgu_ba_scatter_sum_f64"], _scatter_sum_inputs, _c_scatter_sum, inplace=("out",))


def _disp_retr_inputs(dev):
    g = AC._gen(89)
    return dict(disps=AC._randn(g, (4, 6), dev), dz=AC._randn(g, (2, 6), dev), inds=torch.tensor([3, 1], dtype=torch.int64, device=dev))


def _c_disp_retr(lgu, a):        # disps[inds[k]] += dz[k]
    AC._check(lgu, lgu._lib.load().lgu_ba_disp_retr_f32(AC._p(a["disps"]), AC._p(a["dz"]), AC._p(a["inds"]), 2, 6, AC._st(a["disps"])), "ba disp retr")
    return (a["disps"],)


row("c.lgu_ba_disp_retr_f32", ["lgu_ba_disp_retr_f32"], _disp_retr_inputs, _c_disp_retr, inplace=("disps",))

ROWS = list(AC.CASES) + EXTRA
BY_NAME = {c.name: c for c in ROWS}


def captured_rows():
    return [c for c in ROWS if c.name not in HOST_READS and c.name not in NOT_CAPTURED]


def stream_entries():
    """The functions of include/lgu_corr.h whose last parameter is `void* stream`."""
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "lgu_corr.h")).read(), flags=re.S)
    return [name for name, params in re.findall(r"\b(lgu_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", text) if re.search(r"void\s*\*\s*stream\s*$", params.strip())]
