#!/usr/bin/env python3
"""Device-event medians of the fused residual-stage convolutions of the encoders (lgu_slam_amd.encconv, csrc/encconv.hip)
against the module's own autocast calls, with the same seeded weights on the same GPU, at 1 and 16 frames of 384x512
(MotionFilter.track and PoseTrajectoryFiller).  Writes profiles/encconv_prof.json and prints it as ONE JSON line.

Forms, per workload:
  <Cin>-<Cout>-s<stride>/bare       enc_conv3x3(x)                      against conv(x)
  <Cin>-<Cout>-s<stride>/relu       enc_conv3x3(x, relu=True)           against relu_(conv(x))
  <Cin>-<Cout>-s1/residual          enc_conv3x3(x, residual=r)          against relu_(r + relu_(conv(x)))
  <Cin>-<Cout>-s2/down              enc_conv3x3(x, relu=True, down=..)  against enc_conv3x3(x, relu=True) + the module's 1x1
  cnet                              context.install(cnet)               against the module's own forward
  fnet_convs                        features.install(fnet, convs=True)  against features.install(fnet)
and with --ends the two ends of the encoders (csrc/encends.hip), written to profiles/encends_prof.json:
  stem/relu                         enc_stem7x7(x, relu=True)           against relu_(conv1(x))
  stem/bare                         enc_stem7x7(x)                      against conv1(x)
  out128, out256                    enc_out1x1(x)                       against conv2(x) of fnet / cnet
  net_inp                           enc_out1x1(x, split=True)           against conv2(x).split + tanh + relu
  cnet_ends                         ContextEncoder(cnet, ends=True)     against ContextEncoder(cnet)
  fnet_ends                         FeatureEncoder(fnet, convs=True, ends=True)  against FeatureEncoder(fnet, convs=True)
and with --norms the instance norms folded into the convolutions (enc_conv3x3_norm), written to profiles/encnorm_prof.json,
each form in ROUNDS = 3 rounds of alternated calls (`rounds`; `keep_fused` must hold in every round):
  fnet_norms                        FeatureEncoder(fnet, convs=True, ends=True, norms=True)  against the same without norms
  <Cin>-<Cout>-s<stride>/emit       enc_conv3x3_norm(x, emit=True)                against enc_conv3x3(x) (both with the branch
  <Cin>-<Cout>-s<stride>/norm       ..(x, pre=("norm", sx))                       where the stride is 2)
  <Cin>-<Cout>-s<stride>/res        ..(x, pre=("res", sx, y), keep=True)
  <Cin>-<Cout>-s<stride>/res_norm   ..(x, pre=("res_norm", sx, y, sy), keep=True)
`min_norms_pixels`: the rule of `thresholds` over fnet_norms' classes in image pixels N * H * W, for encconv.MIN_NORMS_PIXELS.
`replicas`: R of the library that ran (variant libraries with -DLGU_ES_REPLICAS=1|2|8 under LGU_LIB_PATH give the sweep).
Each layer form runs at the plane its layer sees in a 384x512 frame (32 channels: 192x256, 64: 96x128, 128: 48x64).
Method (tools/prof_conv3.py's): every timed call runs on the next of ROT disjoint input sets, the two sides alternate call
by call in one process, and a spin kernel ahead of the first event keeps the host's enqueue time out of the window.
Reported per side: median, quartiles and spread = p75 - p25 (ms).  `keep_fused`: fused median + spread < other median -
spread.  `min_stem_pixels` / `min_out_pixels` (--ends): the same rule for encconv.MIN_STEM_PIXELS and MIN_OUT_PIXELS.  `min_fused_pixels`: per shape, the smallest number of output pixels N*Ho*Wo from which every measured class of
every layer form of the shape keeps the fused path, the rule by which lgu_slam_amd.encconv.MIN_FUSED_PIXELS is set (0:
every class keeps it).
--spin CYCLES lengthens the spin kernel: a whole forward at one frame is 14 to 27 launches whose enqueue outlasts the default
spin, so its window then holds host time too (a bimodal sample); 2000000 cycles hide it.
Usage: prof_encconv.py [--ends | --norms] [--reps N] [--out PATH] [--forms a,b] [--frames 1,16] [--spin CYCLES]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import lgu_slam_amd  # noqa: E402
from tests import context_restatement as RC  # noqa: E402
from tests import features_restatement as RF  # noqa: E402

ROT = 8
SPIN = 400000
FRAME = (384, 512)
PLANE = {32: (192, 256), 64: (96, 128), 128: (48, 64)}
OUT = os.path.join(ROOT, "profiles", "encconv_prof.json")
E = lgu_slam_amd.encconv


def sid(shape):
    return "%d-%d-s%d" % shape


def layer_forms():
    forms = []
    for shape in E.SHAPES:
        forms += [sid(shape) + "/bare", sid(shape) + "/relu", sid(shape) + ("/residual" if shape[2] == 1 else "/down")]
    return forms


FORMS = layer_forms() + ["cnet", "fnet_convs"]
END_FORMS = ["stem/relu", "stem/bare", "out128", "out256", "net_inp", "cnet_ends", "fnet_ends"]
OUT_ENDS = os.path.join(ROOT, "profiles", "encends_prof.json")
NORM_TAILS = ("emit", "norm", "res", "res_norm")
NORM_FORMS = ["fnet_norms"] + [sid(s) + "/" + t for s in E.SHAPES for t in NORM_TAILS]
OUT_NORMS = os.path.join(ROOT, "profiles", "encnorm_prof.json")
ROUNDS = 3
FORWARD_SPIN = 2000000     # a whole forward's enqueue outlasts the default spin


def stats(ts):
    q = np.percentile(ts, [25, 50, 75])
    return {"median_ms": float(q[1]), "p25_ms": float(q[0]), "p75_ms": float(q[2]), "spread_ms": float(q[2] - q[0]),
            "min_ms": float(np.min(ts))}


def block_of(cnet, shape):
    cin, cout, st = shape
    layer = {32: cnet.layer1, 64: cnet.layer2, 128: cnet.layer3}[cout]
    return layer[0] if cin != cout else layer[1]


def sides_of(form, cnet, fnet, fnet_twin, frames):
    """(fused, other, inputs): two callables of one input and ROT inputs."""
    if form == "cnet":
        xs = [RF.make_images(100 + i, frames, *FRAME).cuda() for i in range(ROT)]
        own = type(cnet).forward
        return lgu_slam_amd.context.ContextEncoder(cnet), (lambda x: own(cnet, x)), xs
    if form == "fnet_convs":
        xs = [RF.make_images(100 + i, frames, *FRAME).cuda() for i in range(ROT)]
        return lgu_slam_amd.features.FeatureEncoder(fnet_twin, convs=True), lgu_slam_amd.features.FeatureEncoder(fnet), xs
    if form == "fnet_norms":
        xs = [RF.make_images(100 + i, frames, *FRAME).cuda() for i in range(ROT)]
        return (lgu_slam_amd.features.FeatureEncoder(fnet_twin, convs=True, ends=True, norms=True),
                lgu_slam_amd.features.FeatureEncoder(fnet, convs=True, ends=True), xs)
    if form in ("cnet_ends", "fnet_ends"):
        xs = [RF.make_images(100 + i, frames, *FRAME).cuda() for i in range(ROT)]
        if form == "cnet_ends":
            twin = RC.make_case("context_cnet_2x40x56")[0].cuda()
            return lgu_slam_amd.context.ContextEncoder(twin, ends=True), lgu_slam_amd.context.ContextEncoder(cnet), xs
        return (lgu_slam_amd.features.FeatureEncoder(fnet_twin, convs=True, ends=True),
                lgu_slam_amd.features.FeatureEncoder(fnet, convs=True), xs)
    if form.startswith("stem/"):
        conv = cnet.conv1
        pack = E.pack_stem(conv.weight, conv.bias)
        xs = [RF.make_images(100 + i, frames, *FRAME)[0].contiguous().cuda() for i in range(ROT)]
        if form == "stem/relu":
            return (lambda x: E.enc_stem7x7(x, pack, relu=True)), (lambda x: torch.relu_(conv(x))), xs
        return (lambda x: E.enc_stem7x7(x, pack)), conv, xs
    if form in ("out128", "out256", "net_inp"):
        conv = fnet.conv2 if form == "out128" else cnet.conv2
        pack = E.pack_out1(conv.weight, conv.bias)
        g = torch.Generator().manual_seed(7 + 128)
        xs = [(torch.randn((frames, 128) + PLANE[128], generator=g) * 2.0).clamp_(min=0.0).half().cuda() for _ in range(ROT)]
        if form != "net_inp":
            return (lambda x: E.enc_out1x1(x, pack)), conv, xs

        def torch_tail(x):
            net, inp = conv(x).split([128, 128], dim=1)
            return net.tanh(), inp.relu()
        return (lambda x: E.enc_out1x1(x, pack, split=True)), torch_tail, xs
    name, tail = form.split("/")
    shape = [s for s in E.SHAPES if sid(s) == name][0]
    cin, cout, st = shape
    blk = block_of(cnet, shape)
    conv = blk.conv1 if st == 2 else blk.conv2
    pack = E.pack_enc3(conv.weight, conv.bias)
    H, W = PLANE[cin]
    g = torch.Generator().manual_seed(7 + cin)
    xs = []
    for _ in range(ROT):
        x = torch.randn((frames, cin, H, W), generator=g) * 2.0
        xs.append(x.clamp_(min=0.0).half().cuda())          # behind a ReLU: exact zeros
    if tail in NORM_TAILS:
        dpack = E.pack_enc1(blk.downsample[0].weight, blk.downsample[0].bias) if st == 2 else None
        bare = lambda x: E.enc_conv3x3(x, pack, stride=st, down=dpack)      # noqa: E731
        if tail == "emit":
            so = E.new_stats(frames, cout, "cuda")
            so = (so, E.new_stats(frames, cout, "cuda")) if st == 2 else so
            return (lambda x: E.enc_conv3x3_norm(x, pack, stride=st, down=dpack, emit=True, stats_out=so)), bare, xs
        # the accumulators of each input set, from an emitting launch whose output is its input
        eye = torch.zeros((cin, cin, 3, 3), device="cuda")
        eye[torch.arange(cin), torch.arange(cin), 1, 1] = 1.0
        ident = E.pack_enc3(eye, torch.zeros(cin, device="cuda"))
        y = (torch.randn((frames, cin, H, W), generator=g) * 2.0).clamp_(min=0.0).half().cuda()
        sy = E.enc_conv3x3_norm(y, ident, emit=True)[3]
        sxs = {x.data_ptr(): E.enc_conv3x3_norm(x, ident, emit=True)[3] for x in xs}
        pre = {"norm": lambda x: ("norm", sxs[x.data_ptr()]), "res": lambda x: ("res", sxs[x.data_ptr()], y),
               "res_norm": lambda x: ("res_norm", sxs[x.data_ptr()], y, sy)}[tail]
        return (lambda x: E.enc_conv3x3_norm(x, pack, stride=st, down=dpack, pre=pre(x), keep=tail != "norm")), bare, xs
    if tail == "bare":
        return (lambda x: E.enc_conv3x3(x, pack, stride=st)), conv, xs
    if tail == "relu":
        return (lambda x: E.enc_conv3x3(x, pack, stride=st, relu=True)), (lambda x: torch.relu_(conv(x))), xs
    if tail == "residual":
        res = (torch.randn((frames, cout) + E.out_size(H, W, st), generator=g) * 2.0).clamp_(min=0.0).half().cuda()
        return (lambda x: E.enc_conv3x3(x, pack, residual=res)), (lambda x: torch.relu_(res + torch.relu_(conv(x)))), xs
    down = blk.downsample[0]
    dpack = E.pack_enc1(down.weight, down.bias)
    return ((lambda x: E.enc_conv3x3(x, pack, stride=2, relu=True, down=dpack)),
            (lambda x: (E.enc_conv3x3(x, pack, stride=2, relu=True), down(x))), xs)


def timed(fns, xs, reps, warmup=3, spin=None):
    """{side: [ms]}: the sides alternate call by call; call k of a side uses input set k % ROT."""
    ts = {k: [] for k in fns}
    for k in range(warmup + reps):
        for name, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda._sleep(spin or SPIN)
            a.record()
            fn(xs[k % ROT])
            b.record()
            b.synchronize()
            if k >= warmup:
                ts[name].append(a.elapsed_time(b))
    return ts


def measure(reps, forms, frames_list):
    res = {}
    cnet = RC.make_case("context_cnet_2x40x56")[0].cuda()
    fnet, fnet_twin = RF.make_case("features_fnet_2x40x56")[0].cuda(), RF.make_case("features_fnet_2x40x56")[0].cuda()
    for frames in frames_list:
        r = {"frames": frames, "H": FRAME[0], "W": FRAME[1], "forms": {}}
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
            for form in forms:
                fused, other, xs = sides_of(form, cnet, fnet, fnet_twin, frames)
                folded = form in NORM_FORMS
                spin = max(SPIN, FORWARD_SPIN) if form == "fnet_norms" else None
                rounds = []
                for _ in range(ROUNDS if folded else 1):
                    ts = timed({"fused": fused, "other": other}, xs, reps, spin=spin)
                    f, o = stats(ts["fused"]), stats(ts["other"])
                    rounds.append({"fused": f, "other": o, "speedup": o["median_ms"] / f["median_ms"],
                                   "keep_fused": bool(f["median_ms"] + f["spread_ms"] < o["median_ms"] - o["spread_ms"])})
                del xs
                torch.cuda.empty_cache()
                d = dict(rounds[len(rounds) // 2])
                if folded:     # the middle round's figures, every round listed, and the verdict of all of them
                    d["rounds"] = rounds
                    d["keep_fused"] = all(r["keep_fused"] for r in rounds)
                if form == "fnet_norms":
                    d["out_pixels"] = frames * FRAME[0] * FRAME[1]
                elif form.startswith("stem/"):
                    ho, wo = E.out_size(*FRAME, 2)
                    d["out_pixels"] = frames * ho * wo
                elif form in ("out128", "out256", "net_inp"):
                    d["out_pixels"] = frames * PLANE[128][0] * PLANE[128][1]
                elif "/" in form:
                    shape = [s for s in E.SHAPES if sid(s) == form.split("/")[0]][0]
                    ho, wo = E.out_size(*PLANE[shape[0]], shape[2])
                    d["out_pixels"] = frames * ho * wo
                r["forms"][form] = d
        res["frames_%d" % frames] = r
    return res


def thresholds(workloads):
    """Per shape: 0 if every class of every layer form keeps the fused path, else the pixel count of the smallest class
    from which all larger ones keep it (1 << 62: none does)."""
    out = {}
    for shape in E.SHAPES:
        per = {}
        for w in workloads.values():
            for form, d in w["forms"].items():
                if form.startswith(sid(shape) + "/"):
                    per[d["out_pixels"]] = per.get(d["out_pixels"], True) and d["keep_fused"]
        classes = sorted(per.items())
        need = 0
        for i, (pixels, keep) in enumerate(classes):
            if not keep:
                need = classes[i + 1][0] if i + 1 < len(classes) else 1 << 62
        out[sid(shape)] = need
    return out


def threshold_of(workloads, forms):
    """The rule of `thresholds` over the classes of the named forms."""
    per = {}
    for w in workloads.values():
        for form, d in w["forms"].items():
            if form in forms:
                per[d["out_pixels"]] = per.get(d["out_pixels"], True) and d["keep_fused"]
    classes = sorted(per.items())
    need = 0
    for i, (pixels, keep) in enumerate(classes):
        if not keep:
            need = classes[i + 1][0] if i + 1 < len(classes) else 1 << 62
    return need


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--ends", action="store_true", help="time the stem and the output layer (csrc/encends.hip) instead: "
                    "profiles/encends_prof.json")
    ap.add_argument("--norms", action="store_true", help="time the folded instance norms (enc_conv3x3_norm, FeatureEncoder(norms=True)) "
                    "instead: profiles/encnorm_prof.json")
    ap.add_argument("--out")
    ap.add_argument("--forms", help="comma-separated subset of the forms to time (e.g. a variant library under LGU_LIB_PATH); "
                    "no thresholds are derived from a subset")
    ap.add_argument("--frames", default="1,16")
    ap.add_argument("--spin", type=int, default=SPIN, help="cycles of the spin kernel ahead of each timed call")
    args = ap.parse_args()
    globals()["SPIN"] = args.spin
    lgu_slam_amd._lib.load()
    E.MIN_FUSED_PIXELS = {s: 0 for s in E.SHAPES}      # measure the fused path at every class; the rule is applied afterwards
    E.MIN_STEM_PIXELS, E.MIN_OUT_PIXELS = 0, {c: 0 for c in E.OUT_COUTS}
    E.MIN_NORMS_PIXELS = 0
    args.out = args.out or (OUT_NORMS if args.norms else OUT_ENDS if args.ends else OUT)
    forms = args.forms.split(",") if args.forms else list(NORM_FORMS if args.norms else END_FORMS if args.ends else FORMS)
    workloads = measure(args.reps, forms, [int(f) for f in args.frames.split(",")])
    doc = {"tool": "prof_encconv", "device": torch.cuda.get_device_name(0), "lib": lgu_slam_amd._lib.version(),
           "reps": args.reps, "rotation": ROT, "spin_cycles": args.spin, "workloads": workloads}
    if args.norms:
        doc["replicas"] = E.stats_replicas()
        if "fnet_norms" in forms:
            doc["min_norms_pixels"] = threshold_of(workloads, ("fnet_norms",))
    elif not args.forms and args.ends:
        doc["min_stem_pixels"] = threshold_of(workloads, ("stem/relu", "stem/bare"))
        doc["min_out_pixels"] = {"128": threshold_of(workloads, ("out128",)), "256": threshold_of(workloads, ("out256", "net_inp"))}
    elif not args.forms:
        doc["min_fused_pixels"] = thresholds(workloads)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(doc, open(args.out, "w"), indent=1, sort_keys=True)
    print(json.dumps(doc, sort_keys=True))


if __name__ == "__main__":
    main()
