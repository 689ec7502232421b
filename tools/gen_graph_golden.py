#!/usr/bin/env python3
"""Writes tests/golden/proximity_*.npz: the reference's own FactorGraph.add_proximity_factors
(droid_slam/factor_graph.py:319-383) run on the CPU on seeded distances, the fixture that tests/graph_restatement.py and
the kernels of csrc/graphsel.hip are held to.

The reference's droid_slam.factor_graph is imported unchanged; stub modules stand in for the imports the method never
touches (lietorch, matplotlib, the correlation blocks, the projective ops).  The method is called on a stand-in object:
`video.distance` returns the seeded array, `add_factors` records what it is handed.

Per file:
  t, t0, t1, rad, nms, thresh, max_factors, stereo, remove    the call's parameters
  known_ii, known_jj (K,) int64     ii ++ ii_bad ++ ii_inac of the stand-in graph (split: n_active, n_bad)
  d (n,) float32                    a seeded permutation of DISTINCT values, scale * (k + 0.5) for k in 0..n-1 (the
                                    reference's unstable argsort cannot matter), about SHARE of them under thresh
  ii, jj (M,) int64                 the edges handed to add_factors, in order
Usage: gen_graph_golden.py [--reference DIR] [--out DIR] [--check]   (--check: compare with the committed files)
"""
import argparse
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
STUBS = ("lietorch", "matplotlib", "matplotlib.pyplot", "droid_slam.modules.corr", "droid_slam.geom.projective_ops")
SHARE = 0.3
# name -> parameters; known = number of known edges (some outside the window), seed
CASES = {
    "proximity_backend_t12": dict(t=12, t0=0, t1=0, rad=2, nms=2, thresh=16.0, max_factors=48, stereo=False, known=0, seed=1),
    "proximity_backend_t40_stereo": dict(t=40, t0=0, t1=0, rad=2, nms=3, thresh=22.0, max_factors=640, stereo=True, known=0,
                                         seed=2),
    "proximity_frontend_t30": dict(t=30, t0=25, t1=5, rad=2, nms=1, thresh=16.0, max_factors=48, stereo=False, known=20, seed=3),
    "proximity_frontend_t9": dict(t=9, t0=4, t1=0, rad=2, nms=2, thresh=16.0, max_factors=64, stereo=False, known=5, seed=4),
    "proximity_default_max": dict(t=16, t0=0, t1=0, rad=2, nms=2, thresh=16.0, max_factors=-1, stereo=False, known=0, seed=5),
    "proximity_nms0": dict(t=20, t0=0, t1=0, rad=1, nms=0, thresh=16.0, max_factors=200, stereo=False, known=6, seed=6),
    "proximity_t70": dict(t=70, t0=0, t1=0, rad=2, nms=2, thresh=12.0, max_factors=1120, stereo=False, known=30, seed=7),
}


def distances(seed, n, thresh):
    """n distinct float32 values in seeded order: thresh / (SHARE * n) * (k + 0.5)."""
    rs = np.random.RandomState(seed)
    scale = thresh / (SHARE * max(n, 1))
    d = (scale * (rs.permutation(n) + 0.5)).astype(np.float32)
    assert np.unique(d).shape[0] == n
    return d


def known_edges(seed, num, t):
    """num edges with |i - j| >= 1 over frames -2 .. t+1: a few lie outside any window."""
    rs = np.random.RandomState(seed + 500)
    ii = rs.randint(-2, t + 2, size=num).astype(np.int64)
    jj = (ii + rs.choice([-1, 1], size=num) * rs.randint(1, 9, size=num)).astype(np.int64)
    return ii, jj


class _Stub(types.ModuleType):
    """A module any name can be imported from: every attribute is a placeholder class."""

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return type(name, (), {})


def import_factor_graph(reference):
    if reference not in sys.path:
        sys.path.insert(0, reference)
    import importlib
    for name in STUBS:
        if name not in sys.modules:
            sys.modules[name] = _Stub(name)
            parent, _, leaf = name.rpartition(".")
            if parent.startswith("droid_slam"):      # `import a.b.c as x` reads c as an attribute of the (empty) package a.b
                setattr(importlib.import_module(parent), leaf, sys.modules[name])
    import droid_slam.factor_graph as fg
    return fg


def run_reference(fg, p, d, kii, kjj):
    """The reference method on a stand-in `self`; returns the (ii, jj, remove) handed to add_factors."""
    calls = []
    na, nb = len(kii) // 2, len(kii) // 4
    cut = (0, na, na + nb, len(kii))
    parts = [(torch.from_numpy(kii[a:b].copy()), torch.from_numpy(kjj[a:b].copy())) for a, b in zip(cut[:-1], cut[1:])]
    video = types.SimpleNamespace(counter=types.SimpleNamespace(value=p["t"]), stereo=p["stereo"],
                                  distance=lambda ii, jj, beta=0.3: torch.from_numpy(d.copy()))
    graph = types.SimpleNamespace(video=video, device="cpu", max_factors=p["max_factors"],
                                  ii=parts[0][0], jj=parts[0][1], ii_bad=parts[1][0], jj_bad=parts[1][1],
                                  ii_inac=parts[2][0], jj_inac=parts[2][1],
                                  add_factors=lambda ii, jj, remove=False: calls.append((ii, jj, remove)))
    fg.FactorGraph.add_proximity_factors(graph, t0=p["t0"], t1=p["t1"], rad=p["rad"], nms=p["nms"], beta=0.25,
                                         thresh=p["thresh"], remove=p["t0"] > 0)
    (ii, jj, remove), = calls
    return ii.numpy().astype(np.int64), jj.numpy().astype(np.int64), bool(remove), na, nb


def generate(reference):
    fg = import_factor_graph(reference)
    out = {}
    for name, p in CASES.items():
        n = (p["t"] - p["t0"]) * (p["t"] - p["t1"])
        d = distances(p["seed"], n, p["thresh"])
        kii, kjj = known_edges(p["seed"], p["known"], p["t"])
        ii, jj, remove, na, nb = run_reference(fg, p, d, kii, kjj)
        out[name] = dict(t=np.int64(p["t"]), t0=np.int64(p["t0"]), t1=np.int64(p["t1"]), rad=np.int64(p["rad"]),
                         nms=np.int64(p["nms"]), thresh=np.float64(p["thresh"]), max_factors=np.int64(p["max_factors"]),
                         stereo=np.bool_(p["stereo"]), remove=np.bool_(remove), known_ii=kii, known_jj=kjj,
                         n_active=np.int64(na), n_bad=np.int64(nb), d=d, ii=ii, jj=jj)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("LGU_REFERENCE", "/root/reference"))
    ap.add_argument("--out", default=GOLDEN)
    ap.add_argument("--check", action="store_true")
    args = ap.parse_args()
    res = generate(args.reference)
    for name, arrays in res.items():
        path = os.path.join(args.out, name + ".npz")
        if args.check:
            with np.load(path) as z:
                assert sorted(z.files) == sorted(arrays), name
                for k, v in arrays.items():
                    assert np.array_equal(z[k], v), (name, k)
            print("%s: matches" % path)
        else:
            np.savez_compressed(path, **arrays)
            print("%s: %d bytes, %d edges" % (path, os.path.getsize(path), arrays["ii"].shape[0]))


if __name__ == "__main__":
    main()
