#!/usr/bin/env python3
"""Writes tests/golden/update_*.npz: the reference's own UpdateModule with its GraphAgg (droid_slam/droid_net.py), imported
unchanged and run in float64 on the CPU, the fixture the tests hold the stand-in tests/update_restatement.py and the fused
update operator to.

droid_net.py pulls in modules that do not exist on a CPU machine (defCorrSample, droid_backends, cv2, lietorch,
torch_scatter).  They are stubbed in sys.modules for the import only; sys.modules and sys.path are restored afterwards and
no bytecode is written.  The only stub that executes is torch_scatter.scatter_mean(src, index, dim=1), written here with
index_add_ and bincount in the source's dtype: nothing of the package under test takes part.  No text of the reference is
copied; only arrays are stored.

Inputs and parameters come from tests/update_restatement.py (make_case: seeded); the reference module takes the stand-in's
state_dict, .double().eval(), and runs under no_grad with update_restatement.record's hooks on it.  No inputs or weights
are stored: the hash pins what make_case regenerates.

Per case of update_restatement.CASES two files, so that each stays under 1 MiB; every float array is the float32 ROUNDING
of the float64 value (2^-24 relative, four orders of magnitude under any half-precision error measured against it):
 update_<case>.npz
  sha256                 case_sha256 of the inputs, ii and the state_dict
  keys                   list(state_dict().keys()) of the reference module
  ii (num,)              the edges' frames
  net, delta, weight, eta, upmask                                             the five results, in their own shapes
 update_<case>_stages.npz
  corr_feat (num,128,ht,wd), flow_feat (num,64,ht,wd), gru (num,128,ht,wd)    outputs of corr_encoder, flow_encoder, gru
  agg1 (num,128,ht,wd)   agg.conv1 behind its ReLU;   mean (U,128,ht,wd)  the input of agg.conv2, the per-frame mean
  agg2 (U,128,ht,wd)     agg.conv2 behind its ReLU
Usage: gen_update_golden.py [--reference DIR] [--out DIR] [--check]
--check compares with the committed files: hash, keys and ii exactly, every float array within 2 float32 ulps of its
largest magnitude (a CPU convolution's summation order may differ with the thread count).
"""
import sys

sys.dont_write_bytecode = True

import argparse  # noqa: E402
import importlib  # noqa: E402
import os  # noqa: E402
import types  # noqa: E402

import numpy as np  # noqa: E402
import torch  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from tests import update_restatement as R  # noqa: E402

ABSENT = ("defCorrSample", "droid_backends", "cv2", "lietorch", "torch_scatter")


def scatter_mean(src, index, dim=1):
    """torch_scatter.scatter_mean for the one call GraphAgg.forward makes: the mean over dim 1 by index, in src's dtype."""
    assert dim == 1 and index.dim() == 1 and index.shape[0] == src.shape[1]
    size = int(index.max()) + 1
    out = torch.zeros((src.shape[0], size) + tuple(src.shape[2:]), dtype=src.dtype, device=src.device)
    out.index_add_(1, index, src)
    count = torch.bincount(index, minlength=size).clamp(min=1).to(src.dtype)
    return out / count.view(1, -1, *([1] * (src.dim() - 2)))


class _Absent(types.ModuleType):
    """A module that is imported and never executed: any name taken from it is a placeholder that refuses to be called."""

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)

        def refuse(*args, **kwargs):
            raise RuntimeError("%s.%s is a stub of the fixture generator" % (self.__name__, name))
        return refuse


def import_reference_update(reference):
    """The reference's UpdateModule class, from droid_slam/droid_net.py imported unchanged over the stubs."""
    if not os.path.isdir(os.path.join(reference, "droid_slam")):
        raise RuntimeError("%s holds no droid_slam: the update fixtures need the reference tree" % reference)
    stubs = {name: _Absent(name) for name in ABSENT}
    stubs["torch_scatter"].scatter_mean = scatter_mean
    saved = {name: sys.modules.get(name) for name in ABSENT}
    before, saved_path = set(sys.modules), list(sys.path)
    try:
        sys.modules.update(stubs)
        sys.path.insert(0, reference)
        droid_net = importlib.import_module("droid_slam.droid_net")
    finally:
        sys.path[:] = saved_path
        for name in set(sys.modules) - before:
            if name.split(".")[0] == "droid_slam":
                del sys.modules[name]
        for name, mod in saved.items():
            if mod is None:
                sys.modules.pop(name, None)
            else:
                sys.modules[name] = mod
    assert os.path.abspath(droid_net.__file__).startswith(os.path.abspath(reference))
    return droid_net.UpdateModule


def generate(reference):
    UpdateModule = import_reference_update(reference)
    out = {}
    for name in sorted(R.CASES):
        u, ins, ii = R.make_case(name)
        ref = UpdateModule()
        ref.load_state_dict(u.state_dict())
        ref.double().eval()
        rec = R.run_recorded(ref, [None if t is None else t.double() for t in ins], ii)
        arrays = {k: rec[k].numpy().astype(np.float32) for k in R.STAGES + R.RESULTS}
        assert all(rec[k].dtype == torch.float64 for k in R.STAGES + R.RESULTS)
        arrays.update(sha256=np.array(R.case_sha256(u, ins, ii)), keys=np.array(list(ref.state_dict().keys())), ii=ii.numpy())
        out[name] = arrays
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("LGU_REFERENCE", "/root/reference"))
    ap.add_argument("--out", default=GOLDEN)
    ap.add_argument("--check", action="store_true")
    args = ap.parse_args()
    res = generate(args.reference)
    for name, every in res.items():
        for suffix, arrays in (("", {k: v for k, v in every.items() if k not in R.STAGES}),
                               ("_stages", {k: every[k] for k in R.STAGES})):
            path = os.path.join(args.out, name + suffix + ".npz")
            if args.check:
                with np.load(path) as z:
                    assert sorted(z.files) == sorted(arrays), (path, sorted(z.files))
                    for k, v in arrays.items():
                        if v.dtype != np.float32:
                            assert np.array_equal(z[k], v), (path, k)
                            continue
                        tol = 2 * float(np.spacing(np.abs(v).max()))
                        worst = float(np.abs(z[k].astype(np.float64) - v.astype(np.float64)).max())
                        assert z[k].shape == v.shape and z[k].dtype == np.float32 and worst <= tol, (path, k, worst, tol)
                print("%s: matches" % path)
            else:
                np.savez_compressed(path, **arrays)
                print("%s: %d bytes" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
