#!/usr/bin/env python3
"""Writes tests/golden/context_cnet_*.npz: the reference's own BasicEncoder(256, 'none'), its context encoder
(droid_slam/modules/extractor.py, droid_slam/droid_net.py), imported unchanged and run in float32 on the CPU, the fixture
the tests hold the stand-in RefEncoder(256, 'none') of tests/features_restatement.py to, bit for bit.

Weights and images come from tests/context_restatement.py (make_case: seeded); the reference module is loaded with that
state_dict and forward hooks record its stages.  No weights are stored: the hash pins what make_case regenerates.

Per file (2 frames of 3x40x56, 1 frame of 3x64x48):
  sha256                         case_sha256 of the images and the state_dict
  stem, layer1, layer2, layer3   the outputs after relu1 and after each layer (N, C, h, w)
  conv2                          the forward's result (1, N, 256, H/8, W/8)
Usage: gen_context_golden.py [--reference DIR] [--out DIR] [--check]   (--check: compare with the committed files)
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from tests import context_restatement as R  # noqa: E402


def import_reference_encoder(reference):
    if reference not in sys.path:
        sys.path.insert(0, reference)
    from droid_slam.modules.extractor import BasicEncoder
    return BasicEncoder


def generate(reference):
    BasicEncoder = import_reference_encoder(reference)
    out = {}
    for name in sorted(R.CASES):
        m, images = R.make_case(name)
        ref = BasicEncoder(output_dim=R.OUTPUT_DIM, norm_fn="none")
        ref.load_state_dict(m.state_dict())
        ref.eval()
        rec = {}

        def hook(key):
            def fn(mod, args, res):
                rec[key] = res.detach().clone()
            return fn
        for key, mod in (("stem", ref.relu1), ("layer1", ref.layer1), ("layer2", ref.layer2), ("layer3", ref.layer3)):
            mod.register_forward_hook(hook(key))
        with torch.no_grad():
            rec["conv2"] = ref(images)
        arrays = {k: rec[k].numpy() for k in R.STAGES}
        arrays["sha256"] = np.array(R.case_sha256(m, images))
        out[name] = arrays
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
                for k, v in arrays.items():
                    assert np.array_equal(z[k], v), (name, k)
            print("%s: matches" % path)
        else:
            np.savez_compressed(path, **arrays)
            print("%s: %d bytes" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
