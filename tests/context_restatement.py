"""The seeded context-encoder cases that tools/gen_context_golden.py and tests/test_context.py share: the stand-in
RefEncoder(256, 'none') of tests/features_restatement.py (the reference's `cnet = BasicEncoder(output_dim=256,
norm_fn='none')`, droid_slam/droid_net.py) with seeded weights and images.  No weights are stored: the fixture's hash
pins what make_case regenerates."""
from tests import features_restatement as R

OUTPUT_DIM = 256
CASES = {"context_cnet_2x40x56": dict(seed=61, N=2, H=40, W=56),
         "context_cnet_1x64x48": dict(seed=62, N=1, H=64, W=48)}
STAGES = R.STAGES


def make_case(name, seed_offset=0):
    """(module, images) of a fixture case, float32 on the CPU; seed_offset != 0 gives further cases of the same shape."""
    cfg = CASES[name]
    m = R.set_weights(R.RefEncoder(OUTPUT_DIM, "none"), cfg["seed"] + 1000 + seed_offset).eval()
    return m, R.make_images(cfg["seed"] + seed_offset, cfg["N"], cfg["H"], cfg["W"])


case_sha256 = R.case_sha256
