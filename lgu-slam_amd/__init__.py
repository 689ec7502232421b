"""lgu_slam_amd — MI355X (gfx950) implementation of LGU-SLAM's deformable
correlation-sampling hot path: hand-written HIP kernels behind a C ABI
(include/lgu_corr.h), the reference's operator signatures (`ops`), and host-side
counterparts of its correlation glue (`corr`, `gaussian_mask`).

The on-disk directory is `lgu-slam_amd/`; `import lgu_slam_amd` works through the alias
module `lgu_slam_amd.py` at the repository root.
"""
import os
import sys

from . import _build, _lib, aggregate, ba, encoder, geom, graph, gru, ops, sharded  # noqa: F401
from .corr import AltCorrBlock, CorrBlock, CorrSampler, DefCorrSampler, per_Corr_Normalization  # noqa: F401
from .encoder import CorrEncoder  # noqa: F401
from .gaussian_mask import GaussianMask, GaussianMaskCuda  # noqa: F401
from .gru import KanBiasGRU  # noqa: F401

__version__ = "0.7.0"

DROPIN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "dropin")
DROPIN_SCATTER_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "dropin_scatter")


def build(force=False, verbose=False):
    """Compile the HIP kernels for gfx950 into lgu-slam_amd/liblgu_corr.so."""
    return _build.build(force=force, verbose=verbose)


def install_dropins(experimental_ba=False, torch_scatter=False):
    """Make `import defCorrSample` / `import droid_backends` resolve to this library, so the
    reference's droid_slam package runs on it unmodified.

    experimental_ba=True additionally binds `droid_backends.ba` to this build's device-side bundle adjustment
    (lgu_slam_amd.ba.ba) — a first version whose parity with the reference is unpinned (the reference BA needs Eigen
    and cannot be built here); by default that name raises, like the out-of-scope corr_index_* entries.

    torch_scatter=True also makes `import torch_scatter` resolve to dropin_scatter/torch_scatter.py (scatter_mean of
    lgu_slam_amd.aggregate; scatter_sum raises), so droid_slam/droid_net.py imports without torch_scatter.  It raises
    if another torch_scatter is already imported.  The default leaves a real torch_scatter alone."""
    if DROPIN_DIR not in sys.path:
        sys.path.insert(0, DROPIN_DIR)
    import defCorrSample  # noqa: F401
    import droid_backends  # noqa: F401
    if experimental_ba:
        sys.modules["droid_backends"].ba = ba.ba
    if torch_scatter:
        _install_torch_scatter()
    return sys.modules["defCorrSample"], sys.modules["droid_backends"]


def _install_torch_scatter():
    mine = os.path.join(DROPIN_SCATTER_DIR, "torch_scatter.py")
    have = sys.modules.get("torch_scatter")
    if have is not None:
        if os.path.abspath(getattr(have, "__file__", "") or "") != mine:
            raise RuntimeError("install_dropins(torch_scatter=True): another torch_scatter is already imported (%s)"
                               % getattr(have, "__file__", have))
        return
    if DROPIN_SCATTER_DIR not in sys.path:
        sys.path.insert(0, DROPIN_SCATTER_DIR)
    import torch_scatter  # noqa: F401
    if os.path.abspath(sys.modules["torch_scatter"].__file__) != mine:
        raise RuntimeError("install_dropins(torch_scatter=True): `import torch_scatter` resolved to %s"
                           % sys.modules["torch_scatter"].__file__)
