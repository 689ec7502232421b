"""lgu_slam_amd — MI355X (gfx950) implementation of LGU-SLAM's deformable
correlation-sampling hot path: hand-written HIP kernels behind a C ABI
(include/lgu_corr.h), the reference's operator signatures (`ops`), host-side
counterparts of its correlation glue (`corr`, `gaussian_mask`), and the SO3 / SE3 / Sim3
group objects its orchestration modules take from lietorch (`lie`).

The on-disk directory is `lgu-slam_amd/`; `import lgu_slam_amd` works through the alias
module `lgu_slam_amd.py` at the repository root.
"""
import os
import sys

from . import _build, _lib, aggregate, ba, cloud, context, conv1, conv3, encconv, encoder, features, flow, geom, graph, gru, heads, intake, lie, ops, render, sharded, upmask  # noqa: F401
from . import update  # noqa: F401
from .conv1 import Conv1  # noqa: F401
from .conv3 import Conv3, Conv3Stack, conv3x3_fanout  # noqa: F401
from .context import ContextEncoder  # noqa: F401
from .corr import AltCorrBlock, CorrBlock, CorrSampler, DefCorrSampler, per_Corr_Normalization  # noqa: F401
from .encconv import enc_conv3x3, enc_conv3x3_norm, enc_out1x1, enc_stem7x7, pack_enc1, pack_enc3, pack_out1, pack_stem  # noqa: F401
from .encoder import CorrEncoder  # noqa: F401
from .features import FeatureEncoder  # noqa: F401
from .flow import FlowEncoder  # noqa: F401
from . import gaussian_mask  # noqa: F401
from .gaussian_mask import GaussianHead, GaussianMask, GaussianMaskCuda, gaussian_head, pack_gaussian_head  # noqa: F401
from .gru import KanBiasGRU, gru_conv3x3, gru_conv_q, gru_conv_zr, pack_gruconv  # noqa: F401
from .heads import Head, head_pair  # noqa: F401
from .upmask import Upmask  # noqa: F401
from .update import UpdateOperator  # noqa: F401

__version__ = "0.8.0"

DROPIN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "dropin")
DROPIN_SCATTER_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "dropin_scatter")
DROPIN_LIETORCH_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "dropin_lietorch")


def build(force=False, verbose=False):
    """Compile the HIP kernels for gfx950 into lgu-slam_amd/liblgu_corr.so."""
    return _build.build(force=force, verbose=verbose)


def install_dropins(experimental_ba=False, torch_scatter=False, lietorch=False):
    """Make `import defCorrSample` / `import droid_backends` resolve to this library.  With lietorch=True and
    torch_scatter=True the modules of the reference's droid_slam package import unmodified; `cv2` and `open3d` remain
    the caller's.

    experimental_ba=True additionally binds `droid_backends.ba` to this build's device-side bundle adjustment
    (lgu_slam_amd.ba.ba) — a first version, held to the reference's own Python BA at lm = 0 (tests/test_ba_reference.py)
    and, for the damping with lm != 0 that `ba_cuda` applies its own way, to a restatement of `ba_cuda` (the reference's
    host driver needs Eigen and cannot be built here); by default that name raises, like the out-of-scope corr_index_*
    entries.

    torch_scatter=True also makes `import torch_scatter` resolve to dropin_scatter/torch_scatter.py (scatter_mean of
    lgu_slam_amd.aggregate; scatter_sum raises), so droid_slam/droid_net.py imports without torch_scatter.  It raises
    if another torch_scatter is already imported.  The default leaves a real torch_scatter alone.

    lietorch=True also makes `import lietorch` resolve to dropin_lietorch/lietorch.py (SO3, SE3, Sim3, cat and stack of
    lgu_slam_amd.lie).  It raises if another lietorch is already imported or if the import resolves elsewhere.  The
    default leaves a real lietorch alone."""
    if DROPIN_DIR not in sys.path:
        sys.path.insert(0, DROPIN_DIR)
    import defCorrSample  # noqa: F401
    import droid_backends  # noqa: F401
    if experimental_ba:
        sys.modules["droid_backends"].ba = ba.ba
    if torch_scatter:
        _install_module("torch_scatter", DROPIN_SCATTER_DIR)
    if lietorch:
        _install_module("lietorch", DROPIN_LIETORCH_DIR)
    return sys.modules["defCorrSample"], sys.modules["droid_backends"]


def _install_module(name, directory):
    mine = os.path.join(directory, name + ".py")
    have = sys.modules.get(name)
    if have is not None:
        if os.path.abspath(getattr(have, "__file__", "") or "") != mine:
            raise RuntimeError("install_dropins(%s=True): another %s is already imported (%s)"
                               % (name, name, getattr(have, "__file__", have)))
        return
    if directory not in sys.path:
        sys.path.insert(0, directory)
    __import__(name)
    if os.path.abspath(sys.modules[name].__file__) != mine:
        raise RuntimeError("install_dropins(%s=True): `import %s` resolved to %s" % (name, name, sys.modules[name].__file__))
