"""Drop-in for torch_scatter (no ROCm build), put on the path by `lgu_slam_amd.install_dropins(torch_scatter=True)`.

Served here: `scatter_mean` in the call form of GraphAgg.forward (droid_slam/droid_net.py:64), on the HIP kernel of
lgu_slam_amd.aggregate.  `scatter_sum` exists so that droid_slam/geom/ba.py imports; its only caller is the
training-side bundle adjustment, which needs autograd, and it raises.
"""
import lgu_slam_amd.aggregate as _agg

scatter_mean = _agg.scatter_mean


def scatter_sum(src, index, dim=-1, out=None, dim_size=None):
    raise NotImplementedError("torch_scatter.scatter_sum is not served by lgu_slam_amd: its only caller in the reference "
                              "is the training-side bundle adjustment (droid_slam/geom/ba.py), which needs autograd")
