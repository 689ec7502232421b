"""Drop-in for lietorch (a CUDA extension with no ROCm build), put on the path by
`lgu_slam_amd.install_dropins(lietorch=True)`: the group objects of lgu_slam_amd.lie under the names the reference's
droid_slam modules import (`import lietorch`, `from lietorch import SE3, Sim3`).  Conventions, what runs on HIP kernels
and what does not: see lgu_slam_amd/lie.py.  There is no autograd."""
from lgu_slam_amd.lie import SE3, SO3, Sim3, cat, stack  # noqa: F401

__all__ = ["SO3", "SE3", "Sim3", "cat", "stack"]
