"""`torch.ops.lgu.*`: the operator layer registered with torch.library, for callers that
dispatch through `torch.ops` (torch.compile graphs, serialized programs) instead of importing
the drop-in modules.  Same names, arguments and in-place side effects as `ops` /
the reference's pybind11 entries (offersample_LGS/droid.cpp:138-147, src/droid.cpp:239-242,246-247);
multi-tensor returns are Python lists exactly like the reference's std::vector<Tensor>.
Importing this module performs the registration once.
"""
from typing import List, Optional

import torch

from . import aggregate as _agg
from . import geom as _geom
from . import gru as _gru
from . import ops as _ops

_NS = "lgu"


def _define(name, mutates, fn):
    return torch.library.custom_op("%s::%s" % (_NS, name), mutates_args=mutates, device_types="cuda")(fn)


def _defCorr_index_forward(volume: torch.Tensor, coords: torch.Tensor, offset: torch.Tensor, radius: int) -> List[torch.Tensor]:
    return _ops.defCorr_index_forward(volume, coords, offset, radius)


def _defCorr_index_backward(volume: torch.Tensor, coords: torch.Tensor, offset: torch.Tensor, corr_grad: torch.Tensor,
                            radius: int) -> List[torch.Tensor]:
    return _ops.defCorr_index_backward(volume, coords, offset, corr_grad, radius)


def _corr_index_forward(volume: torch.Tensor, coords: torch.Tensor, radius: int) -> List[torch.Tensor]:
    return _ops.corr_index_forward(volume, coords, radius)


def _corr_index_backward(volume: torch.Tensor, coords: torch.Tensor, corr_grad: torch.Tensor, radius: int) -> List[torch.Tensor]:
    return _ops.corr_index_backward(volume, coords, corr_grad, radius)


def _gaussianMask(means: torch.Tensor, covs: torch.Tensor, volume: torch.Tensor, radius: int) -> List[torch.Tensor]:
    return _ops.gaussianMask(means, covs, volume, radius)


def _gaussianMask_backward(means: torch.Tensor, covs: torch.Tensor, volume: torch.Tensor, volume_grad: torch.Tensor,
                           radius: int) -> List[torch.Tensor]:
    return _ops.gaussianMask_backward(means, covs, volume, volume_grad, radius)


def _lowMem_defSample(fmap1: torch.Tensor, fmap2: torch.Tensor, coords: torch.Tensor, offset: torch.Tensor,
                      radius: int) -> List[torch.Tensor]:
    return _ops.lowMem_defSample(fmap1, fmap2, coords, offset, radius)


def _altcorr_forward(fmap1: torch.Tensor, fmap2: torch.Tensor, coords: torch.Tensor, radius: int) -> List[torch.Tensor]:
    return _ops.altcorr_forward(fmap1, fmap2, coords, radius)


def _altcorr_backward(fmap1: torch.Tensor, fmap2: torch.Tensor, coords: torch.Tensor, corr_grad: torch.Tensor,
                      radius: int) -> List[torch.Tensor]:
    return _ops.altcorr_backward(fmap1, fmap2, coords, corr_grad, radius)


def _frame_distance(poses: torch.Tensor, disps: torch.Tensor, intrinsics: torch.Tensor, ii: torch.Tensor, jj: torch.Tensor,
                    beta: float) -> torch.Tensor:
    return _geom.frame_distance(poses, disps, intrinsics, ii, jj, beta)


def _projmap(poses: torch.Tensor, disps: torch.Tensor, intrinsics: torch.Tensor, ii: torch.Tensor,
             jj: torch.Tensor) -> List[torch.Tensor]:
    return _geom.projmap(poses, disps, intrinsics, ii, jj)


def _depth_filter(poses: torch.Tensor, disps: torch.Tensor, intrinsics: torch.Tensor, ix: torch.Tensor,
                  thresh: torch.Tensor) -> torch.Tensor:
    return _geom.depth_filter(poses, disps, intrinsics, ix, thresh)


def _iproj(poses: torch.Tensor, disps: torch.Tensor, intrinsics: torch.Tensor) -> torch.Tensor:
    return _geom.iproj(poses, disps, intrinsics)


def _projective_transform(poses: torch.Tensor, disps: torch.Tensor, intrinsics: torch.Tensor, ii: torch.Tensor,
                          jj: torch.Tensor, jacobian: bool = False, return_depth: bool = False) -> List[torch.Tensor]:
    out = _geom.projective_transform(poses, disps, intrinsics, ii, jj, jacobian=jacobian, return_depth=return_depth)
    return [out[0], out[1]] + (list(out[2]) if jacobian else [])


def _motion_features(poses: torch.Tensor, disps: torch.Tensor, intrinsics: torch.Tensor, ii: torch.Tensor, jj: torch.Tensor,
                     target: torch.Tensor, clamp: float = 64.0) -> List[torch.Tensor]:
    return list(_geom.motion_features(poses, disps, intrinsics, ii, jj, target, clamp))



def _scatter_mean(src: torch.Tensor, index: torch.Tensor, dim: int = -1, dim_size: Optional[int] = None) -> torch.Tensor:
    return _agg.scatter_mean(src, index, dim=dim, dim_size=dim_size)


def _cvx_upsample(data: torch.Tensor, mask: torch.Tensor) -> torch.Tensor:
    return _agg.cvx_upsample(data, mask)


def _upsample_disp(disp: torch.Tensor, mask: torch.Tensor) -> torch.Tensor:
    return _agg.upsample_disp(disp, mask)


def _upsample_disps_(disps_up: torch.Tensor, disps: torch.Tensor, ix: torch.Tensor, mask: torch.Tensor) -> None:
    _agg.upsample_disps_(disps_up, disps, ix, mask)


def _kangru_context(net: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor) -> torch.Tensor:
    return _gru.kangru_context(net, weight, bias)


def _kan_heads(glo: torch.Tensor, grid: torch.Tensor, wpack: torch.Tensor) -> torch.Tensor:
    return _gru.kan_heads(glo, grid, wpack)


def _kangru_gates_(net_inp: torch.Tensor, cz: torch.Tensor, cr: torch.Tensor, kz: torch.Tensor, kr: torch.Tensor,
                   net: torch.Tensor) -> torch.Tensor:
    return _gru.kangru_gates_(net_inp, cz, cr, kz, kr, net)


def _kangru_blend(cq: torch.Tensor, kq: torch.Tensor, z: torch.Tensor, net: torch.Tensor) -> torch.Tensor:
    return _gru.kangru_blend(cq, kq, z, net)


REGISTERED = {}
if not hasattr(torch.ops, _NS) or not hasattr(getattr(torch.ops, _NS), "defCorr_index_forward"):
    for _name, _mut, _fn in (
        ("defCorr_index_forward", ("offset",), _defCorr_index_forward),
        ("defCorr_index_backward", ("offset",), _defCorr_index_backward),
        ("corr_index_forward", (), _corr_index_forward),
        ("corr_index_backward", (), _corr_index_backward),
        ("gaussianMask", (), _gaussianMask),
        ("gaussianMask_backward", (), _gaussianMask_backward),
        ("lowMem_defSample", ("offset",), _lowMem_defSample),
        ("altcorr_forward", (), _altcorr_forward),
        ("altcorr_backward", (), _altcorr_backward),
    ):
        REGISTERED[_name] = _define(_name, _mut, _fn)

# the geometry entries of droid_backends (lgu_slam_amd.geom), kept in a table of their own
GEOM_REGISTERED = {}
if not hasattr(getattr(torch.ops, _NS), "frame_distance"):
    for _name, _fn in (("frame_distance", _frame_distance), ("projmap", _projmap), ("depth_filter", _depth_filter),
                       ("iproj", _iproj)):
        GEOM_REGISTERED[_name] = _define(_name, (), _fn)

# projective_transform (list: coords, valid[, Ji, Jj, Jz]) and the motion features (list: coords1, motn)
REPROJ_REGISTERED = {}
if not hasattr(getattr(torch.ops, _NS), "projective_transform"):
    for _name, _fn in (("projective_transform", _projective_transform), ("motion_features", _motion_features)):
        REPROJ_REGISTERED[_name] = _define(_name, (), _fn)

# GraphAgg's segment mean and the convex upsampling (lgu_slam_amd.aggregate); upsample_disps_ writes disps_up in place
AGG_REGISTERED = {}
if not hasattr(getattr(torch.ops, _NS), "scatter_mean"):
    for _name, _mut, _fn in (("scatter_mean", (), _scatter_mean), ("cvx_upsample", (), _cvx_upsample),
                             ("upsample_disp", (), _upsample_disp), ("upsample_disps_", ("disps_up",), _upsample_disps_)):
        AGG_REGISTERED[_name] = _define(_name, _mut, _fn)

# the KAN-bias GRU of the update operator (lgu_slam_amd.gru); kangru_gates_ writes r*net into net_inp in place
GRU_REGISTERED = {}
if not hasattr(getattr(torch.ops, _NS), "kangru_context"):
    for _name, _mut, _fn in (("kangru_context", (), _kangru_context), ("kan_heads", (), _kan_heads),
                             ("kangru_gates_", ("net_inp",), _kangru_gates_), ("kangru_blend", (), _kangru_blend)):
        GRU_REGISTERED[_name] = _define(_name, _mut, _fn)
