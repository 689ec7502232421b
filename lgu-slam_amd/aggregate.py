"""GraphAgg's segment mean and the convex 8x upsampling of the disparity (reference droid_slam/droid_net.py:14-37,
:53-69 and depth_video.py:124-128) on the HIP kernels of csrc/aggregate.hip.

`scatter_mean` stands in for torch_scatter's (which has no ROCm build) in the call form the reference makes; the
drop-in module dropin_scatter/torch_scatter.py exports it.  `cvx_upsample`, `upsample_disp` and `upsample_disps_`
(DepthVideo.upsample in one launch) replace the reference's softmax / unfold / product / sum / permute / index_put
composition.

Index rule: an index outside [0, M) (scatter_mean) or [0, N) (upsample_disps_) is skipped: it is never used as an
address, it is not counted and it writes nothing.

Every input must be contiguous and live on a HIP device (no CPU fallback); every argument error is raised before
anything is launched.  Forward only: inputs that require grad are refused while grad mode is on.  Kernels are enqueued
on the current stream of the inputs' device, without host synchronisation (graph-capturable; scatter_mean only with
`dim_size` given).
"""
import torch

from ._host import FLOAT_OR_HALF, check_contiguous, check_device, check_dtype, check_no_grad, launch, typed
from ._host import ptr as _ptr, stream as _stream

UPS_MASK_F16, UPS_HALF_WEIGHTS = 1, 2     # include/lgu_corr.h LGU_UPS_*
_MASK_CH = 8 * 8 * 9


def scatter_mean(src, index, dim=-1, out=None, dim_size=None):
    """torch_scatter.scatter_mean for the call form the reference makes (GraphAgg.forward, droid_net.py:64): a 1-D int64
    `index` of length src.size(dim), `out=None`.  Returns (..., M, ...) of src's dtype (float32 or float16) with
    M = dim_size, the mean over the entries j with index[j] == m, summed in fp32 in ascending j and rounded once; an
    empty segment gives 0 and an index outside [0, M) is skipped.

    dim_size=None computes int(index.max()) + 1, which synchronises with the host (as torch_scatter does); with
    dim_size given the call is graph-capturable."""
    if out is not None:
        raise NotImplementedError("scatter_mean: only out=None is supported (the reference's call form "
                                  "scatter_mean(src, index, dim=d) with a 1-D index of length src.size(d))")
    if not isinstance(src, torch.Tensor) or not isinstance(index, torch.Tensor):
        raise TypeError("scatter_mean expects tensors src and index")
    nd = src.dim()
    if nd == 0 or not -nd <= dim < nd:
        raise IndexError("dim %d out of range for a %d-D src" % (dim, nd))
    dim = dim % nd
    if index.dim() != 1 or index.shape[0] != src.shape[dim]:
        raise NotImplementedError("scatter_mean: only a 1-D index of length src.size(dim) = %d is supported (the "
                                  "reference's call form), got index of shape %s" % (src.shape[dim], tuple(index.shape)))
    named = [(src, "src"), (index, "index")]
    check_contiguous(named)
    check_dtype(named[:1], FLOAT_OR_HALF)
    check_dtype(named[1:], torch.int64)
    if dim_size is not None and int(dim_size) < 0:
        raise RuntimeError("dim_size must be >= 0, got %d" % int(dim_size))
    check_no_grad("scatter_mean", named)
    check_device(named)
    n = src.shape[dim]
    if dim_size is None:
        M = max(int(index.max()) + 1, 0) if n > 0 else 0     # host sync, as in torch_scatter; all negative: M = 0
    else:
        M = int(dim_size)
    outer = 1
    for s in src.shape[:dim]:
        outer *= s
    inner = 1
    for s in src.shape[dim + 1:]:
        inner *= s
    shape = list(src.shape)
    shape[dim] = M
    res = torch.empty(shape, dtype=src.dtype, device=src.device)
    if res.numel() == 0:
        return res
    launch(typed("lgu_scatter_mean", src.dtype), "scatter_mean", src.device, _ptr(src), _ptr(index), outer, n, inner, M, _ptr(res),
           _stream(src))
    return res


def _mask_flags(mask):
    """LGU_UPS_* for this mask as torch would compute the reference's softmax: a half mask gives half weights, unless
    autocast is on (softmax is on autocast's float32 list, the weights stay float32)."""
    check_dtype([(mask, "mask")], FLOAT_OR_HALF)
    if mask.dtype == torch.float32:
        return 0
    return UPS_MASK_F16 | (0 if torch.is_autocast_enabled() else UPS_HALF_WEIGHTS)


def _check_mask(mask, U, ht, wd):
    """mask must be (U,576,ht,wd), optionally with leading 1s (GraphAgg's upmask is (1,U,576,ht,wd))."""
    shape = tuple(mask.shape)
    while len(shape) > 4 and shape[0] == 1:
        shape = shape[1:]
    if shape != (U, _MASK_CH, ht, wd):
        raise RuntimeError("mask must be (%d,%d,%d,%d), optionally with leading 1s, got %s"
                           % (U, _MASK_CH, ht, wd, tuple(mask.shape)))


def cvx_upsample(data, mask):
    """The reference's cvx_upsample (droid_net.py:15-29) for data width 1: data (B,ht,wd,1) float32, mask (B,576,ht,wd)
    (optionally with leading 1s) float32 or float16 -> (B,8ht,8wd,1) float32.  Each output is the
    softmax over the 9 neighbour weights of its sub-pixel applied to the 3x3 neighbourhood of its coarse pixel (zero
    outside the frame).  A half mask outside autocast gives half weights, as torch.softmax does."""
    if data.dim() != 4:
        raise RuntimeError("data must be (B,ht,wd,dim), got %s" % (tuple(data.shape),))
    if data.shape[3] != 1:
        raise NotImplementedError("cvx_upsample: only data width 1 (the disparity) is supported, got %d" % data.shape[3])
    named = [(data, "data"), (mask, "mask")]
    check_contiguous(named)
    check_dtype(named[:1], torch.float32)
    B, ht, wd, _ = data.shape
    _check_mask(mask, B, ht, wd)
    flags = _mask_flags(mask)
    check_no_grad("cvx_upsample", named)
    check_device(named)
    res = torch.empty((B, 8 * ht, 8 * wd, 1), dtype=torch.float32, device=data.device)
    if res.numel() == 0:
        return res
    launch("lgu_cvx_upsample_f32", "cvx_upsample", data.device, _ptr(data), _ptr(mask), B, ht, wd, flags, _ptr(res),
           _stream(data))
    return res


def upsample_disp(disp, mask):
    """The reference's upsample_disp (droid_net.py:31-35): disp (batch,num,ht,wd) float32, mask (batch,num,576,ht,wd) ->
    (batch,num,8ht,8wd)."""
    if disp.dim() != 4:
        raise RuntimeError("disp must be (batch,num,ht,wd), got %s" % (tuple(disp.shape),))
    batch, num, ht, wd = disp.shape
    check_contiguous([(disp, "disp"), (mask, "mask")])
    if tuple(mask.shape) not in ((batch, num, _MASK_CH, ht, wd), (batch * num, _MASK_CH, ht, wd)):
        raise RuntimeError("mask must be (%d,%d,%d,%d,%d), got %s" % (batch, num, _MASK_CH, ht, wd, tuple(mask.shape)))
    return cvx_upsample(disp.view(batch * num, ht, wd, 1), mask.view(batch * num, _MASK_CH, ht, wd)).view(
        batch, num, 8 * ht, 8 * wd)


def upsample_disps_(disps_up, disps, ix, mask):
    """DepthVideo.upsample (depth_video.py:124-128) in one launch, in place: disps_up[ix[u]] = cvx_upsample of
    disps[ix[u]] with mask[u], for every u.  disps_up (N,8ht,8wd) and disps (N,ht,wd) float32, ix (U,) int64, mask
    (U,576,ht,wd) or GraphAgg's upmask (1,U,576,ht,wd), float32 or float16.  Rows of disps_up not in ix are untouched;
    an ix[u] outside [0, N) writes nothing.  With duplicates in ix one of the rows wins, as with index_put (ix comes
    from torch.unique: there are none).  Returns disps_up."""
    if disps.dim() != 3:
        raise RuntimeError("disps must be (N,ht,wd), got %s" % (tuple(disps.shape),))
    N, ht, wd = disps.shape
    if tuple(disps_up.shape) != (N, 8 * ht, 8 * wd):
        raise RuntimeError("disps_up must be (N,8ht,8wd) = %s, got %s" % ((N, 8 * ht, 8 * wd), tuple(disps_up.shape)))
    if ix.dim() != 1:
        raise RuntimeError("ix must be 1-D, got %s" % (tuple(ix.shape),))
    named = [(disps_up, "disps_up"), (disps, "disps"), (ix, "ix"), (mask, "mask")]
    check_contiguous(named)
    check_dtype(named[:2], torch.float32)
    check_dtype(named[2:3], torch.int64)
    U = ix.shape[0]
    _check_mask(mask, U, ht, wd)
    flags = _mask_flags(mask)
    check_no_grad("upsample_disps_", named)
    check_device(named)
    if U * N * ht * wd == 0:
        return disps_up
    launch("lgu_upsample_disps_f32", "upsample_disps_", disps.device, _ptr(disps), N, ht, wd, _ptr(ix), U, _ptr(mask), flags,
           _ptr(disps_up), _stream(disps))
    return disps_up
