"""Drop-in for the reference's `droid_backends` CUDA extension (src/droid.cpp:237-249).

Served here: the correlation entries `altcorr_forward` / `altcorr_backward` (src/droid.cpp:246-247) and the geometry
entries `frame_distance`, `projmap`, `depth_filter`, `iproj` (src/droid.cpp:239-242, lgu_slam_amd.geom).

DROID's original `corr_index_forward` / `corr_index_backward` (src/droid.cpp:248-249) are outside this build's scope:
they raise with a pointer to the reference extension instead of silently doing something else.  `ba` raises too unless
`lgu_slam_amd.install_dropins(experimental_ba=True)` bound it to this build's first device-side bundle adjustment
(lgu_slam_amd.ba.ba: held to the reference's Python BA at lm = 0 and to a restatement of `ba_cuda` otherwise, see
DESIGN.md §3.5).
"""
import lgu_slam_amd.geom as _geom
import lgu_slam_amd.ops as _ops

altcorr_forward = _ops.altcorr_forward
altcorr_backward = _ops.altcorr_backward

frame_distance = _geom.frame_distance
projmap = _geom.projmap
depth_filter = _geom.depth_filter
iproj = _geom.iproj


def _out_of_scope(name):
    def fn(*args, **kwargs):
        raise NotImplementedError(
            "droid_backends.%s is not part of the lgu_slam_amd hot-path library; "
            "use the reference's droid_backends build for it" % name)
    fn.__name__ = name
    return fn


for _n in ("ba", "corr_index_forward", "corr_index_backward"):
    globals()[_n] = _out_of_scope(_n)
