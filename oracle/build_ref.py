#!/usr/bin/env python3
"""Builds the REFERENCE's own kernels for gfx950 into oracle/_ref/ (test infrastructure).

What it builds, from the sources where they lie under /root/reference:
  ref_defCorrSample.so  <- offersample_LGS/{droid.cpp, defCorrSample_kernel.cu,
                           corrSample_kernel.cu, gaussianAttn.cu, lowMem_defSample.cu}
                           (the whole `defCorrSample` extension, its own pybind11 binding)
  ref_altcorr.so        <- src/altcorr_kernel.cu + oracle/ref_altcorr_bind.cpp (own binding
                           of the two altcorr launchers; the reference binds them in
                           src/droid.cpp next to BA code that needs Eigen/lietorch — absent)
  ref_droid_kernels.so  <- the Eigen-free part of src/droid_kernels.cu (`cut_droid_kernels`: the
  ref_droid_kernels_nofma.so  Eigen includes / typedefs and `class SparseBlock` .. `ba_cuda` dropped)
                           with oracle/ref_droid_bind.cu appended to the same translation unit
                           (own binding of the geometry launchers, accum_cuda and the BA kernels).
                           Two variants: the compiler's default contraction (a*b+c -> FMA, like
                           nvcc's --fmad=true) and -ffp-contract=off (how lgu-slam_amd is built).

How: `torch.utils.cpp_extension.load`, i.e. the standard PyTorch-ROCm extension build that
the reference's own `CUDAExtension` setup.py would run on a ROCm machine: torch's bundled
hipify rewrites the CUDA headers/intrinsics to HIP, hipcc compiles for gfx950.  No stand-in
headers or stubs are written.  hipify needs writable copies, so the sources are copied to a
temporary directory OUTSIDE the repository and removed afterwards; only the .so files
stay, under oracle/_ref/ (git-ignored, but shipped to the GPU box with the snapshot).
They are only ever loaded by the tests, oracle/gen_golden.py and tools/compare_ref.py on the GPU box.
"""
import os
import re
import shutil
import sys
import tempfile

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "_ref")

TARGETS = {
    "ref_defCorrSample": [os.path.join(REF, "offersample_LGS", n) for n in
                          ("droid.cpp", "defCorrSample_kernel.cu", "corrSample_kernel.cu", "gaussianAttn.cu",
                           "lowMem_defSample.cu")],
    "ref_altcorr": [os.path.join(REF, "src", "altcorr_kernel.cu"), os.path.join(HERE, "ref_altcorr_bind.cpp")],
}

# ---- src/droid_kernels.cu without its Eigen part ----------------------------------------------------------------------
DROID_SRC = os.path.join(REF, "src", "droid_kernels.cu")
DROID_BIND = os.path.join(HERE, "ref_droid_bind.cu")
DROID_VARIANTS = {"ref_droid_kernels": [], "ref_droid_kernels_nofma": ["-ffp-contract=off"]}   # name -> extra hipcc flags
# what the binding uses from the cut source: every kernel outside the Eigen part and the host launchers it calls
DROID_KERNELS = ("projective_transform_kernel", "projmap_kernel", "frame_distance_kernel", "depth_filter_kernel",
                 "iproj_kernel", "accum_kernel", "pose_retr_kernel", "disp_retr_kernel", "EEt6x6_kernel", "Ev6x1_kernel",
                 "EvT6x1_kernel")
DROID_LAUNCHERS = ("accum_cuda", "frame_distance_cuda", "projmap_cuda", "depth_filter_cuda", "iproj_cuda")
DROID_CUT_FROM, DROID_CUT_TO = "class SparseBlock", "torch::Tensor frame_distance_cuda("


def cut_droid_kernels(text):
    """The Eigen-free part of droid_kernels.cu: drops the `#include <Eigen/...>` lines, the typedefs that name Eigen and
    everything from `class SparseBlock` up to (not including) `torch::Tensor frame_distance_cuda(`.  Cut by these
    markers, never by line numbers; raises RuntimeError if a marker is missing or repeated or the result fails
    check_droid_cut."""
    kept = [ln for ln in text.splitlines(keepends=True)
            if not re.match(r"\s*#\s*include\s*<Eigen/", ln) and not re.match(r"\s*typedef\b.*\bEigen::", ln)]
    src = "".join(kept)
    for marker in (DROID_CUT_FROM, DROID_CUT_TO):
        if src.count(marker) != 1:
            raise RuntimeError("droid_kernels.cu: marker %r found %d times, expected once" % (marker, src.count(marker)))
    a, b = src.index(DROID_CUT_FROM), src.index(DROID_CUT_TO)
    if a >= b:
        raise RuntimeError("droid_kernels.cu: %r does not come before %r" % (DROID_CUT_FROM, DROID_CUT_TO))
    out = src[:a] + src[b:]
    check_droid_cut(out)
    return out


def check_droid_cut(out):
    """Raises RuntimeError unless `out` holds no Eigen token and no host BA code, and defines every kernel and launcher
    the binding uses."""
    if re.search(r"\bEigen\b", out):
        raise RuntimeError("droid_kernels.cu cut: an `Eigen` token remains")
    for gone in ("SparseBlock", "schur_block", "ba_cuda"):
        if re.search(r"\b%s\b" % gone, out):
            raise RuntimeError("droid_kernels.cu cut: %s remains" % gone)
    missing = [k for k in DROID_KERNELS if not re.search(r"__global__\s+void\s+%s\s*\(" % k, out)]
    missing += [f for f in DROID_LAUNCHERS
                if not re.search(r"^(?:torch::Tensor|std::vector<torch::Tensor>)\s+%s\s*\(" % f, out, re.M)]
    if missing:
        raise RuntimeError("droid_kernels.cu cut: missing %s" % ", ".join(missing))


def write_droid_unit(path):
    """The translation unit of the ref_droid_kernels* builds: the cut source, then the binding (which launches the
    reference's __global__ kernels directly, so it has to be in the same unit)."""
    with open(DROID_SRC) as fh:
        cut = cut_droid_kernels(fh.read())
    with open(DROID_BIND) as fh:
        bind = fh.read()
    with open(path, "w") as fh:
        fh.write(cut + "\n\n" + bind)


def main():
    if not os.path.isdir(REF):
        print("build_ref: %s not present — nothing to do" % REF)
        return 0
    os.environ.setdefault("PYTORCH_ROCM_ARCH", "gfx950")
    from torch.utils import cpp_extension as ce
    os.makedirs(OUT, exist_ok=True)
    jobs = [(name, srcs, None) for name, srcs in TARGETS.items()]
    jobs += [(name, [DROID_SRC, DROID_BIND, os.path.abspath(__file__)], flags) for name, flags in DROID_VARIANTS.items()]
    for name, srcs, droid_flags in jobs:
        so = os.path.join(OUT, name + ".so")
        if os.path.exists(so) and all(os.path.getmtime(so) >= os.path.getmtime(s) for s in srcs):
            print("build_ref: %s up to date" % so)
            continue
        tmp = tempfile.mkdtemp(prefix="lgu_ref_src_")
        bld = tempfile.mkdtemp(prefix="lgu_ref_bld_")
        try:
            if droid_flags is None:
                local = []
                for s in srcs:
                    shutil.copy(s, tmp)
                    local.append(os.path.join(tmp, os.path.basename(s)))
                flags = []
            else:
                local = [os.path.join(tmp, name + ".cu")]
                write_droid_unit(local[0])
                flags = droid_flags
            ce.load(name=name, sources=local, build_directory=bld, extra_cflags=["-O2"],
                    extra_cuda_cflags=["-O2"] + flags, verbose=False, is_python_module=False)
            shutil.copy(os.path.join(bld, name + ".so"), so)
            print("build_ref: built %s" % so)
        finally:
            shutil.rmtree(tmp, ignore_errors=True)
            shutil.rmtree(bld, ignore_errors=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
