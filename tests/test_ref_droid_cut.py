"""oracle/build_ref.py's cut of the reference's src/droid_kernels.cu (the Eigen part dropped for the ref_droid_kernels
builds that tests/test_droid_kernels_vs_reference_build.py loads).  Runs without a GPU wherever the reference source is
present, so that a changed reference fails here and not on the GPU box."""
import os
import re

import pytest

from oracle import build_ref as B

pytestmark = pytest.mark.skipif(not os.path.exists(B.DROID_SRC), reason="reference source not present")


def _source():
    with open(B.DROID_SRC) as fh:
        return fh.read()


def test_cut_drops_the_eigen_part_and_keeps_every_kernel(tmp_path):
    text = _source()
    assert re.search(r"\bEigen\b", text) and B.DROID_CUT_FROM in text      # there is something to cut
    unit = tmp_path / "ref_droid_kernels.cu"
    B.write_droid_unit(str(unit))
    out = unit.read_text()
    cut = B.cut_droid_kernels(text)
    assert out.startswith(cut)
    B.check_droid_cut(cut)
    assert not re.search(r"\bEigen\b", cut)
    for gone in ("SparseBlock", "schur_block", "ba_cuda", "SimplicialLLT"):
        assert gone not in cut, gone
    for k in B.DROID_KERNELS:
        assert re.search(r"__global__\s+void\s+%s\s*\(" % k, cut), k
    # nothing but the Eigen lines and the SparseBlock .. ba_cuda span is dropped: the rest is the source, in order
    head, tail = text.split(B.DROID_CUT_FROM)[0], B.DROID_CUT_TO + text.split(B.DROID_CUT_TO)[1]
    assert cut.endswith(tail)
    kept_head = [ln for ln in head.splitlines() if "Eigen" not in ln]
    assert cut[:len(cut) - len(tail)].splitlines() == kept_head
    # the appended binding launches the kernels and calls the launchers it names, all defined by the cut source
    bind = out[len(cut):]
    for k in ("projective_transform_kernel", "EEt6x6_kernel", "Ev6x1_kernel", "EvT6x1_kernel", "pose_retr_kernel",
              "disp_retr_kernel") + B.DROID_LAUNCHERS:
        assert re.search(r"\b%s\b" % k, bind), k
    assert "PYBIND11_MODULE(TORCH_EXTENSION_NAME" in bind


def test_cut_fails_loudly_when_the_source_changes():
    text = _source()
    with pytest.raises(RuntimeError, match="marker"):
        B.cut_droid_kernels(text.replace(B.DROID_CUT_FROM, "class DenseBlock"))
    with pytest.raises(RuntimeError, match="marker"):
        B.cut_droid_kernels(text + "\n" + B.DROID_CUT_TO + "torch::Tensor a);\n")
    with pytest.raises(RuntimeError, match="Eigen"):
        B.cut_droid_kernels(text + "\nstatic Eigen::VectorXd leftover;\n")
    with pytest.raises(RuntimeError, match="missing EEt6x6_kernel"):
        B.cut_droid_kernels(text.replace("void EEt6x6_kernel(", "void EEt_kernel("))
    with pytest.raises(RuntimeError, match="missing .*accum_cuda"):
        B.cut_droid_kernels(text.replace("torch::Tensor accum_cuda(", "torch::Tensor accum_host("))
