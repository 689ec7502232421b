// Python binding (own code, test infrastructure) of the Eigen-free part of the reference's src/droid_kernels.cu.
// oracle/build_ref.py cuts that file (cut_droid_kernels: the Eigen includes / typedefs and SparseBlock .. ba_cuda go)
// and appends THIS file to it, so that both form one translation unit and the thin launchers below can launch the
// reference's __global__ kernels.  Nothing here computes.  The four geometry entries restate src/droid.cpp's
// contiguity checks (:84-85, :120-166, :220-234) and call the reference's own launchers; accum_cuda is called as it is;
// the BA kernels, which the reference launches only from ba_cuda / schur_block (:1222-1434, Eigen host code), get
// launchers that allocate their outputs as those functions do (zero-filled) and use the same launch geometry: one
// block of THREADS (256) threads per edge / per Schur block / per E row, pose_retr as <<<1, THREADS>>>.
//
// The reference kernels have no index guards and use 32-bit accessors: callers pass in-range ii / jj / ix / idx and
// non-empty inputs only (tests/test_droid_kernels_vs_reference_build.py).

#define REF_CHECK_INPUT(x) TORCH_CHECK(x.is_contiguous(), #x " must be contiguous")

static torch::Tensor ref_frame_distance(torch::Tensor poses, torch::Tensor disps, torch::Tensor intrinsics,
                                        torch::Tensor ii, torch::Tensor jj, const float beta) {
  REF_CHECK_INPUT(poses);
  REF_CHECK_INPUT(disps);
  REF_CHECK_INPUT(intrinsics);
  REF_CHECK_INPUT(ii);
  REF_CHECK_INPUT(jj);
  return frame_distance_cuda(poses, disps, intrinsics, ii, jj, beta);
}

static std::vector<torch::Tensor> ref_projmap(torch::Tensor poses, torch::Tensor disps, torch::Tensor intrinsics,
                                              torch::Tensor ii, torch::Tensor jj) {
  REF_CHECK_INPUT(poses);
  REF_CHECK_INPUT(disps);
  REF_CHECK_INPUT(intrinsics);
  REF_CHECK_INPUT(ii);
  REF_CHECK_INPUT(jj);
  return projmap_cuda(poses, disps, intrinsics, ii, jj);
}

static torch::Tensor ref_iproj(torch::Tensor poses, torch::Tensor disps, torch::Tensor intrinsics) {
  REF_CHECK_INPUT(poses);
  REF_CHECK_INPUT(disps);
  REF_CHECK_INPUT(intrinsics);
  return iproj_cuda(poses, disps, intrinsics);
}

static torch::Tensor ref_depth_filter(torch::Tensor poses, torch::Tensor disps, torch::Tensor intrinsics,
                                      torch::Tensor ix, torch::Tensor thresh) {
  REF_CHECK_INPUT(poses);
  REF_CHECK_INPUT(disps);
  REF_CHECK_INPUT(intrinsics);
  REF_CHECK_INPUT(ix);
  REF_CHECK_INPUT(thresh);
  return depth_filter_cuda(poses, disps, intrinsics, ix, thresh);
}

static torch::Tensor ref_accum(torch::Tensor data, torch::Tensor ix, torch::Tensor jx) {
  REF_CHECK_INPUT(data);
  return accum_cuda(data, ix, jx);
}

// ba_cuda's buffers (:1350-1355) and launch (:1359-1372): [Hs (4,E,6,6), vs (2,E,6), Eii, Eij (E,6,HW), Cii, wi (E,HW)]
static std::vector<torch::Tensor> ref_projective_transform(torch::Tensor targets, torch::Tensor weights,
                                                           torch::Tensor poses, torch::Tensor disps,
                                                           torch::Tensor intrinsics, torch::Tensor ii,
                                                           torch::Tensor jj) {
  REF_CHECK_INPUT(targets);
  REF_CHECK_INPUT(weights);
  REF_CHECK_INPUT(poses);
  REF_CHECK_INPUT(disps);
  REF_CHECK_INPUT(intrinsics);
  REF_CHECK_INPUT(ii);
  REF_CHECK_INPUT(jj);
  auto opts = poses.options();
  const int num = ii.size(0);
  const int ht = disps.size(1);
  const int wd = disps.size(2);
  torch::Tensor Hs = torch::zeros({4, num, 6, 6}, opts);
  torch::Tensor vs = torch::zeros({2, num, 6}, opts);
  torch::Tensor Eii = torch::zeros({num, 6, ht * wd}, opts);
  torch::Tensor Eij = torch::zeros({num, 6, ht * wd}, opts);
  torch::Tensor Cii = torch::zeros({num, ht * wd}, opts);
  torch::Tensor wi = torch::zeros({num, ht * wd}, opts);
  projective_transform_kernel<<<num, THREADS>>>(
      targets.packed_accessor32<float, 4, torch::RestrictPtrTraits>(),
      weights.packed_accessor32<float, 4, torch::RestrictPtrTraits>(),
      poses.packed_accessor32<float, 2, torch::RestrictPtrTraits>(),
      disps.packed_accessor32<float, 3, torch::RestrictPtrTraits>(),
      intrinsics.packed_accessor32<float, 1, torch::RestrictPtrTraits>(),
      ii.packed_accessor32<long, 1, torch::RestrictPtrTraits>(),
      jj.packed_accessor32<long, 1, torch::RestrictPtrTraits>(),
      Hs.packed_accessor32<float, 4, torch::RestrictPtrTraits>(),
      vs.packed_accessor32<float, 3, torch::RestrictPtrTraits>(),
      Eii.packed_accessor32<float, 3, torch::RestrictPtrTraits>(),
      Eij.packed_accessor32<float, 3, torch::RestrictPtrTraits>(),
      Cii.packed_accessor32<float, 2, torch::RestrictPtrTraits>(),
      wi.packed_accessor32<float, 2, torch::RestrictPtrTraits>());
  return {Hs, vs, Eii, Eij, Cii, wi};
}

// schur_block (:1286-1296): S (nblocks,6,6) from idx (nblocks,3) = (row of E, row of E, row of Q)
static torch::Tensor ref_eet(torch::Tensor E, torch::Tensor Q, torch::Tensor idx) {
  REF_CHECK_INPUT(E);
  REF_CHECK_INPUT(Q);
  REF_CHECK_INPUT(idx);
  torch::Tensor S = torch::zeros({idx.size(0), 6, 6}, E.options());
  EEt6x6_kernel<<<idx.size(0), THREADS>>>(
      E.packed_accessor32<float, 3, torch::RestrictPtrTraits>(),
      Q.packed_accessor32<float, 2, torch::RestrictPtrTraits>(),
      idx.packed_accessor32<long, 2, torch::RestrictPtrTraits>(),
      S.packed_accessor32<float, 3, torch::RestrictPtrTraits>());
  return S;
}

// schur_block (:1289-1303): v (n,6) from idx (n,1) = row of Q / w for E row n
static torch::Tensor ref_ev(torch::Tensor E, torch::Tensor Q, torch::Tensor w, torch::Tensor idx) {
  REF_CHECK_INPUT(E);
  REF_CHECK_INPUT(Q);
  REF_CHECK_INPUT(w);
  REF_CHECK_INPUT(idx);
  torch::Tensor v = torch::zeros({idx.size(0), 6}, E.options());
  Ev6x1_kernel<<<idx.size(0), THREADS>>>(
      E.packed_accessor32<float, 3, torch::RestrictPtrTraits>(),
      Q.packed_accessor32<float, 2, torch::RestrictPtrTraits>(),
      w.packed_accessor32<float, 2, torch::RestrictPtrTraits>(),
      idx.packed_accessor32<long, 2, torch::RestrictPtrTraits>(),
      v.packed_accessor32<float, 2, torch::RestrictPtrTraits>());
  return v;
}

// ba_cuda (:1408-1415): dw (n,HW) from the pose index of every E row (rows with index <= 0 or >= P stay zero)
static torch::Tensor ref_evt(torch::Tensor E, torch::Tensor x, torch::Tensor idx) {
  REF_CHECK_INPUT(E);
  REF_CHECK_INPUT(x);
  REF_CHECK_INPUT(idx);
  torch::Tensor dw = torch::zeros({idx.size(0), E.size(2)}, E.options());
  EvT6x1_kernel<<<idx.size(0), THREADS>>>(
      E.packed_accessor32<float, 3, torch::RestrictPtrTraits>(),
      x.packed_accessor32<float, 2, torch::RestrictPtrTraits>(),
      idx.packed_accessor32<long, 1, torch::RestrictPtrTraits>(),
      dw.packed_accessor32<float, 2, torch::RestrictPtrTraits>());
  return dw;
}

// ba_cuda (:1389-1391, :1420-1422): poses[t0:t1] updated in place
static void ref_pose_retr(torch::Tensor poses, torch::Tensor dx, const int t0, const int t1) {
  REF_CHECK_INPUT(poses);
  REF_CHECK_INPUT(dx);
  pose_retr_kernel<<<1, THREADS>>>(
      poses.packed_accessor32<float, 2, torch::RestrictPtrTraits>(),
      dx.packed_accessor32<float, 2, torch::RestrictPtrTraits>(), t0, t1);
}

// ba_cuda (:1425-1428): disps[inds[b]] += dz[b] in place
static void ref_disp_retr(torch::Tensor disps, torch::Tensor dz, torch::Tensor inds) {
  REF_CHECK_INPUT(disps);
  REF_CHECK_INPUT(dz);
  REF_CHECK_INPUT(inds);
  disp_retr_kernel<<<inds.size(0), THREADS>>>(
      disps.packed_accessor32<float, 3, torch::RestrictPtrTraits>(),
      dz.packed_accessor32<float, 2, torch::RestrictPtrTraits>(),
      inds.packed_accessor32<long, 1, torch::RestrictPtrTraits>());
}

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.def("frame_distance", &ref_frame_distance, "frame_distance (reference kernel)");
  m.def("projmap", &ref_projmap, "projmap (reference kernel)");
  m.def("iproj", &ref_iproj, "iproj (reference kernel)");
  m.def("depth_filter", &ref_depth_filter, "depth_filter (reference kernel)");
  m.def("accum", &ref_accum, "accum_cuda (reference kernel)");
  m.def("projective_transform", &ref_projective_transform, "projective_transform_kernel (reference kernel)");
  m.def("eet", &ref_eet, "EEt6x6_kernel (reference kernel)");
  m.def("ev", &ref_ev, "Ev6x1_kernel (reference kernel)");
  m.def("evt", &ref_evt, "EvT6x1_kernel (reference kernel)");
  m.def("pose_retr", &ref_pose_retr, "pose_retr_kernel (reference kernel)");
  m.def("disp_retr", &ref_disp_retr, "disp_retr_kernel (reference kernel)");
}
