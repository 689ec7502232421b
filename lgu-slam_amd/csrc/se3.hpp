// se3.hpp — the reference's SE3 helpers (src/droid_kernels.cu:56-107) in its fp32 evaluation order, shared by the
// bundle adjustment (ba.hip) and the geometry operators (geom.hip).  Built with -ffp-contract=off: no FMA contraction.
#pragma once
#include <hip/hip_runtime.h>

namespace lgu {

__device__ __forceinline__ void cross3(const float* a, const float* b, float* c) {
  c[0] = a[1] * b[2] - a[2] * b[1];
  c[1] = a[2] * b[0] - a[0] * b[2];
  c[2] = a[0] * b[1] - a[1] * b[0];
}
__device__ __forceinline__ void act_so3(const float* q, const float* X, float* Y) {  // :56-67
  float uv[3], t[3];
  cross3(q, X, uv);
  uv[0] *= 2.0f; uv[1] *= 2.0f; uv[2] *= 2.0f;
  cross3(q, uv, t);
  Y[0] = X[0] + q[3] * uv[0] + t[0];
  Y[1] = X[1] + q[3] * uv[1] + t[1];
  Y[2] = X[2] + q[3] * uv[2] + t[2];
}
__device__ __forceinline__ void rel_se3(const float* ti, const float* qi, const float* tj, const float* qj, float* tij,
                                        float* qij) {  // :95-107
  qij[0] = -qj[3] * qi[0] + qj[0] * qi[3] - qj[1] * qi[2] + qj[2] * qi[1];
  qij[1] = -qj[3] * qi[1] + qj[1] * qi[3] - qj[2] * qi[0] + qj[0] * qi[2];
  qij[2] = -qj[3] * qi[2] + qj[2] * qi[3] - qj[0] * qi[1] + qj[1] * qi[0];
  qij[3] = qj[3] * qi[3] + qj[0] * qi[0] + qj[1] * qi[1] + qj[2] * qi[2];
  act_so3(qij, ti, tij);
  tij[0] = tj[0] - tij[0]; tij[1] = tj[1] - tij[1]; tij[2] = tj[2] - tij[2];
}

}  // namespace lgu
