// geom_pixel.hpp — the per-pixel definitions the geometry operators (geom.hip) and the map export (cloud.hip) share: the
// neighbour transforms and the count of depth_filter (reference src/droid_kernels.cu:661-776) and the back-projection of
// iproj (:779-851), each in the reference's fp32 operation order.  One definition each: what geom.hip's tests pin to the
// reference's own build is what cloud.hip computes.  Built with -ffp-contract=off.
#pragma once
#include <limits.h>

#include "se3.hpp"

namespace lgu {

constexpr int GEOM_THREADS = 256;
constexpr int DF_NEIGHBOURS = 6;

// static_cast<int>(floor(x)) as the hardware conversion (v_cvt_i32_f32) performs it, which is what the reference gets on
// every vendor: NaN -> 0, values outside the int range saturate.  Written out so that no input is undefined behaviour.
__device__ __forceinline__ int cvt_i32_sat(float f) {
  if (f != f) return 0;
  if (f >= 2147483648.0f) return INT_MAX;
  if (f < -2147483648.0f) return INT_MIN;
  return (int)f;
}

__device__ __forceinline__ bool valid_index(long long v, int nvalid) { return v >= 0 && v < nvalid; }

// Neighbour n of frame a (valid): ix-1, ix-2, ix-3, ix+3, ix+4, ix+5 (the reference's `neigh < 3 ? ix - neigh - 1 :
// ix + neigh`).  rel = t_ij[3], q_ij[4] and *nbr = the neighbour's frame, or *nbr = -1 for one outside the buffer.
__device__ __forceinline__ void depth_filter_neighbour(const float* __restrict__ poses, long long a, int n, int nvalid,
                                                       float* rel, int* nbr) {
  const int ix = (int)a;
  const long long jx = n < 3 ? a - n - 1 : a + n;
  if (valid_index(jx, nvalid)) {
    rel_se3(poses + ix * 7, poses + ix * 7 + 3, poses + jx * 7, poses + jx * 7 + 3, rel, rel + 3);
    *nbr = (int)jx;
  } else {
    *nbr = -1;
  }
}

// The count of pixel k = (i, j) of frame ix with disparity di: the neighbours in which it projects inside the image with a
// disparity of one of the four pixels around the projection within t.  The disparity comparisons are in double, as in the
// reference; dj_hat / err (computed and unused there) are skipped.
__device__ __forceinline__ int depth_filter_count(const float* __restrict__ disps, float fx, float fy, float cx, float cy,
                                                  double t, const float (*rel)[7], const int* nbr, float di, int i, int j,
                                                  int ht, int wd) {
  const size_t HW = (size_t)(ht * wd);
  const float ui = static_cast<float>(j), vi = static_cast<float>(i);
  const float X[3] = {(ui - cx) / fx, (vi - cy) / fy, 1.0f};
  int cnt = 0;
  for (int n = 0; n < DF_NEIGHBOURS; n++) {
    const int jx = nbr[n];
    if (jx < 0) continue;  // uniform
    const float* R = rel[n];
    float Y[3];
    act_so3(R + 3, X, Y);
    Y[0] += di * R[0];
    Y[1] += di * R[1];
    Y[2] += di * R[2];
    const float uj = fx * (Y[0] / Y[2]) + cx;
    const float vj = fy * (Y[1] / Y[2]) + cy;
    const float dj = di / Y[2];
    const int u0 = cvt_i32_sat(floorf(uj)), v0 = cvt_i32_sat(floorf(vj));
    if (u0 >= 0 && v0 >= 0 && u0 < wd - 1 && v0 < ht - 1) {
      const float* Dj = disps + (size_t)jx * HW + (size_t)v0 * wd + u0;
      const float d00 = Dj[0], d01 = Dj[1], d10 = Dj[wd], d11 = Dj[wd + 1];
      const double r = 1.0 / (double)dj;
      if (fabs(r - 1.0 / (double)d00) < t || fabs(r - 1.0 / (double)d01) < t || fabs(r - 1.0 / (double)d10) < t ||
          fabs(r - 1.0 / (double)d11) < t)
        cnt++;
    }
  }
  return cnt;
}

// P = act_se3(T, (x, y, 1, d))[0:3] / d for pixel (i, j) with disparity di; T = t[0:3], q = t[3:7].
__device__ __forceinline__ void iproj_point(const float* t, float fx, float fy, float cx, float cy, float di, int i, int j,
                                            float* P) {
  const float ui = static_cast<float>(j), vi = static_cast<float>(i);
  const float X[3] = {(ui - cx) / fx, (vi - cy) / fy, 1.0f};
  float Y[3];
  act_so3(t + 3, X, Y);
  Y[0] += di * t[0];
  Y[1] += di * t[1];
  Y[2] += di * t[2];
  P[0] = Y[0] / di;
  P[1] = Y[1] / di;
  P[2] = Y[2] / di;
}

inline bool geom_dims_ok(int np, int nd, int ht, int wd) {
  return np >= 0 && nd >= 0 && ht >= 0 && wd >= 0 && (long long)ht * wd <= (long long)INT_MAX / 3;
}

inline int pixel_blocks(int ht, int wd) { return (ht * wd + GEOM_THREADS - 1) / GEOM_THREADS; }

}  // namespace lgu
