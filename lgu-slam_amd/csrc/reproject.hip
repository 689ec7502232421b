// reproject.hip — projective_transform of the reference's geom/projective_ops.py (:98-128, with iproj / actp / proj at
// :18-96) and the motion features FactorGraph.update builds from it (factor_graph.py:210-212, :268-270), without lietorch.
//
// Per-pixel arithmetic is a fixed fp32 order (built with -ffp-contract=off; fp32 `/` is correctly rounded), held bit for
// bit to the float32 restatement tests/reproject_restatement.py:
//   X0 = ((u - cx_i) / fx_i, (v - cy_i) / fy_i, 1, disp)            intrinsics of frame ii, u = column, v = row
//   G_ij = G_j * G_i^-1 (rel_se3), or t = (-0.1, 0, 0), q = identity where ii == jj (the stereo baseline)
//   X1 = act_so3(q, X0[:3]) + t * disp, homogeneous component disp
//   Z = X1.z < 0.1f ? 1 : X1.z;  d = 1 / Z;  (fx_j * (X1.x * d) + cx_j, fy_j * (X1.y * d) + cy_j[, disp * d])
//   valid = (X1.z > 0.2f) & (1 > 0.2f)                               float32 comparisons, as torch makes them
// Jacobians (JAC): Jp = [[a0, 0, a2, 0], [0, b1, b2, 0]] with a0 = fx_j * d, a2 = ((-fx_j * X) * d) * d (b alike),
// Ja = [[D I, -[X1]x], [0, 0]] in lietorch's tangent order (translation, rotation); Jj = Jp Ja with its structural zeros
// left out; Ji = -(Jj Adj(G_ij)) row by row: (R^T a_t, R^T (a_r + a_t x t)), R^T applied as act_so3 of the conjugate;
// Jz = Jp (t, 1).  Quaternions are used as given (not normalised).
//
// Index rule: an edge is valid when 0 <= ii, jj < min(np, nd, ni).  No kernel dereferences an invalid index; such an
// edge gets NaN coordinates, Jacobians and motion channels and valid = 0.  Every output element is written.
#include <limits.h>

#include "lgu_common.hpp"
#include "se3.hpp"

namespace lgu {

constexpr int RP_THREADS = 256;

__device__ __forceinline__ bool edge_index_ok(long long v, int nvalid) { return v >= 0 && v < nvalid; }


// NaN-propagating clamp (torch.clamp): a NaN fails both comparisons and is returned as it is.
__device__ __forceinline__ float clamp_nan(float v, float lo, float hi) { return v < lo ? lo : (v > hi ? hi : v); }

// One thread per pixel of edge blockIdx.x, batch blockIdx.z.  G_ij and the two intrinsics rows are built once per
// workgroup in LDS.  JAC: Ji, Jj (2x6 each, three 16-byte stores per pixel) and Jz (2x1); DEPTH: a third coordinate
// channel; MOTN: the motion-feature form (coords1 (B,E,H,W,2) and motn (B,E,4,H,W) from target (B,E,H,W,2)).  valid
// may be null.
template <bool JAC, bool DEPTH, bool MOTN>
__global__ __launch_bounds__(RP_THREADS) void reproject_kernel(
    const float* __restrict__ poses, const float* __restrict__ disps, const float* __restrict__ intrinsics,
    const long long* __restrict__ ii, const long long* __restrict__ jj, const float* __restrict__ target,
    float* __restrict__ coords, float* __restrict__ valid, float* __restrict__ Ji, float* __restrict__ Jj,
    float* __restrict__ Jz, float* __restrict__ motn, int np, int nd, int ni, int nvalid, int num, int ht, int wd,
    float bound) {
  __shared__ float sh[15];  // t_ij[3], q_ij[4], fx fy cx cy of frame ii, fx fy cx cy of frame jj
  const int e = blockIdx.x, b = blockIdx.z;
  const int HW = ht * wd;
  const int k = blockIdx.y * RP_THREADS + threadIdx.x;
  const long long a = ii[e], c = jj[e];
  const bool ok = edge_index_ok(a, nvalid) && edge_index_ok(c, nvalid);  // uniform over the workgroup
  if (ok && threadIdx.x == 0) {
    const float* Pi = poses + ((size_t)b * np + a) * 7;
    const float* Pj = poses + ((size_t)b * np + c) * 7;
    if (a == c) {
      sh[0] = -0.1f;
      sh[1] = sh[2] = 0.0f;
      sh[3] = sh[4] = sh[5] = 0.0f;
      sh[6] = 1.0f;
    } else {
      rel_se3(Pi, Pi + 3, Pj, Pj + 3, sh, sh + 3);
    }
    const float* Ki = intrinsics + ((size_t)b * ni + a) * 4;
    const float* Kj = intrinsics + ((size_t)b * ni + c) * 4;
    for (int m = 0; m < 4; m++) {
      sh[7 + m] = Ki[m];
      sh[11 + m] = Kj[m];
    }
  }
  __syncthreads();
  if (k >= HW) return;
  const size_t pix = ((size_t)b * num + e) * HW + k;  // pixel index into the (B,E,H,W) outputs
  const int i = k / wd, j = k - i * wd;
  const float u = static_cast<float>(j), v = static_cast<float>(i);
  if (!ok) {
    const float nan = __builtin_nanf("");
    if (DEPTH) {
      coords[pix * 3] = nan;
      coords[pix * 3 + 1] = nan;
      coords[pix * 3 + 2] = nan;
    } else {
      *reinterpret_cast<f32x2*>(coords + pix * 2) = f32x2{nan, nan};
    }
    if (valid) valid[pix] = 0.0f;
    if (JAC) {
      const f32x4 n4 = {nan, nan, nan, nan};
      f32x4* I4 = reinterpret_cast<f32x4*>(Ji + pix * 12);
      f32x4* J4 = reinterpret_cast<f32x4*>(Jj + pix * 12);
      I4[0] = n4; I4[1] = n4; I4[2] = n4;
      J4[0] = n4; J4[1] = n4; J4[2] = n4;
      *reinterpret_cast<f32x2*>(Jz + pix * 2) = f32x2{nan, nan};
    }
    if (MOTN) {
      float* M = motn + ((size_t)b * num + e) * 4 * HW + k;
      M[0] = nan;
      M[HW] = nan;
      M[2 * HW] = nan;
      M[3 * HW] = nan;
    }
    return;
  }
  const float t[3] = {sh[0], sh[1], sh[2]}, q[4] = {sh[3], sh[4], sh[5], sh[6]};
  const float fxi = sh[7], fyi = sh[8], cxi = sh[9], cyi = sh[10];
  const float fxj = sh[11], fyj = sh[12], cxj = sh[13], cyj = sh[14];
  const float D = disps[((size_t)b * nd + a) * HW + k];
  const float X0[3] = {(u - cxi) / fxi, (v - cyi) / fyi, 1.0f};
  float X1[3];
  act_so3(q, X0, X1);
  X1[0] = X1[0] + t[0] * D;
  X1[1] = X1[1] + t[1] * D;
  X1[2] = X1[2] + t[2] * D;
  const float Z = X1[2] < 0.1f ? 1.0f : X1[2];
  const float d = 1.0f / Z;
  const float cu = fxj * (X1[0] * d) + cxj;
  const float cv = fyj * (X1[1] * d) + cyj;
  if (valid) valid[pix] = (X1[2] > 0.2f && X0[2] > 0.2f) ? 1.0f : 0.0f;
  if (DEPTH) {
    coords[pix * 3] = cu;
    coords[pix * 3 + 1] = cv;
    coords[pix * 3 + 2] = D * d;
  } else {
    *reinterpret_cast<f32x2*>(coords + pix * 2) = f32x2{cu, cv};
  }
  if (JAC) {
    const float a0 = fxj * d, a2 = ((-fxj * X1[0]) * d) * d;
    const float b1 = fyj * d, b2 = ((-fyj * X1[1]) * d) * d;
    float r0[6], r1[6];  // Jj rows
    r0[0] = a0 * D;
    r0[1] = 0.0f;
    r0[2] = a2 * D;
    r0[3] = a2 * X1[1];
    r0[4] = a0 * X1[2] - a2 * X1[0];
    r0[5] = -(a0 * X1[1]);
    r1[0] = 0.0f;
    r1[1] = b1 * D;
    r1[2] = b2 * D;
    r1[3] = b2 * X1[1] - b1 * X1[2];
    r1[4] = -(b2 * X1[0]);
    r1[5] = b1 * X1[0];
    const float qc[4] = {-q[0], -q[1], -q[2], q[3]};
    float s0[6], s1[6];  // Ji rows
    float w[3], rt[3];
    act_so3(qc, r0, s0);
    cross3(r0, t, w);
    rt[0] = r0[3] + w[0]; rt[1] = r0[4] + w[1]; rt[2] = r0[5] + w[2];
    act_so3(qc, rt, s0 + 3);
    act_so3(qc, r1, s1);
    cross3(r1, t, w);
    rt[0] = r1[3] + w[0]; rt[1] = r1[4] + w[1]; rt[2] = r1[5] + w[2];
    act_so3(qc, rt, s1 + 3);
    f32x4* J4 = reinterpret_cast<f32x4*>(Jj + pix * 12);
    J4[0] = f32x4{r0[0], r0[1], r0[2], r0[3]};
    J4[1] = f32x4{r0[4], r0[5], r1[0], r1[1]};
    J4[2] = f32x4{r1[2], r1[3], r1[4], r1[5]};
    f32x4* I4 = reinterpret_cast<f32x4*>(Ji + pix * 12);
    I4[0] = f32x4{-s0[0], -s0[1], -s0[2], -s0[3]};
    I4[1] = f32x4{-s0[4], -s0[5], -s1[0], -s1[1]};
    I4[2] = f32x4{-s1[2], -s1[3], -s1[4], -s1[5]};
    *reinterpret_cast<f32x2*>(Jz + pix * 2) = f32x2{a0 * t[0] + a2 * t[2], b1 * t[1] + b2 * t[2]};
  }
  if (MOTN) {
    const f32x2 tg = *reinterpret_cast<const f32x2*>(target + pix * 2);
    float* M = motn + ((size_t)b * num + e) * 4 * HW + k;
    M[0] = clamp_nan(cu - u, -bound, bound);
    M[HW] = clamp_nan(cv - v, -bound, bound);
    M[2 * HW] = clamp_nan(tg.x - cu, -bound, bound);
    M[3 * HW] = clamp_nan(tg.y - cv, -bound, bound);
  }
}

}  // namespace lgu

namespace lgu {

inline bool rp_dims_ok(int B, int np, int nd, int ni, int ht, int wd, int num) {
  return B >= 0 && np >= 0 && nd >= 0 && ni >= 0 && num >= 0 && ht >= 0 && wd >= 0 &&
         (long long)ht * wd <= (long long)INT_MAX / 3;
}

inline bool aligned(const void* p, size_t n) { return ((uintptr_t)p & (n - 1)) == 0; }

template <bool JAC, bool DEPTH, bool MOTN>
void launch_reproject(const float* poses, const float* disps, const float* intrinsics, const long long* ii,
                      const long long* jj, const float* target, float* coords, float* valid, float* Ji, float* Jj, float* Jz,
                      float* motn, int B, int np, int nd, int ni, int ht, int wd, int num, float bound, void* stream) {
  int nv = np < nd ? np : nd;
  nv = nv < ni ? nv : ni;
  const int nb = (ht * wd + RP_THREADS - 1) / RP_THREADS;
  hipLaunchKernelGGL((reproject_kernel<JAC, DEPTH, MOTN>), dim3(num, nb, B), dim3(RP_THREADS), 0,
                     reinterpret_cast<hipStream_t>(stream), poses, disps, intrinsics, ii, jj, target, coords, valid, Ji, Jj,
                     Jz, motn, np, nd, ni, nv, num, ht, wd, bound);
}

// LGU_E_BADARG for bad sizes / null pointers, LGU_E_UNSUPPORTED for a grid the launch cannot take or misaligned vector
// outputs, LGU_OK with nothing launched for an empty edge set or frame; -1 = go on and launch.
inline int rp_precheck(int B, int np, int nd, int ni, int ht, int wd, int num) {
  if (!rp_dims_ok(B, np, nd, ni, ht, wd, num)) return LGU_E_BADARG;
  if (num == 0 || B == 0 || ht * wd == 0) return LGU_OK;
  if ((ht * wd + RP_THREADS - 1) / RP_THREADS > 65535 || B > 65535) return LGU_E_UNSUPPORTED;
  return -1;
}

}  // namespace lgu

extern "C" {

int lgu_projective_transform_f32(const float* poses, const float* disps, const float* intrinsics, const long long* ii,
                                 const long long* jj, int B, int np, int nd, int ni, int ht, int wd, int num, int flags,
                                 float* coords, float* valid, float* Ji, float* Jj, float* Jz, void* stream) {
  using namespace lgu;
  const int pre = rp_precheck(B, np, nd, ni, ht, wd, num);
  if (pre >= 0) return pre;
  const bool jac = (flags & LGU_REPROJ_JACOBIAN) != 0, depth = (flags & LGU_REPROJ_DEPTH) != 0;
  if ((flags & ~(LGU_REPROJ_JACOBIAN | LGU_REPROJ_DEPTH)) != 0) return LGU_E_BADARG;
  if (!poses || !disps || !intrinsics || !ii || !jj || !coords) return LGU_E_BADARG;
  if (jac && (!Ji || !Jj || !Jz)) return LGU_E_BADARG;
  if ((!depth && !aligned(coords, 8)) || (jac && (!aligned(Ji, 16) || !aligned(Jj, 16) || !aligned(Jz, 8))))
    return LGU_E_UNSUPPORTED;
  if (jac && depth)
    launch_reproject<true, true, false>(poses, disps, intrinsics, ii, jj, nullptr, coords, valid, Ji, Jj, Jz, nullptr, B,
                                        np, nd, ni, ht, wd, num, 0.0f, stream);
  else if (jac)
    launch_reproject<true, false, false>(poses, disps, intrinsics, ii, jj, nullptr, coords, valid, Ji, Jj, Jz, nullptr, B,
                                         np, nd, ni, ht, wd, num, 0.0f, stream);
  else if (depth)
    launch_reproject<false, true, false>(poses, disps, intrinsics, ii, jj, nullptr, coords, valid, nullptr, nullptr,
                                         nullptr, nullptr, B, np, nd, ni, ht, wd, num, 0.0f, stream);
  else
    launch_reproject<false, false, false>(poses, disps, intrinsics, ii, jj, nullptr, coords, valid, nullptr, nullptr,
                                          nullptr, nullptr, B, np, nd, ni, ht, wd, num, 0.0f, stream);
  return launch_status();
}

int lgu_motion_features_f32(const float* poses, const float* disps, const float* intrinsics, const long long* ii,
                            const long long* jj, const float* target, int B, int np, int nd, int ni, int ht, int wd, int num,
                            float bound, float* coords1, float* motn, float* valid, void* stream) {
  using namespace lgu;
  const int pre = rp_precheck(B, np, nd, ni, ht, wd, num);
  if (pre >= 0) return pre;
  if (!poses || !disps || !intrinsics || !ii || !jj || !target || !coords1 || !motn) return LGU_E_BADARG;
  if (!(bound >= 0.0f)) return LGU_E_BADARG;  // NaN or negative
  if (!aligned(coords1, 8) || !aligned(target, 8)) return LGU_E_UNSUPPORTED;
  launch_reproject<false, false, true>(poses, disps, intrinsics, ii, jj, target, coords1, valid, nullptr, nullptr, nullptr,
                                       motn, B, np, nd, ni, ht, wd, num, bound, stream);
  return launch_status();
}

}  // extern "C"
