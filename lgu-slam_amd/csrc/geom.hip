// geom.hip — the geometry entries of the reference's droid_backends (src/droid.cpp:237-249): frame_distance, projmap,
// depth_filter and iproj (src/droid_kernels.cu:427-851, launched from :1436-1541).
//
// Per-pixel arithmetic is the reference's, in its fp32 operation order (built with -ffp-contract=off; fp32 `/` and
// sqrtf are correctly rounded), so every per-pixel value is bit-identical to a float32 restatement of the reference
// (tests/geom_restatement.py).  Only frame_distance's three sums are ordered differently (fixed order, see below).
// The count of depth_filter and the point of iproj are defined in geom_pixel.hpp, which the map export (cloud.hip) shares.
//
// Index rule (the reference reads out of bounds instead): a frame index is valid when 0 <= index < nvalid =
// min(rows of poses, frames of disps).  No kernel dereferences an invalid index; it writes NaN (frame_distance), NaN
// coordinates with channel 2 = 0 and valid = 0 (projmap), a zero row (depth_filter: an invalid ix; an invalid
// neighbour is skipped like the reference's out-of-buffer ones), NaN points (iproj: a frame without a pose).
#include "lgu_common.hpp"
#include "geom_pixel.hpp"

namespace lgu {

constexpr float GEOM_MIN_DEPTH = 0.25f;  // droid_kernels.cu:26 (0.25 is exact in float: same comparisons)
constexpr int FD_MAX_WAVES = 16;
constexpr int FD_LANE_PIXELS = 8;        // target pixels per lane of frame_distance

__device__ __forceinline__ float readlane_f32(float v, int lane) {
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), lane));
}

// ---- frame_distance (:518-658) --------------------------------------------------------------------------------------
// One workgroup per pair, nw = blockDim.x / 64 waves.  Wave w owns the rows [w * rpw, (w + 1) * rpw), lane l the
// columns l, l + 64, ...; each lane sums its pixels column block by column block, row by row; the three wave sums
// (wave_sum_f32) are added in wave order by thread 0.  rpw and nw are functions of (ht, wd) only, so a pair's bits do
// not depend on the batch it is in.  x is computed once per column, y once per row (by lane r of the row block, read
// back with v_readlane): the same IEEE operations as the reference's per-pixel ones, two divisions fewer per pixel.
__global__ __launch_bounds__(FD_MAX_WAVES * kWave) void frame_distance_kernel(
    const float* __restrict__ poses, const float* __restrict__ disps, const float* __restrict__ intrinsics,
    const long long* __restrict__ ii, const long long* __restrict__ jj, float* __restrict__ dist, int nvalid, int ht,
    int wd, int rpw, float beta) {
  __shared__ float red[3 * FD_MAX_WAVES];
  const int p = blockIdx.x;
  const long long a = ii[p], b = jj[p];
  if (!valid_index(a, nvalid) || !valid_index(b, nvalid)) {  // uniform over the workgroup
    if (threadIdx.x == 0) dist[p] = __builtin_nanf("");
    return;
  }
  const int ix = (int)a, jx = (int)b;
  const float fx = intrinsics[0], fy = intrinsics[1], cx = intrinsics[2], cy = intrinsics[3];
  float tij[3], qij[4];
  rel_se3(poses + ix * 7, poses + ix * 7 + 3, poses + jx * 7, poses + jx * 7 + 3, tij, qij);
  const int lane = threadIdx.x & (kWave - 1), w = threadIdx.x / kWave, nw = blockDim.x / kWave;
  const int r0 = w * rpw, r1 = min(r0 + rpw, ht);
  const float* __restrict__ D = disps + (size_t)ix * ht * wd;
  const float wb = beta, wc = 1 - beta;
  float acc = 0.f, val = 0.f, tot = 0.f;
  for (int c0 = 0; c0 < wd; c0 += kWave) {
    const int j = c0 + lane;
    const bool col = j < wd;
    const float u = static_cast<float>(j);
    const float x = (u - cx) / fx;
    for (int rb = r0; rb < r1; rb += kWave) {
      const float vl = static_cast<float>(rb + lane);
      const float yl = (vl - cy) / fy;  // every lane: readlane below reads lanes whatever the branch
      const int nr = min(kWave, r1 - rb);
#pragma nounroll
      for (int r = 0; r < nr; r++) {
        const float v = readlane_f32(vl, r), y = readlane_f32(yl, r);
        if (col) {
          const float d = D[(size_t)(rb + r) * wd + j];
          // full transform: act_se3(T_ij, (x, y, 1, d))
          const float X[3] = {x, y, 1.0f};
          float Y[3];
          act_so3(qij, X, Y);
          Y[0] += d * tij[0];
          Y[1] += d * tij[1];
          Y[2] += d * tij[2];
          float du = fx * (Y[0] / Y[2]) + cx - u;
          float dv = fy * (Y[1] / Y[2]) + cy - v;
          float dd = sqrtf(du * du + dv * dv);
          tot += wb;
          if (Y[2] > GEOM_MIN_DEPTH) {
            acc += wb * dd;
            val += wb;
          }
          // translation only: X + d * t_ij
          const float Z0 = x + d * tij[0], Z1 = y + d * tij[1], Z2 = 1.0f + d * tij[2];
          du = fx * (Z0 / Z2) + cx - u;
          dv = fy * (Z1 / Z2) + cy - v;
          dd = sqrtf(du * du + dv * dv);
          tot += wc;
          if (Z2 > GEOM_MIN_DEPTH) {
            acc += wc * dd;
            val += wc;
          }
        }
      }
    }
  }
  acc = wave_sum_f32(acc);
  val = wave_sum_f32(val);
  tot = wave_sum_f32(tot);
  if (lane == 0) {
    red[w] = acc;
    red[FD_MAX_WAVES + w] = val;
    red[2 * FD_MAX_WAVES + w] = tot;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float A = red[0], V = red[FD_MAX_WAVES], T = red[2 * FD_MAX_WAVES];
    for (int k = 1; k < nw; k++) {
      A += red[k];
      V += red[FD_MAX_WAVES + k];
      T += red[2 * FD_MAX_WAVES + k];
    }
    // :655 — the 1e-8 literal makes the ratio a double
    dist[p] = ((double)V / ((double)T + 1e-8) < 0.75) ? 1000.0f : A / V;
  }
}

// Rows per wave of frame_distance: about FD_LANE_PIXELS pixels per lane, at most FD_MAX_WAVES waves.
inline void fd_layout(int ht, int wd, int* rpw, int* nw) {
  const int ncol = wd > 0 ? (wd + kWave - 1) / kWave : 1;
  int r = FD_LANE_PIXELS / ncol;
  if (r < 1) r = 1;
  int n = ht > 0 ? (ht + r - 1) / r : 1;
  if (n > FD_MAX_WAVES) {
    r = (ht + FD_MAX_WAVES - 1) / FD_MAX_WAVES;
    n = (ht + r - 1) / r;
  }
  *rpw = r;
  *nw = n;
}

// ---- projmap (:427-516) ---------------------------------------------------------------------------------------------
// grid (pair, pixel block); T_ij built once per workgroup.  Every output element is written (channel 2 = 0 included).
__global__ __launch_bounds__(GEOM_THREADS) void projmap_kernel(
    const float* __restrict__ poses, const float* __restrict__ disps, const float* __restrict__ intrinsics,
    const long long* __restrict__ ii, const long long* __restrict__ jj, float* __restrict__ coords,
    float* __restrict__ valid, int nvalid, int ht, int wd) {
  __shared__ float rel[7];
  const int bp = blockIdx.x;
  const int HW = ht * wd;
  const int k = blockIdx.y * GEOM_THREADS + threadIdx.x;
  const long long a = ii[bp], b = jj[bp];
  const bool ok = valid_index(a, nvalid) && valid_index(b, nvalid);  // uniform over the workgroup
  if (ok && threadIdx.x == 0) {
    const int ix = (int)a, jx = (int)b;
    rel_se3(poses + ix * 7, poses + ix * 7 + 3, poses + jx * 7, poses + jx * 7 + 3, rel, rel + 3);
  }
  __syncthreads();
  if (k >= HW) return;
  float* C = coords + ((size_t)bp * HW + k) * 3;
  float* V = valid + (size_t)bp * HW + k;
  if (!ok) {
    C[0] = __builtin_nanf("");
    C[1] = __builtin_nanf("");
    C[2] = 0.0f;
    *V = 0.0f;
    return;
  }
  const float tij[3] = {rel[0], rel[1], rel[2]}, qij[4] = {rel[3], rel[4], rel[5], rel[6]};
  const float fx = intrinsics[0], fy = intrinsics[1], cx = intrinsics[2], cy = intrinsics[3];
  const int i = k / wd, j = k - i * wd;
  const float u = static_cast<float>(j), v = static_cast<float>(i);
  const float d = disps[(size_t)a * HW + k];
  const float X[3] = {(u - cx) / fx, (v - cy) / fy, 1.0f};
  float Y[3];
  act_so3(qij, X, Y);
  Y[0] += d * tij[0];
  Y[1] += d * tij[1];
  Y[2] += d * tij[2];
  float cu = u, cv = v;
  if ((double)Y[2] > 0.01) {  // :507 compares against the double literal 0.01
    cu = fx * (Y[0] / Y[2]) + cx;
    cv = fy * (Y[1] / Y[2]) + cy;
  }
  C[0] = cu;
  C[1] = cv;
  C[2] = 0.0f;
  *V = (Y[2] > GEOM_MIN_DEPTH) ? 1.0f : 0.0f;
}

// ---- depth_filter (:661-776) ----------------------------------------------------------------------------------------
// grid (entry of ix, pixel block), one thread per pixel of frame ix[b] looping over the six neighbours
// ix-1, ix-2, ix-3, ix+3, ix+4, ix+5 (the reference's `neigh < 3 ? ix - neigh - 1 : ix + neigh`).  The six T_ij are built
// once per workgroup; the count stays in a register and is stored once (no atomics, no zero fill).  The disparity
// comparisons are in double, as in the reference; dj_hat / err (computed and unused there) are skipped.
__global__ __launch_bounds__(GEOM_THREADS) void depth_filter_kernel(
    const float* __restrict__ poses, const float* __restrict__ disps, const float* __restrict__ intrinsics,
    const long long* __restrict__ inds, const float* __restrict__ thresh, float* __restrict__ counter, int nvalid, int ht,
    int wd) {
  __shared__ float rel[6][7];  // t_ij[3], q_ij[4] per neighbour
  __shared__ int nbr[6];       // neighbour frame, -1 = skipped
  const int b = blockIdx.x;
  const int HW = ht * wd;
  const int k = blockIdx.y * GEOM_THREADS + threadIdx.x;
  const long long a = inds[b];
  if (!valid_index(a, nvalid)) {  // uniform over the workgroup
    if (k < HW) counter[(size_t)b * HW + k] = 0.0f;
    return;
  }
  const int ix = (int)a;
  if (threadIdx.x < DF_NEIGHBOURS) depth_filter_neighbour(poses, a, threadIdx.x, nvalid, rel[threadIdx.x], &nbr[threadIdx.x]);
  __syncthreads();
  if (k >= HW) return;
  const float fx = intrinsics[0], fy = intrinsics[1], cx = intrinsics[2], cy = intrinsics[3];
  const int i = k / wd, j = k - i * wd;
  const int cnt = depth_filter_count(disps, fx, fy, cx, cy, (double)thresh[b], rel, nbr, disps[(size_t)ix * HW + k], i, j, ht, wd);
  counter[(size_t)b * HW + k] = (float)cnt;
}

// ---- iproj (:779-851) -----------------------------------------------------------------------------------------------
// grid (frame, pixel block): points = act_se3(T_n, (x, y, 1, d))[0:3] / d.
__global__ __launch_bounds__(GEOM_THREADS) void iproj_kernel(
    const float* __restrict__ poses, const float* __restrict__ disps, const float* __restrict__ intrinsics,
    float* __restrict__ points, int np, int ht, int wd) {
  const int n = blockIdx.x;
  const int HW = ht * wd;
  const int k = blockIdx.y * GEOM_THREADS + threadIdx.x;
  if (k >= HW) return;
  float* P = points + ((size_t)n * HW + k) * 3;
  if (n >= np) {  // no pose for this frame
    P[0] = P[1] = P[2] = __builtin_nanf("");
    return;
  }
  const float fx = intrinsics[0], fy = intrinsics[1], cx = intrinsics[2], cy = intrinsics[3];
  const int i = k / wd, j = k - i * wd;
  float Q[3];
  iproj_point(poses + (size_t)n * 7, fx, fy, cx, cy, disps[(size_t)n * HW + k], i, j, Q);
  P[0] = Q[0];
  P[1] = Q[1];
  P[2] = Q[2];
}

}  // namespace lgu

extern "C" {

int lgu_frame_distance_f32(const float* poses, int np, const float* disps, int nd, int ht, int wd, const float* intrinsics,
                           const long long* ii, const long long* jj, int num, float beta, float* dist, void* stream) {
  using namespace lgu;
  if (num < 0 || !geom_dims_ok(np, nd, ht, wd)) return LGU_E_BADARG;
  if (num == 0) return LGU_OK;
  if (!poses || !disps || !intrinsics || !ii || !jj || !dist) return LGU_E_BADARG;
  int rpw, nw;
  fd_layout(ht, wd, &rpw, &nw);
  hipLaunchKernelGGL(frame_distance_kernel, dim3(num), dim3(nw * kWave), 0, reinterpret_cast<hipStream_t>(stream), poses,
                     disps, intrinsics, ii, jj, dist, np < nd ? np : nd, ht, wd, rpw, beta);
  return launch_status();
}

int lgu_projmap_f32(const float* poses, int np, const float* disps, int nd, int ht, int wd, const float* intrinsics,
                    const long long* ii, const long long* jj, int num, float* coords, float* valid, void* stream) {
  using namespace lgu;
  if (num < 0 || !geom_dims_ok(np, nd, ht, wd)) return LGU_E_BADARG;
  if (num == 0 || ht * wd == 0) return LGU_OK;
  if (!poses || !disps || !intrinsics || !ii || !jj || !coords || !valid) return LGU_E_BADARG;
  const int nb = pixel_blocks(ht, wd);
  if (nb > 65535) return LGU_E_UNSUPPORTED;
  hipLaunchKernelGGL(projmap_kernel, dim3(num, nb), dim3(GEOM_THREADS), 0, reinterpret_cast<hipStream_t>(stream), poses, disps,
                     intrinsics, ii, jj, coords, valid, np < nd ? np : nd, ht, wd);
  return launch_status();
}

int lgu_depth_filter_f32(const float* poses, int np, const float* disps, int nd, int ht, int wd, const float* intrinsics,
                         const long long* ix, const float* thresh, int num, float* counter, void* stream) {
  using namespace lgu;
  if (num < 0 || !geom_dims_ok(np, nd, ht, wd)) return LGU_E_BADARG;
  if (num == 0 || ht * wd == 0) return LGU_OK;
  if (!poses || !disps || !intrinsics || !ix || !thresh || !counter) return LGU_E_BADARG;
  const int nb = pixel_blocks(ht, wd);
  if (nb > 65535) return LGU_E_UNSUPPORTED;
  hipLaunchKernelGGL(depth_filter_kernel, dim3(num, nb), dim3(GEOM_THREADS), 0, reinterpret_cast<hipStream_t>(stream), poses,
                     disps, intrinsics, ix, thresh, counter, np < nd ? np : nd, ht, wd);
  return launch_status();
}

int lgu_iproj_f32(const float* poses, int np, const float* disps, int nd, int ht, int wd, const float* intrinsics,
                  float* points, void* stream) {
  using namespace lgu;
  if (!geom_dims_ok(np, nd, ht, wd)) return LGU_E_BADARG;
  if (nd == 0 || ht * wd == 0) return LGU_OK;
  if (!poses && np > 0) return LGU_E_BADARG;
  if (!disps || !intrinsics || !points) return LGU_E_BADARG;
  const int nb = pixel_blocks(ht, wd);
  if (nb > 65535) return LGU_E_UNSUPPORTED;
  hipLaunchKernelGGL(iproj_kernel, dim3(nd, nb), dim3(GEOM_THREADS), 0, reinterpret_cast<hipStream_t>(stream), poses, disps,
                     intrinsics, points, np, ht, wd);
  return launch_status();
}

}  // extern "C"
