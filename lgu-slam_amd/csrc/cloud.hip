// cloud.hip — the map export: the filtered, coloured point cloud of a set of keyframes, compacted on the device.  What the
// reference's visualiser callback (droid_slam/visualization.py:92-129) does with iproj, depth_filter, a per-frame mean,
// four copies to the host and a boolean index per frame, in three launches whose only output is the surviving points.
//
// For entry b of ix and pixel k (row-major) of frame ix[b]:
//   count = depth_filter's count (geom_pixel.hpp: the definition depth_filter_kernel uses), 0 for an invalid ix[b]
//   keep  = count >= min_count && disps[ix[b]][k] > floor[b]        (float comparison: a NaN disparity is dropped)
//   point = iproj's point (geom_pixel.hpp: the definition iproj_kernel uses) under the inverse of poses[ix[b]]
//   colour[c] = float(images[ix[b]][2 - c][phase + stride i][phase + stride j]) * (float)(1.0 / 255.0), or the byte itself
// Kept pixels are written densely in (b, k) order; entry b owns the rows offsets[b] : offsets[b + 1].
//
//   cloud_decide_kernel  grid (num, pixel blocks of GEOM_THREADS): count and keep per pixel, the 64-lane ballot of keep per
//                        wave into scratch, the kept count of the workgroup into scratch
//   cloud_scan_kernel    one workgroup: the exclusive prefix over the num * blocks counts (int64), offsets (num + 1)
//   cloud_write_kernel   grid as the first: re-reads its ballot words, rank of a kept lane = the workgroup's prefix + the
//                        kept lanes of the earlier waves + the kept lower lanes of its own; point and colour are computed
//                        and stored for kept lanes with rank < cap only
// No workgroup waits on another and no position comes from an atomic: the order is that of the launches and the result is
// the same bits on every run.  Every word of scratch that a later launch reads is written by an earlier one.
#include "lgu_common.hpp"
#include "geom_pixel.hpp"

namespace lgu {

constexpr int CLOUD_WAVES = GEOM_THREADS / kWave;
constexpr int SCAN_THREADS = 1024;
constexpr float IMG_INV255 = (float)(1.0 / 255.0);   // lgu_image_normalize_u8's constant (instnorm.hip)

// scratch: ballot words (units * CLOUD_WAVES, u64), exclusive prefix per workgroup (units, i64), kept per workgroup (units,
// i32); units = num * pixel blocks
struct CloudScratch {
  unsigned long long* ballots;
  long long* prefix;
  int* counts;
};

inline long long cloud_scratch_bytes(long long units) { return units * (CLOUD_WAVES * 8 + 8) + ((units * 4 + 7) & ~7LL); }

inline CloudScratch cloud_scratch(void* scratch, long long units) {
  char* p = static_cast<char*>(scratch);
  return {reinterpret_cast<unsigned long long*>(p), reinterpret_cast<long long*>(p + units * CLOUD_WAVES * 8),
          reinterpret_cast<int*>(p + units * (CLOUD_WAVES * 8 + 8))};
}

__global__ __launch_bounds__(GEOM_THREADS) void cloud_decide_kernel(
    const float* __restrict__ poses, const float* __restrict__ disps, const float* __restrict__ intrinsics,
    const long long* __restrict__ inds, const float* __restrict__ thresh, const float* __restrict__ dfloor,
    unsigned long long* __restrict__ ballots, int* __restrict__ counts, int nvalid, int ht, int wd, int min_count) {
  __shared__ float rel[DF_NEIGHBOURS][7];  // t_ij[3], q_ij[4] per neighbour
  __shared__ int nbr[DF_NEIGHBOURS];       // neighbour frame, -1 = skipped
  __shared__ int kept[CLOUD_WAVES];
  const int b = blockIdx.x;
  const int HW = ht * wd;
  const int k = blockIdx.y * GEOM_THREADS + threadIdx.x;
  const int lane = threadIdx.x & (kWave - 1), w = threadIdx.x / kWave;
  const size_t unit = (size_t)b * gridDim.y + blockIdx.y;
  const long long a = inds[b];
  const bool ok = valid_index(a, nvalid);  // uniform over the workgroup
  if (ok && threadIdx.x < DF_NEIGHBOURS)
    depth_filter_neighbour(poses, a, threadIdx.x, nvalid, rel[threadIdx.x], &nbr[threadIdx.x]);
  __syncthreads();
  bool keep = false;
  if (ok && k < HW) {
    const float fx = intrinsics[0], fy = intrinsics[1], cx = intrinsics[2], cy = intrinsics[3];
    const int i = k / wd, j = k - i * wd;
    const float di = disps[(size_t)a * HW + k];
    const int cnt = depth_filter_count(disps, fx, fy, cx, cy, (double)thresh[b], rel, nbr, di, i, j, ht, wd);
    keep = cnt >= min_count && di > dfloor[b];
  }
  const unsigned long long word = __ballot(keep);
  if (lane == 0) {
    ballots[unit * CLOUD_WAVES + w] = word;
    kept[w] = __popcll(word);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int n = 0;
    for (int v = 0; v < CLOUD_WAVES; v++) n += kept[v];
    counts[unit] = n;
  }
}

// Exclusive prefix of counts[0 : units) into prefix, offsets[b] = prefix[b * nb], offsets[num] = the total.  Thread t owns
// the contiguous items [t * per, (t + 1) * per); the SCAN_THREADS chunk sums are scanned in LDS (Hillis-Steele).
__global__ __launch_bounds__(SCAN_THREADS) void cloud_scan_kernel(const int* __restrict__ counts, long long* __restrict__ prefix,
                                                                  long long* __restrict__ offsets, long long units, int nb,
                                                                  int num) {
  __shared__ long long part[SCAN_THREADS];
  const int t = threadIdx.x;
  const long long per = (units + SCAN_THREADS - 1) / SCAN_THREADS;
  const long long lo = t * per < units ? t * per : units;
  const long long hi = lo + per < units ? lo + per : units;
  long long s = 0;
  for (long long u = lo; u < hi; u++) s += counts[u];
  part[t] = s;
  __syncthreads();
  for (int d = 1; d < SCAN_THREADS; d <<= 1) {
    const long long add = t >= d ? part[t - d] : 0;
    __syncthreads();
    part[t] += add;
    __syncthreads();
  }
  long long run = part[t] - s;  // exclusive
  for (long long u = lo; u < hi; u++) {
    prefix[u] = run;
    if (u % nb == 0) offsets[u / nb] = run;
    run += counts[u];
  }
  if (t == SCAN_THREADS - 1) offsets[num] = part[t];
}

// The inverse of the pose (t, q) with the bits of geom.se3_inverse (torch operators): conjugate, uv = 2 (v x t), w = v x uv,
// -((t + q.w uv) + w).  Every product and sum is a torch operator of its own and rounds on its own (__fmul_rn / __fadd_rn
// never contract), except inside torch's cross product, whose a1 b2 - a2 b1 is evaluated on the device (and on the host) as
// fma(a1, b2, -(a2 b1)): the second product rounded, the first exact inside the fused multiply-add.  That is written out
// here, so the flags of this build decide nothing about it.
__device__ __forceinline__ void cross3_rn(const float* a, const float* b, float* c) {
  c[0] = __fmaf_rn(a[1], b[2], -__fmul_rn(a[2], b[1]));
  c[1] = __fmaf_rn(a[2], b[0], -__fmul_rn(a[0], b[2]));
  c[2] = __fmaf_rn(a[0], b[1], -__fmul_rn(a[1], b[0]));
}
__device__ __forceinline__ void se3_inverse_rn(const float* pose, float* inv) {
  const float t[3] = {pose[0], pose[1], pose[2]};
  const float v[3] = {-pose[3], -pose[4], -pose[5]};
  const float qw = pose[6];
  float uv[3], w[3];
  cross3_rn(v, t, uv);
  for (int c = 0; c < 3; c++) uv[c] = __fmul_rn(2.0f, uv[c]);
  cross3_rn(v, uv, w);
  for (int c = 0; c < 3; c++) inv[c] = -__fadd_rn(__fadd_rn(t[c], __fmul_rn(qw, uv[c])), w[c]);
  inv[3] = v[0];
  inv[4] = v[1];
  inv[5] = v[2];
  inv[6] = qw;
}

template <bool U8>
__global__ __launch_bounds__(GEOM_THREADS) void cloud_write_kernel(
    const float* __restrict__ poses, const float* __restrict__ disps, const float* __restrict__ intrinsics,
    const long long* __restrict__ inds, const unsigned char* __restrict__ images, const unsigned long long* __restrict__ ballots,
    const long long* __restrict__ prefix, float* __restrict__ points, void* __restrict__ colors, long long cap, int nvalid,
    int ht, int wd, int H, int W, int stride, int phase) {
  __shared__ float inv[7];
  const int b = blockIdx.x;
  const size_t unit = (size_t)b * gridDim.y + blockIdx.y;
  const int lane = threadIdx.x & (kWave - 1), w = threadIdx.x / kWave;
  const unsigned long long* words = ballots + unit * CLOUD_WAVES;
  unsigned long long any = 0;
  for (int v = 0; v < CLOUD_WAVES; v++) any |= words[v];
  const long long base = prefix[unit];
  if (any == 0 || base >= cap) return;  // uniform: nothing kept here, or every row of this workgroup is past the capacity
  const long long a = inds[b];
  if (!valid_index(a, nvalid)) return;  // the decision pass keeps nothing of an invalid entry
  if (threadIdx.x == 0) se3_inverse_rn(poses + (size_t)a * 7, inv);
  __syncthreads();
  const unsigned long long mine = words[w];
  if (!((mine >> lane) & 1ull)) return;
  long long row = base + __popcll(mine & ((1ull << lane) - 1ull));
  for (int v = 0; v < w; v++) row += __popcll(words[v]);
  if (row >= cap) return;
  const int HW = ht * wd;
  const int k = blockIdx.y * GEOM_THREADS + threadIdx.x;
  if (k >= HW) return;  // the decision pass keeps no lane beyond the frame; a foreign scratch must not index past it
  const float fx = intrinsics[0], fy = intrinsics[1], cx = intrinsics[2], cy = intrinsics[3];
  const int i = k / wd, j = k - i * wd;
  const float T[7] = {inv[0], inv[1], inv[2], inv[3], inv[4], inv[5], inv[6]};
  float Q[3];
  iproj_point(T, fx, fy, cx, cy, disps[(size_t)a * HW + k], i, j, Q);
  float* P = points + row * 3;
  P[0] = Q[0];
  P[1] = Q[1];
  P[2] = Q[2];
  if (images) {
    const size_t plane = (size_t)H * W;
    const unsigned char* src = images + (size_t)a * 3 * plane + (size_t)(phase + stride * i) * W + (phase + stride * j);
    const unsigned char r = src[2 * plane], g = src[plane], bl = src[0];  // BGR planes -> RGB
    if (U8) {
      unsigned char* C = static_cast<unsigned char*>(colors) + row * 3;
      C[0] = r;
      C[1] = g;
      C[2] = bl;
    } else {
      float* C = static_cast<float*>(colors) + row * 3;
      C[0] = (float)r * IMG_INV255;
      C[1] = (float)g * IMG_INV255;
      C[2] = (float)bl * IMG_INV255;
    }
  }
}

inline bool cloud_sizes_ok(const lgu_cloud_args& a) { return a.num >= 0 && geom_dims_ok(a.np, a.nd, a.ht, a.wd); }

}  // namespace lgu

extern "C" {

long long lgu_cloud_scratch_bytes(int num, int ht, int wd) {
  using namespace lgu;
  if (num <= 0 || !geom_dims_ok(0, 0, ht, wd) || ht * wd == 0) return 0;
  return cloud_scratch_bytes((long long)num * pixel_blocks(ht, wd));
}

int lgu_cloud_decide_f32(lgu_cloud_args a, void* stream) {
  using namespace lgu;
  if (!cloud_sizes_ok(a)) return LGU_E_BADARG;
  if (a.num == 0 || a.ht * a.wd == 0) return LGU_OK;
  if (!a.poses || !a.disps || !a.intrinsics || !a.ix || !a.thresh || !a.floor || !a.scratch || !a.offsets) return LGU_E_BADARG;
  if ((reinterpret_cast<uintptr_t>(a.scratch) & 7) != 0 || (reinterpret_cast<uintptr_t>(a.offsets) & 7) != 0) return LGU_E_BADARG;
  const int nb = pixel_blocks(a.ht, a.wd);
  if (nb > 65535) return LGU_E_UNSUPPORTED;
  const long long units = (long long)a.num * nb;
  const CloudScratch s = cloud_scratch(a.scratch, units);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(cloud_decide_kernel, dim3(a.num, nb), dim3(GEOM_THREADS), 0, st, a.poses, a.disps, a.intrinsics, a.ix, a.thresh,
                     a.floor, s.ballots, s.counts, a.np < a.nd ? a.np : a.nd, a.ht, a.wd, a.min_count);
  int rc = launch_status();
  if (rc) return rc;
  hipLaunchKernelGGL(cloud_scan_kernel, dim3(1), dim3(SCAN_THREADS), 0, st, s.counts, s.prefix, a.offsets, units, nb, a.num);
  return launch_status();
}

int lgu_cloud_write_f32(lgu_cloud_args a, void* stream) {
  using namespace lgu;
  if (!cloud_sizes_ok(a) || a.cap < 0) return LGU_E_BADARG;
  if (a.num == 0 || a.ht * a.wd == 0 || a.cap == 0) return LGU_OK;
  if (!a.poses || !a.disps || !a.intrinsics || !a.ix || !a.scratch || !a.points) return LGU_E_BADARG;
  if ((reinterpret_cast<uintptr_t>(a.scratch) & 7) != 0) return LGU_E_BADARG;
  const int nvalid = a.np < a.nd ? a.np : a.nd;
  if (a.images) {  // every valid frame has an image, every pixel a sample inside it
    if (!a.colors || a.ni < nvalid || a.H < 1 || a.W < 1 || a.stride < 1 || a.phase < 0) return LGU_E_BADARG;
    if ((long long)a.phase + (long long)a.stride * (a.ht - 1) >= a.H || (long long)a.phase + (long long)a.stride * (a.wd - 1) >= a.W)
      return LGU_E_BADARG;
  }
  const int nb = pixel_blocks(a.ht, a.wd);
  if (nb > 65535) return LGU_E_UNSUPPORTED;
  const CloudScratch s = cloud_scratch(a.scratch, (long long)a.num * nb);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  auto kern = a.color_u8 ? cloud_write_kernel<true> : cloud_write_kernel<false>;
  hipLaunchKernelGGL(kern, dim3(a.num, nb), dim3(GEOM_THREADS), 0, st, a.poses, a.disps, a.intrinsics, a.ix,
                     static_cast<const unsigned char*>(a.images), s.ballots, s.prefix, a.points, a.colors, a.cap, nvalid, a.ht, a.wd,
                     a.H, a.W, a.stride, a.phase);
  return launch_status();
}

}  // extern "C"
