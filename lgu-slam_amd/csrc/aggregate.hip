// aggregate.hip — the two streaming operators around GraphAgg (reference droid_slam/droid_net.py:14-37, :53-69):
// torch_scatter's scatter_mean over one dimension with a 1-D index, and the convex 8x upsampling of the disparity
// (cvx_upsample with data width 1, used by DepthVideo.upsample, depth_video.py:124-128).
//
// Segment mean: out[o,m,i] = round_out(S / c), S = sum of float(src[o,j,i]) over the j with index[j] == m, added in
// fp32 in ascending j (one rounding per add), c = the number of those j as fp32, `/` correctly rounded; round_out is
// the identity for fp32 and round-to-nearest-even for fp16.  An empty segment gives 0.  Index rule: an index outside
// [0, M) matches no segment: it is never used as an address and never counted.  No atomics: each workgroup owns one
// (o, m, slice of i) and builds its segment's list of j in LDS from the index vector, tile by tile, in ascending j.
// The bits do not depend on the launch geometry.
//
// Convex upsampling: mask channel c = k*64 + a*8 + b, k = ky*3 + kx indexes the neighbour (y+ky-1, x+kx-1) of the
// coarse pixel (zero outside the frame, F.unfold(padding=1)); (a, b) is the sub-pixel, the output pixel is (8y+a, 8x+b)
// (the reference's view (B,1,9,8,8,ht,wd) and permute(0,4,2,5,3,1)).  Per output, in this order:
//   1. m = max_k x_k              (ascending k)
//   2. e_k = expf(x_k - m)
//   3. s = sum_k e_k              (ascending k)
//   4. w_k = e_k / s
//   5. HALF_WEIGHTS: w_k = float(half(w_k)), round to nearest even (torch.softmax of a half mask returns half)
//   6. out = sum_k w_k * d_k      (each product rounded to fp32, summed in ascending k)
// Built with -ffp-contract=off, so no product is fused into an add.
#include <limits.h>

#include "lgu_common.hpp"

namespace lgu {

constexpr int AG_THREADS = 256;
constexpr int AG_WAVES = AG_THREADS / kWave;
constexpr int SM_MAX_N = 65536, SM_MAX_M = 65536;
#ifndef LGU_CVX_XV
#define LGU_CVX_XV 1  // coarse pixels per upsampling thread when wd allows it; 1 measured fastest (A/B: -DLGU_CVX_XV=2 / 4)
#endif
constexpr int CVX_XV = LGU_CVX_XV;
constexpr int SM_UNROLL = 4;  // segment rows loaded before they are added (8 and 16 measured no faster)


// 16 bytes of T: four floats or eight halves.
template <typename T> struct Vec16;
template <> struct Vec16<float> { typedef f32x4 type; static constexpr int n = 4; };
template <> struct Vec16<_Float16> { typedef f16x8 type; static constexpr int n = 8; };

// One workgroup per (o, m, slice of AG_THREADS * V elements of inner); V = 16 bytes of T (VEC, inner % V == 0 and
// 16-byte aligned operands) or 1.  Per tile of AG_THREADS indices the segment's j are compacted into LDS in ascending
// order (wave ballots, then the waves in order); every thread then adds those rows of its slice, SM_UNROLL loads in
// flight.
template <typename T, bool VEC>
__global__ __launch_bounds__(AG_THREADS) void segment_mean_kernel(const T* __restrict__ src,
                                                                  const long long* __restrict__ index,
                                                                  T* __restrict__ out, int n, int M, long long inner,
                                                                  long long chunks) {
  constexpr int V = VEC ? Vec16<T>::n : 1;
  typedef typename Vec16<T>::type VT;
  __shared__ int seg[AG_THREADS];
  __shared__ int wcount[AG_WAVES];
  const long long bx = blockIdx.x;
  const int m = (int)(bx / chunks);
  const long long chunk = bx - (long long)m * chunks;
  const int o = blockIdx.y;
  const long long i0 = (chunk * AG_THREADS + threadIdx.x) * V;
  const bool active = i0 < inner;  // VEC: inner % V == 0, so the whole vector is in range
  const T* base = src + (size_t)o * n * inner + i0;
  const int lane = threadIdx.x & (kWave - 1), w = threadIdx.x / kWave;
  float acc[V];
#pragma unroll
  for (int v = 0; v < V; v++) acc[v] = 0.0f;
  int cnt = 0;
  for (int t0 = 0; t0 < n; t0 += AG_THREADS) {
    const int j = t0 + threadIdx.x;
    const bool hit = j < n && index[j] == (long long)m;
    const unsigned long long bal = __ballot(hit);
    if (lane == 0) wcount[w] = __popcll(bal);
    __syncthreads();
    int off = 0, tot = 0;
#pragma unroll
    for (int q = 0; q < AG_WAVES; q++) {
      off += q < w ? wcount[q] : 0;
      tot += wcount[q];
    }
    if (hit) seg[off + __popcll(bal & ((1ull << lane) - 1ull))] = j;
    __syncthreads();
    if (active) {
      int s = 0;
      if (VEC) {
        for (; s + SM_UNROLL <= tot; s += SM_UNROLL) {
          VT r[SM_UNROLL];
#pragma unroll
          for (int q = 0; q < SM_UNROLL; q++) r[q] = *reinterpret_cast<const VT*>(base + (size_t)seg[s + q] * inner);
#pragma unroll
          for (int q = 0; q < SM_UNROLL; q++)
#pragma unroll
            for (int v = 0; v < V; v++) acc[v] = acc[v] + (float)r[q][v];
        }
        for (; s < tot; s++) {
          const VT r = *reinterpret_cast<const VT*>(base + (size_t)seg[s] * inner);
#pragma unroll
          for (int v = 0; v < V; v++) acc[v] = acc[v] + (float)r[v];
        }
      } else {
        for (; s + 4 <= tot; s += 4) {
          T r[4];
#pragma unroll
          for (int q = 0; q < 4; q++) r[q] = base[(size_t)seg[s + q] * inner];
#pragma unroll
          for (int q = 0; q < 4; q++) acc[0] = acc[0] + (float)r[q];
        }
        for (; s < tot; s++) acc[0] = acc[0] + (float)base[(size_t)seg[s] * inner];
      }
    }
    cnt += tot;
    __syncthreads();  // seg and wcount are rewritten by the next tile
  }
  if (!active) return;
  const float c = (float)cnt;
  T* dst = out + ((size_t)o * M + m) * inner + i0;
  if (VEC) {
    VT r;
#pragma unroll
    for (int v = 0; v < V; v++) r[v] = (T)(cnt ? acc[v] / c : 0.0f);
    *reinterpret_cast<VT*>(dst) = r;
  } else {
    dst[0] = (T)(cnt ? acc[0] / c : 0.0f);
  }
}

// Mask vector of XV consecutive coarse pixels of one channel.
template <typename MT, int XV> struct MaskVec { typedef MT __attribute__((ext_vector_type(XV))) type; };
template <typename MT> struct MaskVec<MT, 1> { typedef MT type; };

template <typename MT, int XV>
__device__ __forceinline__ float mask_at(const typename MaskVec<MT, XV>::type& v, int p) {
  if constexpr (XV == 1) return (float)v;
  else return (float)v[p];
}

// One thread per (frame u, coarse row y, sub-row a, group of XV coarse pixels x0..x0+XV-1): for each sub-column b it
// reads the 9 mask channels k*64 + a*8 + b of its pixels (lanes over x: coalesced channel-planar reads) and writes the
// 8*XV floats of fine row 8y+a starting at column 8*x0 (consecutive lanes write consecutive 8*XV-float runs).  ix
// (the indexed in-place form): frame u reads data row ix[u] and writes out row ix[u]; an ix[u] outside [0, N) writes
// nothing.  Without ix, row u.
template <typename MT, bool HALFW, int XV>
__global__ __launch_bounds__(AG_THREADS) void cvx_upsample_kernel(const float* __restrict__ data,
                                                                  const MT* __restrict__ mask,
                                                                  const long long* __restrict__ ix,
                                                                  float* __restrict__ out, int N, int ht, int wd,
                                                                  int nxg, long long total) {
  typedef typename MaskVec<MT, XV>::type MV;
  const long long t = (long long)blockIdx.x * AG_THREADS + threadIdx.x;
  if (t >= total) return;
  const int xg = (int)(t % nxg);
  long long r = t / nxg;
  const int a = (int)(r & 7);
  r >>= 3;
  const int y = (int)(r % ht);
  const long long u = r / ht;
  long long row = u;
  if (ix) {
    row = ix[u];
    if (row < 0 || row >= N) return;
  }
  const size_t HW = (size_t)ht * wd;
  const int x0 = xg * XV;
  const float* d = data + (size_t)row * HW;
  float nb[3][XV + 2];  // d at rows y-1..y+1, columns x0-1..x0+XV, 0 outside the frame
#pragma unroll
  for (int ky = 0; ky < 3; ky++) {
    const int yy = y + ky - 1;
#pragma unroll
    for (int q = 0; q < XV + 2; q++) {
      const int xx = x0 + q - 1;
      nb[ky][q] = (yy >= 0 && yy < ht && xx >= 0 && xx < wd) ? d[(size_t)yy * wd + xx] : 0.0f;
    }
  }
  const MT* mk = mask + (size_t)u * 576 * HW + (size_t)y * wd + x0;
  float res[8][XV];
#pragma unroll
  for (int b = 0; b < 8; b++) {
    MV mv[9];
#pragma unroll
    for (int k = 0; k < 9; k++) mv[k] = *reinterpret_cast<const MV*>(mk + (size_t)(k * 64 + a * 8 + b) * HW);
#pragma unroll
    for (int p = 0; p < XV; p++) {
      float x[9];
#pragma unroll
      for (int k = 0; k < 9; k++) x[k] = mask_at<MT, XV>(mv[k], p);
      float mx = x[0];
#pragma unroll
      for (int k = 1; k < 9; k++) mx = x[k] > mx ? x[k] : mx;
      float e[9];
      float s = 0.0f;
#pragma unroll
      for (int k = 0; k < 9; k++) {
        e[k] = expf(x[k] - mx);
        s = s + e[k];
      }
      float acc = 0.0f;
#pragma unroll
      for (int k = 0; k < 9; k++) {
        float wk = e[k] / s;
        if (HALFW) wk = (float)(_Float16)wk;
        const float prod = wk * nb[k / 3][p + k % 3];
        acc = k == 0 ? prod : acc + prod;
      }
      res[b][p] = acc;
    }
  }
  float* o = out + (size_t)row * 64 * HW + (size_t)(8 * y + a) * 8 * wd + 8 * x0;
#pragma unroll
  for (int p = 0; p < XV; p++) {
    f32x4* o4 = reinterpret_cast<f32x4*>(o + 8 * p);
    o4[0] = f32x4{res[0][p], res[1][p], res[2][p], res[3][p]};
    o4[1] = f32x4{res[4][p], res[5][p], res[6][p], res[7][p]};
  }
}

inline bool ag_aligned(const void* p, size_t n) { return ((uintptr_t)p & (n - 1)) == 0; }

template <typename T>
int launch_segment_mean(const T* src, const long long* index, int outer, int n, long long inner, int M, T* out,
                        void* stream) {
  if (outer < 0 || n < 0 || inner < 0 || M < 0) return LGU_E_BADARG;
  if ((long long)outer * M * inner == 0) return LGU_OK;  // nothing to write
  if (!src && n > 0) return LGU_E_BADARG;
  if (!out || (n > 0 && !index)) return LGU_E_BADARG;
  if (n > SM_MAX_N || M > SM_MAX_M || outer > 65535) return LGU_E_UNSUPPORTED;
  constexpr int V = Vec16<T>::n;
  const bool vec = inner % V == 0 && ag_aligned(src, 16) && ag_aligned(out, 16);
  const long long per = vec ? (long long)AG_THREADS * V : AG_THREADS;
  const long long chunks = (inner + per - 1) / per;
  if (chunks * M > (long long)(UINT_MAX / AG_THREADS)) return LGU_E_UNSUPPORTED;
  const dim3 grid((unsigned)(chunks * M), (unsigned)outer);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (vec)
    hipLaunchKernelGGL((segment_mean_kernel<T, true>), grid, dim3(AG_THREADS), 0, s, src, index, out, n, M, inner, chunks);
  else
    hipLaunchKernelGGL((segment_mean_kernel<T, false>), grid, dim3(AG_THREADS), 0, s, src, index, out, n, M, inner, chunks);
  return launch_status();
}

template <typename MT, bool HALFW>
void launch_cvx(const float* data, const MT* mask, const long long* ix, float* out, int N, int U, int ht, int wd,
                bool vec, hipStream_t s) {
  const int xv = vec ? CVX_XV : 1;
  const int nxg = (wd + xv - 1) / xv;
  const long long total = (long long)U * ht * 8 * nxg;
  const unsigned nb = (unsigned)((total + AG_THREADS - 1) / AG_THREADS);
  if (vec)
    hipLaunchKernelGGL((cvx_upsample_kernel<MT, HALFW, CVX_XV>), dim3(nb), dim3(AG_THREADS), 0, s, data, mask, ix, out, N, ht,
                       wd, nxg, total);
  else
    hipLaunchKernelGGL((cvx_upsample_kernel<MT, HALFW, 1>), dim3(nb), dim3(AG_THREADS), 0, s, data, mask, ix, out, N, ht,
                       wd, nxg, total);
}

// Shared by both upsampling entries: U frames of mask, N data / out rows (N = U without ix).
int cvx_entry(const float* data, int N, int ht, int wd, const long long* ix, int U, const void* mask, int flags, float* out,
              void* stream) {
  if (N < 0 || U < 0 || ht < 0 || wd < 0) return LGU_E_BADARG;
  if ((flags & ~(LGU_UPS_MASK_F16 | LGU_UPS_HALF_WEIGHTS)) != 0) return LGU_E_BADARG;
  const bool f16 = (flags & LGU_UPS_MASK_F16) != 0, halfw = (flags & LGU_UPS_HALF_WEIGHTS) != 0;
  if (halfw && !f16) return LGU_E_BADARG;
  if ((long long)ht * wd > (long long)INT_MAX / 576) return LGU_E_BADARG;
  if ((long long)U * ht * wd == 0 || N == 0) return LGU_OK;  // nothing to write
  if (!data || !mask || !out) return LGU_E_BADARG;
  const long long total1 = (long long)U * ht * 8 * wd;
  if ((total1 + AG_THREADS - 1) / AG_THREADS > (long long)(UINT_MAX / AG_THREADS)) return LGU_E_UNSUPPORTED;
  if (!ag_aligned(out, 16) || !ag_aligned(mask, f16 ? 2 : 4)) return LGU_E_UNSUPPORTED;
  const bool vec = wd % CVX_XV == 0 && ag_aligned(mask, (f16 ? 2 : 4) * CVX_XV);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (!f16)
    launch_cvx<float, false>(data, static_cast<const float*>(mask), ix, out, N, U, ht, wd, vec, s);
  else if (halfw)
    launch_cvx<_Float16, true>(data, static_cast<const _Float16*>(mask), ix, out, N, U, ht, wd, vec, s);
  else
    launch_cvx<_Float16, false>(data, static_cast<const _Float16*>(mask), ix, out, N, U, ht, wd, vec, s);
  return launch_status();
}

}  // namespace lgu

extern "C" {

int lgu_scatter_mean_f32(const float* src, const long long* index, int outer, int n, long long inner, int M, float* out,
                         void* stream) {
  return lgu::launch_segment_mean<float>(src, index, outer, n, inner, M, out, stream);
}

int lgu_scatter_mean_h16(const void* src, const long long* index, int outer, int n, long long inner, int M, void* out,
                         void* stream) {
  return lgu::launch_segment_mean<_Float16>(static_cast<const _Float16*>(src), index, outer, n, inner, M,
                                            static_cast<_Float16*>(out), stream);
}

int lgu_cvx_upsample_f32(const float* data, const void* mask, int B, int ht, int wd, int flags, float* out, void* stream) {
  return lgu::cvx_entry(data, B, ht, wd, nullptr, B, mask, flags, out, stream);
}

int lgu_upsample_disps_f32(const float* disps, int N, int ht, int wd, const long long* ix, int U, const void* mask,
                           int flags, float* disps_up, void* stream) {
  if (U > 0 && !ix) return LGU_E_BADARG;
  return lgu::cvx_entry(disps, N, ht, wd, ix, U, mask, flags, disps_up, stream);
}

}  // extern "C"
