// instnorm.hip — the element-wise work around the feature encoder's convolutions (reference
// droid_slam/modules/extractor.py:47-55, :183-198: BasicEncoder(128, 'instance')) and the frame upload's normalisation
// (droid_slam/motion_filter.py:56-57).
//
// A plane is one (n, c) slice of a contiguous NCHW tensor, hw elements.  IN(x) = (x - mean) * rstd with
//   mean = S1 / hw,  S1 = sum of x                      (fp32, from the values as stored)
//   var  = S2 / hw,  S2 = sum of (x - mean)^2           (the centred form: the mean is final before S2 starts)
//   rstd = 1 / sqrt(var + eps)                          (correctly rounded sqrt and divisions)
// and per element, all in fp32 and rounded to the tensor type once, at the store:
//   mode 0  relu(IN(a))                 mode 1  relu(b + relu(IN(a)))
//   mode 2  relu(IN(b) + relu(IN(a)))   mode 3  IN(a)
// relu(v) = v < 0 ? 0 : v, so a NaN stays a NaN as in torch.
//
// Resident path (hw <= IN_NV * 1024 vectors of 16 bytes): ONE launch, one workgroup per plane.  Every thread keeps its
// share of the plane (and of b's plane in mode 2) in registers between the statistics and the store: up to IN_NV
// 16-byte vectors per operand plus one scalar of the tail, so global memory is read once per operand and written once.
// The workgroup has 256 threads while the plane fits IN_NV * 256 vectors and 1024 beyond; the choice depends on hw
// alone.  Vector k of a plane is its elements [k V, (k + 1) V) counted from the plane's first element, wherever that
// lies in memory: the 16-byte accesses are declared with the element's alignment only (gfx950 serves them; they are
// aligned whenever hw * sizeof(element) is a multiple of 16 and the tensor is, as for every production plane), so the
// grouping of the sums, and with it every bit of the result, is the same at any address.
//
// Sums are trees: the 4 or 8 values of a vector pairwise, the IN_NV vector sums of a thread pairwise, the tail scalar on
// top, a wave butterfly (6 levels), and the wave totals pairwise in wave order by every thread.  Depth
// <= 3 + 3 + 1 + 6 + 4 = 17 <= log2(hw) + 4 where the plane needs 1024 threads.  No atomics; a plane's bits depend on
// its own values, hw and eps only: not on the other planes of the call, not on its position among them.
//
// Large planes: a statistics launch (one workgroup of 1024 threads per plane, two passes over the plane) and an apply
// launch over all elements.  There a thread adds its ceil(hw / (1024 V)) vector sums one after the other in ascending
// address order before the same wave and workgroup trees, so the depth is 3 + ceil(hw / (1024 V)) + 1 + 10: 12
// sequential adds at twice the resident limit, growing linearly with the plane beyond (each thread's chain covers
// 1/1024 of the plane; the chains' errors are independent).  The
// 16 * planes bytes of statistics between them come from the stream-ordered allocator (hipMallocAsync / hipFreeAsync on
// the caller's stream): no host synchronisation.  No workgroup ever waits on another.
//
// out may be exactly a or exactly b: every thread reads the elements it writes, and only those, before it writes them.
#include <limits.h>

#include "lgu_common.hpp"
#include "image_norm.hpp"

namespace lgu {

constexpr int IN_NV = 6;            // 16-byte vectors per thread and operand on the resident path
static_assert(IN_NV == 6, "six_tree() adds exactly six vector sums");
constexpr int IN_SMALL = 256, IN_BIG = 1024;
constexpr int IN_APPLY_THREADS = 256;
constexpr int IMG_THREADS = 256;


// 16 bytes of T; `mem` is the same vector with the alignment of one element, for accesses at any element address.
template <typename T> struct InVec;
template <> struct InVec<float> {
  typedef f32x4 type;
  typedef f32x4 mem __attribute__((aligned(4)));
  static constexpr int n = 4;
};
template <> struct InVec<_Float16> {
  typedef f16x8 type;
  typedef f16x8 mem __attribute__((aligned(2)));
  static constexpr int n = 8;
};

__device__ __forceinline__ float in_relu(float v) { return v < 0.0f ? 0.0f : v; }

// Pairwise sum of a thread's IN_NV vector sums.
__device__ __forceinline__ float six_tree(const float (&s)[IN_NV]) { return ((s[0] + s[1]) + (s[2] + s[3])) + (s[4] + s[5]); }

// The V values of a packed vector as fp32.  A plane's registers are unpacked three times (sum, centred sum, store);
// the empty asm makes each unpacking its own computation, otherwise the compiler keeps the fp32 copies of a half plane
// alive from the first use on (96 registers in mode 2) and spills.

template <typename T>
__device__ __forceinline__ void unpack(const typename InVec<T>::type& v, float (&x)[InVec<T>::n]) {
  const u32x4 w4 = __builtin_bit_cast(u32x4, v);
#pragma unroll
  for (int i = 0; i < 4; i++) {
    unsigned w = w4[i];
    asm volatile("" : "+v"(w));
    if constexpr (InVec<T>::n == 4) {
      x[i] = __builtin_bit_cast(float, w);
    } else {
      const f16x2 h = __builtin_bit_cast(f16x2, w);
      x[2 * i] = (float)h[0];
      x[2 * i + 1] = (float)h[1];
    }
  }
}

// Pairwise sum of the V values of a vector, (x - shift)^2 each when SQ.
template <typename T, bool SQ>
__device__ __forceinline__ float vec_tree(const typename InVec<T>::type& v, float shift) {
  constexpr int V = InVec<T>::n;
  float x[V];
  unpack<T>(v, x);
#pragma unroll
  for (int k = 0; k < V; k++) {
    const float f = x[k];
    if (SQ) {
      const float d = f - shift;
      x[k] = d * d;
    } else {
      x[k] = f;
    }
  }
#pragma unroll
  for (int s = V / 2; s >= 1; s >>= 1)
#pragma unroll
    for (int k = 0; k < s; k++) x[k] = x[k] + x[k + s];
  return x[0];
}

// Totals of N per-thread values over the workgroup, the same bits in every thread.  red: N * THREADS / 64 floats.
template <int THREADS, int N>
__device__ __forceinline__ void block_sum(float (&v)[N], float* red) {
  constexpr int WAVES = THREADS / kWave;
  const int lane = threadIdx.x & (kWave - 1), w = threadIdx.x / kWave;
#pragma unroll
  for (int q = 0; q < N; q++) {
    const float s = wave_sum_f32(v[q]);
    if (lane == 0) red[q * WAVES + w] = s;
  }
  __syncthreads();
#pragma unroll
  for (int q = 0; q < N; q++) {
    float r[WAVES];
#pragma unroll
    for (int k = 0; k < WAVES; k++) r[k] = red[q * WAVES + k];
#pragma unroll
    for (int s = WAVES / 2; s >= 1; s >>= 1)
#pragma unroll
      for (int k = 0; k < s; k++) r[k] = r[k] + r[k + s];
    v[q] = r[0];
  }
  __syncthreads();  // red is written again by the next reduction
}

// A plane is nvec = hw / V vectors and a tail of hw % V < 8 elements from tail0 on, one per thread of the first 7.
struct PlaneSplit {
  long nvec, tail0;
};

template <typename T>
__device__ __forceinline__ PlaneSplit split_plane(long hw) {
  constexpr int V = InVec<T>::n;
  PlaneSplit s;
  s.nvec = hw / V;
  s.tail0 = s.nvec * V;
  return s;
}

__device__ __forceinline__ long edge_index(const PlaneSplit& s, long hw) {
  const long t = threadIdx.x;
  return t < hw - s.tail0 ? s.tail0 + t : -1;
}

template <int MODE>
__device__ __forceinline__ float in_apply(float xa, float xb, float ma, float ra, float mb, float rb) {
  float y = (xa - ma) * ra;
  if (MODE == 0) return in_relu(y);
  if (MODE == 1) return in_relu(xb + in_relu(y));
  if (MODE == 2) {
    const float yb = (xb - mb) * rb;
    return in_relu(yb + in_relu(y));
  }
  return y;
}

// One workgroup per plane; a, b and out may alias exactly (no __restrict__).
// At least 4 waves per SIMD, i.e. at most 128 registers, for the 256-thread form too: left to itself the compiler spends
// 138 (236 in fp32 mode 2) there on hoisted loads and unpacked copies and drops to 3 (1) waves per SIMD.
template <typename T, int MODE, int THREADS>
__global__ __launch_bounds__(THREADS) __attribute__((amdgpu_waves_per_eu(4, 8))) void instnorm_resident_kernel(const T* a, const T* b, T* out, long hw, float eps) {
  constexpr int V = InVec<T>::n;
  constexpr int NOPS = MODE == 2 ? 2 : 1;
  typedef typename InVec<T>::type VT;
  typedef typename InVec<T>::mem VM;
  __shared__ float red[NOPS * THREADS / kWave];
  const size_t base = (size_t)blockIdx.x * (size_t)hw;
  const T* pa = a + base;
  const T* pb = MODE == 1 || MODE == 2 ? b + base : nullptr;
  T* po = out + base;
  const PlaneSplit sp = split_plane<T>(hw);
  const long edge = edge_index(sp, hw);
  const int t = threadIdx.x;

  VT va[IN_NV], vb[NOPS == 2 ? IN_NV : 1];
  float ea = 0.0f, eb = 0.0f;
#pragma unroll
  for (int j = 0; j < IN_NV; j++) {
    const long idx = (long)j * THREADS + t;
    if (idx < sp.nvec) {
      va[j] = *reinterpret_cast<const VM*>(pa + idx * V);
      if constexpr (NOPS == 2) vb[j] = *reinterpret_cast<const VM*>(pb + idx * V);
    } else {
      va[j] = VT(0);
      if constexpr (NOPS == 2) vb[j] = VT(0);
    }
  }
  if (edge >= 0) {
    ea = (float)pa[edge];
    if constexpr (NOPS == 2) eb = (float)pb[edge];
  }

  const float n = (float)hw;
  float mean[NOPS], rstd[NOPS];
  {
    float s[NOPS][IN_NV];
#pragma unroll
    for (int j = 0; j < IN_NV; j++) {
      s[0][j] = vec_tree<T, false>(va[j], 0.0f);
      if constexpr (NOPS == 2) s[1][j] = vec_tree<T, false>(vb[j], 0.0f);
    }
    float tot[NOPS];
#pragma unroll
    for (int q = 0; q < NOPS; q++)
      tot[q] = six_tree(s[q]) + (q == 0 ? ea : eb);
    block_sum<THREADS, NOPS>(tot, red);
#pragma unroll
    for (int q = 0; q < NOPS; q++) mean[q] = tot[q] / n;
  }
  {
    float s[NOPS][IN_NV];
#pragma unroll
    for (int j = 0; j < IN_NV; j++) {
      const bool have = (long)j * THREADS + t < sp.nvec;
      s[0][j] = have ? vec_tree<T, true>(va[j], mean[0]) : 0.0f;
      if constexpr (NOPS == 2) s[1][j] = have ? vec_tree<T, true>(vb[j], mean[1]) : 0.0f;
    }
    float tot[NOPS];
#pragma unroll
    for (int q = 0; q < NOPS; q++) {
      const float d = (q == 0 ? ea : eb) - mean[q];
      tot[q] = six_tree(s[q]) + (edge >= 0 ? d * d : 0.0f);
    }
    block_sum<THREADS, NOPS>(tot, red);
#pragma unroll
    for (int q = 0; q < NOPS; q++) rstd[q] = 1.0f / sqrtf(tot[q] / n + eps);
  }
  const float mb = NOPS == 2 ? mean[NOPS - 1] : 0.0f, rb = NOPS == 2 ? rstd[NOPS - 1] : 0.0f;

#pragma unroll
  for (int j = 0; j < IN_NV; j++) {
    const long idx = (long)j * THREADS + t;
    if (idx < sp.nvec) {
      VT xb = VT(0);
      if constexpr (MODE == 1) xb = *reinterpret_cast<const VM*>(pb + idx * V);
      if constexpr (MODE == 2) xb = vb[j];
      float xa[V], xr[V];
      unpack<T>(va[j], xa);
      unpack<T>(xb, xr);
      VT r;
#pragma unroll
      for (int k = 0; k < V; k++) r[k] = (T)in_apply<MODE>(xa[k], xr[k], mean[0], rstd[0], mb, rb);
      *reinterpret_cast<VM*>(po + idx * V) = r;
    }
  }
  if (edge >= 0) {
    if constexpr (MODE == 1) eb = (float)pb[edge];
    po[edge] = (T)in_apply<MODE>(ea, eb, mean[0], rstd[0], mb, rb);
  }
}

// Sum over one plane (SQ: of (x - shift)^2) by a workgroup of IN_BIG threads: per thread its vectors in ascending
// address order, each a tree, then the edge scalar; the caller reduces over the workgroup.
template <typename T, bool SQ>
__device__ __forceinline__ float plane_partial(const T* p, long hw, float shift) {
  constexpr int V = InVec<T>::n;
  typedef typename InVec<T>::type VT;
  typedef typename InVec<T>::mem VM;
  const PlaneSplit sp = split_plane<T>(hw);
  float acc = 0.0f;
  for (long idx = threadIdx.x; idx < sp.nvec; idx += IN_BIG)
    acc = acc + vec_tree<T, SQ>(VT(*reinterpret_cast<const VM*>(p + idx * V)), shift);
  const long edge = edge_index(sp, hw);
  if (edge >= 0) {
    const float f = (float)p[edge];
    const float d = f - shift;
    acc = acc + (SQ ? d * d : f);
  }
  return acc;
}

// stats[4 p + {0, 1}] = mean, rstd of a's plane p; + {2, 3} of b's plane when NOPS == 2.
template <typename T, int NOPS>
__global__ __launch_bounds__(IN_BIG) void instnorm_stats_kernel(const T* a, const T* b, float* __restrict__ stats, long hw,
                                                                float eps) {
  __shared__ float red[IN_BIG / kWave];
  const size_t base = (size_t)blockIdx.x * (size_t)hw;
  const float n = (float)hw;
#pragma unroll
  for (int q = 0; q < NOPS; q++) {
    const T* p = (q == 0 ? a : b) + base;
    float v[1];
    v[0] = plane_partial<T, false>(p, hw, 0.0f);
    block_sum<IN_BIG, 1>(v, red);
    const float mean = v[0] / n;
    v[0] = plane_partial<T, true>(p, hw, mean);
    block_sum<IN_BIG, 1>(v, red);
    if (threadIdx.x == 0) {
      stats[4 * (size_t)blockIdx.x + 2 * q] = mean;
      stats[4 * (size_t)blockIdx.x + 2 * q + 1] = 1.0f / sqrtf(v[0] / n + eps);
    }
  }
}

// One thread per vector of a plane, and one more for the tail; grid (chunks per plane) * planes, flattened.
template <typename T, int MODE>
__global__ __launch_bounds__(IN_APPLY_THREADS) void instnorm_apply_kernel(const T* a, const T* b, T* out,
                                                                          const float* __restrict__ stats, long hw,
                                                                          long chunks) {
  constexpr int V = InVec<T>::n;
  typedef typename InVec<T>::type VT;
  typedef typename InVec<T>::mem VM;
  const long p = blockIdx.x / chunks;
  const long slot = (long)(blockIdx.x - p * chunks) * IN_APPLY_THREADS + threadIdx.x;
  const PlaneSplit sp = split_plane<T>(hw);
  if (slot > sp.nvec) return;
  const float ma = stats[4 * p], ra = stats[4 * p + 1];
  const float mb = MODE == 2 ? stats[4 * p + 2] : 0.0f, rb = MODE == 2 ? stats[4 * p + 3] : 0.0f;
  const size_t at = (size_t)p * (size_t)hw + (size_t)slot * V;
  if (slot < sp.nvec) {
    const VT xa = *reinterpret_cast<const VM*>(a + at);
    VT xb = VT(0);
    if constexpr (MODE == 1 || MODE == 2) xb = *reinterpret_cast<const VM*>(b + at);
    VT r;
#pragma unroll
    for (int k = 0; k < V; k++) r[k] = (T)in_apply<MODE>((float)xa[k], (float)xb[k], ma, ra, mb, rb);
    *reinterpret_cast<VM*>(out + at) = r;
  } else {
    for (long k = 0; k < hw - sp.tail0; k++) {
      float xb = 0.0f;
      if constexpr (MODE == 1 || MODE == 2) xb = (float)b[at + k];
      out[at + k] = (T)in_apply<MODE>((float)a[at + k], xb, ma, ra, mb, rb);
    }
  }
}

inline bool in_aligned(const void* p, size_t n) { return ((uintptr_t)p & (n - 1)) == 0; }

template <typename T> constexpr long resident_limit() { return (long)IN_NV * IN_BIG * InVec<T>::n; }

template <typename T, int MODE>
int launch_instnorm_mode(const T* a, const T* b, T* out, long planes, long hw, float eps, hipStream_t s) {
  constexpr int V = InVec<T>::n;
  if (hw <= resident_limit<T>()) {
    const dim3 grid((unsigned)planes);
    if (hw <= (long)IN_NV * IN_SMALL * V)
      hipLaunchKernelGGL((instnorm_resident_kernel<T, MODE, IN_SMALL>), grid, dim3(IN_SMALL), 0, s, a, b, out, hw, eps);
    else
      hipLaunchKernelGGL((instnorm_resident_kernel<T, MODE, IN_BIG>), grid, dim3(IN_BIG), 0, s, a, b, out, hw, eps);
    return launch_status();
  }
  const long chunks = (hw / V + 1 + IN_APPLY_THREADS - 1) / IN_APPLY_THREADS;  // hw / V vectors and the tail's slot
  if (chunks > (long)INT_MAX / planes) return LGU_E_UNSUPPORTED;
  float* stats = nullptr;
  hipError_t e = hipMallocAsync(reinterpret_cast<void**>(&stats), sizeof(float) * 4 * (size_t)planes, s);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL((instnorm_stats_kernel<T, MODE == 2 ? 2 : 1>), dim3((unsigned)planes), dim3(IN_BIG), 0, s, a, b, stats,
                     hw, eps);
  int rc = launch_status();
  if (rc == LGU_OK) {
    hipLaunchKernelGGL((instnorm_apply_kernel<T, MODE>), dim3((unsigned)(chunks * planes)), dim3(IN_APPLY_THREADS), 0, s, a, b,
                       out, stats, hw, chunks);
    rc = launch_status();
  }
  e = hipFreeAsync(stats, s);
  return rc != LGU_OK ? rc : (e == hipSuccess ? LGU_OK : (int)e);
}

template <typename T>
int launch_instnorm(const T* a, const T* b, T* out, long planes, long hw, float eps, int mode, void* stream) {
  if (hw < 1 || planes < 0 || mode < 0 || mode > 3 || !(eps >= 0.0f)) return LGU_E_BADARG;
  if (planes == 0) return LGU_OK;
  const bool uses_b = mode == 1 || mode == 2;
  if (!a || !out || (uses_b && !b)) return LGU_E_BADARG;
  if (!in_aligned(a, sizeof(T)) || !in_aligned(out, sizeof(T)) || (uses_b && !in_aligned(b, sizeof(T)))) return LGU_E_BADARG;
  if (planes > (long)INT_MAX) return LGU_E_UNSUPPORTED;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  switch (mode) {
    case 0: return launch_instnorm_mode<T, 0>(a, b, out, planes, hw, eps, s);
    case 1: return launch_instnorm_mode<T, 1>(a, b, out, planes, hw, eps, s);
    case 2: return launch_instnorm_mode<T, 2>(a, b, out, planes, hw, eps, s);
    default: return launch_instnorm_mode<T, 3>(a, b, out, planes, hw, eps, s);
  }
}

struct Rgb {
  float v[3];
};

// out[n, c, i] = image_normalize_value(img[n, 2 - c, i], mean[c], std[c]) (image_norm.hpp: (float(px) * IMG_INV255 - mean)
// / std); one thread per XV consecutive pixels of one output channel.

template <int XV>
__global__ __launch_bounds__(IMG_THREADS) void image_normalize_kernel(const unsigned char* __restrict__ img,
                                                                      float* __restrict__ out, long hw, long groups,
                                                                      long total, Rgb mean, Rgb stdv) {
  const long t = (long)blockIdx.x * IMG_THREADS + threadIdx.x;
  if (t >= total) return;
  const long g = t % groups;
  const long nc = t / groups;
  const int c = (int)(nc % 3);
  const long n = nc / 3;
  const float m = mean.v[c], sd = stdv.v[c];
  const size_t src = ((size_t)n * 3 + (2 - c)) * (size_t)hw + (size_t)g * XV;
  const size_t dst = (size_t)nc * (size_t)hw + (size_t)g * XV;
  if (XV == 4) {
    const u8x4 px = *reinterpret_cast<const u8x4*>(img + src);
    f32x4 r;
#pragma unroll
    for (int k = 0; k < 4; k++) r[k] = image_normalize_value(px[k], m, sd);
    *reinterpret_cast<f32x4*>(out + dst) = r;
  } else {
    out[dst] = image_normalize_value(img[src], m, sd);
  }
}

}  // namespace lgu

extern "C" {

int lgu_instnorm_relu_f32(const float* a, const float* b, float* out, long planes, long hw, float eps, int mode,
                          void* stream) {
  return lgu::launch_instnorm<float>(a, b, out, planes, hw, eps, mode, stream);
}

int lgu_instnorm_relu_h16(const void* a, const void* b, void* out, long planes, long hw, float eps, int mode,
                          void* stream) {
  return lgu::launch_instnorm<_Float16>(static_cast<const _Float16*>(a), static_cast<const _Float16*>(b),
                                        static_cast<_Float16*>(out), planes, hw, eps, mode, stream);
}

long lgu_instnorm_resident_limit(int elem_bytes) {
  if (elem_bytes == 2) return lgu::resident_limit<_Float16>();
  if (elem_bytes == 4) return lgu::resident_limit<float>();
  return 0;
}

int lgu_image_normalize_u8(const unsigned char* img, float* out, long n, long hw, const float mean[3], const float std[3],
                           void* stream) {
  using namespace lgu;
  if (n < 0 || hw < 0 || !mean || !std) return LGU_E_BADARG;
  if (n == 0 || hw == 0) return LGU_OK;
  if (!img || !out || !in_aligned(out, 4)) return LGU_E_BADARG;
  if (n > (long)INT_MAX / 3 || hw > (long)INT_MAX) return LGU_E_UNSUPPORTED;
  Rgb m, s;
  for (int c = 0; c < 3; c++) {
    m.v[c] = mean[c];
    s.v[c] = std[c];
  }
  const bool vec = hw % 4 == 0 && in_aligned(img, 4) && in_aligned(out, 16);
  const long groups = vec ? hw / 4 : hw;
  const long total = n * 3 * groups;
  const long blocks = (total + IMG_THREADS - 1) / IMG_THREADS;
  if (blocks > (long)INT_MAX) return LGU_E_UNSUPPORTED;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (vec)
    hipLaunchKernelGGL((image_normalize_kernel<4>), dim3((unsigned)blocks), dim3(IMG_THREADS), 0, st, img, out, hw, groups,
                       total, m, s);
  else
    hipLaunchKernelGGL((image_normalize_kernel<1>), dim3((unsigned)blocks), dim3(IMG_THREADS), 0, st, img, out, hw, groups,
                       total, m, s);
  return launch_status();
}

}  // extern "C"
