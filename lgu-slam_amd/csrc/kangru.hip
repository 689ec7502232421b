// kangru.hip — the element-wise and small-GEMM work of LGU-SLAM's KAN-bias GRU (reference
// droid_slam/modules/gru_kanBias.py, modules/kan.py), in the reference configuration only: C = 128 hidden channels,
// 448 = 128 + 320 input channels of the three 3x3 convolutions, KANLinear(128, 128, grid_size=3, spline_order=3) heads
// with SiLU and a standalone spline scaler.  The three 3x3 convolutions stay library calls (lgu-slam_amd/gru.py).
//
// T = float (fp32 mode) or _Float16 (autocast mode).  rnd<T>(v) rounds an fp32 value to T and back: the identity for
// fp32, round-to-nearest-even to half otherwise; each one stands where the reference's autocast composition returns a
// half tensor.  Built with -ffp-contract=off, so no product is fused into an add.
//
// 1. context  glo[e,c] = mean_p rnd(rnd(s) * net[e,c,p]),  s = sigmoid(rnd(W_w·net[e,:,p] + b_w[c])): the 1x1
//    convolution on the matrix cores (v_mfma_f32_16x16x32_f16 / v_mfma_f32_16x16x4_f32, fp32 accumulation), the gate
//    and product in registers.  Workgroup (t, e) covers pixels [t*256, t*256+256) of edge e and writes the per-channel
//    fp32 sum of its pixels to partial[e,t,:] (each lane adds its pixels in ascending order, then a fixed butterfly
//    over the 16 lanes of a channel); the finalize adds partial[e,0..T-1,c] in ascending t and divides by H*W.  No
//    atomics: the bits depend only on the edge's own data and H*W, not on E or on the other edges of the launch.
// 2. heads    k[h,e,:] = rnd(rnd(silu_T(x)·W_base[h]ᵀ) + rnd(B_h(x)·(W_spline[h] ⊙ scaler[h])ᵀ)), x = glo[e,:]: one
//    launch for the three heads; 16 edges form the M side of an MFMA tile, the packed (384, 896) weight the N side.
//    B_h(x) is the Cox–de Boor recursion on the head's own knots, in the reference's operation order, in fp32.
// 3. gates    z = rnd(sigmoid(rnd(cz + kz))), net_inp[:, 0:128] = rnd(rnd(sigmoid(rnd(cr + kr))) * net) in place.
// 4. blend    q = rnd(tanh(rnd(cq + kq))), out = rnd(rnd(rnd(1 - z) * net) + rnd(z * q)).
// sigmoid(v) = 1 / (1 + expf(-v)), tanh = tanhf, silu(v) = v / (1 + expf(-v)): torch's device formulas in float.
#include <limits.h>

#include "kangru_math.hpp"   // rnd<T>, kg_sigmoid
#include "lgu_common.hpp"

namespace lgu {

constexpr int KG_C = 128;                  // hidden channels = KAN in / out features
constexpr int KG_CIN = 448;                // net_inp channels
constexpr int KG_NG = 10;                  // knots per input feature (grid_size + 2 * order + 1)
constexpr int KG_NB = 6;                   // bases per input feature (grid_size + order)
constexpr int KG_K = KG_C + KG_C * KG_NB;  // 896: [silu(x) | B(x)] per edge
constexpr int KG_THREADS = 256;
constexpr int KG_CTX_PIX = LGU_KANGRU_CTX_PIXELS;  // pixels per context workgroup
constexpr int KG_TILE = 64;                        // pixels per LDS tile (4 MFMA column tiles)
constexpr int KG_MT = 16;                          // edges per heads workgroup

// MFMA step: A = 16 rows x k-slice, B = k-slice x 16 columns; C/D: lane l holds rows 4(l>>4)+i, column l&15.
// half (16x16x32): lane l holds A[l&15][8(l>>4)+j] and B[8(l>>4)+j][l&15], j < 8.
// float (16x16x4): lane l holds A[l&15][l>>4] and B[l>>4][l&15].
template <typename T> struct KgMma;
template <> struct KgMma<_Float16> {
  static constexpr int KS = 32;  // k per instruction
  typedef f16x8 frag;
  static __device__ __forceinline__ frag ld(const _Float16* p) { return *reinterpret_cast<const frag*>(p); }
  static __device__ __forceinline__ f32x4 mma(frag a, frag b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
  }
  static constexpr int kofs(int kg) { return 8 * kg; }
};
template <> struct KgMma<float> {
  static constexpr int KS = 4;
  typedef float frag;
  static __device__ __forceinline__ frag ld(const float* p) { return *p; }
  static __device__ __forceinline__ f32x4 mma(frag a, frag b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
  }
  static constexpr int kofs(int kg) { return kg; }
};

template <typename T> struct KgPad { static constexpr int v = 8; };  // half rows stay 16-byte aligned
template <> struct KgPad<float> { static constexpr int v = 4; };

// ---- 1. context ------------------------------------------------------------------------------------------------
// Grid (T, E), 4 waves.  The LDS tile holds 64 pixels x 128 channels transposed ([pixel][channel]) so that a lane's
// k-slice of the B operand (channels at one pixel) is contiguous.  Wave w owns output channels [32w, 32w+32) (two
// 16-row tiles); its W_w fragments stay in registers for the whole workgroup.  VEC: 16-byte loads of 16 / sizeof(T)
// pixels (H*W a multiple of it and net 16-byte aligned).
template <typename T, bool VEC>
__global__ __launch_bounds__(KG_THREADS) void kangru_context_kernel(const T* __restrict__ net, const T* __restrict__ wt,
                                                                   const T* __restrict__ bias, float* __restrict__ partial,
                                                                   int HW, int ntiles) {
  typedef KgMma<T> M;
  constexpr int PITCH = KG_C + KgPad<T>::v;
  constexpr int NKS = KG_C / M::KS;
  __shared__ __attribute__((aligned(16))) T tile[KG_TILE * PITCH];
  const int t = blockIdx.x, e = blockIdx.y;
  const int lane = threadIdx.x & (kWave - 1), w = threadIdx.x >> 6;
  const int lr = lane & 15, kg = lane >> 4;
  const T* src = net + (size_t)e * KG_C * HW;

  typename M::frag a[2][NKS];
#pragma unroll
  for (int ct = 0; ct < 2; ct++)
#pragma unroll
    for (int ks = 0; ks < NKS; ks++) a[ct][ks] = M::ld(wt + (32 * w + 16 * ct + lr) * KG_C + ks * M::KS + M::kofs(kg));
  float bz[2][4];
#pragma unroll
  for (int ct = 0; ct < 2; ct++)
#pragma unroll
    for (int i = 0; i < 4; i++) bz[ct][i] = (float)bias[32 * w + 16 * ct + 4 * kg + i];
  float sum[2][4];
#pragma unroll
  for (int ct = 0; ct < 2; ct++)
#pragma unroll
    for (int i = 0; i < 4; i++) sum[ct][i] = 0.0f;

  const int p0 = t * KG_CTX_PIX;
  const int p1 = min(p0 + KG_CTX_PIX, HW);
  for (int pb = p0; pb < p1; pb += KG_TILE) {
    __syncthreads();  // the previous tile's readers are done
    if constexpr (VEC) {
      constexpr int V = 16 / sizeof(T);
      constexpr int PER = KG_TILE / V;  // vectors per channel row of the tile
      typedef T vt __attribute__((ext_vector_type(V)));
#pragma unroll
      for (int q = 0; q < KG_C * PER / KG_THREADS; q++) {
        const int idx = q * KG_THREADS + threadIdx.x;
        const int c = idx / PER, pv = (idx % PER) * V;
        vt v;
        if (pb + pv < p1) {  // H*W % V == 0 and pb % V == 0: the whole vector is in range
          v = *reinterpret_cast<const vt*>(src + (size_t)c * HW + pb + pv);
        } else {
#pragma unroll
          for (int j = 0; j < V; j++) v[j] = (T)0;
        }
#pragma unroll
        for (int j = 0; j < V; j++) tile[(pv + j) * PITCH + c] = v[j];
      }
    } else {
#pragma unroll 4
      for (int q = 0; q < KG_C * KG_TILE / KG_THREADS; q++) {
        const int idx = q * KG_THREADS + threadIdx.x;
        const int c = idx / KG_TILE, pp = idx % KG_TILE;
        tile[pp * PITCH + c] = pb + pp < p1 ? src[(size_t)c * HW + pb + pp] : (T)0;
      }
    }
    __syncthreads();
#pragma unroll
    for (int pt = 0; pt < KG_TILE / 16; pt++) {
      if (pb + pt * 16 >= p1) break;  // wave-uniform
      const int p = pt * 16 + lr;
      const bool valid = pb + p < p1;
      typename M::frag b[NKS];
#pragma unroll
      for (int ks = 0; ks < NKS; ks++) b[ks] = M::ld(tile + p * PITCH + ks * M::KS + M::kofs(kg));
#pragma unroll
      for (int ct = 0; ct < 2; ct++) {
        f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int ks = 0; ks < NKS; ks++) acc = M::mma(a[ct][ks], b[ks], acc);
#pragma unroll
        for (int i = 0; i < 4; i++) {
          const int c = 32 * w + 16 * ct + 4 * kg + i;
          const float y = rnd<T>(acc[i] + bz[ct][i]);  // the library adds the bias before its one rounding
          const float s = rnd<T>(kg_sigmoid(y));
          const float pr = rnd<T>(s * (float)tile[p * PITCH + c]);
          if (valid) sum[ct][i] += pr;
        }
      }
    }
  }
#pragma unroll
  for (int ct = 0; ct < 2; ct++)
#pragma unroll
    for (int i = 0; i < 4; i++) {
      float v = sum[ct][i];
#pragma unroll
      for (int m = 1; m < 16; m <<= 1) v += __shfl_xor(v, m, kWave);
      if (lr == 0) partial[((size_t)e * ntiles + t) * KG_C + 32 * w + 16 * ct + 4 * kg + i] = v;
    }
}

template <typename T>
__global__ __launch_bounds__(KG_THREADS) void kangru_context_finalize_kernel(const float* __restrict__ partial,
                                                                            T* __restrict__ glo, int E, int ntiles, int HW) {
  const int idx = blockIdx.x * KG_THREADS + threadIdx.x;
  if (idx >= E * KG_C) return;
  const int e = idx / KG_C, c = idx % KG_C;
  float s = 0.0f;
  for (int t = 0; t < ntiles; t++) s += partial[((size_t)e * ntiles + t) * KG_C + c];
  glo[idx] = (T)(s / (float)HW);
}

// ---- 2. KAN heads ----------------------------------------------------------------------------------------------
// Grid (ceil(E/16), 3 heads), 4 waves.  The 16 feature rows [silu(x) | B(x)] of the workgroup's edges are built in LDS
// (rows past E are zero and never stored); wave w computes outputs [32w, 32w+32) of head h with two accumulators per
// output (base, spline), the B operand read straight from the packed weight (L2-resident).
template <typename T>
__global__ __launch_bounds__(KG_THREADS) void kan_heads_kernel(const T* __restrict__ glo, const float* __restrict__ grid,
                                                              const T* __restrict__ wpack, T* __restrict__ out, int E) {
  typedef KgMma<T> M;
  constexpr int PITCH = KG_K + KgPad<T>::v;
  __shared__ __attribute__((aligned(16))) T feat[KG_MT * PITCH];
  const int e0 = blockIdx.x * KG_MT, h = blockIdx.y;
  const int lane = threadIdx.x & (kWave - 1), w = threadIdx.x >> 6;
  const int lr = lane & 15, kg = lane >> 4;

  for (int idx = threadIdx.x; idx < KG_MT * KG_C; idx += KG_THREADS) {
    const int r = idx / KG_C, i = idx % KG_C, e = e0 + r;
    T* row = feat + r * PITCH;
    if (e >= E) {
      row[i] = (T)0;
#pragma unroll
      for (int k = 0; k < KG_NB; k++) row[KG_C + i * KG_NB + k] = (T)0;
      continue;
    }
    const float x = (float)glo[(size_t)e * KG_C + i];
    row[i] = (T)(x / (1.0f + expf(-x)));
    const float* gp = grid + ((size_t)h * KG_C + i) * KG_NG;
    float g[KG_NG];
#pragma unroll
    for (int j = 0; j < KG_NG; j++) g[j] = gp[j];
    float b[KG_NG - 1];
#pragma unroll
    for (int j = 0; j < KG_NG - 1; j++) b[j] = (x >= g[j] && x < g[j + 1]) ? 1.0f : 0.0f;
#pragma unroll
    for (int k = 1; k <= 3; k++)
#pragma unroll
      for (int j = 0; j < KG_NG - 1 - k; j++)  // b[j + 1] is still of order k - 1 here
        b[j] = (x - g[j]) / (g[j + k] - g[j]) * b[j] + (g[j + k + 1] - x) / (g[j + k + 1] - g[j + 1]) * b[j + 1];
#pragma unroll
    for (int k = 0; k < KG_NB; k++) row[KG_C + i * KG_NB + k] = (T)b[k];
  }
  __syncthreads();

  const T* arow = feat + lr * PITCH + M::kofs(kg);
#pragma unroll
  for (int nt = 0; nt < 2; nt++) {
    const int o = 32 * w + 16 * nt + lr;
    const T* wrow = wpack + ((size_t)h * KG_C + o) * KG_K + M::kofs(kg);
    f32x4 accb = {0.0f, 0.0f, 0.0f, 0.0f}, accs = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int k0 = 0; k0 < KG_C; k0 += M::KS) accb = M::mma(M::ld(arow + k0), M::ld(wrow + k0), accb);
#pragma unroll 8
    for (int k0 = KG_C; k0 < KG_K; k0 += M::KS) accs = M::mma(M::ld(arow + k0), M::ld(wrow + k0), accs);
    const int oc = 32 * w + 16 * nt + lr;
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const int e = e0 + 4 * kg + i;
      if (e < E) out[((size_t)h * E + e) * KG_C + oc] = (T)(rnd<T>(accb[i]) + rnd<T>(accs[i]));
    }
  }
}

// ---- 3. gates, 4. blend ----------------------------------------------------------------------------------------
// One thread per V consecutive pixels of one (edge, channel) row; V = 16 / sizeof(T) when H*W is a multiple of it and
// every operand is 16-byte aligned, 1 otherwise.
template <typename T, int V>
__global__ __launch_bounds__(KG_THREADS) void kangru_gates_kernel(const T* __restrict__ cz, const T* __restrict__ cr,
                                                                 const T* __restrict__ kz, const T* __restrict__ kr,
                                                                 const T* __restrict__ net, T* __restrict__ z,
                                                                 T* __restrict__ net_inp, int HW, long long nvec) {
  typedef T vt __attribute__((ext_vector_type(V)));
  const long long idx = (long long)blockIdx.x * KG_THREADS + threadIdx.x;
  if (idx >= nvec) return;
  const long long el = idx * V;
  const long long row = el / HW;  // e * 128 + c
  const int p = (int)(el - row * HW);
  const long long e = row / KG_C;
  const int c = (int)(row - e * KG_C);
  const vt vz = *reinterpret_cast<const vt*>(cz + el), vr = *reinterpret_cast<const vt*>(cr + el);
  const vt vn = *reinterpret_cast<const vt*>(net + el);
  const float bz = (float)kz[row], br = (float)kr[row];
  vt oz, orn;
#pragma unroll
  for (int j = 0; j < V; j++) {
    oz[j] = (T)kg_sigmoid(rnd<T>((float)vz[j] + bz));
    const float r = rnd<T>(kg_sigmoid(rnd<T>((float)vr[j] + br)));
    orn[j] = (T)(r * (float)vn[j]);
  }
  *reinterpret_cast<vt*>(z + el) = oz;
  *reinterpret_cast<vt*>(net_inp + ((size_t)e * KG_CIN + c) * HW + p) = orn;
}

template <typename T, int V>
__global__ __launch_bounds__(KG_THREADS) void kangru_blend_kernel(const T* __restrict__ cq, const T* __restrict__ kq,
                                                                 const T* __restrict__ z, const T* __restrict__ net,
                                                                 T* __restrict__ out, int HW, long long nvec) {
  typedef T vt __attribute__((ext_vector_type(V)));
  const long long idx = (long long)blockIdx.x * KG_THREADS + threadIdx.x;
  if (idx >= nvec) return;
  const long long el = idx * V;
  const long long row = el / HW;
  const vt vq = *reinterpret_cast<const vt*>(cq + el), vz = *reinterpret_cast<const vt*>(z + el);
  const vt vn = *reinterpret_cast<const vt*>(net + el);
  const float bq = (float)kq[row];
  vt o;
#pragma unroll
  for (int j = 0; j < V; j++) {
    const float q = rnd<T>(tanhf(rnd<T>((float)vq[j] + bq)));
    const float zz = (float)vz[j], n = (float)vn[j];
    const float t1 = rnd<T>(rnd<T>(1.0f - zz) * n);
    const float t2 = rnd<T>(zz * q);
    o[j] = (T)(t1 + t2);
  }
  *reinterpret_cast<vt*>(out + el) = o;
}

// ---- launchers ---------------------------------------------------------------------------------------------------
static inline bool kg_aligned(const void* p, int n) { return (reinterpret_cast<uintptr_t>(p) % n) == 0; }

static inline bool kg_sizes_ok(int E, int HW) {
  return E >= 0 && HW >= 0 && (long long)E * KG_CIN * HW <= (long long)INT_MAX * 64;
}

template <typename T>
int context_entry(const T* net, const T* wt, const T* bias, int E, int HW, float* partial, T* glo, void* stream) {
  if (!kg_sizes_ok(E, HW)) return LGU_E_BADARG;
  if (E == 0) return LGU_OK;
  if (HW == 0 || !net || !wt || !bias || !partial || !glo) return LGU_E_BADARG;
  if (E > 65535) return LGU_E_UNSUPPORTED;
  if (!kg_aligned(wt, 16)) return LGU_E_UNSUPPORTED;
  const int ntiles = (HW + KG_CTX_PIX - 1) / KG_CTX_PIX;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const bool vec = HW % (16 / (int)sizeof(T)) == 0 && kg_aligned(net, 16);
  if (vec)
    hipLaunchKernelGGL((kangru_context_kernel<T, true>), dim3(ntiles, E), dim3(KG_THREADS), 0, s, net, wt, bias, partial,
                       HW, ntiles);
  else
    hipLaunchKernelGGL((kangru_context_kernel<T, false>), dim3(ntiles, E), dim3(KG_THREADS), 0, s, net, wt, bias, partial,
                       HW, ntiles);
  const int nb = (E * KG_C + KG_THREADS - 1) / KG_THREADS;
  hipLaunchKernelGGL((kangru_context_finalize_kernel<T>), dim3(nb), dim3(KG_THREADS), 0, s, partial, glo, E, ntiles, HW);
  return launch_status();
}

template <typename T>
int heads_entry(const T* glo, const float* grid, const T* wpack, int E, T* out, void* stream) {
  if (E < 0) return LGU_E_BADARG;
  if (E == 0) return LGU_OK;
  if (!glo || !grid || !wpack || !out) return LGU_E_BADARG;
  if (E > INT_MAX / KG_C) return LGU_E_UNSUPPORTED;
  if (!kg_aligned(wpack, 16)) return LGU_E_UNSUPPORTED;
  const int nb = (E + KG_MT - 1) / KG_MT;
  hipLaunchKernelGGL((kan_heads_kernel<T>), dim3(nb, 3), dim3(KG_THREADS), 0, reinterpret_cast<hipStream_t>(stream), glo,
                     grid, wpack, out, E);
  return launch_status();
}

template <typename T>
int gates_entry(const T* cz, const T* cr, const T* kz, const T* kr, const T* net, int E, int HW, T* z, T* net_inp,
                void* stream) {
  if (!kg_sizes_ok(E, HW)) return LGU_E_BADARG;
  if ((long long)E * HW == 0) return LGU_OK;
  if (!cz || !cr || !kz || !kr || !net || !z || !net_inp) return LGU_E_BADARG;
  constexpr int V = 16 / sizeof(T);
  const bool vec = HW % V == 0 && kg_aligned(cz, 16) && kg_aligned(cr, 16) && kg_aligned(net, 16) && kg_aligned(z, 16) &&
                   kg_aligned(net_inp, 16);
  const long long nvec = (long long)E * KG_C * HW / (vec ? V : 1);
  const long long nb = (nvec + KG_THREADS - 1) / KG_THREADS;
  if (nb > INT_MAX) return LGU_E_UNSUPPORTED;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (vec)
    hipLaunchKernelGGL((kangru_gates_kernel<T, V>), dim3((unsigned)nb), dim3(KG_THREADS), 0, s, cz, cr, kz, kr, net, z,
                       net_inp, HW, nvec);
  else
    hipLaunchKernelGGL((kangru_gates_kernel<T, 1>), dim3((unsigned)nb), dim3(KG_THREADS), 0, s, cz, cr, kz, kr, net, z,
                       net_inp, HW, nvec);
  return launch_status();
}

template <typename T>
int blend_entry(const T* cq, const T* kq, const T* z, const T* net, int E, int HW, T* out, void* stream) {
  if (!kg_sizes_ok(E, HW)) return LGU_E_BADARG;
  if ((long long)E * HW == 0) return LGU_OK;
  if (!cq || !kq || !z || !net || !out) return LGU_E_BADARG;
  constexpr int V = 16 / sizeof(T);
  const bool vec = HW % V == 0 && kg_aligned(cq, 16) && kg_aligned(z, 16) && kg_aligned(net, 16) && kg_aligned(out, 16);
  const long long nvec = (long long)E * KG_C * HW / (vec ? V : 1);
  const long long nb = (nvec + KG_THREADS - 1) / KG_THREADS;
  if (nb > INT_MAX) return LGU_E_UNSUPPORTED;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (vec)
    hipLaunchKernelGGL((kangru_blend_kernel<T, V>), dim3((unsigned)nb), dim3(KG_THREADS), 0, s, cq, kq, z, net, out, HW,
                       nvec);
  else
    hipLaunchKernelGGL((kangru_blend_kernel<T, 1>), dim3((unsigned)nb), dim3(KG_THREADS), 0, s, cq, kq, z, net, out, HW,
                       nvec);
  return launch_status();
}

}  // namespace lgu

extern "C" {

typedef _Float16 lgu_h16;
#define LGU_H(p) static_cast<const lgu_h16*>(p)
#define LGU_HW(p) static_cast<lgu_h16*>(p)

int lgu_kangru_context_f32(const float* net, const float* weight, const float* bias, int E, int HW, float* partial,
                           float* glo, void* stream) {
  return lgu::context_entry<float>(net, weight, bias, E, HW, partial, glo, stream);
}

int lgu_kangru_context_h16(const void* net, const void* weight, const void* bias, int E, int HW, float* partial, void* glo,
                           void* stream) {
  return lgu::context_entry<lgu_h16>(LGU_H(net), LGU_H(weight), LGU_H(bias), E, HW, partial, LGU_HW(glo), stream);
}

int lgu_kan_heads_f32(const float* glo, const float* grid, const float* wpack, int E, float* out, void* stream) {
  return lgu::heads_entry<float>(glo, grid, wpack, E, out, stream);
}

int lgu_kan_heads_h16(const void* glo, const float* grid, const void* wpack, int E, void* out, void* stream) {
  return lgu::heads_entry<lgu_h16>(LGU_H(glo), grid, LGU_H(wpack), E, LGU_HW(out), stream);
}

int lgu_kangru_gates_f32(const float* cz, const float* cr, const float* kz, const float* kr, const float* net, int E,
                         int HW, float* z, float* net_inp, void* stream) {
  return lgu::gates_entry<float>(cz, cr, kz, kr, net, E, HW, z, net_inp, stream);
}

int lgu_kangru_gates_h16(const void* cz, const void* cr, const void* kz, const void* kr, const void* net, int E, int HW,
                         void* z, void* net_inp, void* stream) {
  return lgu::gates_entry<lgu_h16>(LGU_H(cz), LGU_H(cr), LGU_H(kz), LGU_H(kr), LGU_H(net), E, HW, LGU_HW(z),
                                   LGU_HW(net_inp), stream);
}

int lgu_kangru_blend_f32(const float* cq, const float* kq, const float* z, const float* net, int E, int HW, float* out,
                         void* stream) {
  return lgu::blend_entry<float>(cq, kq, z, net, E, HW, out, stream);
}

int lgu_kangru_blend_h16(const void* cq, const void* kq, const void* z, const void* net, int E, int HW, void* out,
                         void* stream) {
  return lgu::blend_entry<lgu_h16>(LGU_H(cq), LGU_H(kq), LGU_H(z), LGU_H(net), E, HW, LGU_HW(out), stream);
}

}  // extern "C"
