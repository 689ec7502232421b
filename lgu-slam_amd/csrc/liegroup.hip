// liegroup.hip — SO3 / SE3 group operations behind lgu_slam_amd.lie (the surface the reference's droid_slam uses of
// lietorch), float32, in plain HIP.  Built with -ffp-contract=off like the rest of the library.
//
// Conventions (the contract of include/lgu_corr.h, "Lie groups"):
//   SO3 = q (x, y, z, w);  SE3 = t, q;  tangents phi (3) and (tau, phi) (6), translation first.
//   Quaternions are used as given: never normalised, never sign-flipped (log picks the rotation of norm <= pi itself).
//   R(q) X = X + w (2 v x X) + v x (2 v x X) (se3.hpp act_so3), the product is Hamilton's, G H = (t_G + R_G t_H, q_G q_H).
//   exp(tau, phi) = (V tau, [sin(th/2) phi / th, cos(th/2)]), V = I + B [phi]x + C [phi]x^2, B = (1 - cos th) / th^2
//   evaluated as 2 (sin(th/2) / th)^2 (no cancellation), C = (th - sin th) / th^3; log is its inverse with
//   V^-1 = I - [phi]x / 2 + D [phi]x^2, D = (1 - (th/2) cot(th/2)) / th^2.  Series below the thresholds named at each
//   function; exp(0) and log(identity) are exact.
//
// Two kernel families:
//   * per-element (inv, mul, retr, exp, log, matrix): one thread per element, one launch per call — these run on a few
//     hundred poses and are launch-bound;
//   * broadcast (act on 3- or 4-component points, adj, adjT): a pure stream over `rows` operand rows, row r using group
//     element r / g_div read from the COMPACT group tensor (7 or 4 floats, a wave-wide broadcast out of the L1/L2) — an
//     expanded copy of G is never read.  4-component points are one 16-byte load and store per lane.  3-float rows
//     (points, SO3 tangents) and 6-float rows (SE3 tangents) are taken 12 floats per lane: a workgroup moves 3072
//     consecutive floats through LDS with 16-byte, lane-contiguous global accesses, and each lane then owns 12 of them =
//     4 rows of 3 or 2 rows of 6, read from LDS as three b128 accesses (stride 3 slots: conflict-free).
#include <limits.h>

#include "lgu_common.hpp"
#include "se3.hpp"

namespace lgu {

constexpr int LIE_ELEM_THREADS = 64;
constexpr int LIE_THREADS = 256;
constexpr int LIE_CHUNK = 12;                               // floats per lane of the 12-float stream
constexpr int LIE_BLOCK_FLOATS = LIE_THREADS * LIE_CHUNK;   // 3072: a multiple of 3, 4 and 6


enum { LIE_INV, LIE_MUL, LIE_RETR, LIE_EXP, LIE_LOG, LIE_MATRIX };
enum { LIE_ACT3, LIE_ADJ, LIE_ADJT };

__device__ __forceinline__ float dot3(const float* a, const float* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }

// Hamilton product c = a b of quaternions (x, y, z, w)
__device__ __forceinline__ void quat_mul(const float* a, const float* b, float* c) {
  c[0] = a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1];
  c[1] = a[3] * b[1] + a[1] * b[3] + a[2] * b[0] - a[0] * b[2];
  c[2] = a[3] * b[2] + a[2] * b[3] + a[0] * b[1] - a[1] * b[0];
  c[3] = a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2];
}

// K = 7: (t, q); K = 4: q alone, t = 0
template <int K>
__device__ __forceinline__ void load_elem(const float* p, float* t, float* q) {
  if (K == 7) {
    t[0] = p[0]; t[1] = p[1]; t[2] = p[2];
    q[0] = p[3]; q[1] = p[4]; q[2] = p[5]; q[3] = p[6];
  } else {
    t[0] = t[1] = t[2] = 0.0f;
    q[0] = p[0]; q[1] = p[1]; q[2] = p[2]; q[3] = p[3];
  }
}
template <int K>
__device__ __forceinline__ void store_elem(float* p, const float* t, const float* q) {
  if (K == 7) {
    p[0] = t[0]; p[1] = t[1]; p[2] = t[2];
    p[3] = q[0]; p[4] = q[1]; p[5] = q[2]; p[6] = q[3];
  } else {
    p[0] = q[0]; p[1] = q[1]; p[2] = q[2]; p[3] = q[3];
  }
}

// q = [sin(th/2) phi / th, cos(th/2)]; returns im = sin(th/2) / th.  th^2 < 1e-4: series through th^4 (the next terms,
// th^6 / 645120 and th^6 / 46080, are below 1e-16).
__device__ __forceinline__ float so3_exp(const float* phi, float* q) {
  const float th2 = dot3(phi, phi);
  float im, re;
  if (th2 < 1e-4f) {
    im = 0.5f - th2 * (1.0f / 48.0f) + th2 * th2 * (1.0f / 3840.0f);
    re = 1.0f - th2 * (1.0f / 8.0f) + th2 * th2 * (1.0f / 384.0f);
  } else {
    const float th = sqrtf(th2);
    im = sinf(0.5f * th) / th;
    re = cosf(0.5f * th);
  }
  q[0] = im * phi[0]; q[1] = im * phi[1]; q[2] = im * phi[2]; q[3] = re;
  return im;
}

// phi = 2 atan2(|v|, w) v / |v| after q -> -q where w < 0 (|phi| <= pi).  |v|^2 < 1e-4 w^2: the series of 2 atan(x) / x.
__device__ __forceinline__ void so3_log(const float* q, float* phi) {
  const float s = q[3] < 0.0f ? -1.0f : 1.0f;
  const float v[3] = {s * q[0], s * q[1], s * q[2]};
  const float w = s * q[3];
  const float n2 = dot3(v, v);
  float k;
  if (n2 < 1e-4f * (w * w)) {
    const float x2 = n2 / (w * w);
    k = (2.0f / w) * (1.0f - x2 * (1.0f / 3.0f) + x2 * x2 * (1.0f / 5.0f) - x2 * x2 * x2 * (1.0f / 7.0f));
  } else {
    const float n = sqrtf(n2);
    k = 2.0f * atan2f(n, w) / n;
  }
  phi[0] = k * v[0]; phi[1] = k * v[1]; phi[2] = k * v[2];
}

// t = V tau.  C by its series through th^6 for th^2 < 1e-2.
__device__ __forceinline__ void se3_exp(const float* a, float* t, float* q) {
  const float* tau = a;
  const float* phi = a + 3;
  const float im = so3_exp(phi, q);
  const float th2 = dot3(phi, phi);
  const float B = 2.0f * (im * im);
  float C;
  if (th2 < 1e-2f) {
    C = 1.0f / 6.0f - th2 * (1.0f / 120.0f) + th2 * th2 * (1.0f / 5040.0f) - th2 * th2 * th2 * (1.0f / 362880.0f);
  } else {
    const float th = sqrtf(th2);
    C = (th - sinf(th)) / (th2 * th);
  }
  float c1[3], c2[3];
  cross3(phi, tau, c1);
  cross3(phi, c1, c2);
  t[0] = tau[0] + B * c1[0] + C * c2[0];
  t[1] = tau[1] + B * c1[1] + C * c2[1];
  t[2] = tau[2] + B * c1[2] + C * c2[2];
}

// tau = V^-1 t.  D by its series through th^6 for th^2 < 1e-2.
__device__ __forceinline__ void se3_log(const float* t, const float* q, float* a) {
  float* tau = a;
  float* phi = a + 3;
  so3_log(q, phi);
  const float th2 = dot3(phi, phi);
  float D;
  if (th2 < 1e-2f) {
    D = 1.0f / 12.0f + th2 * (1.0f / 720.0f) + th2 * th2 * (1.0f / 30240.0f) + th2 * th2 * th2 * (1.0f / 1209600.0f);
  } else {
    const float h = 0.5f * sqrtf(th2);
    D = (1.0f - h * cosf(h) / sinf(h)) / th2;
  }
  float c1[3], c2[3];
  cross3(phi, t, c1);
  cross3(phi, c1, c2);
  tau[0] = t[0] - 0.5f * c1[0] + D * c2[0];
  tau[1] = t[1] - 0.5f * c1[1] + D * c2[1];
  tau[2] = t[2] - 0.5f * c1[2] + D * c2[2];
}

__device__ __forceinline__ void elem_mul(const float* tg, const float* qg, const float* th, const float* qh, float* t,
                                         float* q) {
  float r[3];
  act_so3(qg, th, r);
  t[0] = tg[0] + r[0]; t[1] = tg[1] + r[1]; t[2] = tg[2] + r[2];
  quat_mul(qg, qh, q);
}

// One thread per element.  a: the group element (INV, MUL, RETR, LOG, MATRIX) or the tangent (EXP); b: the second
// element (MUL) or the tangent (RETR).
template <int OP, int K>
__global__ __launch_bounds__(LIE_ELEM_THREADS) void lie_elem_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                                    float* __restrict__ out, int n) {
  constexpr int T = K == 7 ? 6 : 3;  // tangent size
  const int i = blockIdx.x * LIE_ELEM_THREADS + threadIdx.x;
  if (i >= n) return;
  float t[3], q[4], t2[3], q2[4], to[3], qo[4];
  if (OP == LIE_EXP) {
    float v[6];
    for (int m = 0; m < T; m++) v[m] = a[(size_t)i * T + m];
    if (K == 7) {
      se3_exp(v, to, qo);
    } else {
      so3_exp(v, qo);
    }
    store_elem<K>(out + (size_t)i * K, to, qo);
    return;
  }
  load_elem<K>(a + (size_t)i * K, t, q);
  if (OP == LIE_INV) {
    qo[0] = -q[0]; qo[1] = -q[1]; qo[2] = -q[2]; qo[3] = q[3];
    float r[3];
    act_so3(qo, t, r);
    to[0] = -r[0]; to[1] = -r[1]; to[2] = -r[2];
    store_elem<K>(out + (size_t)i * K, to, qo);
  } else if (OP == LIE_MUL) {
    load_elem<K>(b + (size_t)i * K, t2, q2);
    elem_mul(t, q, t2, q2, to, qo);
    store_elem<K>(out + (size_t)i * K, to, qo);
  } else if (OP == LIE_RETR) {  // exp(b) * a
    float v[6];
    for (int m = 0; m < T; m++) v[m] = b[(size_t)i * T + m];
    if (K == 7) {
      se3_exp(v, t2, q2);
    } else {
      so3_exp(v, q2);
      t2[0] = t2[1] = t2[2] = 0.0f;
    }
    elem_mul(t2, q2, t, q, to, qo);
    store_elem<K>(out + (size_t)i * K, to, qo);
  } else if (OP == LIE_LOG) {
    float v[6];
    if (K == 7) {
      se3_log(t, q, v);
    } else {
      so3_log(q, v);
    }
    for (int m = 0; m < T; m++) out[(size_t)i * T + m] = v[m];
  } else {  // LIE_MATRIX: [[R, t], [0, 1]] row-major, four 16-byte stores (out is 64-byte aligned per element)
    const float x = q[0], y = q[1], z = q[2], w = q[3];
    f32x4* M = reinterpret_cast<f32x4*>(out + (size_t)i * 16);
    M[0] = f32x4{1.0f - 2.0f * (y * y + z * z), 2.0f * (x * y - z * w), 2.0f * (x * z + y * w), t[0]};
    M[1] = f32x4{2.0f * (x * y + z * w), 1.0f - 2.0f * (x * x + z * z), 2.0f * (y * z - x * w), t[1]};
    M[2] = f32x4{2.0f * (x * z - y * w), 2.0f * (y * z + x * w), 1.0f - 2.0f * (x * x + y * y), t[2]};
    M[3] = f32x4{0.0f, 0.0f, 0.0f, 1.0f};
  }
}

// Group element of a row: row / g_div.  `narrow` (rows and g_div < 2^32, uniform over the launch) takes the 32-bit division.
__device__ __forceinline__ long long group_of(long long row, long long g_div, bool narrow) {
  return narrow ? (long long)((unsigned)row / (unsigned)g_div) : row / g_div;
}

// (X, Y, Z, W) -> (R XYZ + t W, W): one row = one 16-byte load and store per lane.
template <int K, bool VEC>
__global__ __launch_bounds__(LIE_THREADS) void lie_act4_kernel(const float* __restrict__ G, const float* __restrict__ in,
                                                               float* __restrict__ out, long long rows, long long g_div,
                                                               bool narrow) {
  const long long row = (long long)blockIdx.x * LIE_THREADS + threadIdx.x;
  if (row >= rows) return;
  float t[3], q[4];
  load_elem<K>(G + group_of(row, g_div, narrow) * K, t, q);
  f32x4 p;
  if (VEC) {
    p = reinterpret_cast<const f32x4*>(in)[row];
  } else {
    p = f32x4{in[row * 4], in[row * 4 + 1], in[row * 4 + 2], in[row * 4 + 3]};
  }
  const float X[3] = {p.x, p.y, p.z};
  float Y[3];
  act_so3(q, X, Y);
  const f32x4 r = {Y[0] + t[0] * p.w, Y[1] + t[1] * p.w, Y[2] + t[2] * p.w, p.w};
  if (VEC) {
    reinterpret_cast<f32x4*>(out)[row] = r;
  } else {
    out[row * 4] = r.x; out[row * 4 + 1] = r.y; out[row * 4 + 2] = r.z; out[row * 4 + 3] = r.w;
  }
}

// One row of the 12-float stream, in place in v (W floats).
template <int OP, int K>
__device__ __forceinline__ void stream_row(const float* t, const float* q, float* v) {
  if (OP == LIE_ACT3) {  // R p + t
    float Y[3];
    act_so3(q, v, Y);
    v[0] = Y[0] + t[0]; v[1] = Y[1] + t[1]; v[2] = Y[2] + t[2];
  } else if (K == 4) {  // SO3: Adj = R
    const float qc[4] = {-q[0], -q[1], -q[2], q[3]};
    float Y[3];
    act_so3(OP == LIE_ADJ ? q : qc, v, Y);
    v[0] = Y[0]; v[1] = Y[1]; v[2] = Y[2];
  } else if (OP == LIE_ADJ) {  // (R tau + t x (R phi), R phi)
    float rt[3], rp[3], c[3];
    act_so3(q, v, rt);
    act_so3(q, v + 3, rp);
    cross3(t, rp, c);
    v[0] = rt[0] + c[0]; v[1] = rt[1] + c[1]; v[2] = rt[2] + c[2];
    v[3] = rp[0]; v[4] = rp[1]; v[5] = rp[2];
  } else {  // Adj^T: (R^T tau, R^T (phi + tau x t))
    const float qc[4] = {-q[0], -q[1], -q[2], q[3]};
    float c[3], s[3], a[3], b[3];
    cross3(v, t, c);
    s[0] = v[3] + c[0]; s[1] = v[4] + c[1]; s[2] = v[5] + c[2];
    act_so3(qc, v, a);
    act_so3(qc, s, b);
    v[0] = a[0]; v[1] = a[1]; v[2] = a[2];
    v[3] = b[0]; v[4] = b[1]; v[5] = b[2];
  }
}

// A workgroup streams floats [base, base + 3072) of the operand through LDS; lane l owns floats 12 l .. 12 l + 11 of
// them = RPT whole rows (3072 is a multiple of the row width, so no row straddles lanes or workgroups).
template <int OP, int K, bool VEC>
__global__ __launch_bounds__(LIE_THREADS) void lie_stream12_kernel(const float* __restrict__ G, const float* __restrict__ in,
                                                                   float* __restrict__ out, long long rows, long long g_div,
                                                                   bool narrow) {
  constexpr int W = (OP != LIE_ACT3 && K == 7) ? 6 : 3;
  constexpr int RPT = LIE_CHUNK / W;
  __shared__ __attribute__((aligned(16))) float sh[LIE_BLOCK_FLOATS];
  const int tid = threadIdx.x;
  const long long base = (long long)blockIdx.x * LIE_BLOCK_FLOATS;
  const long long left = rows * W - base;
  const int cnt = left < LIE_BLOCK_FLOATS ? (int)left : LIE_BLOCK_FLOATS;
  if (VEC) {
#pragma unroll
    for (int j = 0; j < 3; j++) {
      const int idx = (tid + j * LIE_THREADS) * 4;
      if (idx + 3 < cnt) {
        *reinterpret_cast<f32x4*>(sh + idx) = *reinterpret_cast<const f32x4*>(in + base + idx);
      } else {
        for (int m = 0; m < 4; m++)
          if (idx + m < cnt) sh[idx + m] = in[base + idx + m];
      }
    }
  } else {
#pragma unroll
    for (int j = 0; j < LIE_CHUNK; j++) {
      const int idx = tid + j * LIE_THREADS;
      if (idx < cnt) sh[idx] = in[base + idx];
    }
  }
  __syncthreads();
  const long long row0 = base / W + (long long)tid * RPT;
  if (row0 < rows) {
    f32x4* mine = reinterpret_cast<f32x4*>(sh + tid * LIE_CHUNK);
    const f32x4 a0 = mine[0], a1 = mine[1], a2 = mine[2];
    float v[LIE_CHUNK] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w, a2.x, a2.y, a2.z, a2.w};
    long long have = -1;
    float t[3], q[4];
#pragma unroll
    for (int r = 0; r < RPT; r++) {
      if (row0 + r < rows) {  // rows past the end hold unstaged LDS: left alone, never stored
        const long long g = group_of(row0 + r, g_div, narrow);
        if (g != have) {
          load_elem<K>(G + g * K, t, q);
          have = g;
        }
        stream_row<OP, K>(t, q, v + r * W);
      }
    }
    mine[0] = f32x4{v[0], v[1], v[2], v[3]};
    mine[1] = f32x4{v[4], v[5], v[6], v[7]};
    mine[2] = f32x4{v[8], v[9], v[10], v[11]};
  }
  __syncthreads();
  if (VEC) {
#pragma unroll
    for (int j = 0; j < 3; j++) {
      const int idx = (tid + j * LIE_THREADS) * 4;
      if (idx + 3 < cnt) {
        *reinterpret_cast<f32x4*>(out + base + idx) = *reinterpret_cast<const f32x4*>(sh + idx);
      } else {
        for (int m = 0; m < 4; m++)
          if (idx + m < cnt) out[base + idx + m] = sh[idx + m];
      }
    }
  } else {
#pragma unroll
    for (int j = 0; j < LIE_CHUNK; j++) {
      const int idx = tid + j * LIE_THREADS;
      if (idx < cnt) out[base + idx] = sh[idx];
    }
  }
}

inline bool lie_aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// LGU_OK / an error to return at once, or -1 = launch.
inline int lie_elem_precheck(int group, int n) {
  if ((group != LGU_LIE_SO3 && group != LGU_LIE_SE3) || n < 0) return LGU_E_BADARG;
  return n == 0 ? LGU_OK : -1;
}

template <int OP>
int lie_elem_launch(int group, const float* a, const float* b, float* out, int n, void* stream) {
  const int nb = (n + LIE_ELEM_THREADS - 1) / LIE_ELEM_THREADS;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (group == LGU_LIE_SE3)
    hipLaunchKernelGGL((lie_elem_kernel<OP, 7>), dim3(nb), dim3(LIE_ELEM_THREADS), 0, s, a, b, out, n);
  else
    hipLaunchKernelGGL((lie_elem_kernel<OP, 4>), dim3(nb), dim3(LIE_ELEM_THREADS), 0, s, a, b, out, n);
  return launch_status();
}

inline int lie_bcast_precheck(int group, const float* G, long long ng, const float* in, long long rows, long long g_div,
                              const float* out, int width) {
  if (group != LGU_LIE_SO3 && group != LGU_LIE_SE3) return LGU_E_BADARG;
  if (rows < 0 || ng < 0 || g_div < 1) return LGU_E_BADARG;
  if (rows == 0) return LGU_OK;
  if (!G || !in || !out) return LGU_E_BADARG;
  if (rows > LLONG_MAX / 8 || (rows - 1) / g_div >= ng) return LGU_E_BADARG;  // a row would read past the group tensor
  const long long per_block = width == 4 ? LIE_THREADS : LIE_BLOCK_FLOATS / width;
  if ((rows + per_block - 1) / per_block > INT_MAX) return LGU_E_UNSUPPORTED;
  return -1;
}

template <int OP, int K>
void lie_stream12_launch(const float* G, const float* in, float* out, long long rows, long long g_div, hipStream_t s) {
  constexpr int W = (OP != LIE_ACT3 && K == 7) ? 6 : 3;
  const long long per_block = LIE_BLOCK_FLOATS / W;
  const unsigned nb = (unsigned)((rows + per_block - 1) / per_block);
  const bool narrow = rows <= 0xffffffffLL && g_div <= 0xffffffffLL;
  if (lie_aligned16(in) && lie_aligned16(out))
    hipLaunchKernelGGL((lie_stream12_kernel<OP, K, true>), dim3(nb), dim3(LIE_THREADS), 0, s, G, in, out, rows, g_div, narrow);
  else
    hipLaunchKernelGGL((lie_stream12_kernel<OP, K, false>), dim3(nb), dim3(LIE_THREADS), 0, s, G, in, out, rows, g_div, narrow);
}

template <int K>
void lie_act4_launch(const float* G, const float* in, float* out, long long rows, long long g_div, hipStream_t s) {
  const unsigned nb = (unsigned)((rows + LIE_THREADS - 1) / LIE_THREADS);
  const bool narrow = rows <= 0xffffffffLL && g_div <= 0xffffffffLL;
  if (lie_aligned16(in) && lie_aligned16(out))
    hipLaunchKernelGGL((lie_act4_kernel<K, true>), dim3(nb), dim3(LIE_THREADS), 0, s, G, in, out, rows, g_div, narrow);
  else
    hipLaunchKernelGGL((lie_act4_kernel<K, false>), dim3(nb), dim3(LIE_THREADS), 0, s, G, in, out, rows, g_div, narrow);
}

}  // namespace lgu

extern "C" {

int lgu_lie_inv_f32(int group, const float* G, int n, float* out, void* stream) {
  using namespace lgu;
  const int pre = lie_elem_precheck(group, n);
  if (pre >= 0) return pre;
  if (!G || !out) return LGU_E_BADARG;
  return lie_elem_launch<LIE_INV>(group, G, nullptr, out, n, stream);
}

int lgu_lie_mul_f32(int group, const float* G, const float* H, int n, float* out, void* stream) {
  using namespace lgu;
  const int pre = lie_elem_precheck(group, n);
  if (pre >= 0) return pre;
  if (!G || !H || !out) return LGU_E_BADARG;
  return lie_elem_launch<LIE_MUL>(group, G, H, out, n, stream);
}

int lgu_lie_retr_f32(int group, const float* G, const float* a, int n, float* out, void* stream) {
  using namespace lgu;
  const int pre = lie_elem_precheck(group, n);
  if (pre >= 0) return pre;
  if (!G || !a || !out) return LGU_E_BADARG;
  return lie_elem_launch<LIE_RETR>(group, G, a, out, n, stream);
}

int lgu_lie_exp_f32(int group, const float* a, int n, float* out, void* stream) {
  using namespace lgu;
  const int pre = lie_elem_precheck(group, n);
  if (pre >= 0) return pre;
  if (!a || !out) return LGU_E_BADARG;
  return lie_elem_launch<LIE_EXP>(group, a, nullptr, out, n, stream);
}

int lgu_lie_log_f32(int group, const float* G, int n, float* out, void* stream) {
  using namespace lgu;
  const int pre = lie_elem_precheck(group, n);
  if (pre >= 0) return pre;
  if (!G || !out) return LGU_E_BADARG;
  return lie_elem_launch<LIE_LOG>(group, G, nullptr, out, n, stream);
}

int lgu_lie_matrix_f32(int group, const float* G, int n, float* out, void* stream) {
  using namespace lgu;
  const int pre = lie_elem_precheck(group, n);
  if (pre >= 0) return pre;
  if (!G || !out) return LGU_E_BADARG;
  if (!lie_aligned16(out)) return LGU_E_UNSUPPORTED;
  return lie_elem_launch<LIE_MATRIX>(group, G, nullptr, out, n, stream);
}

int lgu_lie_act_f32(int group, const float* G, long long ng, const float* p, int width, long long rows, long long g_div,
                    float* out, void* stream) {
  using namespace lgu;
  if (width != 3 && width != 4) return LGU_E_BADARG;
  const int pre = lie_bcast_precheck(group, G, ng, p, rows, g_div, out, width);
  if (pre >= 0) return pre;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (width == 4) {
    if (group == LGU_LIE_SE3)
      lie_act4_launch<7>(G, p, out, rows, g_div, s);
    else
      lie_act4_launch<4>(G, p, out, rows, g_div, s);
  } else {
    if (group == LGU_LIE_SE3)
      lie_stream12_launch<LIE_ACT3, 7>(G, p, out, rows, g_div, s);
    else
      lie_stream12_launch<LIE_ACT3, 4>(G, p, out, rows, g_div, s);
  }
  return launch_status();
}

int lgu_lie_adj_f32(int group, const float* G, long long ng, const float* a, int transpose, long long rows, long long g_div,
                    float* out, void* stream) {
  using namespace lgu;
  if (transpose != 0 && transpose != 1) return LGU_E_BADARG;
  const int pre = lie_bcast_precheck(group, G, ng, a, rows, g_div, out, group == LGU_LIE_SE3 ? 6 : 3);
  if (pre >= 0) return pre;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (group == LGU_LIE_SE3) {
    if (transpose)
      lie_stream12_launch<LIE_ADJT, 7>(G, a, out, rows, g_div, s);
    else
      lie_stream12_launch<LIE_ADJ, 7>(G, a, out, rows, g_div, s);
  } else {
    if (transpose)
      lie_stream12_launch<LIE_ADJT, 4>(G, a, out, rows, g_div, s);
    else
      lie_stream12_launch<LIE_ADJ, 4>(G, a, out, rows, g_div, s);
  }
  return launch_status();
}

}  // extern "C"
