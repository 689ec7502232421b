// graphsel.hip — the proximity edges of the factor graph (reference droid_slam/factor_graph.py:319-383,
// FactorGraph.add_proximity_factors) selected on the device, without a host round trip per candidate.
//
// Window: rows i in [t0, t), columns j in [t1, t), W = t - t1, cell (i, j) at flat index f = (i - t0) * W + (j - t1),
// n = (t - t0) * W cells, one float distance per cell.
//
// A cell is dead when i - rad < j, or d > 100, or it is a neighbourhood cell (j in [max(i - rad - 1, 0), i)), or the
// stereo diagonal (i == j), or it lies in the diamond |di| + |dj| <= max(min(|i - j| - 2, nms), 0) around a known edge
// or around an edge accepted earlier.  Live cells with d <= thresh are visited in ascending (d, f); a live one is
// accepted while len(edges) <= max_factors, appends (i, j), (j, i) and kills its diamond.  A NaN is never selected.
//
// Keys: 63 bits, (m(d) << 31) | f with m the order-preserving image of the float's bits (sign bit set for d >= +0, all
// bits flipped below; -0 counts as +0), so unsigned / non-negative signed order is (d, f) order.  Dead cells and cells
// above thresh get the sentinel INT64_MAX, which sorts last.
//
// Greedy pass (one wave): the sorted keys are taken 64 at a time.  Every lane holds one candidate and its live bit
// (valid key and not marked in the bitmap).  Loop: ballot the live lanes; the lowest one is accepted; every lane drops
// its own bit if its cell lies in the accepted diamond (arithmetic on registers); the lanes write the diamond's cells
// into the bitmap for the windows to come; lane 0 appends the two edges.  The pass ends at the first sentinel or when
// len(edges) > max_factors meets a live candidate.  Sequential depth: accepted edges + windows visited, not n.
#include <limits.h>

#include "lgu_common.hpp"

namespace lgu {

constexpr int GS_SMALL_MAX = LGU_PROXIMITY_SMALL_MAX;   // cells of the one-launch form (keys sorted in LDS)
constexpr long long GS_MAX_CELLS = 1ll << 24;
constexpr int GS_MAX_T = 1 << 30;
constexpr long long GS_MAX_PREFIX = 1ll << 30;           // count is an int: prefix + 2 n stays below 2^31
constexpr int GS_THREADS = 256;
constexpr int GS_LDS_WORDS = 16000;                     // bitmap words the sorted form keeps in LDS (512 000 cells)
constexpr unsigned long long GS_SENTINEL = 0x7fffffffffffffffull;
constexpr long long GS_FAR = 1ll << 40;                 // a known edge beyond this cannot reach any window

struct GsWin {
  int t, t0, t1, W, n, rad, nms, stereo;
  double thresh;
};

__device__ __forceinline__ int gs_radius(long long i, long long j, int nms) {
  long long a = (i > j ? i - j : j - i) - 2;
  if (a > nms) a = nms;
  return a > 0 ? (int)a : 0;
}

// S(x) = sum over k < x of min(m, k): neighbourhood edges (pairs) of the rows below x.
__host__ __device__ __forceinline__ long long gs_pairs_below(long long x, long long m) {
  return x <= m ? x * (x - 1) / 2 : m * (m - 1) / 2 + (x - m) * m;
}

__host__ __device__ __forceinline__ long long gs_row_offset(long long i, int t0, int rad, int stereo) {
  const long long m = (long long)rad + 1;
  return (stereo ? i - t0 : 0) + 2 * (gs_pairs_below(i, m) - gs_pairs_below(t0, m));
}

__device__ __forceinline__ bool gs_bit(const unsigned* bm, unsigned f) { return (bm[f >> 5] >> (f & 31)) & 1u; }

// Marks the cells of the diamond of radius r around (ci, cj) that fall inside the window; one thread walks it.
__device__ __forceinline__ void gs_mark_diamond(unsigned* bm, long long ci, long long cj, int r, const GsWin& w) {
  const long long ilo = ci - r > w.t0 ? ci - r : w.t0, ihi = ci + r < w.t - 1 ? ci + r : w.t - 1;
  for (long long i1 = ilo; i1 <= ihi; i1++) {
    const long long rem = r - (i1 > ci ? i1 - ci : ci - i1);
    const long long jlo = cj - rem > w.t1 ? cj - rem : w.t1, jhi = cj + rem < w.t - 1 ? cj + rem : w.t - 1;
    for (long long j1 = jlo; j1 <= jhi; j1++) {
      const unsigned f = (unsigned)((i1 - w.t0) * w.W + (j1 - w.t1));
      atomicOr(&bm[f >> 5], 1u << (f & 31));
    }
  }
}

__device__ __forceinline__ void gs_mark_known(unsigned* bm, const long long* kii, const long long* kjj, int e,
                                              const GsWin& w) {
  const long long i = kii[e], j = kjj[e];
  if (i > GS_FAR || i < -GS_FAR || j > GS_FAR || j < -GS_FAR) return;
  gs_mark_diamond(bm, i, j, gs_radius(i, j, w.nms), w);
}

// Key of cell f with distance d; `marked`: the cell lies in a known edge's diamond.
__device__ __forceinline__ unsigned long long gs_cell_key(unsigned f, float d, bool marked, const GsWin& w) {
  const int i = w.t0 + (int)(f / (unsigned)w.W), j = w.t1 + (int)(f % (unsigned)w.W);
  const int nb = i - w.rad - 1 > 0 ? i - w.rad - 1 : 0;
  const bool dead = marked || (i - w.rad < j) || (j >= nb && j < i) || (w.stereo && i == j);
  if (dead || !(d <= 100.0f) || !((double)d <= w.thresh)) return GS_SENTINEL;   // a NaN fails d <= 100
  if (d == 0.0f) d = 0.0f;                                                       // -0 orders as +0
  unsigned b = __float_as_uint(d);
  b = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
  return ((unsigned long long)b << 31) | f;
}

// The fixed prefix: for i = t0 .. t-1, (i, i) if stereo, then (i, j), (j, i) for j = max(i - rad - 1, 0) .. i - 1.
__device__ __forceinline__ void gs_write_prefix(const GsWin& w, long long* e_ii, long long* e_jj, int tid, int nt) {
  const long long m = (long long)w.rad + 1, items = (long long)(w.t - w.t0) * (m + 1);
  for (long long x = tid; x < items; x += nt) {
    const long long i = w.t0 + x / (m + 1), q = x % (m + 1);
    const long long off = gs_row_offset(i, w.t0, w.rad, w.stereo);
    if (q == m) {
      if (w.stereo) {
        e_ii[off] = i;
        e_jj[off] = i;
      }
      continue;
    }
    const long long cnt = m < i ? m : i;
    if (q >= cnt) continue;
    const long long j = i - cnt + q, o = off + (w.stereo ? 1 : 0) + 2 * q;
    e_ii[o] = i;
    e_jj[o] = j;
    e_ii[o + 1] = j;
    e_jj[o + 1] = i;
  }
}

// The greedy pass, run by the 64 lanes of one wave.  keys: sorted ascending (LDS or global), nkeys of them.  bm: the
// dead-cell bitmap with the known edges' diamonds marked; GLOBAL_BM: it lives in global memory (read past the L1,
// ordered by agent fences) instead of LDS.  len: the prefix length.
template <bool GLOBAL_BM>
__device__ __forceinline__ void gs_greedy(const unsigned long long* keys, int nkeys, unsigned* bm, const GsWin& w, long long len,
                                          long long max_factors, long long* e_ii, long long* e_jj, int* count) {
  const int lane = threadIdx.x & (kWave - 1);
  bool stop = false;
  unsigned long long next = lane < nkeys ? keys[lane] : GS_SENTINEL;
  for (int base = 0; base < nkeys && !stop; base += kWave) {
    const unsigned long long key = next;
    const int ahead = base + kWave + lane;
    next = ahead < nkeys ? keys[ahead] : GS_SENTINEL;   // the next window's keys travel while this one is worked
    const bool valid = key != GS_SENTINEL;
    const unsigned long long vbal = __ballot(valid);
    if (vbal == 0) break;
    stop = vbal != ~0ull;                               // a sentinel in this window: it is the last one
    const unsigned f = (unsigned)(key & 0x7fffffffull);
    int i = 0, j = 0;
    bool live = false;
    if (valid) {
      i = w.t0 + (int)(f / (unsigned)w.W);
      j = w.t1 + (int)(f % (unsigned)w.W);
      const unsigned word = GLOBAL_BM ? __hip_atomic_load(&bm[f >> 5], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
                                      : *reinterpret_cast<volatile unsigned*>(&bm[f >> 5]);
      live = !((word >> (f & 31)) & 1u);
    }
    for (;;) {
      const unsigned long long bal = __ballot(live);
      if (bal == 0) break;
      if (len > max_factors) {
        stop = true;
        break;
      }
      const int l = __ffsll((long long)bal) - 1;
      const int ai = __shfl(i, l, kWave), aj = __shfl(j, l, kWave);
      if (lane == 0) {
        e_ii[len] = ai;
        e_jj[len] = aj;
        e_ii[len + 1] = aj;
        e_jj[len + 1] = ai;
      }
      len += 2;
      const int r = gs_radius(ai, aj, w.nms);
      const int di = i > ai ? i - ai : ai - i, dj = j > aj ? j - aj : aj - j;
      if (di + dj <= r) live = false;                   // lane l itself: 0 <= r
      if (!stop) {                                      // later windows learn of the diamond through the bitmap
        const int ilo = ai - r > w.t0 ? ai - r : w.t0, ihi = ai + r < w.t - 1 ? ai + r : w.t - 1;
        const int jlo = aj - r > w.t1 ? aj - r : w.t1, jhi = aj + r < w.t - 1 ? aj + r : w.t - 1;
        const int bw = jhi - jlo + 1, cells = (ihi - ilo + 1) * bw;   // clipped to the window: <= n
        for (int k = lane; k < cells; k += kWave) {
          const int i1 = ilo + k / bw, j1 = jlo + k % bw;
          const int a = (i1 > ai ? i1 - ai : ai - i1) + (j1 > aj ? j1 - aj : aj - j1);
          if (a <= r) {
            const unsigned g = (unsigned)(i1 - w.t0) * (unsigned)w.W + (unsigned)(j1 - w.t1);
            atomicOr(&bm[g >> 5], 1u << (g & 31));
          }
        }
      }
    }
    // the marks of this window are read by other lanes in the next one
    if (GLOBAL_BM) __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "agent");
    else __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
  }
  if (lane == 0) *count = (int)len;
}

// ---- the one-launch form: n <= GS_SMALL_MAX ---------------------------------------------------------------------
// One workgroup of blockDim.x = max(64, P / 2) threads (<= 1024), P = the power of two >= max(n, 64): bitmap, keys,
// a bitonic sort of the P keys in LDS, the prefix and the greedy pass.
__global__ __launch_bounds__(1024) void proximity_small_kernel(const float* __restrict__ dist, const long long* __restrict__ kii,
                                                               const long long* __restrict__ kjj, int nk, GsWin w, int P,
                                                               long long max_factors, long long prefix,
                                                               long long* __restrict__ e_ii, long long* __restrict__ e_jj,
                                                               int* __restrict__ count) {
  __shared__ unsigned long long keys[GS_SMALL_MAX];
  __shared__ unsigned bm[GS_SMALL_MAX / 32];
  const int tid = threadIdx.x, nt = blockDim.x;
  for (int k = tid; k < GS_SMALL_MAX / 32; k += nt) bm[k] = 0u;
  __syncthreads();
  for (int e = tid; e < nk; e += nt) gs_mark_known(bm, kii, kjj, e, w);
  __syncthreads();
  for (int f = tid; f < P; f += nt) keys[f] = f < w.n ? gs_cell_key((unsigned)f, dist[f], gs_bit(bm, (unsigned)f), w) : GS_SENTINEL;
  __syncthreads();
  for (int k = 2; k <= P; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int x = tid; x < P / 2; x += nt) {
        const int a = ((x & ~(j - 1)) << 1) | (x & (j - 1)), b = a | j;
        const unsigned long long ka = keys[a], kb = keys[b];
        if ((ka > kb) == ((a & k) == 0)) {
          keys[a] = kb;
          keys[b] = ka;
        }
      }
      __syncthreads();
    }
  }
  gs_write_prefix(w, e_ii, e_jj, tid, nt);
  if (tid < kWave) gs_greedy<false>(keys, w.n, bm, w, prefix, max_factors, e_ii, e_jj, count);
}

// ---- the three-step form: any n --------------------------------------------------------------------------------
__global__ __launch_bounds__(GS_THREADS) void proximity_mark_kernel(const long long* __restrict__ kii, const long long* __restrict__ kjj,
                                                                    int nk, GsWin w, unsigned* __restrict__ bm) {
  const int e = blockIdx.x * GS_THREADS + threadIdx.x;
  if (e < nk) gs_mark_known(bm, kii, kjj, e, w);
}

// The bitmap is cleared by a kernel, not by hipMemsetAsync: recorded into a graph that call becomes a memset node, and a
// second replay of such a graph left other bytes than zero in `work` (tests/test_capture.py).
__global__ __launch_bounds__(GS_THREADS) void proximity_clear_kernel(unsigned* __restrict__ bm, int words) {
  const int k = blockIdx.x * GS_THREADS + threadIdx.x;
  if (k < words) bm[k] = 0u;
}

__global__ __launch_bounds__(GS_THREADS) void proximity_keys_kernel(const float* __restrict__ dist, const unsigned* __restrict__ bm,
                                                                    GsWin w, long long* __restrict__ keys) {
  const int f = blockIdx.x * GS_THREADS + threadIdx.x;
  if (f < w.n) keys[f] = (long long)gs_cell_key((unsigned)f, dist[f], gs_bit(bm, (unsigned)f), w);
}

template <bool GLOBAL_BM>
__global__ __launch_bounds__(GS_THREADS) void proximity_sorted_kernel(const long long* __restrict__ keys, unsigned* __restrict__ work,
                                                                      GsWin w, long long max_factors, long long prefix,
                                                                      long long* __restrict__ e_ii, long long* __restrict__ e_jj,
                                                                      int* __restrict__ count) {
  extern __shared__ unsigned lbm[];
  const int tid = threadIdx.x;
  if (!GLOBAL_BM) {
    const int words = (w.n + 31) / 32;
    for (int k = tid; k < words; k += GS_THREADS) lbm[k] = work[k];
  }
  gs_write_prefix(w, e_ii, e_jj, tid, GS_THREADS);
  __syncthreads();
  if (tid < kWave)
    gs_greedy<GLOBAL_BM>(reinterpret_cast<const unsigned long long*>(keys), w.n, GLOBAL_BM ? work : lbm, w, prefix, max_factors,
                         e_ii, e_jj, count);
}

// Argument rules shared by the entries; *n = cells of the window.
static int gs_check(int t, int t0, int t1, int rad, int nms, long long* n) {
  if (t < 0 || t1 < 0 || t1 > t0 || t0 > t || rad < 0 || nms < 0) return LGU_E_BADARG;
  const long long lim = (long long)t0 - rad - 1;
  if (t1 > (lim > 0 ? lim : 0)) return LGU_E_BADARG;
  if (t > GS_MAX_T) return LGU_E_UNSUPPORTED;
  *n = (long long)(t - t0) * (t - t1);
  return *n > GS_MAX_CELLS ? LGU_E_UNSUPPORTED : LGU_OK;
}

static GsWin gs_window(int t, int t0, int t1, int rad, int nms, double thresh, int stereo, long long n) {
  GsWin w;
  w.t = t;
  w.t0 = t0;
  w.t1 = t1;
  w.W = t - t1;
  w.n = (int)n;
  w.rad = rad < t ? rad : t;   // every rad >= t selects what rad = t selects
  w.nms = nms;
  w.stereo = stereo ? 1 : 0;
  w.thresh = thresh;
  return w;
}

static long long gs_prefix(int t, int t0, int rad, int stereo) { return gs_row_offset(t, t0, rad < t ? rad : t, stereo ? 1 : 0); }

// The final length is <= max(prefix, max_factors + 2) and, every cell accepted at most once, <= prefix + 2 n.
static long long gs_capacity(long long prefix, long long max_factors, long long n) {
  const long long a = max_factors >= 0 && max_factors + 2 > prefix ? max_factors + 2 : prefix;
  return a < prefix + 2 * n ? a : prefix + 2 * n;
}

}  // namespace lgu

extern "C" {

long long lgu_proximity_prefix_len(int t, int t0, int rad, int stereo) {
  if (t < 0 || t0 < 0 || t0 > t || rad < 0) return -1;
  return lgu::gs_prefix(t, t0, rad, stereo);
}

long long lgu_proximity_capacity(int t, int t0, int t1, int rad, int stereo, long long max_factors) {
  const long long p = lgu_proximity_prefix_len(t, t0, rad, stereo);
  if (p < 0 || t1 < 0 || t1 > t0 || max_factors > LLONG_MAX - 2) return -1;
  return lgu::gs_capacity(p, max_factors, (long long)(t - t0) * (t - t1));
}

long long lgu_proximity_work_bytes(int t, int t0, int t1) {
  if (t < 0 || t1 < 0 || t1 > t0 || t0 > t) return -1;
  const long long n = (long long)(t - t0) * (t - t1);
  return n > lgu::GS_MAX_CELLS ? -1 : 4 * ((n + 31) / 32);
}

int lgu_proximity_select_small(const float* dist, const long long* known_ii, const long long* known_jj, int num_known, int t,
                               int t0, int t1, int rad, int nms, double thresh, long long max_factors, int stereo,
                               long long* e_ii, long long* e_jj, long long capacity, int* count, void* stream) {
  using namespace lgu;
  long long n = 0;
  const int rc = gs_check(t, t0, t1, rad, nms, &n);
  if (rc != LGU_OK) return rc;
  if (n > GS_SMALL_MAX) return LGU_E_UNSUPPORTED;
  if (num_known < 0 || max_factors > LLONG_MAX - 2 || !count) return LGU_E_BADARG;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (n == 0) {   // no rows: the prefix is empty
    hipLaunchKernelGGL(proximity_clear_kernel, dim3(1), dim3(GS_THREADS), 0, st, reinterpret_cast<unsigned*>(count), 1);
    return launch_status();
  }
  const long long prefix = gs_prefix(t, t0, rad, stereo);
  if (prefix > GS_MAX_PREFIX || capacity < gs_capacity(prefix, max_factors, n)) return LGU_E_BADARG;
  if (!dist || !e_ii || !e_jj || (num_known > 0 && (!known_ii || !known_jj))) return LGU_E_BADARG;
  int P = kWave;
  while (P < n) P <<= 1;
  const int threads = P / 2 < kWave ? kWave : (P / 2 > 1024 ? 1024 : P / 2);
  hipLaunchKernelGGL(proximity_small_kernel, dim3(1), dim3(threads), 0, st, dist, known_ii, known_jj, num_known,
                     gs_window(t, t0, t1, rad, nms, thresh, stereo, n), P, max_factors, prefix, e_ii, e_jj, count);
  return launch_status();
}

int lgu_proximity_keys(const float* dist, const long long* known_ii, const long long* known_jj, int num_known, int t, int t0,
                       int t1, int rad, int nms, double thresh, int stereo, long long* keys, void* work, void* stream) {
  using namespace lgu;
  long long n = 0;
  const int rc = gs_check(t, t0, t1, rad, nms, &n);
  if (rc != LGU_OK) return rc;
  if (num_known < 0) return LGU_E_BADARG;
  if (n == 0) return LGU_OK;
  if (!dist || !keys || !work || (num_known > 0 && (!known_ii || !known_jj))) return LGU_E_BADARG;
  if ((reinterpret_cast<uintptr_t>(work) & 3) != 0) return LGU_E_BADARG;  // the bitmap is read and or-ed as 32-bit words
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const GsWin w = gs_window(t, t0, t1, rad, nms, thresh, stereo, n);
  const int words = (int)((n + 31) / 32);   // n <= GS_MAX_CELLS = 2^24
  hipLaunchKernelGGL(proximity_clear_kernel, dim3((unsigned)((words + GS_THREADS - 1) / GS_THREADS)), dim3(GS_THREADS), 0, st,
                     reinterpret_cast<unsigned*>(work), words);
  const int rz = launch_status();
  if (rz != LGU_OK) return rz;
  if (num_known > 0) {
    hipLaunchKernelGGL(proximity_mark_kernel, dim3((num_known + GS_THREADS - 1) / GS_THREADS), dim3(GS_THREADS), 0, st, known_ii,
                       known_jj, num_known, w, reinterpret_cast<unsigned*>(work));
    const int rm = launch_status();
    if (rm != LGU_OK) return rm;
  }
  hipLaunchKernelGGL(proximity_keys_kernel, dim3((unsigned)((n + GS_THREADS - 1) / GS_THREADS)), dim3(GS_THREADS), 0, st, dist,
                     reinterpret_cast<const unsigned*>(work), w, keys);
  return launch_status();
}

int lgu_proximity_select_sorted(const long long* sorted_keys, void* work, int t, int t0, int t1, int rad, int nms,
                                long long max_factors, int stereo, long long* e_ii, long long* e_jj, long long capacity,
                                int* count, void* stream) {
  using namespace lgu;
  long long n = 0;
  const int rc = gs_check(t, t0, t1, rad, nms, &n);
  if (rc != LGU_OK) return rc;
  if (max_factors > LLONG_MAX - 2 || !count) return LGU_E_BADARG;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (n == 0) {
    hipLaunchKernelGGL(proximity_clear_kernel, dim3(1), dim3(GS_THREADS), 0, st, reinterpret_cast<unsigned*>(count), 1);
    return launch_status();
  }
  const long long prefix = gs_prefix(t, t0, rad, stereo);
  if (prefix > GS_MAX_PREFIX || capacity < gs_capacity(prefix, max_factors, n)) return LGU_E_BADARG;
  if (!sorted_keys || !work || !e_ii || !e_jj) return LGU_E_BADARG;
  if ((reinterpret_cast<uintptr_t>(work) & 3) != 0) return LGU_E_BADARG;  // 32-bit words, as lgu_proximity_keys left them
  const GsWin w = gs_window(t, t0, t1, rad, nms, 0.0, stereo, n);
  const long long words = (n + 31) / 32;
  if (words <= GS_LDS_WORDS)
    hipLaunchKernelGGL(proximity_sorted_kernel<false>, dim3(1), dim3(GS_THREADS), (size_t)words * 4, st, sorted_keys,
                       reinterpret_cast<unsigned*>(work), w, max_factors, prefix, e_ii, e_jj, count);
  else
    hipLaunchKernelGGL(proximity_sorted_kernel<true>, dim3(1), dim3(GS_THREADS), 0, st, sorted_keys,
                       reinterpret_cast<unsigned*>(work), w, max_factors, prefix, e_ii, e_jj, count);
  return launch_status();
}

}  // extern "C"
