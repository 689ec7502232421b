// encstats.hpp — exact per-plane statistics of IEEE half tensors as 64-bit integer sums, and the one (mean, rstd) function
// that every consumer of them shares (include/lgu_corr.h, "exact plane statistics").  csrc/encconv.hip emits the sums in its
// write-out and normalises with them in its staging loop; the stem and the output layer can take the same functions.
//
// A finite half h is m 2^(k-24) with integers 0 <= m < 2048 and 0 <= k <= 29 (k = max(e, 1) - 1 of the biased exponent e,
// m the significand with its hidden bit), so xi = h 2^24 = +-(m << k) is an integer below 2^40 and xi^2 = m^2 << 2k one below
// 2^80.  A plane's accumulator is four 64-bit words,
//   S1 = sum xi (two's complement),  LO = sum (xi^2 mod 2^40),  HI = sum (xi^2 >> 40),  BAD = number of non-finite values,
// each below 2^62 in magnitude for planes of at most 2^22 pixels.  Integer sums do not depend on their order: the words are
// exact for every schedule, tile and replica count.
#pragma once
#include "lgu_common.hpp"

namespace lgu {

#ifndef LGU_ES_REPLICAS
#define LGU_ES_REPLICAS 8
#endif
constexpr int ES_REPLICAS = LGU_ES_REPLICAS;   // R: slots per plane, slot = tile index mod R
constexpr int ES_WORDS = 4;                    // S1, LO, HI, BAD
constexpr long long ES_MAX_PLANE = 1LL << 22;  // pixels per plane the 64-bit words are proved for
static_assert(ES_REPLICAS == 1 || ES_REPLICAS == 2 || ES_REPLICAS == 4 || ES_REPLICAS == 8, "replicas");

struct EsSums {
  long long s1;
  unsigned long long lo, hi;
  unsigned bad;
};

__device__ __forceinline__ EsSums es_zero() { return EsSums{0, 0, 0, 0}; }

// add one stored half to a lane's partial sums
__device__ __forceinline__ void es_add(EsSums& s, _Float16 h) {
  const unsigned b = __builtin_bit_cast(unsigned short, h);
  const unsigned e = (b >> 10) & 31u, f = b & 1023u;
  if (e == 31u) {
    s.bad += 1u;
    return;
  }
  const unsigned m = e ? (f | 1024u) : f, k = e ? e - 1u : 0u;
  const long long xi = (long long)((unsigned long long)m << k);
  s.s1 += (b & 0x8000u) ? -xi : xi;
  const unsigned long long q = (unsigned long long)(m * m);   // below 2^22
  const unsigned sh = 2u * k;                                  // at most 58
  if (sh >= 40u) {
    s.hi += q << (sh - 40u);
  } else {
    const unsigned long long sq = q << sh;                     // below 2^61
    s.lo += sq & ((1ULL << 40) - 1ULL);
    s.hi += sq >> 40;
  }
}

// the sums of the LANES neighbouring lanes (a power of two, aligned) in every one of them
template <int LANES>
__device__ __forceinline__ void es_reduce(EsSums& s) {
#pragma unroll
  for (int m = LANES / 2; m >= 1; m >>= 1) {
    s.s1 += __shfl_xor(s.s1, m, kWave);
    s.lo += __shfl_xor(s.lo, m, kWave);
    s.hi += __shfl_xor(s.hi, m, kWave);
    s.bad += (unsigned)__shfl_xor((int)s.bad, m, kWave);
  }
}

// one workgroup's share of a plane into the plane's slot: integer vector-memory atomics (global_atomic_add_x2)
__device__ __forceinline__ void es_commit(unsigned long long* plane, int slot, const EsSums& s) {
  unsigned long long* q = plane + (size_t)slot * ES_WORDS;
  atomicAdd(q + 0, (unsigned long long)s.s1);
  atomicAdd(q + 1, s.lo);
  atomicAdd(q + 2, s.hi);
  if (s.bad) atomicAdd(q + 3, (unsigned long long)s.bad);
}

// (mean, rstd) of a plane of cnt pixels from its ES_REPLICAS slots: double arithmetic, every step rounded once, in the
// order of include/lgu_corr.h (the same lines in numpy give the same bits); BAD != 0 gives NaN for both
__device__ __forceinline__ void es_mean_rstd(const unsigned long long* plane, double cnt, float eps, float& mean, float& rstd) {
  long long s1 = 0;
  unsigned long long lo = 0, hi = 0, bad = 0;
#pragma unroll
  for (int r = 0; r < ES_REPLICAS; r++) {
    s1 += (long long)plane[r * ES_WORDS + 0];
    lo += plane[r * ES_WORDS + 1];
    hi += plane[r * ES_WORDS + 2];
    bad += plane[r * ES_WORDS + 3];
  }
  const double a = (double)s1;
  const double q = (double)(long long)hi * 1099511627776.0 + (double)(long long)lo;   // 2^40
  const double m = a / (cnt * 16777216.0);                                            // 2^24
  const double sq = a * a;
  const double d = q - sq / cnt;
  double var = d / (cnt * 281474976710656.0);                                         // 2^48
  var = var > 0.0 ? var : 0.0;
  const double rs = 1.0 / __builtin_sqrt(var + (double)eps);
  const float nan = __builtin_nanf("");
  mean = bad ? nan : (float)m;
  rstd = bad ? nan : (float)rs;
}

}  // namespace lgu
