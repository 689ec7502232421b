// conv1.hip — the update operator's Conv2d(Cin, 128, 1) with its bias and an optional ReLU as float16 autocast evaluates
// it, 1 <= Cin <= 224 (reference droid_slam/droid_net.py: corr_encoder[0] = Conv2d(196, 128, 1) + ReLU, the consumer of
// the correlation lookup), NCHW in and NCHW out, in one launch:
//
//   x_h = half(x), w_h = half(weight), b_h = half(bias)            (round to nearest even; a half x is used as it is)
//   p   = sum_{c < Cin} x_h[c] * w_h[co,c]                          (exact products; fp32 accumulation from zero in seven
//                                                                    steps of 32 channels, kc = 0..6)
//   y   = act(half(b_h + p))                                        (one fp32 addition, one rounding; ReLU keeps a NaN)
//
// Mapping: the layer is the GEMM (pixels x 224) . (224 x 128) on v_mfma_f32_16x16x32_f16 with A = 16 pixels and
// B = 16 output channels of the packed weights (K padded to 224 with zero weights), so lane l = 16 g + p of an
// accumulator owns the four consecutive pixels 4 g + i of the channel 16 ct + p: one 8-byte store.  Wave q of a
// workgroup's four owns the channel tiles ct = 2 q, 2 q + 1 and keeps their 14 weight fragments (56 VGPRs) for all its
// pixel groups; two workgroups fit a CU.
//
// Pixels are numbered through the whole batch (gp = n * H * W + y * W + x); a group is 32 consecutive gp (two pixel tiles)
// and may span frames, every lane resolves its own pixels.  A workgroup takes a contiguous range of groups.  Per group
// thread (sp, so) = (tid & 31, tid >> 5) stages the pixel sp of the channel octets so, so + 8, so + 16 (and so + 24 for
// so < 4): 8 element loads per octet from the channel planes, 32 lanes along the pixels (a float row of a group is one
// 128-byte line), rounded to half, one 16-byte LDS store into the pixel's 448-byte channel row (pitch 464 bytes: the 16
// pixels of a ds_read_b128 lane group fall in 16 different 16-byte slots).  A channel >= Cin is never read: the load goes
// to channel Cin - 1 and the staged value is written as zero; an octet wholly >= Cin issues no load.  A pixel past the end
// re-reads the last pixel (its results are never stored).  The four waves then read their A fragments (lane: pixel p of
// the tile, channels 32 kc + 8 g ..+8) from the same staged group.  The LDS buffer is double: the loads of the next
// group are issued before the MFMAs of this one, one barrier per group.  No atomics, no workspace, no host
// synchronisation; the bits of a pixel depend on that pixel's Cin inputs only (MFMA rows are independent), not on N, the
// group or the grid.
#include <limits.h>

#include <type_traits>

#include "lgu_common.hpp"

namespace lgu {

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

constexpr int C1_CO = LGU_CONV1_COUT;
constexpr int C1_KB = LGU_CONV1_MAX_CIN / 32;      // K steps
constexpr int C1_OCT = LGU_CONV1_MAX_CIN / 8;      // channel octets of a staged pixel
constexpr int C1_THREADS = 256;
constexpr int C1_GROUP = 32;                       // pixels per staged group: two MFMA pixel tiles
constexpr int C1_SLOTS = (C1_OCT + 7) / 8;         // octets a staging thread may own
constexpr int C1_PITCH = 2 * LGU_CONV1_MAX_CIN + 16;   // bytes per staged pixel: 448 of channels + one 16-byte slot
constexpr int C1_BUF = C1_GROUP * C1_PITCH;        // one staged group

static_assert(LGU_CONV1_MAX_CIN % 32 == 0 && C1_CO == 128, "whole K steps; four waves of two channel tiles");
static_assert(LGU_CONV1_WPACK_HALVES == C1_KB * (C1_CO / 16) * kWave * 8, "weight pack size");
static_assert(C1_THREADS == C1_GROUP * 8, "thread = (pixel, octet mod 8)");
static_assert((C1_PITCH / 16) % 2 == 1, "an odd number of 16-byte slots per pixel: conflict-free fragment reads");

template <bool XH>
__global__ __launch_bounds__(C1_THREADS, 2) void conv1x1_o128_kernel(const void* __restrict__ xv, const f16x8* __restrict__ wpack,
                                                                     const _Float16* __restrict__ bias,
                                                                     _Float16* __restrict__ out, int Cin, int HW, int total,
                                                                     int groups, int per, int relu, int vec) {
  using XT = typename std::conditional<XH, _Float16, float>::type;
  __shared__ __attribute__((aligned(16))) unsigned char smem[2 * C1_BUF];
  const int g0 = blockIdx.x * per;
  const int g1 = g0 + per < groups ? g0 + per : groups;
  if (g0 >= g1) return;
  const int tid = threadIdx.x, lane = tid & (kWave - 1), q = tid >> 6;
  const int p = lane & 15, g = lane >> 4;

  // the wave's weight fragments and the lane's two bias values stay in registers for all its groups
  f16x8 bw[2][C1_KB];
#pragma unroll
  for (int t = 0; t < 2; t++)
#pragma unroll
    for (int kc = 0; kc < C1_KB; kc++) bw[t][kc] = wpack[(kc * (C1_CO / 16) + 2 * q + t) * kWave + lane];
  float bz[2];
#pragma unroll
  for (int t = 0; t < 2; t++) bz[t] = (float)bias[32 * q + 16 * t + p];

  // staging: thread = (pixel sp of the group, octets so + 8 k); every load has a valid address
  const int sp = tid & (C1_GROUP - 1), so = tid >> 5;
  const int noct = (Cin + 7) >> 3;
  const XT* xb = static_cast<const XT*>(xv);
  XT raw[C1_SLOTS][8] = {};
  // which halves of the thread's staged octets are channels < Cin, as bit masks of the octet's four dwords (kept as
  // values: per-element conditions would each hold a lane mask for the whole kernel)
  u32x4 live[C1_SLOTS];
#pragma unroll
  for (int k = 0; k < C1_SLOTS; k++) {
    const int nl = Cin - 8 * (so + 8 * k);   // channels of the octet below Cin (<= 0: none, >= 8: all)
#pragma unroll
    for (int d = 0; d < 4; d++) live[k][d] = nl >= 2 * d + 2 ? 0xffffffffu : (nl == 2 * d + 1 ? 0x0000ffffu : 0u);
  }
  auto load_group = [&](int grp) {
    int gp = C1_GROUP * grp + sp;
    gp = gp < total ? gp : total - 1;
    const int n = gp / HW, pi = gp - n * HW;
    const XT* src = xb + (size_t)n * Cin * HW + pi;
#pragma unroll
    for (int k = 0; k < C1_SLOTS; k++) {
      const int o = so + 8 * k;
      if (o < noct) {
#pragma unroll
        for (int ch = 0; ch < 8; ch++) {
          const int c = 8 * o + ch;
          raw[k][ch] = src[(size_t)(c < Cin ? c : Cin - 1) * HW];
        }
      }
    }
  };
  load_group(g0);

  for (int grp = g0; grp < g1; grp++) {
    unsigned char* buf = smem + ((grp - g0) & 1) * C1_BUF;
#pragma unroll
    for (int k = 0; k < C1_SLOTS; k++) {
      const int o = so + 8 * k;
      if (o < C1_OCT) {
        f16x8 v;
#pragma unroll
        for (int ch = 0; ch < 8; ch++) v[ch] = (_Float16)raw[k][ch];
        *reinterpret_cast<u32x4*>(buf + sp * C1_PITCH + 16 * o) = __builtin_bit_cast(u32x4, v) & live[k];
      }
    }
    // one barrier per group: the buffer written two groups later is this one, and a wave gets there only through the
    // next group's barrier, which every wave reaches after its reads of this group
    __syncthreads();
    if (grp + 1 < g1) load_group(grp + 1);

#pragma unroll
    for (int mt = 0; mt < 2; mt++) {
      f16x8 a[C1_KB];
#pragma unroll
      for (int kc = 0; kc < C1_KB; kc++)
        a[kc] = *reinterpret_cast<const f16x8*>(buf + (16 * mt + p) * C1_PITCH + 64 * kc + 16 * g);
      const int gpb = C1_GROUP * grp + 16 * mt + 4 * g;   // the lane's four pixels gpb .. gpb + 3
#pragma unroll
      for (int t = 0; t < 2; t++) {
        f32x4 acc = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int kc = 0; kc < C1_KB; kc++) acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(a[kc], bw[t][kc], acc, 0, 0, 0);
        f16x4 o;
#pragma unroll
        for (int i = 0; i < 4; i++) {
          const _Float16 h = (_Float16)(bz[t] + acc[i]);
          o[i] = (relu && h < (_Float16)0.0f) ? (_Float16)0.0f : h;   // a NaN compares false and is kept
        }
        const int co = 32 * q + 16 * t + p;
        if (vec) {   // H * W % 4 == 0 and out 8-byte aligned: the four pixels lie in one frame, in or out together
          if (gpb < total) {
            const int n = gpb / HW, pi = gpb - n * HW;
            *reinterpret_cast<f16x4*>(out + ((size_t)n * C1_CO + co) * HW + pi) = o;
          }
        } else {
#pragma unroll
          for (int i = 0; i < 4; i++) {
            const int gp = gpb + i;
            if (gp < total) {
              const int n = gp / HW, pi = gp - n * HW;
              out[((size_t)n * C1_CO + co) * HW + pi] = o[i];
            }
          }
        }
      }
    }
  }
}

static inline bool c1_aligned(const void* p, int n) { return (reinterpret_cast<uintptr_t>(p) % n) == 0; }

template <bool XH>
static int c1_launch(const lgu_conv1_args& a, int total, hipStream_t s) {
  const int HW = a.H * a.W;
  const int groups = (total + C1_GROUP - 1) / C1_GROUP;
  const int want = 2 * device_cu_count();
  const int per = (groups + want - 1) / want;
  const int blocks = (groups + per - 1) / per;
  const int vec = (HW % 4 == 0 && c1_aligned(a.out, 8)) ? 1 : 0;
  hipLaunchKernelGGL((conv1x1_o128_kernel<XH>), dim3(blocks), dim3(C1_THREADS), 0, s, a.x, static_cast<const f16x8*>(a.wpack),
                     static_cast<const _Float16*>(a.bias), static_cast<_Float16*>(a.out), a.Cin, HW, total, groups, per,
                     (a.flags & LGU_CONV1_RELU) ? 1 : 0, vec);
  return launch_status();
}

}  // namespace lgu

extern "C" int lgu_conv1x1_o128_h16(lgu_conv1_args a, void* stream) {
  using namespace lgu;
  if (a.N < 0 || a.H < 0 || a.W < 0 || (a.flags & ~(LGU_CONV1_X_HALF | LGU_CONV1_RELU))) return LGU_E_BADARG;
  if (a.N == 0 || a.H == 0 || a.W == 0) return LGU_OK;
  if (!a.x || !a.wpack || !a.bias || !a.out) return LGU_E_BADARG;
  const bool xh = (a.flags & LGU_CONV1_X_HALF) != 0;
  if (!c1_aligned(a.x, xh ? 2 : 4) || !c1_aligned(a.bias, 2) || !c1_aligned(a.out, 2)) return LGU_E_BADARG;
  if (a.Cin < 1 || a.Cin > LGU_CONV1_MAX_CIN) return LGU_E_UNSUPPORTED;
  if (!c1_aligned(a.wpack, 16)) return LGU_E_UNSUPPORTED;
  const long long total = (long long)a.N * a.H * a.W;
  if (total > INT_MAX - C1_GROUP) return LGU_E_UNSUPPORTED;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  return xh ? c1_launch<true>(a, (int)total, s) : c1_launch<false>(a, (int)total, s);
}
