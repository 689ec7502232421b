// conv3.hip — the update operator's Conv2d(128, 64 | 128, 3, padding=1) with its bias and an optional ReLU, as it is
// evaluated under float16 autocast (reference droid_slam/droid_net.py: corr_encoder[2], flow_encoder[2], delta[0],
// weight[0], agg.conv1, agg.conv2), NCHW in and NCHW out, in one launch:
//
//   x_h = half(x), w_h = half(weight), b_h = half(bias)            (round to nearest even; a half x is used as it is)
//   s   = b_h + sum_{c,ky,kx} x_h[c, y+ky-1, x+kx-1] * w_h[co,c,ky,kx]   (exact products, fp32 accumulation, zero padding)
//   y   = act(half(s))                                             (one rounding; ReLU keeps a NaN)
//
// An implicit GEMM on the matrix cores (v_mfma_f32_16x16x32_f16): M = 16 pixels along x, N = 16 output channels, K = 9
// taps x 128 channels = 36 steps of 32 channels of one tap, always in the order tap-major (ky, kx), then channel block:
// an output element's bits depend on its own image only, not on the tile, the batch or N.
//
// Workgroup: 4 waves, an image tile of C3_TXM x 16 pixels by TY rows (8 MFMA pixel tiles: 64 x 2 or 32 x 4, chosen per
// call by the smaller padded area), all output channels.  The tile with its 1-pixel halo is staged in LDS as half,
// channel-last: a thread reads one pixel of 8 channel planes (lanes along x, so each plane's load is contiguous) and
// writes one 16-byte piece of the pixel's 256-byte channel row.  The +-1 shifts of the window are then whole-row shifts
// of the A fragment's address (lane l: pixel l & 15, channels 32 kc + 8 (l >> 4) ..+8, one ds_read_b128).  The pixel pitch
// is 272 bytes: the 16 pixels of a 16-lane read group fall in 16 different 16-byte slots of the 256-byte bank row.
// Wave w owns pixel tiles [4 (w >> 1), +4) and channels [Cout/2 (w & 1), +Cout/2): per K step 4 A fragments from LDS and
// Cout/32 B fragments of the packed weights from global memory (prefetched six steps ahead) feed Cout/8 MFMAs.  The
// accumulators start at the bias.  The result goes back through LDS as [channel][pixel] so that a store instruction
// writes 64- or 128-byte runs of a channel's row, 16 bytes per lane (or by element where out or W do not allow).
// No atomics, no workspace, no host synchronisation.
//
// conv3x3_fanout_c128_kernel runs two or three such 128 -> 128 layers of ONE input (delta[0], weight[0], agg.conv1 behind
// the GRU) in one launch: the same staging once, then the same K loop per group.  The phases are device functions shared
// by both kernels, so an output of the fan-out has the bits of the single layer.
#include <limits.h>

#include <type_traits>

#include "lgu_common.hpp"

namespace lgu {

constexpr int C3_CI = 128;                 // input channels
constexpr int C3_THREADS = 256;
constexpr int C3_PITCH = 2 * C3_CI + 16;   // bytes per staged pixel: 256 of channels + one 16-byte slot
constexpr int C3_MT = 8;                   // MFMA pixel tiles per workgroup
constexpr int C3_OPITCH = 2 * 16 * C3_MT + 16;   // bytes per channel of the output image in LDS
// experiments only (variant builds): the depth of the weight prefetch in K steps, the staging items whose
// loads a thread issues before it converts and writes any of them, and a forced tile (4: 64 x 2, 2: 32 x 4); every
// setting computes the same bits
#ifndef LGU_C3_PF
#define LGU_C3_PF 6
#endif
#ifndef LGU_C3_SU
#define LGU_C3_SU 6
#endif
#ifndef LGU_C3_FORCE_TXM
#define LGU_C3_FORCE_TXM 0
#endif
constexpr int C3_PF = LGU_C3_PF, C3_SU = LGU_C3_SU;
static_assert(C3_PF >= 1 && C3_PF <= 8 && C3_SU >= 1 && C3_SU <= 8, "prefetch depth and staging batch");

static_assert(LGU_CONV3_WPACK_HALVES_128 == 9 * 4 * (128 / 16) * kWave * 8, "weight pack size, Cout 128");
static_assert(LGU_CONV3_WPACK_HALVES_64 == 9 * 4 * (64 / 16) * kWave * 8, "weight pack size, Cout 64");

template <int TXM>
constexpr int c3_lds_bytes() {
  return (C3_MT / TXM + 2) * (16 * TXM + 2) * C3_PITCH;
}

// ---- the three phases every kernel of this file is made of.  They are shared, not copied: an output element's bits are
// those of c3_mma's order and nothing else.
// the first C3_PF K steps' weight fragments of a wave (wp: the pack at the wave's first channel tile and lane)
template <int NCT, int CTS>
__device__ __forceinline__ void c3_prefetch(const f16x8* __restrict__ wp, f16x8 (&bf)[C3_PF][NCT]) {
#pragma unroll
  for (int s = 0; s < C3_PF; s++)
#pragma unroll
    for (int ct = 0; ct < NCT; ct++) bf[s][ct] = wp[((size_t)s * CTS + ct) * kWave];
}

// stage: one (channel octet, row, pixel) per thread and item, lanes along x; the loads of C3_SU items are issued before
// the first of them is converted and written (a pixel outside the image re-reads the image's first pixel and is then
// zeroed: every load is unconditional)
template <int TXM, typename XT>
__device__ __forceinline__ void c3_stage(unsigned char* smem, const XT* __restrict__ src, int y0, int x0, int H, int W, size_t HW,
                                         int tid) {
  constexpr int TX = 16 * TXM, TY = C3_MT / TXM;
  constexpr int LW = TX + 2, LH = TY + 2;
  constexpr int ITEMS = 16 * LH * LW;
  for (int base = tid; base < ITEMS; base += C3_SU * C3_THREADS) {
    XT raw[C3_SU][8];
    bool inside[C3_SU];
#pragma unroll
    for (int u = 0; u < C3_SU; u++) {
      const int idx = base + u * C3_THREADS;
      const int c = idx % LW, t = idx / LW;
      const int r = t % LH, o = t / LH;
      const int gy = y0 + r - 1, gx = x0 + c - 1;
      inside[u] = idx < ITEMS && in_bounds(gy, gx, H, W);
      const XT* q = src + (inside[u] ? (size_t)(8 * o) * HW + (size_t)gy * W + gx : (size_t)0);
#pragma unroll
      for (int ch = 0; ch < 8; ch++) raw[u][ch] = q[ch * HW];
    }
#pragma unroll
    for (int u = 0; u < C3_SU; u++) {
      const int idx = base + u * C3_THREADS;
      if (idx < ITEMS) {
        const int c = idx % LW, t = idx / LW;
        const int r = t % LH;
        f16x8 v;
#pragma unroll
        for (int ch = 0; ch < 8; ch++) v[ch] = inside[u] ? (_Float16)raw[u][ch] : (_Float16)0.0f;
        *reinterpret_cast<f16x8*>(smem + (r * LW + c) * C3_PITCH + 16 * (t / LH)) = v;
      }
    }
  }
}

// the 36 K steps of a wave's 4 pixel tiles x NCT channel tiles, from the bias: tap-major (ky, kx), then channel block.
// bf holds the fragments of steps 0 .. C3_PF - 1 on entry and is used up on return.
template <int NCT, int CTS, int TXM>
__device__ __forceinline__ void c3_mma(const unsigned char* abase, const f16x8* __restrict__ wp, f16x8 (&bf)[C3_PF][NCT],
                                       const float (&bz)[NCT], int wr, f32x4 (&acc)[4][NCT]) {
  constexpr int LW = 16 * TXM + 2;
#pragma unroll
  for (int m = 0; m < 4; m++)
#pragma unroll
    for (int ct = 0; ct < NCT; ct++) acc[m][ct] = f32x4{bz[ct], bz[ct], bz[ct], bz[ct]};
#pragma unroll
  for (int s = 0; s < 36; s++) {
    const int tap = s >> 2, kc = s & 3, ky = tap / 3, kx = tap % 3;
    f16x8 bw[NCT];
#pragma unroll
    for (int ct = 0; ct < NCT; ct++) bw[ct] = bf[s % C3_PF][ct];
    if (s + C3_PF < 36) {   // the slot just read takes the fragments of step s + C3_PF
#pragma unroll
      for (int ct = 0; ct < NCT; ct++) bf[s % C3_PF][ct] = wp[((size_t)(s + C3_PF) * CTS + ct) * kWave];
    }
    f16x8 a[4];
#pragma unroll
    for (int m = 0; m < 4; m++) {
      const int mt = 4 * wr + m, row = mt / TXM, mtx = mt % TXM;   // wr is wave-uniform: the offset is one select
      a[m] = *reinterpret_cast<const f16x8*>(abase + ((row + ky) * LW + 16 * mtx + kx) * C3_PITCH + 64 * kc);
    }
#pragma unroll
    for (int m = 0; m < 4; m++)
#pragma unroll
      for (int ct = 0; ct < NCT; ct++)
        acc[m][ct] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a[m], bw[ct], acc[m][ct], 0, 0, 0);
  }
}

// one rounding to half, then the ReLU (a NaN compares false and is kept)
__device__ __forceinline__ f16x4 c3_round(const f32x4& v, int relu) {
  f16x4 o;
#pragma unroll
  for (int i = 0; i < 4; i++) {
    const _Float16 h = (_Float16)v[i];
    o[i] = (relu && h < (_Float16)0.0f) ? (_Float16)0.0f : h;
  }
  return o;
}

template <int COUT, int TXM, bool XH>
__global__ __launch_bounds__(C3_THREADS) void conv3x3_c128_kernel(const void* __restrict__ xv, const f16x8* __restrict__ wpack,
                                                                 const _Float16* __restrict__ bias,
                                                                 _Float16* __restrict__ out, int H, int W, int tiles_x,
                                                                 int tiles_y, int relu, int vec) {
  using XT = typename std::conditional<XH, _Float16, float>::type;
  constexpr int TX = 16 * TXM, TY = C3_MT / TXM;
  constexpr int LW = TX + 2, LH = TY + 2;
  constexpr int NCT = COUT / 32;           // channel tiles per wave
  constexpr int CTS = COUT / 16;           // channel tiles in the pack
  static_assert(COUT * C3_OPITCH <= LH * LW * C3_PITCH, "the output image reuses the input tile's LDS");
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];

  int b = blockIdx.x;
  const int x0 = (b % tiles_x) * TX;
  b /= tiles_x;
  const int y0 = (b % tiles_y) * TY;
  const int n = b / tiles_y;
  const int tid = threadIdx.x, lane = tid & (kWave - 1), w = tid >> 6;
  const int p = lane & 15, g = lane >> 4;
  const int wr = w >> 1, wc = w & 1;
  const size_t HW = (size_t)H * W;

  // the wave's first weight fragments and its bias are in flight while the tile is staged
  const f16x8* wp = wpack + (size_t)(wc * NCT) * kWave + lane;
  f16x8 bf[C3_PF][NCT];
  c3_prefetch<NCT, CTS>(wp, bf);
  float bz[NCT];
#pragma unroll
  for (int ct = 0; ct < NCT; ct++) bz[ct] = (float)bias[wc * 16 * NCT + 16 * ct + p];

  c3_stage<TXM, XT>(smem, static_cast<const XT*>(xv) + (size_t)n * C3_CI * HW, y0, x0, H, W, HW, tid);
  __syncthreads();

  f32x4 acc[4][NCT];
  c3_mma<NCT, CTS, TXM>(smem + p * C3_PITCH + 16 * g, wp, bf, bz, wr, acc);
  __syncthreads();   // every wave has read its last A fragment: the tile's LDS becomes the output image

  // [channel][pixel tile][16 pixels] half; a lane's four accumulators are four consecutive pixels of one channel
#pragma unroll
  for (int m = 0; m < 4; m++)
#pragma unroll
    for (int ct = 0; ct < NCT; ct++) {
      const int co = wc * 16 * NCT + 16 * ct + p, mt = 4 * wr + m;
      *reinterpret_cast<f16x4*>(smem + co * C3_OPITCH + 2 * (16 * mt + 4 * g)) = c3_round(acc[m][ct], relu);
    }
  __syncthreads();

  // pixel tile mt = row * TXM + mtx, so a channel's 16 * C3_MT pixels are its TY rows of TX pixels in order
  _Float16* dst = out + (size_t)n * COUT * HW;
  for (int idx = tid; idx < COUT * TY * (TX / 8); idx += C3_THREADS) {
    const int ch8 = idx % (TX / 8), t = idx / (TX / 8);
    const int row = t % TY, co = t / TY;
    const int y = y0 + row, xo = x0 + 8 * ch8;
    if (y >= H || xo >= W) continue;
    const f16x8 v = *reinterpret_cast<const f16x8*>(smem + co * C3_OPITCH + 2 * (row * TX + 8 * ch8));
    _Float16* q = dst + (size_t)co * HW + (size_t)y * W + xo;
    if (vec) {
      *reinterpret_cast<f16x8*>(q) = v;   // W % 8 == 0 and out 16-byte aligned: eight pixels in or out together
    } else {
#pragma unroll
      for (int i = 0; i < 8; i++)
        if (xo + i < W) q[i] = v[i];
    }
  }
}

// ---- fan-out: G = 2 or 3 convolutions 128 -> 128 of ONE input.  The tile is staged once; each group then takes its own
// 36 K steps (c3_mma, so output g has the bits of conv3x3_c128_kernel with pack g) and is stored straight from the
// accumulators, because the tile must survive to the last group: a lane's four accumulators are four consecutive pixels
// of one channel, one 8-byte store where W % 4 == 0 and the outputs are 8-byte aligned, by element otherwise.  The next
// group's first weight fragments are in flight while a group is stored.
struct C3FanOperands {
  const f16x8* wpack[3];
  const _Float16* bias[3];
  _Float16* out[3];
};

template <int TXM, bool XH>
__global__ __launch_bounds__(C3_THREADS, 2) void conv3x3_fanout_c128_kernel(const void* __restrict__ xv, C3FanOperands ops, int G,
                                                                        int H, int W, int tiles_x, int tiles_y, int relu,
                                                                        int vec) {
  using XT = typename std::conditional<XH, _Float16, float>::type;
  constexpr int COUT = 128, NCT = COUT / 32, CTS = COUT / 16;
  constexpr int TX = 16 * TXM, TY = C3_MT / TXM;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];

  int b = blockIdx.x;
  const int x0 = (b % tiles_x) * TX;
  b /= tiles_x;
  const int y0 = (b % tiles_y) * TY;
  const int n = b / tiles_y;
  const int tid = threadIdx.x, lane = tid & (kWave - 1), w = tid >> 6;
  const int p = lane & 15, g = lane >> 4;
  const int wr = w >> 1, wc = w & 1;
  const size_t HW = (size_t)H * W;
  const size_t woff = (size_t)(wc * NCT) * kWave + lane;

  f16x8 bf[C3_PF][NCT];
  c3_prefetch<NCT, CTS>(ops.wpack[0] + woff, bf);
  c3_stage<TXM, XT>(smem, static_cast<const XT*>(xv) + (size_t)n * C3_CI * HW, y0, x0, H, W, HW, tid);
  __syncthreads();

#pragma unroll 1
  for (int grp = 0; grp < G; grp++) {
    // the staged tile does not change between the groups, and the compiler knows it: without this it hoists all 144 A
    // fragments of the K loop (576 registers) out of the group loop and spills them
    asm volatile("" ::: "memory");
    // block-uniform selects of kernel arguments: no indexed private array
    const f16x8* wp = (grp == 0 ? ops.wpack[0] : grp == 1 ? ops.wpack[1] : ops.wpack[2]) + woff;
    const _Float16* bias = grp == 0 ? ops.bias[0] : grp == 1 ? ops.bias[1] : ops.bias[2];
    _Float16* dst = (grp == 0 ? ops.out[0] : grp == 1 ? ops.out[1] : ops.out[2]) + (size_t)n * COUT * HW;
    float bz[NCT];
#pragma unroll
    for (int ct = 0; ct < NCT; ct++) bz[ct] = (float)bias[wc * 16 * NCT + 16 * ct + p];
    f32x4 acc[4][NCT];
    c3_mma<NCT, CTS, TXM>(smem + p * C3_PITCH + 16 * g, wp, bf, bz, wr, acc);
    if (grp + 1 < G) c3_prefetch<NCT, CTS>((grp == 0 ? ops.wpack[1] : ops.wpack[2]) + woff, bf);
#pragma unroll
    for (int m = 0; m < 4; m++) {
      const int mt = 4 * wr + m, row = mt / TXM, mtx = mt % TXM;
      const int y = y0 + row, xo = x0 + 16 * mtx + 4 * g;
      if (y >= H || xo >= W) continue;
#pragma unroll
      for (int ct = 0; ct < NCT; ct++) {
        const f16x4 o = c3_round(acc[m][ct], relu);
        _Float16* q = dst + (size_t)(wc * 16 * NCT + 16 * ct + p) * HW + (size_t)y * W + xo;
        if (vec) {
          *reinterpret_cast<f16x4*>(q) = o;   // W % 4 == 0 and out 8-byte aligned: four pixels in or out together
        } else {
#pragma unroll
          for (int i = 0; i < 4; i++)
            if (xo + i < W) q[i] = o[i];
        }
      }
    }
  }
}

static inline bool c3_aligned(const void* p, int n) { return (reinterpret_cast<uintptr_t>(p) % n) == 0; }

template <int COUT, int TXM, bool XH>
static int c3_launch(const lgu_conv3_args& a, hipStream_t s) {
  constexpr int TX = 16 * TXM, TY = C3_MT / TXM;
  const int tiles_x = (a.W - 1) / TX + 1, tiles_y = (a.H - 1) / TY + 1;
  const long long blocks = (long long)a.N * tiles_x * tiles_y;
  if (blocks > INT_MAX) return LGU_E_UNSUPPORTED;
  auto kern = conv3x3_c128_kernel<COUT, TXM, XH>;
  if (allow_max_dynamic_lds<conv3x3_c128_kernel<COUT, TXM, XH>>() != hipSuccess) return launch_status();
  const int vec = (a.W % 8 == 0 && c3_aligned(a.out, 16)) ? 1 : 0;
  hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(C3_THREADS), c3_lds_bytes<TXM>(), s, a.x,
                     static_cast<const f16x8*>(a.wpack), static_cast<const _Float16*>(a.bias), static_cast<_Float16*>(a.out),
                     a.H, a.W, tiles_x, tiles_y, (a.flags & LGU_CONV3_RELU) ? 1 : 0, vec);
  return launch_status();
}

template <int COUT, int TXM>
static int c3_launch_x(const lgu_conv3_args& a, hipStream_t s) {
  return (a.flags & LGU_CONV3_X_HALF) ? c3_launch<COUT, TXM, true>(a, s) : c3_launch<COUT, TXM, false>(a, s);
}

template <int TXM, bool XH>
static int c3_fan_launch(const lgu_conv3_fanout_args& a, hipStream_t s) {
  constexpr int TX = 16 * TXM, TY = C3_MT / TXM;
  const int tiles_x = (a.W - 1) / TX + 1, tiles_y = (a.H - 1) / TY + 1;
  const long long blocks = (long long)a.N * tiles_x * tiles_y;
  if (blocks > INT_MAX) return LGU_E_UNSUPPORTED;
  auto kern = conv3x3_fanout_c128_kernel<TXM, XH>;
  if (allow_max_dynamic_lds<conv3x3_fanout_c128_kernel<TXM, XH>>() != hipSuccess) return launch_status();
  C3FanOperands ops;
  int vec = a.W % 4 == 0 ? 1 : 0;
  for (int g = 0; g < 3; g++) {   // an unused third slot repeats the second: the kernel never reads it
    const int k = g < a.G ? g : a.G - 1;
    ops.wpack[g] = static_cast<const f16x8*>(a.wpack[k]);
    ops.bias[g] = static_cast<const _Float16*>(a.bias[k]);
    ops.out[g] = static_cast<_Float16*>(a.out[k]);
    if (!c3_aligned(a.out[k], 8)) vec = 0;
  }
  hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(C3_THREADS), c3_lds_bytes<TXM>(), s, a.x, ops, a.G, a.H, a.W, tiles_x,
                     tiles_y, (a.flags & LGU_CONV3_RELU) ? 1 : 0, vec);
  return launch_status();
}

template <int TXM>
static int c3_fan_launch_x(const lgu_conv3_fanout_args& a, hipStream_t s) {
  return (a.flags & LGU_CONV3_X_HALF) ? c3_fan_launch<TXM, true>(a, s) : c3_fan_launch<TXM, false>(a, s);
}

}  // namespace lgu

extern "C" int lgu_conv3x3_fanout_c128_h16(lgu_conv3_fanout_args a, void* stream) {
  using namespace lgu;
  if (a.N < 0 || a.H < 1 || a.W < 1 || (a.flags & ~(LGU_CONV3_X_HALF | LGU_CONV3_RELU))) return LGU_E_BADARG;
  if (a.N == 0) return LGU_OK;
  if (a.G != 2 && a.G != 3) return LGU_E_UNSUPPORTED;
  if (!a.x || !c3_aligned(a.x, (a.flags & LGU_CONV3_X_HALF) ? 2 : 4)) return LGU_E_BADARG;
  for (int g = 0; g < a.G; g++) {
    if (!a.wpack[g] || !a.bias[g] || !a.out[g]) return LGU_E_BADARG;
    if (!c3_aligned(a.bias[g], 2) || !c3_aligned(a.out[g], 2)) return LGU_E_BADARG;
  }
  for (int g = 0; g < a.G; g++)
    if (!c3_aligned(a.wpack[g], 16)) return LGU_E_UNSUPPORTED;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  // always 32 x 4 pixels per workgroup (the bits do not depend on the tile): the 64-wide tile's whole 128-byte lines come
  // from the write-out through LDS, which this kernel does not have, and the taller tile stages less halo; measured
  // faster at every shape class
#if LGU_C3_FORCE_TXM == 4
  return c3_fan_launch_x<4>(a, s);
#else
  return c3_fan_launch_x<2>(a, s);
#endif
}

extern "C" int lgu_conv3x3_c128_h16(lgu_conv3_args a, void* stream) {
  using namespace lgu;
  if (a.N < 0 || a.H < 1 || a.W < 1 || (a.flags & ~(LGU_CONV3_X_HALF | LGU_CONV3_RELU))) return LGU_E_BADARG;
  if (a.N == 0) return LGU_OK;
  if (!a.x || !a.wpack || !a.bias || !a.out) return LGU_E_BADARG;
  if (!c3_aligned(a.x, (a.flags & LGU_CONV3_X_HALF) ? 2 : 4) || !c3_aligned(a.bias, 2) || !c3_aligned(a.out, 2))
    return LGU_E_BADARG;
  if (a.Cout != 64 && a.Cout != 128) return LGU_E_UNSUPPORTED;
  if (!c3_aligned(a.wpack, 16)) return LGU_E_UNSUPPORTED;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  // 64 x 2 or 32 x 4 pixels per workgroup: the one that pads the image less (ties: the wider one, whole 128-byte lines)
  const long long pad64 = (long long)((a.W + 63) / 64 * 64) * ((a.H + 1) / 2 * 2);
  const long long pad32 = (long long)((a.W + 31) / 32 * 32) * ((a.H + 3) / 4 * 4);
  if (LGU_C3_FORCE_TXM ? LGU_C3_FORCE_TXM == 4 : pad64 <= pad32) return a.Cout == 128 ? c3_launch_x<128, 4>(a, s) : c3_launch_x<64, 4>(a, s);
  return a.Cout == 128 ? c3_launch_x<128, 2>(a, s) : c3_launch_x<64, 2>(a, s);
}
