// flowenc.hip — the first layer of LGU-SLAM's motion encoder (reference droid_slam/droid_net.py:82-84,
// Conv2d(4, 128, 7, padding=3) + ReLU) as it is evaluated under float16 autocast, in one launch:
//
//   x_h = half(x), w_h = half(weight), b_h = half(bias)            (round to nearest even)
//   s   = b_h + sum_{c,ky,kx} x_h * w_h                            (exact products, fp32 accumulation)
//   y   = relu(half(s))                                            (one rounding; NaN stays NaN)
//
// An implicit GEMM on the matrix cores (v_mfma_f32_16x16x32_f16): M = 16 pixels along x, N = 16 output channels,
// K = 7 window rows x (8 x-slots x 4 channels).  The 8th x-slot is padding: its weights are zero in the pack AND its
// inputs are zeroed in the A fragment (0 * NaN would otherwise carry a NaN one pixel past the window).  One window row
// is one K step of 32, so an output tile is 7 MFMAs per 16 channels.
//
// Workgroup: 4 waves, an image tile of FE_TX x FE_TY pixels, all 128 channels.  The tile with its 3-pixel halo is
// converted to half while it is staged in LDS, channel-last (y, x, 4): lane l of an A fragment (pixel l & 15, k =
// 8 (l >> 4) + j) reads the two x-slots 2 (l >> 4) and 2 (l >> 4) + 1, 16 contiguous bytes.  Wave w owns channels
// [32 w, 32 w + 32): its two channel tiles of the packed weights (2 x 7 fragments, 56 registers) stay resident while it
// sweeps the tile's pixels two rows at a time (8 A fragments feed 28 MFMAs in four independent chains, each in ascending
// window row, so a value does not depend on the tile it falls in).  The accumulators start at the bias.  A
// lane's four accumulators are four consecutive pixels of one channel: one 8-byte NCHW store (VEC), or four element
// stores with the same values.  No atomics, no workspace; an image's bits depend on that image alone.
#include <limits.h>

#include "lgu_common.hpp"

namespace lgu {

constexpr int FE_CO = 128;              // output channels
constexpr int FE_CI = 4;                // input channels
constexpr int FE_KW = 7;                // window
constexpr int FE_PAD = 3;
constexpr int FE_TX = 64;               // pixels per tile row: four MFMA pixel tiles = one 128-byte line of a channel
#ifndef LGU_FE_TY
#define LGU_FE_TY 4                     // experiments only (-DLGU_FE_TY=2 | 4 | 8 | 16 in a variant build): DESIGN.md 3.14
#endif
constexpr int FE_TY = LGU_FE_TY;        // tile rows
constexpr int FE_LW = FE_TX + 8;        // x-slots per LDS row: 64 + 6 halo + the padding slot, rounded to 72
constexpr int FE_LH = FE_TY + FE_KW - 1;
constexpr int FE_THREADS = 256;

static_assert(FE_TX % 16 == 0 && FE_TY % 2 == 0, "pixel tiles of 16, rows in pairs");
static_assert(FE_LW >= FE_TX + FE_KW, "a fragment of the last pixel reads x-slots up to TX - 1 + 7");
static_assert(LGU_FLOW_CONV7_WPACK_HALVES == FE_KW * (FE_CO / 16) * kWave * 8, "weight pack size");

template <bool VEC>
__global__ __launch_bounds__(FE_THREADS) void flow_conv7_relu_kernel(const float* __restrict__ x,
                                                                    const f16x8* __restrict__ wpack,
                                                                    const _Float16* __restrict__ bias,
                                                                    _Float16* __restrict__ out, int H, int W, int tiles_x,
                                                                    int tiles_y) {
  __shared__ __attribute__((aligned(16))) f16x4 tile[FE_LH * FE_LW];
  int b = blockIdx.x;
  const int x0 = (b % tiles_x) * FE_TX;
  b /= tiles_x;
  const int y0 = (b % tiles_y) * FE_TY;
  const int n = b / tiles_y;
  const int lane = threadIdx.x & (kWave - 1), w = threadIdx.x >> 6;
  const int p = lane & 15, g = lane >> 4;
  const size_t HW = (size_t)H * W;

  // the wave's weights and bias; the loads are in flight while the tile is staged
  f16x8 wf[2][FE_KW];
#pragma unroll
  for (int ct = 0; ct < 2; ct++)
#pragma unroll
    for (int ky = 0; ky < FE_KW; ky++) wf[ct][ky] = wpack[(ky * (FE_CO / 16) + 2 * w + ct) * kWave + lane];
  float bz[2];
#pragma unroll
  for (int ct = 0; ct < 2; ct++) bz[ct] = (float)bias[32 * w + 16 * ct + p];

  // stage: one (row, x-slot) per thread and step, the four channels converted and written as 8 bytes
  const float* src = x + (size_t)n * FE_CI * HW;
  for (int idx = threadIdx.x; idx < FE_LH * FE_LW; idx += FE_THREADS) {
    const int r = idx / FE_LW, c = idx % FE_LW;
    const int gy = y0 + r - FE_PAD, gx = x0 + c - FE_PAD;
    f16x4 v = {(_Float16)0.0f, (_Float16)0.0f, (_Float16)0.0f, (_Float16)0.0f};
    if (in_bounds(gy, gx, H, W)) {
      const float* q = src + (size_t)gy * W + gx;
#pragma unroll
      for (int ch = 0; ch < FE_CI; ch++) v[ch] = (_Float16)q[ch * HW];
    }
    tile[idx] = v;
  }
  __syncthreads();

  const f16x4 zero4 = {(_Float16)0.0f, (_Float16)0.0f, (_Float16)0.0f, (_Float16)0.0f};
  _Float16* dst = out + ((size_t)n * FE_CO + 32 * w + p) * HW;   // channel 32 w + p of image n; + 16 ct channels below
#pragma unroll 1
  for (int t = 0; t < FE_TX / 16; t++) {
    const int xt = x0 + 16 * t;
    if (xt >= W) break;   // wave-uniform
    const f16x4* col = tile + 16 * t + p + 2 * g;
#pragma unroll 1
    for (int yy = 0; yy < FE_TY; yy += 2) {
      if (y0 + yy >= H) break;   // wave-uniform
      f16x8 a[FE_KW + 1];
#pragma unroll
      for (int r = 0; r < FE_KW + 1; r++) {
        const f16x4 lo = col[(yy + r) * FE_LW];
        const f16x4 hi = g == 3 ? zero4 : col[(yy + r) * FE_LW + 1];   // x-slot 7 is padding
        a[r] = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
      }
      // four independent chains (2 rows x 2 channel tiles), each in ascending ky; the epilogue follows all of them
      f32x4 acc[2][2];
#pragma unroll
      for (int dy = 0; dy < 2; dy++)
#pragma unroll
        for (int ct = 0; ct < 2; ct++) acc[dy][ct] = f32x4{bz[ct], bz[ct], bz[ct], bz[ct]};
#pragma unroll
      for (int ky = 0; ky < FE_KW; ky++)
#pragma unroll
        for (int dy = 0; dy < 2; dy++)
#pragma unroll
          for (int ct = 0; ct < 2; ct++)
            acc[dy][ct] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a[dy + ky], wf[ct][ky], acc[dy][ct], 0, 0, 0);
      const int xo = xt + 4 * g;
#pragma unroll
      for (int dy = 0; dy < 2; dy++) {
        const int y = y0 + yy + dy;
        f16x4 o[2];
#pragma unroll
        for (int ct = 0; ct < 2; ct++)
#pragma unroll
          for (int i = 0; i < 4; i++) {
            const _Float16 h = (_Float16)acc[dy][ct][i];
            o[ct][i] = h < (_Float16)0.0f ? (_Float16)0.0f : h;   // a NaN compares false and is kept
          }
        _Float16* q = dst + (size_t)y * W + xo;
        if (y < H && xo < W) {
#pragma unroll
          for (int ct = 0; ct < 2; ct++) {
            if constexpr (VEC) {
              *reinterpret_cast<f16x4*>(q + (size_t)(16 * ct) * HW) = o[ct];   // W % 4 == 0: four pixels in or out together
            } else {
#pragma unroll
              for (int i = 0; i < 4; i++)
                if (xo + i < W) q[(size_t)(16 * ct) * HW + i] = o[ct][i];
            }
          }
        }
      }
    }
  }
}

static inline bool fe_aligned(const void* p, int n) { return (reinterpret_cast<uintptr_t>(p) % n) == 0; }

}  // namespace lgu

extern "C" int lgu_flow_conv7_relu_h16(lgu_flow_conv7_args a, void* stream) {
  using namespace lgu;
  if (a.N < 0 || a.H < 1 || a.W < 1) return LGU_E_BADARG;
  if (a.N == 0) return LGU_OK;
  if (!a.x || !a.wpack || !a.bias || !a.out) return LGU_E_BADARG;
  if (!fe_aligned(a.x, 4) || !fe_aligned(a.bias, 2) || !fe_aligned(a.out, 2)) return LGU_E_BADARG;
  if (!fe_aligned(a.wpack, 16)) return LGU_E_UNSUPPORTED;
  const int tiles_x = (a.W - 1) / FE_TX + 1, tiles_y = (a.H - 1) / FE_TY + 1;
  const long long blocks = (long long)a.N * tiles_x * tiles_y;
  if (blocks > INT_MAX) return LGU_E_UNSUPPORTED;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const f16x8* wp = static_cast<const f16x8*>(a.wpack);
  const _Float16* bs = static_cast<const _Float16*>(a.bias);
  _Float16* o = static_cast<_Float16*>(a.out);
  if (a.W % 4 == 0 && fe_aligned(a.out, 8))
    hipLaunchKernelGGL((flow_conv7_relu_kernel<true>), dim3((unsigned)blocks), dim3(FE_THREADS), 0, s, a.x, wp, bs, o, a.H, a.W,
                       tiles_x, tiles_y);
  else
    hipLaunchKernelGGL((flow_conv7_relu_kernel<false>), dim3((unsigned)blocks), dim3(FE_THREADS), 0, s, a.x, wp, bs, o, a.H,
                       a.W, tiles_x, tiles_y);
  return launch_status();
}
