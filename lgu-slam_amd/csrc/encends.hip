// encends.hip — the two ends of the reference's BasicEncoder (droid_slam/modules/extractor.py: conv1 and conv2) as they are
// evaluated under float16 autocast, NCHW in and NCHW half out, one launch each:
//
//   lgu_encstem7x7_h16       Conv2d(3, 32, 7, stride=2, padding=3) + bias, optional ReLU
//   lgu_encout1x1_c128_h16   Conv2d(128, Cout, 1) + bias, Cout 128 or 256; with SPLIT (Cout 256) the context encoder's
//                            tail net = tanh(h[:128]), inp = relu(h[128:]) as its epilogue
//
// The stem (the layout of flowenc.hip with a stride):
//   x_h = half(x), w_h = half(weight), b_h = half(bias)            (x in the kernel, the others in the pack)
//   s   = b_h + sum_{ky,kx,c} x_h[c, 2 y + ky - 3, 2 x + kx - 3] * w_h[co,c,ky,kx]   (exact products, fp32 accumulation
//                                                                   from the bias, window rows in ascending ky, zero padding)
//   y0  = half(s);  y = y0 | (y0 < 0 ? 0 : y0)                      (one rounding; a NaN compares false and is kept)
// An implicit GEMM on v_mfma_f32_16x16x32_f16: M = 16 output pixels along x, N = 16 output channels, a K step is one window
// row of 8 x-slots x 4 channels.  The 4th channel and the 8th x-slot are padding: their weights are zero in the pack, the
// 4th channel is staged as an exact zero and the 8th x-slot, which holds a real pixel of the image one column past the
// window, is zeroed in the A fragment (0 * NaN would otherwise carry a NaN one pixel past the window).  7 MFMAs per 16
// channels.  Workgroup: 4 waves, ES_TX x ES_TY output pixels, all 32 channels.  The input tile with its halo,
// (2 ES_TY + 5) rows of 2 ES_TX + 8 x-slots, is converted to half while it is staged in LDS channel-last (y, x, 4): output
// pixel p of a tile starts at x-slot 2 p, so lane (p, g) reads the x-slots 2 p + 2 g and 2 p + 2 g + 1, 16 contiguous and
// 16-byte aligned bytes at 16 (p + g): each 16-lane group of a ds_read_b128 (lanes {0-3, 12-15, 20-27}, ..) touches 15
// different 16-byte slots of a 256-byte bank row and one address twice (a broadcast), no conflict.  A wave owns
// pixel tiles (16 pixels of one row) and both channel tiles; its 14 weight fragments stay in registers.  A lane's four
// accumulators are four consecutive pixels of one channel: one 8-byte store, or element stores of the same values.
//
// The output layer (upmask.hip's rounding points, NCHW out):
//   p = sum_c x[c] * w_h[co,c]      (exact products; fp32 accumulation from zero in four steps of 32 channels, kc = 0..3)
//   h = half(b_h + p)               (one fp32 addition, one rounding)
//   SPLIT: net = half(tanhf(float(h[:128]))), inp = h[128:] < 0 ? 0 : h[128:]
// M = 16 pixels of one image, N = 16 output channels: a wave owns 16 consecutive pixels and 64 output channels, its A
// fragments (pixel p, channels 32 kc + 8 g ..+8) loaded from the channel planes straight into registers (no other wave
// wants them) and its 16 weight fragments from the pack.  A workgroup is 64 pixels x 64 channels; blockIdx runs over the
// channel groups fastest, so the workgroups that read the same pixels are neighbours.  A pixel past the end of the image
// re-reads the last one (an MFMA row of its own, never stored).  Stores as in the stem.
// Neither kernel uses atomics, a workspace or a host synchronisation; an output's bits depend on its own window only.
#include <limits.h>

#include <type_traits>

#include "lgu_common.hpp"

namespace lgu {

constexpr int ES_CI = 3, ES_CO = 32, ES_KW = 7, ES_PAD = 3;
constexpr int ES_THREADS = 256;
constexpr int ES_TX = 32;                       // output pixels per tile row: two MFMA pixel tiles
#ifndef LGU_ES_TY
#define LGU_ES_TY 4                             // experiments only (a variant build): every setting computes the same bits
#endif
constexpr int ES_TY = LGU_ES_TY;                // output rows per tile
constexpr int ES_MT = (ES_TX / 16) * ES_TY;     // pixel tiles per workgroup
constexpr int ES_LW = 2 * ES_TX + 8;            // x-slots per staged row: 2 (TX - 1) + 7 and the padding slot, rounded up
constexpr int ES_LH = 2 * (ES_TY - 1) + ES_KW;  // staged rows

static_assert(ES_TY >= 1 && ES_TY <= 16 && ES_TX % 16 == 0, "tile");
static_assert(ES_LW >= 2 * (ES_TX - 1) + ES_KW + 1 && ES_LW % 2 == 0, "the last pixel's fragment reads x-slots up to 2 (TX - 1) + 7");
static_assert(LGU_ENCSTEM_WPACK_HALVES == ES_KW * (ES_CO / 16) * kWave * 8, "weight pack size");

template <bool XH>
__global__ __launch_bounds__(ES_THREADS) void encstem7x7_kernel(const void* __restrict__ xv, const f16x8* __restrict__ wpack,
                                                               const _Float16* __restrict__ bias, _Float16* __restrict__ out,
                                                               int H, int W, int Ho, int Wo, int tiles_x, int tiles_y, int relu,
                                                               int vec) {
  using XT = typename std::conditional<XH, _Float16, float>::type;
  __shared__ __attribute__((aligned(16))) f16x4 tile[ES_LH * ES_LW];
  int b = blockIdx.x;
  const int x0 = (b % tiles_x) * ES_TX;
  b /= tiles_x;
  const int y0 = (b % tiles_y) * ES_TY;
  const int n = b / tiles_y;
  const int tid = threadIdx.x, lane = tid & (kWave - 1), w = tid >> 6;
  const int p = lane & 15, g = lane >> 4;
  const size_t HW = (size_t)H * W, HWo = (size_t)Ho * Wo;

  // the wave's weights and bias; the loads are in flight while the tile is staged
  f16x8 wf[2][ES_KW];
#pragma unroll
  for (int ct = 0; ct < 2; ct++)
#pragma unroll
    for (int ky = 0; ky < ES_KW; ky++) wf[ct][ky] = wpack[(ky * (ES_CO / 16) + ct) * kWave + lane];
  float bz[2];
#pragma unroll
  for (int ct = 0; ct < 2; ct++) bz[ct] = (float)bias[16 * ct + p];

  // stage: one (row, x-slot) per thread and step, lanes along x; the three channels converted, the fourth an exact zero
  {
    const XT* src = static_cast<const XT*>(xv) + (size_t)n * ES_CI * HW;
    const int iy0 = 2 * y0 - ES_PAD, ix0 = 2 * x0 - ES_PAD;
    for (int idx = tid; idx < ES_LH * ES_LW; idx += ES_THREADS) {
      const int r = idx / ES_LW, c = idx % ES_LW;
      const int gy = iy0 + r, gx = ix0 + c;
      f16x4 v = {(_Float16)0.0f, (_Float16)0.0f, (_Float16)0.0f, (_Float16)0.0f};
      if (in_bounds(gy, gx, H, W)) {
        const XT* q = src + (size_t)gy * W + gx;
#pragma unroll
        for (int ch = 0; ch < ES_CI; ch++) v[ch] = (_Float16)q[ch * HW];
      }
      tile[idx] = v;
    }
  }
  __syncthreads();

#pragma unroll 1
  for (int mt = w; mt < ES_MT; mt += ES_THREADS / kWave) {
    const int row = mt / (ES_TX / 16), t = mt % (ES_TX / 16);   // wave-uniform
    const int y = y0 + row, xt = x0 + 16 * t;
    if (y >= Ho || xt >= Wo) continue;
    // window row ky of output row `row` is staged row 2 row + ky; the lane's two x-slots start at 2 (16 t + p) + 2 g
    const f16x4* col = tile + (2 * row) * ES_LW + 2 * (16 * t + p + g);
    f16x8 a[ES_KW];
#pragma unroll
    for (int ky = 0; ky < ES_KW; ky++) {
      a[ky] = *reinterpret_cast<const f16x8*>(col + ky * ES_LW);
      if (g == 3) {   // x-slot 7 is padding
#pragma unroll
        for (int j = 4; j < 8; j++) a[ky][j] = (_Float16)0.0f;
      }
    }
    f32x4 acc[2];
#pragma unroll
    for (int ct = 0; ct < 2; ct++) acc[ct] = f32x4{bz[ct], bz[ct], bz[ct], bz[ct]};
#pragma unroll
    for (int ky = 0; ky < ES_KW; ky++)
#pragma unroll
      for (int ct = 0; ct < 2; ct++) acc[ct] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a[ky], wf[ct][ky], acc[ct], 0, 0, 0);
    const int xo = xt + 4 * g;
    if (xo >= Wo) continue;
#pragma unroll
    for (int ct = 0; ct < 2; ct++) {
      f16x4 o;
#pragma unroll
      for (int i = 0; i < 4; i++) {
        const _Float16 h = (_Float16)acc[ct][i];
        o[i] = (relu && h < (_Float16)0.0f) ? (_Float16)0.0f : h;   // a NaN compares false and is kept
      }
      _Float16* q = out + ((size_t)n * ES_CO + 16 * ct + p) * HWo + (size_t)y * Wo + xo;
      if (vec) {
        *reinterpret_cast<f16x4*>(q) = o;   // Wo % 4 == 0 and out 8-byte aligned: four pixels in or out together
      } else {
#pragma unroll
        for (int i = 0; i < 4; i++)
          if (xo + i < Wo) q[i] = o[i];
      }
    }
  }
}

constexpr int EO_CI = 128;
constexpr int EO_THREADS = 256;
constexpr int EO_PIX = 16 * (EO_THREADS / kWave);   // pixels per workgroup
constexpr int EO_NCO = 64;                          // output channels per workgroup

template <bool SPLIT>
__global__ __launch_bounds__(EO_THREADS) void encout1x1_kernel(const _Float16* __restrict__ x, const f16x8* __restrict__ wpack,
                                                              const _Float16* __restrict__ bias, _Float16* __restrict__ out,
                                                              _Float16* __restrict__ inp, int HW, int per_image, int cout, int vec) {
  constexpr int NCT = EO_NCO / 16, KC = EO_CI / 32;
  const int cts = cout / 16, cgs = cout / EO_NCO;
  int b = blockIdx.x;
  const int cg = b % cgs;
  b /= cgs;
  const int pb = b % per_image;
  const int n = b / per_image;
  const int tid = threadIdx.x, lane = tid & (kWave - 1), w = tid >> 6;
  const int p = lane & 15, g = lane >> 4;
  const int pi0 = EO_PIX * pb + 16 * w;
  if (pi0 >= HW) return;   // wave-uniform; the kernel has no barrier

  f16x8 bw[KC][NCT];
#pragma unroll
  for (int kc = 0; kc < KC; kc++)
#pragma unroll
    for (int ct = 0; ct < NCT; ct++) bw[kc][ct] = wpack[((size_t)kc * cts + cg * NCT + ct) * kWave + lane];
  float bz[NCT];
#pragma unroll
  for (int ct = 0; ct < NCT; ct++) bz[ct] = (float)bias[cg * EO_NCO + 16 * ct + p];

  // the lane's A fragments: pixel p of the wave's 16 (the image's last pixel past its end), channels 32 kc + 8 g ..+8
  const int pix = pi0 + p < HW ? pi0 + p : HW - 1;
  const _Float16* src = x + ((size_t)n * EO_CI + 8 * g) * HW + pix;
  f16x8 a[KC];
#pragma unroll
  for (int kc = 0; kc < KC; kc++)
#pragma unroll
    for (int j = 0; j < 8; j++) a[kc][j] = src[(size_t)(32 * kc + j) * HW];

  const int po = pi0 + 4 * g;   // the lane's four pixels
#pragma unroll
  for (int ct = 0; ct < NCT; ct++) {
    f32x4 acc = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int kc = 0; kc < KC; kc++) acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(a[kc], bw[kc][ct], acc, 0, 0, 0);
    const int c = cg * EO_NCO + 16 * ct + p;
    f16x4 o;
#pragma unroll
    for (int i = 0; i < 4; i++) o[i] = (_Float16)(bz[ct] + acc[i]);
    _Float16* q;
    if constexpr (SPLIT) {
      if (c < 128) {   // wave-uniform: a channel group lies on one side
#pragma unroll
        for (int i = 0; i < 4; i++) o[i] = (_Float16)tanhf((float)o[i]);
        q = out + ((size_t)n * 128 + c) * HW + po;
      } else {
#pragma unroll
        for (int i = 0; i < 4; i++) o[i] = o[i] < (_Float16)0.0f ? (_Float16)0.0f : o[i];
        q = inp + ((size_t)n * 128 + (c - 128)) * HW + po;
      }
    } else {
      q = out + ((size_t)n * cout + c) * HW + po;
    }
    if (po >= HW) continue;
    if (vec) {
      *reinterpret_cast<f16x4*>(q) = o;   // H W % 4 == 0 and the outputs 8-byte aligned
    } else {
#pragma unroll
      for (int i = 0; i < 4; i++)
        if (po + i < HW) q[i] = o[i];
    }
  }
}

static inline bool ee_aligned(const void* p, int n) { return (reinterpret_cast<uintptr_t>(p) % n) == 0; }

}  // namespace lgu

extern "C" int lgu_encstem7x7_h16(lgu_encstem_args a, void* stream) {
  using namespace lgu;
  if (a.N < 0 || a.H < 1 || a.W < 1 || (a.flags & ~(LGU_ENCSTEM_X_HALF | LGU_ENCSTEM_RELU))) return LGU_E_BADARG;
  if (a.N == 0) return LGU_OK;
  if (!a.x || !a.wpack || !a.bias || !a.out) return LGU_E_BADARG;
  const bool xh = (a.flags & LGU_ENCSTEM_X_HALF) != 0;
  if (!ee_aligned(a.x, xh ? 2 : 4) || !ee_aligned(a.bias, 2) || !ee_aligned(a.out, 2)) return LGU_E_BADARG;
  if (a.Cin != ES_CI || a.Cout != ES_CO) return LGU_E_UNSUPPORTED;
  if (!ee_aligned(a.wpack, 16)) return LGU_E_UNSUPPORTED;
  const int Ho = a.H / 2 + (a.H & 1), Wo = a.W / 2 + (a.W & 1);
  const int tiles_x = (Wo - 1) / ES_TX + 1, tiles_y = (Ho - 1) / ES_TY + 1;
  const long long blocks = (long long)a.N * tiles_x * tiles_y;
  if (blocks > INT_MAX) return LGU_E_UNSUPPORTED;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const f16x8* wp = static_cast<const f16x8*>(a.wpack);
  const _Float16* bs = static_cast<const _Float16*>(a.bias);
  _Float16* o = static_cast<_Float16*>(a.out);
  const int relu = (a.flags & LGU_ENCSTEM_RELU) ? 1 : 0;
  const int vec = (Wo % 4 == 0 && ee_aligned(a.out, 8)) ? 1 : 0;
  if (xh)
    hipLaunchKernelGGL((encstem7x7_kernel<true>), dim3((unsigned)blocks), dim3(ES_THREADS), 0, s, a.x, wp, bs, o, a.H, a.W, Ho, Wo,
                       tiles_x, tiles_y, relu, vec);
  else
    hipLaunchKernelGGL((encstem7x7_kernel<false>), dim3((unsigned)blocks), dim3(ES_THREADS), 0, s, a.x, wp, bs, o, a.H, a.W, Ho, Wo,
                       tiles_x, tiles_y, relu, vec);
  return launch_status();
}

extern "C" int lgu_encout1x1_c128_h16(lgu_encout_args a, void* stream) {
  using namespace lgu;
  if (a.N < 0 || a.H < 1 || a.W < 1 || (a.flags & ~LGU_ENCOUT_SPLIT)) return LGU_E_BADARG;
  const bool split = (a.flags & LGU_ENCOUT_SPLIT) != 0;
  if (split && a.Cout != 256) return LGU_E_BADARG;
  if (a.N == 0) return LGU_OK;
  if (!a.x || !a.wpack || !a.bias || !a.out || split != (a.inp != nullptr)) return LGU_E_BADARG;
  if (!ee_aligned(a.x, 2) || !ee_aligned(a.bias, 2) || !ee_aligned(a.out, 2) || !ee_aligned(a.inp, 2)) return LGU_E_BADARG;
  if (a.Cin != EO_CI || (a.Cout != 128 && a.Cout != 256)) return LGU_E_UNSUPPORTED;
  if (!ee_aligned(a.wpack, 16)) return LGU_E_UNSUPPORTED;
  const long long hw = (long long)a.H * a.W;
  if (hw > INT_MAX - EO_PIX) return LGU_E_UNSUPPORTED;
  const int per_image = (int)((hw - 1) / EO_PIX + 1);
  const long long blocks = (long long)a.N * per_image * (a.Cout / EO_NCO);
  if (blocks > INT_MAX) return LGU_E_UNSUPPORTED;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const _Float16* x = static_cast<const _Float16*>(a.x);
  const f16x8* wp = static_cast<const f16x8*>(a.wpack);
  const _Float16* bs = static_cast<const _Float16*>(a.bias);
  _Float16* o = static_cast<_Float16*>(a.out);
  _Float16* o2 = static_cast<_Float16*>(a.inp);
  const int vec = (hw % 4 == 0 && ee_aligned(a.out, 8) && ee_aligned(a.inp, 8)) ? 1 : 0;
  if (split)
    hipLaunchKernelGGL((encout1x1_kernel<true>), dim3((unsigned)blocks), dim3(EO_THREADS), 0, s, x, wp, bs, o, o2, (int)hw, per_image,
                       a.Cout, vec);
  else
    hipLaunchKernelGGL((encout1x1_kernel<false>), dim3((unsigned)blocks), dim3(EO_THREADS), 0, s, x, wp, bs, o, o2, (int)hw, per_image,
                       a.Cout, vec);
  return launch_status();
}
