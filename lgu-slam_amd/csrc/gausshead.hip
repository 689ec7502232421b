// gausshead.hip — the Gaussian mask's parameter head in one launch (reference droid_slam/gaussianMask_cuda.py:69-73:
// mapA = Linear(256, 16) + Tanh, meanMap and covMap = Linear(16, 2) each), per pixel p of x (E,h,w,256) channel-last:
//
//   u  = b1 + W1 . x[p]            (16)
//   tt = tanh(u)                   (16)
//   [mean_ofs[p]; cov_raw[p]] = [bm; bc] + [Wm; Wc] . tt      (2 + 2)
//
// Half mode (what float16 autocast evaluates): parameters rounded to half in the pack, x half or fp32 rounded to half once
// in the load, exact products, fp32 accumulation from zero, u = half(b1 + sum), tt = half(tanhf(u)), each output
// half(b + sum).  fp32 mode (LGU_GAUSSHEAD_FP32): everything fp32 on the fp32 matrix cores, no half rounding.
//
// Mapping: both layers are computed transposed, so that nothing moves between lanes and there is no LDS.  A tile is 16
// consecutive pixels (numbered through the whole tensor, gp = (e h + y) w + x; a tile may span samples).  Layer 1 puts W1 on
// the A operand (row = hidden unit) and the tile on the B operand (column = pixel) of v_mfma_f32_16x16x32_f16: lane
// l = 16 g + p loads, for each of the 8 K steps kc, the 16 bytes of channels 32 kc + 8 g .. + 8 of its pixel's row (the
// four lanes of a pixel read 64 consecutive bytes; a fp32 x takes two 16-byte loads and one rounding).  The accumulator
// holds pixel p on the lane and the hidden units 4 g + i in its registers, which after bias, rounding and tanh IS the B
// fragment (k = 4 g + i, column p) of one v_mfma_f32_16x16x16_f16 whose A operand holds [Wm; Wc] in rows 0..3 and zeros in
// rows 4..15.  Lanes 0..15 then hold their pixel's four outputs in the four accumulator registers.  The fp32 mode does
// the same with v_mfma_f32_16x16x4_f32: 64 K steps (step s = 4 m + i takes element i of the lane's 16-byte load m, channel
// 16 m + 4 g + i) into two accumulators (even and odd m, added once), and 4 K steps for the second layer.
//
// A wave keeps the W1 fragments (32 VGPRs half, 64 fp32) for all its tiles and takes the tiles wave, wave + waves, ...;
// the next tile's loads are issued before this tile's MFMAs.  A pixel past the end re-reads the last pixel and stores
// nothing.  A column of an MFMA depends on that column of B only: a pixel's bits depend on its own 256 inputs, not on E,
// the tile or the grid, and a NaN reaches only its own pixel (rows 4..15 of the second product are never stored).  No
// atomics, no workspace, no LDS, no host synchronisation.
#include <limits.h>

#include <type_traits>

#include "lgu_common.hpp"

namespace lgu {

constexpr int GH_CIN = LGU_GAUSSHEAD_CIN;
constexpr int GH_HID = LGU_GAUSSHEAD_HIDDEN;
constexpr int GH_THREADS = 256;
constexpr int GH_TILE = 16;                               // pixels per MFMA tile
constexpr int GH_W1 = GH_HID * GH_CIN;                    // elements of the W1 fragments; the W2 fragments follow
constexpr int GH_WAVES_PER_CU = 8;

static_assert(GH_CIN == 256 && GH_HID == 16, "8 K steps of 32 channels; one 16-row tile of hidden units");
static_assert(LGU_GAUSSHEAD_WPACK_ELEMS == GH_W1 + kWave * 4, "pack size");
static_assert(LGU_GAUSSHEAD_BIAS_ELEMS == GH_HID + 4, "bias size");

// ---- half mode --------------------------------------------------------------------------------------------------------
template <bool XH>
struct GhTileH {
  using XT = typename std::conditional<XH, _Float16, float>::type;
  using V = typename std::conditional<XH, f16x8, f32x4>::type;
  static constexpr int NV = XH ? 8 : 16;
  V v[NV];
  __device__ __forceinline__ void load(const XT* row) {     // row: the lane's pixel row + 8 g
#pragma unroll
    for (int kc = 0; kc < 8; kc++) {
      if constexpr (XH) {
        v[kc] = *reinterpret_cast<const V*>(row + 32 * kc);
      } else {
        v[2 * kc] = *reinterpret_cast<const V*>(row + 32 * kc);
        v[2 * kc + 1] = *reinterpret_cast<const V*>(row + 32 * kc + 4);
      }
    }
  }
  __device__ __forceinline__ f16x8 frag(int kc) const {
    if constexpr (XH) {
      return v[kc];
    } else {
      f16x8 f;
#pragma unroll
      for (int j = 0; j < 4; j++) {
        f[j] = (_Float16)v[2 * kc][j];
        f[4 + j] = (_Float16)v[2 * kc + 1][j];
      }
      return f;
    }
  }
};

template <bool XH>
__global__ __launch_bounds__(GH_THREADS) void gausshead_h16_kernel(const void* __restrict__ xv, const _Float16* __restrict__ wpack,
                                                                   const _Float16* __restrict__ bias,
                                                                   _Float16* __restrict__ mean_ofs, _Float16* __restrict__ cov_raw,
                                                                   _Float16* __restrict__ hidden, int total, int tiles) {
  using XT = typename GhTileH<XH>::XT;
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = blockIdx.x * (GH_THREADS / kWave) + (threadIdx.x >> 6);
  const int waves = gridDim.x * (GH_THREADS / kWave);
  if (wave >= tiles) return;                                // wave-uniform
  const int p = lane & 15, g = lane >> 4;

  f16x8 w1[8];
#pragma unroll
  for (int kc = 0; kc < 8; kc++) w1[kc] = reinterpret_cast<const f16x8*>(wpack)[kc * kWave + lane];
  const f16x4 w2 = reinterpret_cast<const f16x4*>(wpack + GH_W1)[lane];
  float b1[4], b2[4];
#pragma unroll
  for (int i = 0; i < 4; i++) {
    b1[i] = (float)bias[4 * g + i];
    b2[i] = (float)bias[GH_HID + i];
  }

  const XT* xb = static_cast<const XT*>(xv);
  auto row_of = [&](int tile) {
    int gp = GH_TILE * tile + p;
    gp = gp < total ? gp : total - 1;
    return xb + (size_t)gp * GH_CIN + 8 * g;
  };
  GhTileH<XH> cur, nxt;
  cur.load(row_of(wave));
  for (int tile = wave; tile < tiles; tile += waves) {
    const bool more = tile + waves < tiles;                 // wave-uniform; tile + waves < 2 tiles: no overflow
    if (more) nxt.load(row_of(tile + waves));

    f32x4 acc = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int kc = 0; kc < 8; kc++) acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(w1[kc], cur.frag(kc), acc, 0, 0, 0);
    f16x4 tt;
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const _Float16 u = (_Float16)(b1[i] + acc[i]);
      tt[i] = (_Float16)tanhf((float)u);
    }
    const f32x4 o = __builtin_amdgcn_mfma_f32_16x16x16f16(w2, tt, f32x4{0.0f, 0.0f, 0.0f, 0.0f}, 0, 0, 0);

    const int gp = GH_TILE * tile + p;
    if (gp < total) {
      if (hidden) {
#pragma unroll
        for (int i = 0; i < 4; i++) hidden[(size_t)gp * GH_HID + 4 * g + i] = tt[i];
      }
      if (g == 0) {
        mean_ofs[2 * (size_t)gp] = (_Float16)(b2[0] + o[0]);
        mean_ofs[2 * (size_t)gp + 1] = (_Float16)(b2[1] + o[1]);
        cov_raw[2 * (size_t)gp] = (_Float16)(b2[2] + o[2]);
        cov_raw[2 * (size_t)gp + 1] = (_Float16)(b2[3] + o[3]);
      }
    }
    if (more) cur = nxt;
  }
}

// ---- fp32 mode --------------------------------------------------------------------------------------------------------
struct GhTileF {
  f32x4 v[16];
  __device__ __forceinline__ void load(const float* row) {  // row: the lane's pixel row + 4 g
#pragma unroll
    for (int m = 0; m < 16; m++) v[m] = *reinterpret_cast<const f32x4*>(row + 16 * m);
  }
};

__global__ __launch_bounds__(GH_THREADS) void gausshead_f32_kernel(const float* __restrict__ xb, const float* __restrict__ wpack,
                                                                   const float* __restrict__ bias, float* __restrict__ mean_ofs,
                                                                   float* __restrict__ cov_raw, float* __restrict__ hidden,
                                                                   int total, int tiles) {
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = blockIdx.x * (GH_THREADS / kWave) + (threadIdx.x >> 6);
  const int waves = gridDim.x * (GH_THREADS / kWave);
  if (wave >= tiles) return;
  const int p = lane & 15, g = lane >> 4;

  float w1[64];
#pragma unroll
  for (int s = 0; s < 64; s++) w1[s] = wpack[s * kWave + lane];
  float w2[4], b1[4], b2[4];
#pragma unroll
  for (int i = 0; i < 4; i++) {
    w2[i] = wpack[GH_W1 + i * kWave + lane];
    b1[i] = bias[4 * g + i];
    b2[i] = bias[GH_HID + i];
  }

  auto row_of = [&](int tile) {
    int gp = GH_TILE * tile + p;
    gp = gp < total ? gp : total - 1;
    return xb + (size_t)gp * GH_CIN + 4 * g;
  };
  GhTileF cur, nxt;
  cur.load(row_of(wave));
  for (int tile = wave; tile < tiles; tile += waves) {
    const bool more = tile + waves < tiles;
    if (more) nxt.load(row_of(tile + waves));

    f32x4 acc[2] = {f32x4{0.0f, 0.0f, 0.0f, 0.0f}, f32x4{0.0f, 0.0f, 0.0f, 0.0f}};
#pragma unroll
    for (int m = 0; m < 16; m++)
#pragma unroll
      for (int i = 0; i < 4; i++)
        acc[m & 1] = __builtin_amdgcn_mfma_f32_16x16x4f32(w1[4 * m + i], cur.v[m][i], acc[m & 1], 0, 0, 0);
    float tt[4];
#pragma unroll
    for (int i = 0; i < 4; i++) tt[i] = tanhf(b1[i] + (acc[0][i] + acc[1][i]));
    f32x4 o = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int i = 0; i < 4; i++) o = __builtin_amdgcn_mfma_f32_16x16x4f32(w2[i], tt[i], o, 0, 0, 0);

    const int gp = GH_TILE * tile + p;
    if (gp < total) {
      if (hidden) {
#pragma unroll
        for (int i = 0; i < 4; i++) hidden[(size_t)gp * GH_HID + 4 * g + i] = tt[i];
      }
      if (g == 0) {
        mean_ofs[2 * (size_t)gp] = b2[0] + o[0];
        mean_ofs[2 * (size_t)gp + 1] = b2[1] + o[1];
        cov_raw[2 * (size_t)gp] = b2[2] + o[2];
        cov_raw[2 * (size_t)gp + 1] = b2[3] + o[3];
      }
    }
    if (more) cur = nxt;
  }
}

static inline bool gh_aligned(const void* p, int n) { return (reinterpret_cast<uintptr_t>(p) % n) == 0; }

}  // namespace lgu

extern "C" int lgu_gaussian_head(lgu_gausshead_args a, void* stream) {
  using namespace lgu;
  if (a.E < 0 || a.H < 0 || a.W < 0 || (a.flags & ~(LGU_GAUSSHEAD_X_HALF | LGU_GAUSSHEAD_FP32))) return LGU_E_BADARG;
  const bool xh = (a.flags & LGU_GAUSSHEAD_X_HALF) != 0, f32 = (a.flags & LGU_GAUSSHEAD_FP32) != 0;
  if (xh && f32) return LGU_E_BADARG;
  if (a.E == 0 || a.H == 0 || a.W == 0) return LGU_OK;
  if (!a.x || !a.wpack || !a.bias || !a.mean_ofs || !a.cov_raw) return LGU_E_BADARG;
  const int oe = f32 ? 4 : 2;                               // bytes of a parameter and of an output element
  if (!gh_aligned(a.bias, oe) || !gh_aligned(a.mean_ofs, oe) || !gh_aligned(a.cov_raw, oe) || !gh_aligned(a.hidden, oe))
    return LGU_E_BADARG;
  if (!gh_aligned(a.x, 16) || !gh_aligned(a.wpack, 16)) return LGU_E_UNSUPPORTED;
  const long long total = (long long)a.E * a.H * a.W;
  if (total > INT_MAX - GH_TILE) return LGU_E_UNSUPPORTED;
  const int tiles = (int)((total + GH_TILE - 1) / GH_TILE);
  const int cap = GH_WAVES_PER_CU * device_cu_count();
  const int waves = tiles < cap ? tiles : cap;
  const dim3 grid((waves + GH_THREADS / kWave - 1) / (GH_THREADS / kWave)), block(GH_THREADS);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (f32) {
    hipLaunchKernelGGL(gausshead_f32_kernel, grid, block, 0, s, static_cast<const float*>(a.x), static_cast<const float*>(a.wpack),
                       static_cast<const float*>(a.bias), static_cast<float*>(a.mean_ofs), static_cast<float*>(a.cov_raw),
                       static_cast<float*>(a.hidden), (int)total, tiles);
  } else if (xh) {
    hipLaunchKernelGGL((gausshead_h16_kernel<true>), grid, block, 0, s, a.x, static_cast<const _Float16*>(a.wpack),
                       static_cast<const _Float16*>(a.bias), static_cast<_Float16*>(a.mean_ofs), static_cast<_Float16*>(a.cov_raw),
                       static_cast<_Float16*>(a.hidden), (int)total, tiles);
  } else {
    hipLaunchKernelGGL((gausshead_h16_kernel<false>), grid, block, 0, s, a.x, static_cast<const _Float16*>(a.wpack),
                       static_cast<const _Float16*>(a.bias), static_cast<_Float16*>(a.mean_ofs), static_cast<_Float16*>(a.cov_raw),
                       static_cast<_Float16*>(a.hidden), (int)total, tiles);
  }
  return launch_status();
}
