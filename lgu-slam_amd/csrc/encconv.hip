// encconv.hip — the residual stages' convolutions of the reference's BasicEncoder (droid_slam/modules/extractor.py:
// layer1..3, two ResidualBlocks each, DIM = 32) as they are evaluated under float16 autocast, NCHW half in and NCHW half
// out, one launch each: Conv2d(Cin, Cout, 3, stride=s, padding=1) for (Cin, Cout, s) in (32,32,1), (32,64,2), (64,64,1),
// (64,128,2), (128,128,1), with the pointwise tail of the norm-free context encoder as the epilogue and, on the strided
// shapes, the block's 1x1 stride-2 downsample branch from the same staged tile:
//
//   w_h = half(weight), b_h = half(bias)                      (rounded in the pack; x is half and used as it is)
//   s   = b_h + sum_{ky,kx,c} x[c, s y + ky - 1, s x + kx - 1] * w_h[co,c,ky,kx]   (exact products, fp32 accumulation from
//                                                             the bias, zero padding, row H and column W included)
//   y0  = half(s)                                             (one rounding)
//   y   = y0 | relu(y0) | relu(half(res + relu(y0)))          (identity | RELU | RESIDUAL; the add in fp32, one rounding)
//   r   = half(b'_h + sum_c x[c, 2 y, 2 x] * w'_h[co,c])      (the downsample branch, identity epilogue always)
//
// An implicit GEMM on the matrix cores (v_mfma_f32_16x16x32_f16): M = 16 output pixels along x, N = 16 output channels, a K
// step is one tap x 32 input channels, always in the order tap-major (ky, kx), then channel block: an output element's bits
// depend on its own image, H and W only, not on the tile, the channel split, the batch or N.
//
// Workgroup: 4 waves, an output tile of 16 TXM x TY pixels (MT = TXM TY = 4 or 8 MFMA pixel tiles, MT / 4 per wave) by NCO
// output channels (NCO / 16 channel tiles, all of them in every wave), both chosen per shape class and grid size by the
// launcher; blockIdx runs over the channel groups fastest, so the workgroups that stage the same input tile are
// neighbours.  The input tile with its halo, ((TY - 1) s + 3) rows of
// ((16 TXM - 1) s + 3) columns, is staged in LDS channel-last, 2 Cin + 16 bytes per pixel: a thread reads one pixel of 8
// channel planes (lanes along x, so each plane's load is contiguous) and writes one 16-byte piece of the pixel's channel
// row.  With stride 2 the columns are stored even ones first, then odd ones: the A fragment of tap kx, pixel 2 p + kx, is then
// 16 NEIGHBOURING staged pixels for every kx (even columns from p, odd ones from p, even ones from p + 1), as with
// stride 1, and its 16-byte reads fall in 16 different slots of a bank row.  The weights' B fragments come from global
// memory, prefetched EC_PF steps ahead.  The downsample branch reads the centre tap's A fragments again for Cin / 32 more
// K steps into accumulators of its own.  y0 and r go back through LDS as [channel][pixel], and the write-out applies the
// epilogue to 8 pixels of a channel row at a time: 16-byte loads of res and 16-byte stores where W_out % 8 == 0 and the
// pointer is 16-byte aligned, by element otherwise.  No atomics, no workspace, no host synchronisation.
#include <limits.h>

#include "lgu_common.hpp"

namespace lgu {

constexpr int EC_THREADS = 256;
// experiments only (variant builds): the depth of the weight prefetch in K steps, the staging items whose
// loads a thread issues before it writes any of them, and forced tile settings (0: the launcher's choice per shape);
// every setting computes the same bits
#ifndef LGU_EC_PF
#define LGU_EC_PF 4
#endif
#ifndef LGU_EC_SU
#define LGU_EC_SU 4
#endif
#ifndef LGU_EC_FORCE_NCO
#define LGU_EC_FORCE_NCO 0
#endif
#ifndef LGU_EC_FORCE_MT
#define LGU_EC_FORCE_MT 0
#endif
constexpr int EC_PF = LGU_EC_PF, EC_SU = LGU_EC_SU;
static_assert(EC_PF >= 1 && EC_PF <= 8 && EC_SU >= 1 && EC_SU <= 8, "prefetch depth and staging batch");
static_assert(LGU_EC_FORCE_NCO == 0 || LGU_EC_FORCE_NCO == 16 || LGU_EC_FORCE_NCO == 32 || LGU_EC_FORCE_NCO == 64, "forced channel group");
static_assert(LGU_EC_FORCE_MT == 0 || LGU_EC_FORCE_MT == 4 || LGU_EC_FORCE_MT == 8, "forced pixel tiles");

template <int CIN, int S, int TXM, int TY>
struct EcTile {
  static constexpr int TX = 16 * TXM, MT = TXM * TY;
  static constexpr int LW = (TX - 1) * S + 3, LH = (TY - 1) * S + 3;   // staged columns and rows
  static constexpr int HALF = (LW + 1) / 2;                            // stride 2: the even columns come first
  static constexpr int PITCH = 2 * CIN + 16;                           // bytes per staged pixel
  static constexpr int OPITCH = 2 * 16 * MT + 16;                      // bytes per channel of an output image in LDS
  static constexpr int IN_BYTES = LH * LW * PITCH;
  __host__ __device__ static constexpr int pos(int c) { return S == 2 ? (c & 1) * HALF + (c >> 1) : c; }
  __host__ __device__ static constexpr int lds_bytes(int nco, bool down) {
    const int o = nco * OPITCH * (down ? 2 : 1);
    return IN_BYTES > o ? IN_BYTES : o;
  }
};

// one rounding to half already made; the epilogues on half values (a NaN compares false and is kept)
__device__ __forceinline__ _Float16 ec_relu(_Float16 h) { return h < (_Float16)0.0f ? (_Float16)0.0f : h; }

struct EcOperands {
  const _Float16* x; const f16x8* wpack; const _Float16* bias; const _Float16* res; _Float16* out;
  const f16x8* dpack; const _Float16* dbias; _Float16* r;
  int H, W, Ho, Wo, tiles_x, tiles_y, mode, vec;   // mode 0 identity, 1 relu, 2 residual; vec bit 0 out, 1 res, 2 r
};

template <int CIN, int COUT, int S, int NCO, int TXM, int TY, bool DOWN>
__global__ __launch_bounds__(EC_THREADS) void encconv3x3_kernel(EcOperands a) {
  using T = EcTile<CIN, S, TXM, TY>;
  constexpr int TX = T::TX, MT = T::MT, LW = T::LW, LH = T::LH, PITCH = T::PITCH, OPITCH = T::OPITCH;
  constexpr int MTW = MT / 4;              // pixel tiles per wave
  constexpr int NCT = NCO / 16;            // channel tiles per workgroup, all in every wave
  constexpr int CTS = COUT / 16;           // channel tiles in the pack
  constexpr int CG = COUT / NCO;           // channel groups
  constexpr int KC = CIN / 32, KS = 9 * KC;
  constexpr int PF = EC_PF < KS ? EC_PF : KS;
  static_assert(MT % 4 == 0 && COUT % NCO == 0 && NCO % 16 == 0 && (S == 1 || S == 2) && (!DOWN || S == 2), "tile");
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];

  int b = blockIdx.x;
  const int cg = b % CG;
  b /= CG;
  const int x0 = (b % a.tiles_x) * TX;
  b /= a.tiles_x;
  const int y0 = (b % a.tiles_y) * TY;
  const int n = b / a.tiles_y;
  const int tid = threadIdx.x, lane = tid & (kWave - 1), w = tid >> 6;
  const int p = lane & 15, g = lane >> 4;
  const int H = a.H, W = a.W, Ho = a.Ho, Wo = a.Wo;
  const size_t HW = (size_t)H * W, HWo = (size_t)Ho * Wo;

  // the wave's first weight fragments and its bias are in flight while the tile is staged
  const f16x8* wp = a.wpack + (size_t)(cg * NCT) * kWave + lane;
  f16x8 bf[PF][NCT];
#pragma unroll
  for (int s = 0; s < PF; s++)
#pragma unroll
    for (int ct = 0; ct < NCT; ct++) bf[s][ct] = wp[((size_t)s * CTS + ct) * kWave];
  float bz[NCT];
#pragma unroll
  for (int ct = 0; ct < NCT; ct++) bz[ct] = (float)a.bias[cg * NCO + 16 * ct + p];

  // stage: one (channel octet, row, column) per thread and item, lanes along x; the loads of EC_SU items are issued before
  // the first of them is written (a pixel outside the image re-reads the image's first pixel and is then zeroed: every
  // load is unconditional and inside x)
  {
    const _Float16* src = a.x + (size_t)n * CIN * HW;
    const int iy0 = y0 * S - 1, ix0 = x0 * S - 1;
    constexpr int ITEMS = (CIN / 8) * LH * LW;
    for (int base = tid; base < ITEMS; base += EC_SU * EC_THREADS) {
      _Float16 raw[EC_SU][8];
      bool inside[EC_SU];
#pragma unroll
      for (int u = 0; u < EC_SU; u++) {
        const int idx = base + u * EC_THREADS;
        const int c = idx % LW, t = idx / LW;
        const int r = t % LH, o = t / LH;
        const int gy = iy0 + r, gx = ix0 + c;
        inside[u] = idx < ITEMS && in_bounds(gy, gx, H, W);
        const _Float16* q = src + (inside[u] ? (size_t)(8 * o) * HW + (size_t)gy * W + gx : (size_t)0);
#pragma unroll
        for (int ch = 0; ch < 8; ch++) raw[u][ch] = q[ch * HW];
      }
#pragma unroll
      for (int u = 0; u < EC_SU; u++) {
        const int idx = base + u * EC_THREADS;
        if (idx < ITEMS) {
          const int c = idx % LW, t = idx / LW;
          const int r = t % LH, o = t / LH;
          f16x8 v;
#pragma unroll
          for (int ch = 0; ch < 8; ch++) v[ch] = inside[u] ? raw[u][ch] : (_Float16)0.0f;
          *reinterpret_cast<f16x8*>(smem + (r * LW + T::pos(c)) * PITCH + 16 * o) = v;
        }
      }
    }
  }
  __syncthreads();

  // the KS steps of the wave's MTW pixel tiles x NCT channel tiles, from the bias: tap-major (ky, kx), then channel block
  const unsigned char* abase = smem + p * PITCH + 16 * g;
  f32x4 acc[MTW][NCT];
#pragma unroll
  for (int m = 0; m < MTW; m++)
#pragma unroll
    for (int ct = 0; ct < NCT; ct++) acc[m][ct] = f32x4{bz[ct], bz[ct], bz[ct], bz[ct]};
#pragma unroll
  for (int s = 0; s < KS; s++) {
    const int tap = s / KC, kc = s % KC, ky = tap / 3, kx = tap % 3;
    f16x8 bw[NCT];
#pragma unroll
    for (int ct = 0; ct < NCT; ct++) bw[ct] = bf[s % PF][ct];
    if (s + PF < KS) {   // the slot just read takes the fragments of step s + PF
#pragma unroll
      for (int ct = 0; ct < NCT; ct++) bf[s % PF][ct] = wp[((size_t)(s + PF) * CTS + ct) * kWave];
    }
#pragma unroll
    for (int m = 0; m < MTW; m++) {
      const int mt = MTW * w + m, row = mt / TXM, mtx = mt % TXM;   // wave-uniform
      // pixel (16 mtx + p) S + kx of the staged row: pos() of it is pos(16 mtx S + kx) + p for either stride
      const f16x8 av = *reinterpret_cast<const f16x8*>(abase + ((row * S + ky) * LW + T::pos(16 * mtx * S + kx)) * PITCH + 64 * kc);
#pragma unroll
      for (int ct = 0; ct < NCT; ct++) acc[m][ct] = __builtin_amdgcn_mfma_f32_16x16x32_f16(av, bw[ct], acc[m][ct], 0, 0, 0);
    }
  }

  // the downsample branch: Cin / 32 more K steps on the centre tap, pixel (2 y, 2 x), from its own bias
  f32x4 racc[MTW][NCT];
  if constexpr (DOWN) {
    const f16x8* dp = a.dpack + (size_t)(cg * NCT) * kWave + lane;
    f16x8 dw[KC][NCT];
#pragma unroll
    for (int kc = 0; kc < KC; kc++)
#pragma unroll
      for (int ct = 0; ct < NCT; ct++) dw[kc][ct] = dp[((size_t)kc * CTS + ct) * kWave];
#pragma unroll
    for (int ct = 0; ct < NCT; ct++) {
      const float dz = (float)a.dbias[cg * NCO + 16 * ct + p];
#pragma unroll
      for (int m = 0; m < MTW; m++) racc[m][ct] = f32x4{dz, dz, dz, dz};
    }
#pragma unroll
    for (int kc = 0; kc < KC; kc++)
#pragma unroll
      for (int m = 0; m < MTW; m++) {
        const int mt = MTW * w + m, row = mt / TXM, mtx = mt % TXM;
        const f16x8 av = *reinterpret_cast<const f16x8*>(abase + ((row * S + 1) * LW + T::pos(16 * mtx * S + 1)) * PITCH + 64 * kc);
#pragma unroll
        for (int ct = 0; ct < NCT; ct++) racc[m][ct] = __builtin_amdgcn_mfma_f32_16x16x32_f16(av, dw[kc][ct], racc[m][ct], 0, 0, 0);
      }
  }
  __syncthreads();   // every wave has read its last A fragment: the tile's LDS becomes the output images

  // [channel][pixel tile][16 pixels] half, y0 then r; a lane's four accumulators are four consecutive pixels of one channel
#pragma unroll
  for (int m = 0; m < MTW; m++)
#pragma unroll
    for (int ct = 0; ct < NCT; ct++) {
      const int cl = 16 * ct + p, mt = MTW * w + m;
      f16x4 o;
#pragma unroll
      for (int i = 0; i < 4; i++) o[i] = (_Float16)acc[m][ct][i];
      *reinterpret_cast<f16x4*>(smem + cl * OPITCH + 2 * (16 * mt + 4 * g)) = o;
      if constexpr (DOWN) {
#pragma unroll
        for (int i = 0; i < 4; i++) o[i] = (_Float16)racc[m][ct][i];
        *reinterpret_cast<f16x4*>(smem + (NCO + cl) * OPITCH + 2 * (16 * mt + 4 * g)) = o;
      }
    }
  __syncthreads();

  // pixel tile mt = row * TXM + mtx, so a channel's 16 MT pixels are its TY rows of TX pixels in order
  constexpr int IMGS = DOWN ? 2 : 1;
  for (int idx = tid; idx < IMGS * NCO * TY * (TX / 8); idx += EC_THREADS) {
    const int ch8 = idx % (TX / 8), t = idx / (TX / 8);
    const int row = t % TY, ci = t / TY;          // ci: channel of y0, then channel of r
    const int y = y0 + row, xo = x0 + 8 * ch8;
    if (y >= Ho || xo >= Wo) continue;
    f16x8 v = *reinterpret_cast<const f16x8*>(smem + ci * OPITCH + 2 * (row * TX + 8 * ch8));
    const bool is_r = DOWN && ci >= NCO;
    const size_t off = ((size_t)n * COUT + cg * NCO + (is_r ? ci - NCO : ci)) * HWo + (size_t)y * Wo + xo;
    if (is_r) {
      _Float16* q = a.r + off;
      if (a.vec & 4) {
        *reinterpret_cast<f16x8*>(q) = v;
      } else {
#pragma unroll
        for (int i = 0; i < 8; i++)
          if (xo + i < Wo) q[i] = v[i];
      }
      continue;
    }
    if (a.mode == 1) {
#pragma unroll
      for (int i = 0; i < 8; i++) v[i] = ec_relu(v[i]);
    } else if (a.mode == 2) {
      const _Float16* rq = a.res + off;
      f16x8 rv;
      if (a.vec & 2) {
        rv = *reinterpret_cast<const f16x8*>(rq);
      } else {
#pragma unroll
        for (int i = 0; i < 8; i++) rv[i] = xo + i < Wo ? rq[i] : (_Float16)0.0f;
      }
#pragma unroll
      for (int i = 0; i < 8; i++) v[i] = ec_relu((_Float16)((float)rv[i] + (float)ec_relu(v[i])));
    }
    _Float16* q = a.out + off;
    if (a.vec & 1) {
      *reinterpret_cast<f16x8*>(q) = v;   // W_out % 8 == 0 and out 16-byte aligned: eight pixels together
    } else {
#pragma unroll
      for (int i = 0; i < 8; i++)
        if (xo + i < Wo) q[i] = v[i];
    }
  }
}

static inline bool ec_aligned(const void* p, int n) { return (reinterpret_cast<uintptr_t>(p) % n) == 0; }

template <int CIN, int COUT, int S, int NCO, int TXM, int TY, bool DOWN>
static int ec_launch_k(const lgu_encconv_args& a, hipStream_t s) {
  using T = EcTile<CIN, S, TXM, TY>;
  constexpr int LDS = T::lds_bytes(NCO, DOWN);
  static_assert(LDS <= 160 * 1024, "LDS per CU");
  if constexpr (LDS > 64 * 1024) {   // forced tiles only: every default tile is below the default limit
    if (allow_max_dynamic_lds<encconv3x3_kernel<CIN, COUT, S, NCO, TXM, TY, DOWN>>() != hipSuccess) return launch_status();
  }
  EcOperands o;
  o.H = a.H;
  o.W = a.W;
  o.Ho = (a.H + S - 1) / S;
  o.Wo = (a.W + S - 1) / S;
  o.tiles_x = (o.Wo - 1) / T::TX + 1;
  o.tiles_y = (o.Ho - 1) / TY + 1;
  const long long blocks = (long long)a.N * o.tiles_x * o.tiles_y * (COUT / NCO);
  if (blocks > INT_MAX) return LGU_E_UNSUPPORTED;
  o.x = static_cast<const _Float16*>(a.x);
  o.wpack = static_cast<const f16x8*>(a.wpack);
  o.bias = static_cast<const _Float16*>(a.bias);
  o.res = static_cast<const _Float16*>(a.res);
  o.out = static_cast<_Float16*>(a.out);
  o.dpack = static_cast<const f16x8*>(a.dpack);
  o.dbias = static_cast<const _Float16*>(a.dbias);
  o.r = static_cast<_Float16*>(a.r);
  o.mode = (a.flags & LGU_ENCCONV_RESIDUAL) ? 2 : (a.flags & LGU_ENCCONV_RELU) ? 1 : 0;
  const bool w8 = o.Wo % 8 == 0;
  o.vec = (w8 && ec_aligned(a.out, 16) ? 1 : 0) | (w8 && a.res && ec_aligned(a.res, 16) ? 2 : 0) | (w8 && a.r && ec_aligned(a.r, 16) ? 4 : 0);
  hipLaunchKernelGGL((encconv3x3_kernel<CIN, COUT, S, NCO, TXM, TY, DOWN>), dim3((unsigned)blocks), dim3(EC_THREADS), LDS, s, o);
  return launch_status();
}

template <int CIN, int COUT, int S, int NCO, int MT>
static int ec_launch_d(const lgu_encconv_args& a, hipStream_t s) {
  if constexpr (S == 2) {
    if (a.dpack) return ec_launch_k<CIN, COUT, S, NCO, 2, MT / 2, true>(a, s);
  }
  return ec_launch_k<CIN, COUT, S, NCO, 2, MT / 2, false>(a, s);
}

// the tile per shape class and call: MT pixel tiles as 32 x (MT / 2) pixels, NCO channels per workgroup.
// The small tile (NCO_S, MT_S) is the one that fills the machine with one 384x512 frame; the large one (NCO_L, MT_L) stages
// each input pixel for more outputs and is taken when its own grid still has two workgroups per CU (16 frames: 3 to 6 per
// CU).  The bits do not depend on the choice.
template <int CIN, int COUT, int S, int NCO_S, int MT_S, int NCO_L, int MT_L>
static int ec_launch(const lgu_encconv_args& a, hipStream_t s) {
  if constexpr ((LGU_EC_FORCE_NCO | LGU_EC_FORCE_MT) != 0) {
    constexpr int NCO = (LGU_EC_FORCE_NCO && LGU_EC_FORCE_NCO <= COUT) ? LGU_EC_FORCE_NCO : NCO_S;
    return ec_launch_d<CIN, COUT, S, NCO, LGU_EC_FORCE_MT ? LGU_EC_FORCE_MT : MT_S>(a, s);
  } else if constexpr (NCO_S == NCO_L && MT_S == MT_L) {
    return ec_launch_d<CIN, COUT, S, NCO_S, MT_S>(a, s);
  } else {
    const long long Ho = (a.H + S - 1) / S, Wo = (a.W + S - 1) / S;
    const long long large = (long long)a.N * ((Wo + 31) / 32) * ((Ho + MT_L / 2 - 1) / (MT_L / 2)) * (COUT / NCO_L);
    if (large >= 2LL * device_cu_count()) return ec_launch_d<CIN, COUT, S, NCO_L, MT_L>(a, s);
    return ec_launch_d<CIN, COUT, S, NCO_S, MT_S>(a, s);
  }
}

}  // namespace lgu

extern "C" int lgu_encconv3x3_h16(lgu_encconv_args a, void* stream) {
  using namespace lgu;
  if (a.N < 0 || a.H < 1 || a.W < 1 || (a.flags & ~(LGU_ENCCONV_RELU | LGU_ENCCONV_RESIDUAL))) return LGU_E_BADARG;
  if ((a.flags & LGU_ENCCONV_RELU) && (a.flags & LGU_ENCCONV_RESIDUAL)) return LGU_E_BADARG;
  if (a.N == 0) return LGU_OK;
  if (!a.x || !a.wpack || !a.bias || !a.out) return LGU_E_BADARG;
  if (((a.flags & LGU_ENCCONV_RESIDUAL) != 0) != (a.res != nullptr)) return LGU_E_BADARG;
  const bool down = a.dpack || a.dbias || a.r;
  if (down && (!a.dpack || !a.dbias || !a.r || a.stride != 2)) return LGU_E_BADARG;
  if (!ec_aligned(a.x, 2) || !ec_aligned(a.bias, 2) || !ec_aligned(a.out, 2) || !ec_aligned(a.res, 2) || !ec_aligned(a.dbias, 2) ||
      !ec_aligned(a.r, 2))
    return LGU_E_BADARG;
  const int shape = a.stride == 1   ? (a.Cin == 32 && a.Cout == 32 ? 1 : a.Cin == 64 && a.Cout == 64 ? 3 : a.Cin == 128 && a.Cout == 128 ? 5 : 0)
                    : a.stride == 2 ? (a.Cin == 32 && a.Cout == 64 ? 2 : a.Cin == 64 && a.Cout == 128 ? 4 : 0)
                                    : 0;
  if (!shape) return LGU_E_UNSUPPORTED;
  if (!ec_aligned(a.wpack, 16) || !ec_aligned(a.dpack, 16)) return LGU_E_UNSUPPORTED;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  switch (shape) {
    case 1: return ec_launch<32, 32, 1, 32, 8, 32, 8>(a, s);
    case 2: return ec_launch<32, 64, 2, 32, 4, 64, 8>(a, s);
    case 3: return ec_launch<64, 64, 1, 32, 4, 64, 8>(a, s);
    case 4: return ec_launch<64, 128, 2, 32, 4, 64, 4>(a, s);
    default: return ec_launch<128, 128, 1, 32, 4, 64, 8>(a, s);
  }
}
