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
//
// lgu_encconv3x3_norm_h16 is the same kernel with the feature encoder's instance norms folded in (template parameters PRO
// and EMIT, every statement of theirs under `if constexpr`, so the instantiations above are unchanged): with a prologue the
// workgroup first fills a (mean, rstd) table behind the tile region from the planes' exact integer sums (encstats.hpp) and
// the staging loop writes h = half(relu(IN(x))), half(relu(y + relu(IN(x)))) or half(relu(IN(y) + relu(IN(x)))) instead of x
// (a second operand through the same loop; padding is zeros of h), channel group 0 also storing the pixels its tile owns
// to `keep`; with EMIT the write-out adds the exact sums of the stored outputs to the planes' accumulators, reduced over
// the lanes that hold a channel of the tile, one integer vector-memory atomic add per channel and word.  The producer is
// an earlier launch on the same stream: no workgroup waits on another, no fences.
#include <limits.h>

#include <type_traits>

#include "encstats.hpp"
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

// lgu_encconv3x3_norm_h16: the instance norms of the feature encoder folded into the launch.  PRO = prologue mode + 4 keep:
// mode 0 none, 1 NORM, 2 RES, 3 RES_NORM (include/lgu_corr.h); EMIT: the exact sums of the stored outputs.
struct EcNormOperands : EcOperands {
  const _Float16* y;                 // RES, RES_NORM: the second staged operand, x's shape
  const unsigned long long* sx;      // accumulators of x's planes (N,Cin,R,4)
  const unsigned long long* sy;      // RES_NORM: of y's planes
  _Float16* keep;                    // the staged tensor h (N,Cin,H,W)
  unsigned long long* so;            // EMIT: accumulators of out's planes (N,Cout,R,4), and of r's
  unsigned long long* sr;
  float eps;
};

template <int PRO, bool EMIT>
using EcArgs = std::conditional_t<PRO != 0 || EMIT, EcNormOperands, EcOperands>;

template <int CIN, int COUT, int S, int NCO, int TXM, int TY, bool DOWN, int PRO = 0, bool EMIT = false>
__global__ __launch_bounds__(EC_THREADS) void encconv3x3_kernel(EcArgs<PRO, EMIT> a) {
  using T = EcTile<CIN, S, TXM, TY>;
  constexpr int MODE = PRO & 3;
  constexpr bool KEEP = (PRO & 4) != 0;
  static_assert(PRO >= 0 && PRO < 8 && (MODE != 0 || !KEEP), "prologue");
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

  // the (mean, rstd) table of this image's input planes, past the tile region: x's CIN pairs, then y's with RES_NORM
  [[maybe_unused]] float* const tab = reinterpret_cast<float*>(smem + T::lds_bytes(NCO, DOWN));
  if constexpr (MODE != 0) {
    constexpr int NT = (MODE == 3 ? 2 : 1) * CIN;
    const double cnt = (double)HW;
    for (int i = tid; i < NT; i += EC_THREADS) {
      const int c = i < CIN ? i : i - CIN;
      const unsigned long long* q = (i < CIN ? a.sx : a.sy) + ((size_t)n * CIN + c) * (ES_REPLICAS * ES_WORDS);
      float m, rs;
      es_mean_rstd(q, cnt, a.eps, m, rs);
      tab[2 * i] = m;
      tab[2 * i + 1] = rs;
    }
    __syncthreads();
  }

  // stage: one (channel octet, row, column) per thread and item, lanes along x; the loads of EC_SU items are issued before
  // the first of them is written (a pixel outside the image re-reads the image's first pixel and is then zeroed: every
  // load is unconditional and inside x)
  {
    const _Float16* src = a.x + (size_t)n * CIN * HW;
    const int iy0 = y0 * S - 1, ix0 = x0 * S - 1;
    constexpr int ITEMS = (CIN / 8) * LH * LW;
    for (int base = tid; base < ITEMS; base += EC_SU * EC_THREADS) {
      _Float16 raw[EC_SU][8];
      [[maybe_unused]] _Float16 raw2[MODE >= 2 ? EC_SU : 1][8];
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
        if constexpr (MODE >= 2) {
          const _Float16* q2 = a.y + (q - a.x);
#pragma unroll
          for (int ch = 0; ch < 8; ch++) raw2[u][ch] = q2[ch * HW];
        }
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
          if constexpr (MODE != 0) {
            // the prologue on a pixel inside the image (padding is zeros of the normalised tensor): fp32 subtraction, fp32
            // product, select, for RES / RES_NORM one fp32 add and select, ONE rounding to half
            const float* tb = tab + 16 * o;
#pragma unroll
            for (int ch = 0; ch < 8; ch++) {
              float t = ((float)raw[u][ch] - tb[2 * ch]) * tb[2 * ch + 1];
              t = t < 0.0f ? 0.0f : t;
              if constexpr (MODE == 2) t = (float)raw2[u][ch] + t;
              if constexpr (MODE == 3) t = ((float)raw2[u][ch] - tb[2 * CIN + 2 * ch]) * tb[2 * CIN + 2 * ch + 1] + t;
              if constexpr (MODE >= 2) t = t < 0.0f ? 0.0f : t;
              v[ch] = inside[u] ? (_Float16)t : (_Float16)0.0f;
            }
            if constexpr (KEEP) {
              // channel group 0 of the tile that owns the pixel: input rows [S y0, S (y0 + TY)), columns likewise
              if (cg == 0 && inside[u] && r >= 1 && r <= S * TY && c >= 1 && c <= S * TX) {
                _Float16* kq = a.keep + ((size_t)n * CIN + 8 * o) * HW + (size_t)(iy0 + r) * W + (ix0 + c);
#pragma unroll
                for (int ch = 0; ch < 8; ch++) kq[ch * HW] = v[ch];
              }
            }
          }
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
    if constexpr (!EMIT) {
      if (y >= Ho || xo >= Wo) continue;
    }
    f16x8 v = *reinterpret_cast<const f16x8*>(smem + ci * OPITCH + 2 * (row * TX + 8 * ch8));
    const bool is_r = DOWN && ci >= NCO;
    if constexpr (EMIT) {
      // a channel's TY rows of TX pixels are GRP neighbouring items of one wave: their exact sums over the pixels inside
      // the image, reduced over the lanes, are the workgroup's one add per word to the plane's slot
      constexpr int GRP = TY * (TX / 8);
      static_assert(GRP <= kWave && (GRP & (GRP - 1)) == 0 && (IMGS * NCO * GRP) % kWave == 0, "a channel per lane group");
      const bool live = y < Ho && xo < Wo;
      EsSums es = es_zero();
#pragma unroll
      for (int i = 0; i < 8; i++)
        if (live && xo + i < Wo) es_add(es, v[i]);
      es_reduce<GRP>(es);
      if (tid % GRP == 0) {
        const int tile = (y0 / TY) * a.tiles_x + x0 / TX;
        unsigned long long* plane = (is_r ? a.sr : a.so) + ((size_t)n * COUT + cg * NCO + (is_r ? ci - NCO : ci)) * (ES_REPLICAS * ES_WORDS);
        es_commit(plane, tile % ES_REPLICAS, es);
      }
      if (!live) continue;
    }
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

// PRO, EMIT and the parameter block A: lgu_encconv_args for the plain form, lgu_encconv_norm_args for the folded ones
template <int CIN, int COUT, int S, int NCO, int TXM, int TY, bool DOWN, int PRO = 0, bool EMIT = false, class A = lgu_encconv_args>
static int ec_launch_k(const A& a, hipStream_t s) {
  using T = EcTile<CIN, S, TXM, TY>;
  constexpr bool NORM = PRO != 0 || EMIT;
  // the (mean, rstd) table follows the tile region
  constexpr int LDS = T::lds_bytes(NCO, DOWN) + ((PRO & 3) == 0 ? 0 : (PRO & 3) == 3 ? 16 * CIN : 8 * CIN);
  static_assert(LDS <= 160 * 1024, "LDS per CU");
  if constexpr (LDS > 64 * 1024) {   // forced tiles only: every default tile is below the default limit
    if (allow_max_dynamic_lds<encconv3x3_kernel<CIN, COUT, S, NCO, TXM, TY, DOWN, PRO, EMIT>>() != hipSuccess) return launch_status();
  }
  EcArgs<PRO, EMIT> o;
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
  if constexpr (!NORM) o.res = static_cast<const _Float16*>(a.res);
  o.out = static_cast<_Float16*>(a.out);
  o.dpack = static_cast<const f16x8*>(a.dpack);
  o.dbias = static_cast<const _Float16*>(a.dbias);
  o.r = static_cast<_Float16*>(a.r);
  const bool w8 = o.Wo % 8 == 0;
  if constexpr (NORM) {   // the identity epilogue always
    o.res = nullptr;
    o.mode = 0;
    o.vec = (w8 && ec_aligned(a.out, 16) ? 1 : 0) | (w8 && a.r && ec_aligned(a.r, 16) ? 4 : 0);
    o.y = static_cast<const _Float16*>(a.y);
    o.sx = static_cast<const unsigned long long*>(a.stats_x);
    o.sy = static_cast<const unsigned long long*>(a.stats_y);
    o.keep = static_cast<_Float16*>(a.keep);
    o.so = static_cast<unsigned long long*>(a.stats_out);
    o.sr = static_cast<unsigned long long*>(a.stats_r);
    o.eps = a.eps;
  } else {
    o.mode = (a.flags & LGU_ENCCONV_RESIDUAL) ? 2 : (a.flags & LGU_ENCCONV_RELU) ? 1 : 0;
    o.vec = (w8 && ec_aligned(a.out, 16) ? 1 : 0) | (w8 && a.res && ec_aligned(a.res, 16) ? 2 : 0) | (w8 && a.r && ec_aligned(a.r, 16) ? 4 : 0);
  }
  hipLaunchKernelGGL((encconv3x3_kernel<CIN, COUT, S, NCO, TXM, TY, DOWN, PRO, EMIT>), dim3((unsigned)blocks), dim3(EC_THREADS), LDS, s, o);
  return launch_status();
}

template <int CIN, int COUT, int S, int NCO, int MT, int PRO = 0, bool EMIT = false, class A = lgu_encconv_args>
static int ec_launch_d(const A& a, hipStream_t s) {
  if constexpr (S == 2) {
    if (a.dpack) return ec_launch_k<CIN, COUT, S, NCO, 2, MT / 2, true, PRO, EMIT, A>(a, s);
  }
  return ec_launch_k<CIN, COUT, S, NCO, 2, MT / 2, false, PRO, EMIT, A>(a, s);
}

// the tile per shape class and call: MT pixel tiles as 32 x (MT / 2) pixels, NCO channels per workgroup.
// The small tile (NCO_S, MT_S) is the one that fills the machine with one 384x512 frame; the large one (NCO_L, MT_L) stages
// each input pixel for more outputs and is taken when its own grid still has two workgroups per CU (16 frames: 3 to 6 per
// CU).  The bits do not depend on the choice.
template <int CIN, int COUT, int S, int NCO_S, int MT_S, int NCO_L, int MT_L, int PRO = 0, bool EMIT = false, class A = lgu_encconv_args>
static int ec_launch(const A& a, hipStream_t s) {
  if constexpr ((LGU_EC_FORCE_NCO | LGU_EC_FORCE_MT) != 0) {
    constexpr int NCO = (LGU_EC_FORCE_NCO && LGU_EC_FORCE_NCO <= COUT) ? LGU_EC_FORCE_NCO : NCO_S;
    return ec_launch_d<CIN, COUT, S, NCO, LGU_EC_FORCE_MT ? LGU_EC_FORCE_MT : MT_S, PRO, EMIT, A>(a, s);
  } else if constexpr (NCO_S == NCO_L && MT_S == MT_L) {
    return ec_launch_d<CIN, COUT, S, NCO_S, MT_S, PRO, EMIT, A>(a, s);
  } else {
    const long long Ho = (a.H + S - 1) / S, Wo = (a.W + S - 1) / S;
    const long long large = (long long)a.N * ((Wo + 31) / 32) * ((Ho + MT_L / 2 - 1) / (MT_L / 2)) * (COUT / NCO_L);
    if (large >= 2LL * device_cu_count()) return ec_launch_d<CIN, COUT, S, NCO_L, MT_L, PRO, EMIT, A>(a, s);
    return ec_launch_d<CIN, COUT, S, NCO_S, MT_S, PRO, EMIT, A>(a, s);
  }
}

// the thirteen folded forms: mode 0 with emit, modes 1..3 with and without keep and emit
template <int CIN, int COUT, int S, int NCO_S, int MT_S, int NCO_L, int MT_L>
static int ec_launch_norm(const lgu_encconv_norm_args& a, hipStream_t s) {
  const bool emit = (a.flags & LGU_ENCNORM_EMIT) != 0;
#define LGU_EC_FORM(PRO)                                                                                                    \
  case PRO:                                                                                                                 \
    return emit ? ec_launch<CIN, COUT, S, NCO_S, MT_S, NCO_L, MT_L, PRO, true, lgu_encconv_norm_args>(a, s)                 \
                : ec_launch<CIN, COUT, S, NCO_S, MT_S, NCO_L, MT_L, PRO, false, lgu_encconv_norm_args>(a, s);
  switch (a.mode + (a.keep ? 4 : 0)) {
    case 0: return ec_launch<CIN, COUT, S, NCO_S, MT_S, NCO_L, MT_L, 0, true, lgu_encconv_norm_args>(a, s);
    LGU_EC_FORM(1)
    LGU_EC_FORM(2)
    LGU_EC_FORM(3)
    LGU_EC_FORM(5)
    LGU_EC_FORM(6)
    LGU_EC_FORM(7)
  }
#undef LGU_EC_FORM
  return LGU_E_BADARG;
}

// acc (planes,R,4) -> mean_rstd (planes,2): the shared function, one thread per plane
__global__ __launch_bounds__(EC_THREADS) void encstats_finalize_kernel(const unsigned long long* acc, long planes, double cnt, float eps,
                                                                       float* out) {
  const long i = (long)blockIdx.x * EC_THREADS + threadIdx.x;
  if (i >= planes) return;
  float m, rs;
  es_mean_rstd(acc + (size_t)i * (ES_REPLICAS * ES_WORDS), cnt, eps, m, rs);
  out[2 * i] = m;
  out[2 * i + 1] = rs;
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

extern "C" int lgu_encstats_replicas(void) { return lgu::ES_REPLICAS; }

extern "C" int lgu_encstats_finalize(lgu_encstats_args a, void* stream) {
  using namespace lgu;
  const void* acc = a.acc;
  float* mean_rstd = static_cast<float*>(a.mean_rstd);
  const long planes = a.planes, cnt = a.cnt;
  const float eps = a.eps;
  if (planes < 0 || cnt < 1 || !(eps >= 0.0f)) return LGU_E_BADARG;
  if (planes == 0) return LGU_OK;
  if (!acc || !mean_rstd || !ec_aligned(acc, 8) || !ec_aligned(mean_rstd, 4)) return LGU_E_BADARG;
  if (cnt > ES_MAX_PLANE) return LGU_E_UNSUPPORTED;
  const long blocks = (planes + EC_THREADS - 1) / EC_THREADS;
  if (blocks > INT_MAX) return LGU_E_UNSUPPORTED;
  hipLaunchKernelGGL(encstats_finalize_kernel, dim3((unsigned)blocks), dim3(EC_THREADS), 0, reinterpret_cast<hipStream_t>(stream),
                     static_cast<const unsigned long long*>(acc), planes, (double)cnt, eps, mean_rstd);
  return launch_status();
}

extern "C" int lgu_encconv3x3_norm_h16(lgu_encconv_norm_args a, void* stream) {
  using namespace lgu;
  const bool emit = (a.flags & LGU_ENCNORM_EMIT) != 0;
  if (a.N < 0 || a.H < 1 || a.W < 1 || (a.flags & ~LGU_ENCNORM_EMIT) || a.mode < 0 || a.mode > 3 || !(a.eps >= 0.0f)) return LGU_E_BADARG;
  if (a.mode == 0 && !emit) return LGU_E_BADARG;   // nothing folded: that call is lgu_encconv3x3_h16
  if (a.N == 0) return LGU_OK;
  if (!a.x || !a.wpack || !a.bias || !a.out) return LGU_E_BADARG;
  const bool down = a.dpack || a.dbias || a.r;
  if (down && (!a.dpack || !a.dbias || !a.r || a.stride != 2)) return LGU_E_BADARG;
  if ((a.mode >= 1) != (a.stats_x != nullptr) || (a.mode >= 2) != (a.y != nullptr) || (a.mode == 3) != (a.stats_y != nullptr)) return LGU_E_BADARG;
  if (a.keep && a.mode == 0) return LGU_E_BADARG;
  if (emit != (a.stats_out != nullptr) || (emit && down) != (a.stats_r != nullptr)) return LGU_E_BADARG;
  if (!ec_aligned(a.x, 2) || !ec_aligned(a.bias, 2) || !ec_aligned(a.out, 2) || !ec_aligned(a.dbias, 2) || !ec_aligned(a.r, 2) ||
      !ec_aligned(a.y, 2) || !ec_aligned(a.keep, 2) || !ec_aligned(a.stats_x, 8) || !ec_aligned(a.stats_y, 8) ||
      !ec_aligned(a.stats_out, 8) || !ec_aligned(a.stats_r, 8))
    return LGU_E_BADARG;
  const int shape = a.stride == 1   ? (a.Cin == 32 && a.Cout == 32 ? 1 : a.Cin == 64 && a.Cout == 64 ? 3 : a.Cin == 128 && a.Cout == 128 ? 5 : 0)
                    : a.stride == 2 ? (a.Cin == 32 && a.Cout == 64 ? 2 : a.Cin == 64 && a.Cout == 128 ? 4 : 0)
                                    : 0;
  if (!shape) return LGU_E_UNSUPPORTED;
  if (!ec_aligned(a.wpack, 16) || !ec_aligned(a.dpack, 16)) return LGU_E_UNSUPPORTED;
  if ((long long)a.H * a.W > ES_MAX_PLANE) return LGU_E_UNSUPPORTED;   // the input planes bound the output planes
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  switch (shape) {
    case 1: return ec_launch_norm<32, 32, 1, 32, 8, 32, 8>(a, s);
    case 2: return ec_launch_norm<32, 64, 2, 32, 4, 64, 8>(a, s);
    case 3: return ec_launch_norm<64, 64, 1, 32, 4, 64, 8>(a, s);
    case 4: return ec_launch_norm<64, 128, 2, 32, 4, 64, 4>(a, s);
    default: return ec_launch_norm<128, 128, 1, 32, 4, 64, 8>(a, s);
  }
}
