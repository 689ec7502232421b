// gruconv.hip — the three Conv2d(448, 128, 3, padding=1) of LGU-SLAM's KAN-bias GRU (reference
// droid_slam/modules/gru_kanBias.py: convz, convr, convq) as they are evaluated under float16 autocast, with the GRU's
// gates and blend as their epilogue, NCHW in and NCHW out, one launch per call (lgu_gruconv3x3_c448_h16):
//
//   w_h = half(weight), b_h = half(bias)                                       (in the pack; round to nearest even)
//   s   = b_h + sum_{c,ky,kx} x[c, y+ky-1, x+kx-1] * w_h[co,c,ky,kx]           (exact products, fp32 accumulation, zero padding)
//   c   = half(s)                                                              (one rounding)
//   PLAIN  out  = c                                                            Cout 128 or 256
//   ZR     z    = half(sigmoid(half(c_z + kz)))                                Cout 256: outputs 0..127 are convz,
//          rnet = half(half(sigmoid(half(c_r + kr))) * net)                    128..255 convr (kangru_gates_kernel's arithmetic)
//   Q      out  = half(half(half(1 - z) * net) + half(z * half(tanh(half(c + kq)))))   Cout 128 (kangru_blend_kernel's)
//
// x is the concatenation along the channels of up to four NCHW half tensors (segments) whose channel counts are multiples
// of 32 and sum to 448; the concatenated tensor never exists.
//
// K order.  An implicit GEMM on the matrix cores (v_mfma_f32_16x16x32_f16): M = 16 pixels along x, N = 16 output
// channels, K = 126 steps of 32 channels of one tap, ALWAYS in the order
//     step = (c64 * 9 + tap) * 2 + kc,   c64 < 7 (64-channel chunk), tap = 3 ky + kx < 9, kc < 2 (32-channel block)
// (chunk-major, tap-major within a chunk), covering input channels 64 c64 + 32 kc .. + 32.  The accumulator starts at
// b_h.  The order does not depend on the mode, the tile, N, the segment split or any build setting below: an output
// element's bits depend on its own image, H and W only.  The pack is in the same order: wpack[step][ct][lane][j] =
// w_h[16 ct + (lane & 15)][64 c64 + 32 kc + 8 (lane >> 4) + j][tap / 3][tap % 3].
//
// Workgroup: GC_NW waves.  A wave owns GC_MW pixel tiles and 64 output channels (GC_MW x 4 accumulator tiles); the waves
// are Cout/64 channel groups by NW/(Cout/64) pixel groups, so the workgroup's image tile is MT = GC_MW * NW * 64 / Cout
// pixel tiles: 16 x TXM pixels by MT / TXM rows, TXM = 4 or 2 chosen per call by the smaller padded area.  The tile with
// its 1-pixel halo is staged in LDS as in conv3.hip (channel-last, 16-byte pieces, pitch = channels * 2 + 16 bytes, so the
// window shifts are whole-row shifts of the A fragment's address), but one chunk of GC_CH channels at a time: 448
// channels of the tile do not fit.  With GC_DB the next chunk's items are loaded a few at a time between the current
// chunk's 18 (or 36) K steps and written to the other LDS buffer GC_LAT steps later: one barrier per chunk.  The B fragments come from the
// packed weights in global memory through a register ring GC_PF steps deep.  The result goes back through LDS as
// [channel][pixel], 128 channels per pass; the pass that stores a channel's rows (16 bytes per lane, or by element where
// W, an output, net or z do not allow) applies the epilogue, reading net and z at the pixels it writes.
// No atomics, no workspace, no host synchronisation.
#include <limits.h>

#include "kangru_math.hpp"
#include "lgu_common.hpp"

// experiments only (variant builds); every setting computes the same bits
#ifndef LGU_GC_NW
#define LGU_GC_NW 8      // waves per workgroup: 4 or 8
#endif
#ifndef LGU_GC_MW
#define LGU_GC_MW 4      // pixel tiles per wave
#endif
#ifndef LGU_GC_CH
#define LGU_GC_CH 64     // channels per staged chunk: 64 or 128
#endif
#ifndef LGU_GC_DB
#define LGU_GC_DB 1      // two LDS buffers (the next chunk is loaded under the current chunk's MFMAs) or one
#endif
#ifndef LGU_GC_PF
#define LGU_GC_PF 3      // depth of the weight prefetch in K steps: a divisor of 18
#endif
#ifndef LGU_GC_LAT
#define LGU_GC_LAT 4     // two buffers: K steps between a staging item's loads and its LDS write
#endif
#ifndef LGU_GC_SU
#define LGU_GC_SU 4      // one buffer and the first chunk: staging items whose loads are issued together
#endif

namespace lgu {

constexpr int GC_CIN = LGU_GRUCONV_CIN;    // 448 input channels
constexpr int GC_C64 = GC_CIN / 64;        // 7 chunks of 64 channels in the K order
constexpr int GC_STEPS = GC_C64 * 18;      // 126 K steps
constexpr int GC_BLK = GC_CIN / 32;        // 14 blocks of 32 channels: a block never straddles a segment
constexpr int GC_NW = LGU_GC_NW, GC_MW = LGU_GC_MW, GC_CH = LGU_GC_CH, GC_PF = LGU_GC_PF;
constexpr bool GC_DB = LGU_GC_DB != 0;
constexpr int GC_LAT = LGU_GC_LAT, GC_SU = LGU_GC_SU;
static_assert(GC_NW == 4 || GC_NW == 8, "waves per workgroup");
static_assert(GC_CH == 64 || GC_CH == 128, "channels per staged chunk");
static_assert(GC_PF >= 1 && 18 % GC_PF == 0, "the ring slot of a K step must not depend on the chunk");
static_assert(LGU_GRUCONV_WPACK_HALVES_128 == GC_STEPS * (128 / 16) * kWave * 8, "weight pack size, Cout 128");
static_assert(LGU_GRUCONV_WPACK_HALVES_256 == GC_STEPS * (256 / 16) * kWave * 8, "weight pack size, Cout 256");

struct GcParams {
  const _Float16* blk[GC_BLK];   // per 32-channel block of the concatenated input: its first plane in image 0
  long long img[GC_BLK];         // elements from one image to the next in that block's segment
  const f16x8* wpack;
  const _Float16* bias;
  const _Float16 *k0, *k1, *net, *z;   // ZR: kz, kr, net, -; Q: kq, -, net, z
  _Float16 *out0, *out1;               // PLAIN: out, -; ZR: z, rnet; Q: the new net, -
  int H, W, tiles_x, tiles_y, vec;
};

template <int COUT, int TXM>
struct GcGeom {
  static constexpr int NT = kWave * GC_NW;
  static constexpr int CG = COUT / 64, PG = GC_NW / CG, MT = GC_MW * PG;
  static_assert(GC_NW % CG == 0 && MT % TXM == 0, "waves = channel groups x pixel groups; whole rows of pixel tiles");
  static constexpr int TX = 16 * TXM, TY = MT / TXM, LW = TX + 2, LH = TY + 2;
  static constexpr int PITCH = 2 * GC_CH + 16;          // bytes per staged pixel
  static constexpr int OPITCH = 2 * 16 * MT + 16;       // bytes per channel of the output image in LDS
  static constexpr int BUF = LH * LW * PITCH;
  static constexpr int STAGE = (GC_DB ? 2 : 1) * BUF, OUTB = 128 * OPITCH;
  static constexpr int LDS = STAGE > OUTB ? STAGE : OUTB;
  static_assert(LDS <= 160 * 1024, "the staged chunk(s) do not fit the LDS");
};

// one output element's epilogue on c = half(s); ps: the 128-channel pass (ZR: 0 = z, 1 = r)
template <int MODE>
__device__ __forceinline__ _Float16 gc_epilogue(_Float16 c, int ps, float kk, float nn, float zz) {
  if constexpr (MODE == LGU_GRUCONV_ZR) {
    if (ps == 0) return (_Float16)kg_sigmoid(rnd<_Float16>((float)c + kk));
    const float r = rnd<_Float16>(kg_sigmoid(rnd<_Float16>((float)c + kk)));
    return (_Float16)(r * nn);
  } else if constexpr (MODE == LGU_GRUCONV_Q) {
    const float q = rnd<_Float16>(tanhf(rnd<_Float16>((float)c + kk)));
    const float t1 = rnd<_Float16>(rnd<_Float16>(1.0f - zz) * nn);
    const float t2 = rnd<_Float16>(zz * q);
    return (_Float16)(t1 + t2);
  } else {
    return c;
  }
}

template <int MODE, int COUT, int TXM>
__global__ __launch_bounds__(kWave * GC_NW) void gruconv3x3_c448_kernel(const GcParams P) {
  using G = GcGeom<COUT, TXM>;
  constexpr int NT = G::NT, CG = G::CG, TX = G::TX, TY = G::TY, LW = G::LW, LH = G::LH;
  constexpr int PITCH = G::PITCH, OPITCH = G::OPITCH, BUF = G::BUF;
  constexpr int SUBS = GC_CH / 64, NCH = (GC_C64 + SUBS - 1) / SUBS;   // 64-channel chunks per staged chunk; staged chunks
  constexpr int CTS = COUT / 16;                                       // channel tiles in the pack
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];

  const int H = P.H, W = P.W;
  int b = blockIdx.x;
  const int x0 = (b % P.tiles_x) * TX;
  b /= P.tiles_x;
  const int y0 = (b % P.tiles_y) * TY;
  const int n = b / P.tiles_y;
  const int tid = threadIdx.x, lane = tid & (kWave - 1), w = tid >> 6;
  const int p = lane & 15, g = lane >> 4;
  const int wc = w % CG, wr = w / CG;
  const size_t HW = (size_t)H * W;

  // the wave's first weight fragments and its bias are in flight while the first chunk is staged
  const char* wbase = reinterpret_cast<const char*>(P.wpack);   // + a uniform step offset + the lane's own 32-bit offset
  const unsigned woff = 16u * (unsigned)(4 * wc * kWave + lane);
  auto wfrag = [&](int s, int ct) {
    return *reinterpret_cast<const f16x8*>(wbase + (size_t)(s * CTS + ct) * (kWave * 16) + woff);
  };
  f16x8 bf[GC_PF][4];
#pragma unroll
  for (int s = 0; s < GC_PF; s++)
#pragma unroll
    for (int ct = 0; ct < 4; ct++) bf[s][ct] = wfrag(s, ct);
  float bz[4];
#pragma unroll
  for (int ct = 0; ct < 4; ct++) bz[ct] = (float)P.bias[64 * wc + 16 * ct + p];

  // stage: a thread owns PPT pixels of the tile with its halo (lanes along x) and, per item, reads one pixel of the 8
  // planes of one channel octet and writes one 16-byte piece of the pixel's channel row.  The octet is the same for the
  // whole workgroup, so the planes' addresses are uniform and a lane keeps one 32-bit byte offset per pixel.  Every load
  // is unconditional: a pixel outside the image re-reads the plane's first pixel, an octet past the 448 channels (the
  // last chunk of 128) re-reads segment 0, and both are then zeroed.
  constexpr int PIX = LH * LW, PPT = (PIX + NT - 1) / NT, NIT = (GC_CH / 8) * PPT;
  unsigned goff[PPT];
  bool pin[PPT];
#pragma unroll
  for (int i = 0; i < PPT; i++) {
    const int pix = tid + i * NT;
    const int gy = y0 + pix / LW - 1, gx = x0 + pix % LW - 1;
    pin[i] = pix < PIX && in_bounds(gy, gx, H, W);
    goff[i] = pin[i] ? 2u * ((unsigned)gy * (unsigned)W + (unsigned)gx) : 0u;
  }
  f16x8 raw[NIT];
  auto load_item = [&](int u, int k) {
    const int o = u / PPT, i = u % PPT;
    const int ch = GC_CH * k + 8 * o;
    const bool okc = ch < GC_CIN;
    const int bk = okc ? ch >> 5 : 0;
    const char* base = reinterpret_cast<const char*>(P.blk[bk] + (size_t)n * P.img[bk] + (size_t)(okc ? ch & 31 : 0) * HW);
#pragma unroll
    for (int j = 0; j < 8; j++) raw[u][j] = *reinterpret_cast<const _Float16*>(base + (size_t)j * HW * 2 + goff[i]);
  };
  auto write_item = [&](int u, int k, unsigned char* buf) {
    const int o = u / PPT, i = u % PPT;
    const int pix = tid + i * NT;
    if (pix < PIX) {
      const bool keep = pin[i] && GC_CH * k + 8 * o < GC_CIN;
      f16x8 v;
#pragma unroll
      for (int j = 0; j < 8; j++) v[j] = keep ? raw[u][j] : (_Float16)0.0f;
      *reinterpret_cast<f16x8*>(buf + pix * PITCH + 16 * o) = v;
    }
  };
  auto stage_now = [&](int k, unsigned char* buf) {   // a whole chunk at once, GC_SU items' loads in flight together
#pragma unroll
    for (int u0 = 0; u0 < NIT; u0 += GC_SU) {
#pragma unroll
      for (int u = u0; u < u0 + GC_SU && u < NIT; u++) load_item(u, k);
#pragma unroll
      for (int u = u0; u < u0 + GC_SU && u < NIT; u++) write_item(u, k, buf);
    }
  };
  stage_now(0, smem);
  __syncthreads();

  f32x4 acc[GC_MW][4];
#pragma unroll
  for (int m = 0; m < GC_MW; m++)
#pragma unroll
    for (int ct = 0; ct < 4; ct++) acc[m][ct] = f32x4{bz[ct], bz[ct], bz[ct], bz[ct]};

  // with two buffers the next chunk travels under this chunk's K steps: item u is loaded at step u * STRIDE of the chunk
  // and written to the other buffer GC_LAT steps later (that buffer was last read before the barrier that ended the
  // chunk before this one)
  constexpr int SPC = 18 * SUBS;                                 // K steps per staged chunk
  constexpr int STRIDE = GC_DB ? (SPC - GC_LAT) / NIT : 1;
  static_assert(!GC_DB || STRIDE >= 1, "the chunk's K steps are too few to carry the next chunk's items");
#pragma unroll 1
  for (int k = 0; k < NCH; k++) {
    const unsigned char* abase = smem + (GC_DB ? (k & 1) * BUF : 0) + p * PITCH + 16 * g;
    unsigned char* nxt = smem + ((k + 1) & 1) * BUF;
    const bool more = k + 1 < NCH;
#pragma unroll
    for (int sub = 0; sub < SUBS; sub++) {
      const int c64 = k * SUBS + sub;
      if (c64 < GC_C64) {   // workgroup-uniform: the last staged chunk of 128 holds one chunk of 64
#pragma unroll
        for (int t = 0; t < 18; t++) {
          const int tap = t >> 1, kc = t & 1, ky = tap / 3, kx = tap % 3;
          const int s = c64 * 18 + t;
          if (GC_DB && more) {
            const int tt = 18 * sub + t;
#pragma unroll
            for (int u = 0; u < NIT; u++) {
              if (tt == u * STRIDE + GC_LAT) write_item(u, k + 1, nxt);
              if (tt == u * STRIDE) load_item(u, k + 1);
            }
          }
          f16x8 bw[4];
#pragma unroll
          for (int ct = 0; ct < 4; ct++) bw[ct] = bf[t % GC_PF][ct];
          if (s + GC_PF < GC_STEPS) {   // the slot just read takes the fragments of step s + GC_PF
#pragma unroll
            for (int ct = 0; ct < 4; ct++) bf[t % GC_PF][ct] = wfrag(s + GC_PF, ct);
          }
          f16x8 a[GC_MW];
#pragma unroll
          for (int m = 0; m < GC_MW; m++) {
            const int mt = GC_MW * wr + m, row = mt / TXM, mtx = mt % TXM;
            a[m] = *reinterpret_cast<const f16x8*>(abase + ((row + ky) * LW + 16 * mtx + kx) * PITCH + 128 * sub + 64 * kc);
          }
#pragma unroll
          for (int m = 0; m < GC_MW; m++)
#pragma unroll
            for (int ct = 0; ct < 4; ct++)
              acc[m][ct] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a[m], bw[ct], acc[m][ct], 0, 0, 0);
        }
      }
    }
    __syncthreads();   // every wave has read this chunk (and, with two buffers, written its share of the next)
    if (!GC_DB) {
      if (more) stage_now(k + 1, smem);
      __syncthreads();
    }
  }
  // every wave has read its last A fragment: the LDS becomes the output image, 128 channels per pass

  for (int ps = 0; ps < COUT / 128; ps++) {
    if (ps) __syncthreads();   // the previous pass has been stored
    if (wc / 2 == ps) {
      // [channel][pixel tile][16 pixels] half; a lane's four accumulators are four consecutive pixels of one channel
#pragma unroll
      for (int m = 0; m < GC_MW; m++)
#pragma unroll
        for (int ct = 0; ct < 4; ct++) {
          f16x4 o;
#pragma unroll
          for (int i = 0; i < 4; i++) o[i] = (_Float16)acc[m][ct][i];
          const int cl = 64 * (wc & 1) + 16 * ct + p, mt = GC_MW * wr + m;
          *reinterpret_cast<f16x4*>(smem + cl * OPITCH + 2 * (16 * mt + 4 * g)) = o;
        }
    }
    __syncthreads();

    // pixel tile mt = row * TXM + mtx, so a channel's 16 * MT pixels are its TY rows of TX pixels in order
    _Float16* dst = (MODE == LGU_GRUCONV_ZR && ps == 1) ? P.out1 : P.out0;
    const _Float16* kv = (MODE == LGU_GRUCONV_ZR && ps == 1) ? P.k1 : P.k0;
    const bool need_net = MODE == LGU_GRUCONV_Q || (MODE == LGU_GRUCONV_ZR && ps == 1);
    for (int idx = tid; idx < 128 * TY * (TX / 8); idx += NT) {
      const int ch8 = idx % (TX / 8), t = idx / (TX / 8);
      const int row = t % TY, cl = t / TY;
      const int y = y0 + row, xo = x0 + 8 * ch8;
      if (y >= H || xo >= W) continue;
      f16x8 v = *reinterpret_cast<const f16x8*>(smem + cl * OPITCH + 2 * (row * TX + 8 * ch8));
      const size_t at = ((size_t)n * 128 + cl) * HW + (size_t)y * W + xo;   // in an (N,128,H,W) tensor
      if constexpr (MODE != LGU_GRUCONV_PLAIN) {
        const float kk = (float)kv[(size_t)n * 128 + cl];
        f16x8 vn = {0, 0, 0, 0, 0, 0, 0, 0}, vz = {0, 0, 0, 0, 0, 0, 0, 0};
        if (P.vec) {
          if (need_net) vn = *reinterpret_cast<const f16x8*>(P.net + at);
          if (MODE == LGU_GRUCONV_Q) vz = *reinterpret_cast<const f16x8*>(P.z + at);
        } else {
#pragma unroll
          for (int i = 0; i < 8; i++)
            if (xo + i < W) {
              if (need_net) vn[i] = P.net[at + i];
              if (MODE == LGU_GRUCONV_Q) vz[i] = P.z[at + i];
            }
        }
#pragma unroll
        for (int i = 0; i < 8; i++) v[i] = gc_epilogue<MODE>(v[i], ps, kk, (float)vn[i], (float)vz[i]);
      }
      _Float16* q = (MODE == LGU_GRUCONV_PLAIN) ? dst + ((size_t)n * COUT + 128 * ps + cl) * HW + (size_t)y * W + xo : dst + at;
      if (P.vec) {
        *reinterpret_cast<f16x8*>(q) = v;   // W % 8 == 0 and every tensor touched here 16-byte aligned
      } else {
#pragma unroll
        for (int i = 0; i < 8; i++)
          if (xo + i < W) q[i] = v[i];
      }
    }
  }
}

static inline bool gc_aligned(const void* p, int n) { return (reinterpret_cast<uintptr_t>(p) % n) == 0; }

template <int COUT>
static bool gc_wide_tile(int H, int W) {   // 16 x 4 pixels wide or 16 x 2: the one that pads the image less (ties: the wider)
  constexpr int TY4 = GcGeom<COUT, 4>::TY, TY2 = GcGeom<COUT, 2>::TY;
  const long long pad4 = (long long)((W + 63) / 64 * 64) * ((H + TY4 - 1) / TY4 * TY4);
  const long long pad2 = (long long)((W + 31) / 32 * 32) * ((H + TY2 - 1) / TY2 * TY2);
  return pad4 <= pad2;
}

template <int COUT>
static long long gc_blocks(const lgu_gruconv_args& a) {
  const bool wide = gc_wide_tile<COUT>(a.H, a.W);
  const int TX = wide ? 64 : 32, TY = wide ? GcGeom<COUT, 4>::TY : GcGeom<COUT, 2>::TY;
  return (long long)a.N * ((a.W - 1) / TX + 1) * ((a.H - 1) / TY + 1);
}

template <int MODE, int COUT, int TXM>
static int gc_launch(const lgu_gruconv_args& a, hipStream_t s) {
  using G = GcGeom<COUT, TXM>;
  GcParams P;
  const size_t HW = (size_t)a.H * a.W;
  int bk = 0;
  for (int i = 0; i < a.nseg; i++)
    for (int c = 0; c < a.seg_ch[i]; c += 32, bk++) {
      P.blk[bk] = static_cast<const _Float16*>(a.seg[i]) + (size_t)c * HW;
      P.img[bk] = (long long)a.seg_ch[i] * (long long)HW;
    }
  P.wpack = static_cast<const f16x8*>(a.wpack);
  P.bias = static_cast<const _Float16*>(a.bias);
  P.k0 = static_cast<const _Float16*>(a.k0);
  P.k1 = static_cast<const _Float16*>(a.k1);
  P.net = static_cast<const _Float16*>(a.net);
  P.z = static_cast<const _Float16*>(a.z);
  P.out0 = static_cast<_Float16*>(a.out0);
  P.out1 = static_cast<_Float16*>(a.out1);
  P.H = a.H;
  P.W = a.W;
  P.tiles_x = (a.W - 1) / G::TX + 1;
  P.tiles_y = (a.H - 1) / G::TY + 1;
  bool vec = a.W % 8 == 0 && gc_aligned(a.out0, 16);
  if (MODE == LGU_GRUCONV_ZR) vec = vec && gc_aligned(a.out1, 16) && gc_aligned(a.net, 16);
  if (MODE == LGU_GRUCONV_Q) vec = vec && gc_aligned(a.net, 16) && gc_aligned(a.z, 16);
  P.vec = vec ? 1 : 0;
  const long long blocks = (long long)a.N * P.tiles_x * P.tiles_y;
  if (allow_max_dynamic_lds<gruconv3x3_c448_kernel<MODE, COUT, TXM>>() != hipSuccess) return launch_status();
  hipLaunchKernelGGL((gruconv3x3_c448_kernel<MODE, COUT, TXM>), dim3((unsigned)blocks), dim3(G::NT), G::LDS, s, P);
  return launch_status();
}

template <int MODE, int COUT>
static int gc_launch_tile(const lgu_gruconv_args& a, hipStream_t s) {
  return gc_wide_tile<COUT>(a.H, a.W) ? gc_launch<MODE, COUT, 4>(a, s) : gc_launch<MODE, COUT, 2>(a, s);
}

}  // namespace lgu

extern "C" int lgu_gruconv3x3_c448_h16(lgu_gruconv_args a, void* stream) {
  using namespace lgu;
  if (a.N < 0 || a.H < 1 || a.W < 1 || a.flags != 0) return LGU_E_BADARG;
  if (a.mode != LGU_GRUCONV_PLAIN && a.mode != LGU_GRUCONV_ZR && a.mode != LGU_GRUCONV_Q) return LGU_E_BADARG;
  if (a.nseg < 1 || a.nseg > LGU_GRUCONV_MAX_SEGMENTS) return LGU_E_BADARG;
  if (a.N == 0) return LGU_OK;
  // the operands of the mode: present and at their element's alignment
  const void* need[LGU_GRUCONV_MAX_SEGMENTS + 8];
  int nn = 0;
  for (int i = 0; i < a.nseg; i++) need[nn++] = a.seg[i];
  need[nn++] = a.wpack;
  need[nn++] = a.bias;
  need[nn++] = a.out0;
  if (a.mode != LGU_GRUCONV_PLAIN) {
    need[nn++] = a.k0;
    need[nn++] = a.net;
  }
  if (a.mode == LGU_GRUCONV_ZR) {
    need[nn++] = a.k1;
    need[nn++] = a.out1;
  }
  if (a.mode == LGU_GRUCONV_Q) need[nn++] = a.z;
  for (int i = 0; i < nn; i++)
    if (!need[i] || !gc_aligned(need[i], 2)) return LGU_E_BADARG;
  int sum = 0;
  for (int i = 0; i < a.nseg; i++) {
    if (a.seg_ch[i] < 32 || a.seg_ch[i] > GC_CIN || a.seg_ch[i] % 32 != 0) return LGU_E_UNSUPPORTED;
    sum += a.seg_ch[i];
  }
  if (sum != GC_CIN) return LGU_E_UNSUPPORTED;
  const bool cout_ok = a.mode == LGU_GRUCONV_PLAIN ? (a.Cout == 128 || a.Cout == 256)
                                                   : a.Cout == (a.mode == LGU_GRUCONV_ZR ? 256 : 128);
  if (!cout_ok) return LGU_E_UNSUPPORTED;
  if (!gc_aligned(a.wpack, 16)) return LGU_E_UNSUPPORTED;
  if ((long long)a.H * a.W > (1 << 30)) return LGU_E_UNSUPPORTED;   // a pixel's byte offset in its plane is 32 bits
  if ((a.Cout == 256 ? gc_blocks<256>(a) : gc_blocks<128>(a)) > INT_MAX) return LGU_E_UNSUPPORTED;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (a.mode == LGU_GRUCONV_ZR) return gc_launch_tile<LGU_GRUCONV_ZR, 256>(a, s);
  if (a.mode == LGU_GRUCONV_Q) return gc_launch_tile<LGU_GRUCONV_Q, 128>(a, s);
  return a.Cout == 256 ? gc_launch_tile<LGU_GRUCONV_PLAIN, 256>(a, s) : gc_launch_tile<LGU_GRUCONV_PLAIN, 128>(a, s);
}
