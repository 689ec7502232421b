// heads.hip — the update operator's narrow output heads, Conv2d(128, 1 | 2, 3, padding=1) with the bias and an optional
// sigmoid or softplus, as they are evaluated under float16 autocast (reference droid_slam/droid_net.py: delta[2],
// weight[2] + Sigmoid, GraphAgg.eta + GradientClip + Softplus), NCHW in and NCHW out, in one launch:
//
//   x_h = half(x), w_h = half(weight), b_h = half(bias)            (round to nearest even; a half x is used as it is)
//   p_t = sum_c x_h[c, y+ky-1, x+kx-1] * w_h[co,c,ky,kx]            (t = 3 ky + kx; exact products, fp32 accumulation)
//   s   = b_h + p_0 + p_1 + ... + p_8                               (fp32, left to right; zero padding)
//   h   = half(s)                                                   (one rounding)
//   y   = h | half(sigmoid_f32(h)) | softplus_f32(h) as float32     (all three keep a NaN)
//
// Mapping: pixels on M, the 9 * Cout per-tap partial sums on N.  With 16 output channels per MFMA tile these layers would
// be seven-eighths padding; instead the layer is a 1x1 GEMM over K = 128 (v_mfma_f32_16x16x32_f16, four K steps of 32
// channels, always kc = 0..3) whose 9 * Cout columns are the products of a STAGED pixel with the weights of each tap,
// followed by the shifted 9-tap sum of those partials.  Cout 2: 18 columns in two tiles of 16 (14 zero columns); Cout 1: 9
// columns in one tile (7 zero columns).  There is no im2col restaging: a staged pixel enters exactly one MFMA row.
//
// Workgroup: 4 waves, an image tile of 32 x 4 pixels.  The tile with its 1-pixel halo (34 x 6 = 204 pixels, 13 groups of
// 16) is staged in LDS as half, channel-last, exactly as csrc/conv3.hip stages it (a thread reads one pixel of 8 channel
// planes, lanes along x, and writes one 16-byte piece of the pixel's 256-byte channel row; pixel pitch 272 bytes, so the
// 16 pixels of a 16-lane read group fall in 16 different 16-byte slots of the bank row).  Wave w takes the pixel groups
// w, w + 4, w + 8 (and 12 for w = 0): per group 4 A fragments (lane l: pixel l & 15, channels 32 kc + 8 (l >> 4) ..+8,
// one ds_read_b128) against the wave's resident B fragments of the packed weights.  The partials go to a second LDS
// region as [column][staged pixel] fp32 (a lane's four accumulators are four consecutive pixels of one column: one
// 16-byte store).  After the barrier thread (co, ty, tx) adds its nine partials to the bias in the order t = 0..8 (lanes
// along tx: conflict-free) and stores one element, lanes along x.  The order never depends on the tile, the batch or N.
// A pixel outside the image is staged as zero and its partials are +0.  No atomics, no workspace, no host synchronisation.
//
// head3x3_pair_c128_kernel runs delta[2] and weight[2] + Sigmoid in one launch (the head follows the block index) and
// writes them edge-major, (N,H,W,2), one store per pixel; optionally as float32 with delta added to the coordinates.
#include <limits.h>

#include <type_traits>

#include "kangru_math.hpp"
#include "lgu_common.hpp"

namespace lgu {

constexpr int HD_CI = 128;                  // input channels
constexpr int HD_THREADS = 256;
constexpr int HD_TX = 32, HD_TY = 4;        // output pixels per workgroup
constexpr int HD_LW = HD_TX + 2, HD_LH = HD_TY + 2;
constexpr int HD_PIX = HD_LW * HD_LH;       // 204 staged pixels
constexpr int HD_GROUPS = (HD_PIX + 15) / 16;   // 13 MFMA row groups
constexpr int HD_PITCH = 2 * HD_CI + 16;    // bytes per staged pixel: 256 of channels + one 16-byte slot
constexpr int HD_XBYTES = 16 * HD_GROUPS * HD_PITCH;
constexpr int HD_PPITCH = 16 * HD_GROUPS + 4;   // floats per column of partials
constexpr int HD_SU = 13;                   // staging items whose loads a thread issues before it converts any of them: all
                                            // of a thread's (16 * 204 items over 256 threads), one round trip to memory

static_assert(LGU_HEAD_WPACK_HALVES_1 == 4 * 1 * kWave * 8, "weight pack size, Cout 1");
static_assert(LGU_HEAD_WPACK_HALVES_2 == 4 * 2 * kWave * 8, "weight pack size, Cout 2");
static_assert(HD_TX * HD_TY * 2 == HD_THREADS, "one thread per output element at Cout 2");

template <int COUT>
constexpr int hd_lds_bytes() {
  return HD_XBYTES + 9 * COUT * HD_PPITCH * 4;
}

__device__ __forceinline__ float hd_softplus(float v) {   // beta 1, threshold 20; a NaN compares false and goes through log1p(exp)
  return v > 20.0f ? v : log1pf(expf(v));
}

// ---- the phases every kernel of this file shares: the wave's weight fragments, the staging of the tile, the MFMA phase
// and the partials in LDS.  On return (behind a barrier) part holds [column][staged pixel] fp32.
template <int NT, int NP, typename XT>
__device__ __forceinline__ void hd_partials(unsigned char* smem, float* part, const XT* __restrict__ src,
                                            const f16x8* __restrict__ wpack, int y0, int x0, int H, int W, size_t HW) {
  const int tid = threadIdx.x, lane = tid & (kWave - 1), w = tid >> 6;
  const int p = lane & 15, g = lane >> 4;
  // the wave's weight fragments are in flight while the tile is staged
  f16x8 bw[4][NT];
#pragma unroll
  for (int kc = 0; kc < 4; kc++)
#pragma unroll
    for (int nt = 0; nt < NT; nt++) bw[kc][nt] = wpack[(kc * NT + nt) * kWave + lane];

  // stage (csrc/conv3.hip): one (channel octet, row, pixel) per thread and item, lanes along x; a pixel outside the image
  // re-reads the image's first pixel and is then zeroed, so every load is unconditional
  constexpr int ITEMS = 16 * HD_PIX;
  for (int base = tid; base < ITEMS; base += HD_SU * HD_THREADS) {
    XT raw[HD_SU][8];
    bool inside[HD_SU];
#pragma unroll
    for (int u = 0; u < HD_SU; u++) {
      const int idx = base + u * HD_THREADS;
      const int c = idx % HD_LW, t = idx / HD_LW;
      const int r = t % HD_LH, o = t / HD_LH;
      const int gy = y0 + r - 1, gx = x0 + c - 1;
      inside[u] = idx < ITEMS && in_bounds(gy, gx, H, W);
      const XT* q = src + (inside[u] ? (size_t)(8 * o) * HW + (size_t)gy * W + gx : (size_t)0);
#pragma unroll
      for (int ch = 0; ch < 8; ch++) raw[u][ch] = q[ch * HW];
    }
#pragma unroll
    for (int u = 0; u < HD_SU; u++) {
      const int idx = base + u * HD_THREADS;
      if (idx < ITEMS) {
        const int c = idx % HD_LW, t = idx / HD_LW;
        const int r = t % HD_LH;
        f16x8 v;
#pragma unroll
        for (int ch = 0; ch < 8; ch++) v[ch] = inside[u] ? (_Float16)raw[u][ch] : (_Float16)0.0f;
        *reinterpret_cast<f16x8*>(smem + (r * HD_LW + c) * HD_PITCH + 16 * (t / HD_LH)) = v;
      }
    }
  }
  // the rows that fill the last group of 16: zero, so that their (unread) partials are zero too
  if (tid < 16 * (16 * HD_GROUPS - HD_PIX)) {
    f16x8 z;
#pragma unroll
    for (int ch = 0; ch < 8; ch++) z[ch] = (_Float16)0.0f;
    *reinterpret_cast<f16x8*>(smem + (HD_PIX + (tid >> 4)) * HD_PITCH + 16 * (tid & 15)) = z;
  }
  __syncthreads();

  for (int grp = w; grp < HD_GROUPS; grp += HD_THREADS / kWave) {
    const unsigned char* abase = smem + (16 * grp + p) * HD_PITCH + 16 * g;
    f32x4 acc[NT];
#pragma unroll
    for (int nt = 0; nt < NT; nt++) acc[nt] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int kc = 0; kc < 4; kc++) {
      const f16x8 a = *reinterpret_cast<const f16x8*>(abase + 64 * kc);
#pragma unroll
      for (int nt = 0; nt < NT; nt++) acc[nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, bw[kc][nt], acc[nt], 0, 0, 0);
    }
    // a lane's four accumulators: staged pixels 16 grp + 4 g ..+4 of column 16 nt + p
#pragma unroll
    for (int nt = 0; nt < NT; nt++) {
      const int col = 16 * nt + p;
      if (col < NP) *reinterpret_cast<f32x4*>(part + col * HD_PPITCH + 16 * grp + 4 * g) = acc[nt];
    }
  }
  __syncthreads();
}

template <int COUT, bool XH, int ACT>   // ACT 0: none, 1: sigmoid, 2: softplus (float32 out)
__global__ __launch_bounds__(HD_THREADS) void head3x3_c128_kernel(const void* __restrict__ xv, const f16x8* __restrict__ wpack,
                                                                 const _Float16* __restrict__ bias, void* __restrict__ outv,
                                                                 int H, int W, int tiles_x, int tiles_y) {
  using XT = typename std::conditional<XH, _Float16, float>::type;
  using OT = typename std::conditional<ACT == 2, float, _Float16>::type;
  constexpr int NP = 9 * COUT;             // columns of partials
  constexpr int NT = (NP + 15) / 16;       // MFMA column tiles
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  float* part = reinterpret_cast<float*>(smem + HD_XBYTES);

  int b = blockIdx.x;
  const int x0 = (b % tiles_x) * HD_TX;
  b /= tiles_x;
  const int y0 = (b % tiles_y) * HD_TY;
  const int n = b / tiles_y;
  const int tid = threadIdx.x;
  const size_t HW = (size_t)H * W;

  hd_partials<NT, NP, XT>(smem, part, static_cast<const XT*>(xv) + (size_t)n * HD_CI * HW, wpack, y0, x0, H, W, HW);

  const int co = tid / (HD_TX * HD_TY), pix = tid % (HD_TX * HD_TY);
  const int ty = pix / HD_TX, tx = pix % HD_TX;
  const int y = y0 + ty, xo = x0 + tx;
  if (co >= COUT || y >= H || xo >= W) return;
  float s = (float)bias[co];
#pragma unroll
  for (int t = 0; t < 9; t++) s += part[(t * COUT + co) * HD_PPITCH + (ty + t / 3) * HD_LW + tx + t % 3];
  const _Float16 h = (_Float16)s;
  OT* dst = static_cast<OT*>(outv) + ((size_t)n * COUT + co) * HW + (size_t)y * W + xo;
  if (ACT == 1) {
    *dst = (OT)kg_sigmoid((float)h);
  } else if (ACT == 2) {
    *dst = (OT)hd_softplus((float)h);
  } else {
    *dst = (OT)h;
  }
}

static inline bool hd_aligned(const void* p, int n) { return (reinterpret_cast<uintptr_t>(p) % n) == 0; }

template <int COUT, bool XH, int ACT>
static int hd_launch(const lgu_head_args& a, unsigned blocks, int tiles_x, int tiles_y, hipStream_t s) {
  auto kern = head3x3_c128_kernel<COUT, XH, ACT>;
  if (allow_max_dynamic_lds<head3x3_c128_kernel<COUT, XH, ACT>>() != hipSuccess) return launch_status();
  hipLaunchKernelGGL(kern, dim3(blocks), dim3(HD_THREADS), hd_lds_bytes<COUT>(), s, a.x, static_cast<const f16x8*>(a.wpack),
                     static_cast<const _Float16*>(a.bias), a.out, a.H, a.W, tiles_x, tiles_y);
  return launch_status();
}

// ---- the pair: delta[2] (head 0, no activation) and weight[2] (head 1, sigmoid) in one launch, edge-major.  Blocks
// [0, tiles) are head 0 and [tiles, 2 tiles) head 1; the input, pack, bias and output follow the head.  hd_partials and
// the nine-tap sum are head3x3_c128_kernel<2, XH, .>'s, so h has its bits.  One thread owns one pixel and stores both
// channels together: (N,H,W,2) half, or float32 with F32, where head 0 adds h to coords at that element (one fp32 add).
struct HdPairOperands {
  const void* x[2];
  const f16x8* wpack[2];
  const _Float16* bias[2];
  void* out[2];
  const float* coords;
};

template <bool XH, bool F32>
__global__ __launch_bounds__(HD_THREADS) void head3x3_pair_c128_kernel(HdPairOperands ops, int H, int W, int tiles_x, int tiles_y,
                                                                      int tiles) {
  using XT = typename std::conditional<XH, _Float16, float>::type;
  constexpr int NP = 18, NT = 2;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  float* part = reinterpret_cast<float*>(smem + HD_XBYTES);

  int b = blockIdx.x;
  const int head = b >= tiles ? 1 : 0;     // block-uniform
  b -= head * tiles;
  const int x0 = (b % tiles_x) * HD_TX;
  b /= tiles_x;
  const int y0 = (b % tiles_y) * HD_TY;
  const int n = b / tiles_y;
  const int tid = threadIdx.x;
  const size_t HW = (size_t)H * W;
  const XT* src = static_cast<const XT*>(head ? ops.x[1] : ops.x[0]) + (size_t)n * HD_CI * HW;
  const _Float16* bias = head ? ops.bias[1] : ops.bias[0];

  hd_partials<NT, NP, XT>(smem, part, src, head ? ops.wpack[1] : ops.wpack[0], y0, x0, H, W, HW);

  const int ty = tid / HD_TX, tx = tid % HD_TX;
  const int y = y0 + ty, xo = x0 + tx;
  if (tid >= HD_TX * HD_TY || y >= H || xo >= W) return;
  _Float16 h[2];
#pragma unroll
  for (int co = 0; co < 2; co++) {
    float s = (float)bias[co];
#pragma unroll
    for (int t = 0; t < 9; t++) s += part[(t * 2 + co) * HD_PPITCH + (ty + t / 3) * HD_LW + tx + t % 3];
    h[co] = (_Float16)s;
  }
  if (head) {
#pragma unroll
    for (int co = 0; co < 2; co++) h[co] = (_Float16)kg_sigmoid((float)h[co]);
  }
  const size_t pix = (size_t)n * HW + (size_t)y * W + xo;
  void* outv = head ? ops.out[1] : ops.out[0];
  if (F32) {
    f32x2 v = f32x2{(float)h[0], (float)h[1]};
    if (!head) {
      const f32x2 c = reinterpret_cast<const f32x2*>(ops.coords)[pix];
      v = f32x2{c[0] + v[0], c[1] + v[1]};
    }
    static_cast<f32x2*>(outv)[pix] = v;
  } else {
    static_cast<f16x2*>(outv)[pix] = f16x2{h[0], h[1]};
  }
}

template <bool XH, bool F32>
static int hd_pair_launch(const lgu_head_pair_args& a, int tiles_x, int tiles_y, int tiles, hipStream_t s) {
  auto kern = head3x3_pair_c128_kernel<XH, F32>;
  if (allow_max_dynamic_lds<head3x3_pair_c128_kernel<XH, F32>>() != hipSuccess) return launch_status();
  HdPairOperands ops;
  for (int k = 0; k < 2; k++) {
    ops.x[k] = a.x[k];
    ops.wpack[k] = static_cast<const f16x8*>(a.wpack[k]);
    ops.bias[k] = static_cast<const _Float16*>(a.bias[k]);
    ops.out[k] = a.out[k];
  }
  ops.coords = static_cast<const float*>(a.coords);
  hipLaunchKernelGGL(kern, dim3(2u * (unsigned)tiles), dim3(HD_THREADS), hd_lds_bytes<2>(), s, ops, a.H, a.W, tiles_x, tiles_y,
                     tiles);
  return launch_status();
}

template <int COUT, bool XH>
static int hd_launch_act(const lgu_head_args& a, unsigned blocks, int tiles_x, int tiles_y, hipStream_t s) {
  if (a.flags & LGU_HEAD_SIGMOID) return hd_launch<COUT, XH, 1>(a, blocks, tiles_x, tiles_y, s);
  if (a.flags & LGU_HEAD_SOFTPLUS) return hd_launch<COUT, XH, 2>(a, blocks, tiles_x, tiles_y, s);
  return hd_launch<COUT, XH, 0>(a, blocks, tiles_x, tiles_y, s);
}

}  // namespace lgu

extern "C" int lgu_head3x3_c128_h16(lgu_head_args a, void* stream) {
  using namespace lgu;
  constexpr int kFlags = LGU_HEAD_X_HALF | LGU_HEAD_SIGMOID | LGU_HEAD_SOFTPLUS;
  if (a.N < 0 || a.H < 0 || a.W < 0 || (a.flags & ~kFlags)) return LGU_E_BADARG;
  if (a.N == 0 || a.H == 0 || a.W == 0) return LGU_OK;
  if (!a.x || !a.wpack || !a.bias || !a.out) return LGU_E_BADARG;
  const bool xh = (a.flags & LGU_HEAD_X_HALF) != 0;
  if (!hd_aligned(a.x, xh ? 2 : 4) || !hd_aligned(a.bias, 2) || !hd_aligned(a.out, (a.flags & LGU_HEAD_SOFTPLUS) ? 4 : 2))
    return LGU_E_BADARG;
  if (a.Cout != 1 && a.Cout != 2) return LGU_E_UNSUPPORTED;
  if ((a.flags & LGU_HEAD_SIGMOID) && (a.flags & LGU_HEAD_SOFTPLUS)) return LGU_E_UNSUPPORTED;
  if (!hd_aligned(a.wpack, 16)) return LGU_E_UNSUPPORTED;
  const int tiles_x = (a.W - 1) / HD_TX + 1, tiles_y = (a.H - 1) / HD_TY + 1;
  const long long blocks = (long long)a.N * tiles_x * tiles_y;
  if (blocks > INT_MAX) return LGU_E_UNSUPPORTED;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (a.Cout == 2)
    return xh ? hd_launch_act<2, true>(a, (unsigned)blocks, tiles_x, tiles_y, s) : hd_launch_act<2, false>(a, (unsigned)blocks, tiles_x, tiles_y, s);
  return xh ? hd_launch_act<1, true>(a, (unsigned)blocks, tiles_x, tiles_y, s) : hd_launch_act<1, false>(a, (unsigned)blocks, tiles_x, tiles_y, s);
}

extern "C" int lgu_head3x3_pair_c128_h16(lgu_head_pair_args a, void* stream) {
  using namespace lgu;
  constexpr int kFlags = LGU_HEAD_X_HALF | LGU_HEAD_PAIR_F32;
  if (a.N < 0 || a.H < 0 || a.W < 0 || (a.flags & ~kFlags)) return LGU_E_BADARG;
  const bool xh = (a.flags & LGU_HEAD_X_HALF) != 0, f32 = (a.flags & LGU_HEAD_PAIR_F32) != 0;
  if (f32 != (a.coords != nullptr)) return LGU_E_BADARG;      // the float32 mode is the one with coords
  if (a.N == 0 || a.H == 0 || a.W == 0) return LGU_OK;
  for (int k = 0; k < 2; k++) {
    if (!a.x[k] || !a.wpack[k] || !a.bias[k] || !a.out[k]) return LGU_E_BADARG;
    if (!hd_aligned(a.x[k], xh ? 2 : 4) || !hd_aligned(a.bias[k], 2) || !hd_aligned(a.out[k], f32 ? 4 : 2)) return LGU_E_BADARG;
  }
  if (f32 && !hd_aligned(a.coords, 4)) return LGU_E_BADARG;
  for (int k = 0; k < 2; k++)      // a pixel's two channels are one store
    if (!hd_aligned(a.wpack[k], 16) || !hd_aligned(a.out[k], f32 ? 8 : 4)) return LGU_E_UNSUPPORTED;
  if (f32 && !hd_aligned(a.coords, 8)) return LGU_E_UNSUPPORTED;
  const int tiles_x = (a.W - 1) / HD_TX + 1, tiles_y = (a.H - 1) / HD_TY + 1;
  const long long tiles = (long long)a.N * tiles_x * tiles_y;
  if (2 * tiles > INT_MAX) return LGU_E_UNSUPPORTED;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (f32) return xh ? hd_pair_launch<true, true>(a, tiles_x, tiles_y, (int)tiles, s) : hd_pair_launch<false, true>(a, tiles_x, tiles_y, (int)tiles, s);
  return xh ? hd_pair_launch<true, false>(a, tiles_x, tiles_y, (int)tiles, s) : hd_pair_launch<false, false>(a, tiles_x, tiles_y, (int)tiles, s);
}
