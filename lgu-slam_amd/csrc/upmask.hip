// upmask.hip — GraphAgg's upsampling-mask layer, Conv2d(128, 576, 1) with its bias as float16 autocast evaluates it
// (reference droid_slam/droid_net.py:50-51,67), in two forms that share ONE GEMM main loop (um_gemm):
//
//   lgu_upmask1x1_c128_h16   the layer: x (N,128,H,W) -> h (N,576,H,W) half, NCHW in and NCHW out
//   lgu_upmask_upsample_f32  the layer, the 9-way softmax and the convex combination of the disparity (DepthVideo.upsample,
//                            depth_video.py:124-128; csrc/aggregate.hip) in one launch: the 576 planes never reach memory
//
//   x_h = half(x), w_h = half(weight), b_h = half(bias)            (round to nearest even; a half x is used as it is)
//   p   = sum_c x_h[c] * w_h[co,c]                                  (exact products; fp32 accumulation from zero in four
//                                                                    steps of 32 channels, kc = 0..3)
//   h   = half(b_h + p)                                             (one fp32 addition, one rounding to half)
//
// Mapping: the layer is the GEMM (576 x 128) . (128 x pixels) on v_mfma_f32_16x16x32_f16 with A = weights (16 output
// channels per tile, 36 row tiles mt) and B = a group of 16 pixels, so lane l = 16 g + p owns the four consecutive channels
// 16 mt + 4 g + i of pixel p.  Wave q of a workgroup's four owns the nine tiles mt = 4 k + q, k = 0..8: channel
// 64 k + 16 q + 4 g + i = k * 64 + a * 8 + b with a = 2 q + (g >> 1), b = 4 (g & 1) + i, which is all nine taps k of the four
// neighbouring sub-pixels (a, b .. b + 3) of one coarse pixel.  The softmax over k and the nine-tap sum of the fused form
// are therefore register-only, and a lane's result is one 16-byte store (16 pixels along x: 512 contiguous bytes per
// fine row).  A wave keeps its 36 weight fragments (144 VGPRs) for all its pixel groups; two workgroups fit a CU.
//
// Pixels are numbered through the whole batch (gp = n * H * W + y * W + x); a group is 16 consecutive gp and may span two
// frames, every lane resolves its own pixel.  A workgroup takes a contiguous range of groups.  Per group each of the 256
// threads stages one (pixel, channel octet): 8 element loads from the channel planes (16 lanes along the pixels), rounded
// to half, one 16-byte LDS store into the pixel's 256-byte channel row (pitch 272 bytes); the four waves then read their B
// fragments (lane: pixel p, channels 32 kc + 8 g ..+8, one ds_read_b128 per kc) from the same staged group.  The LDS
// buffer is double: the loads of the next group are issued before the MFMAs of this one, one barrier per group.
// The eager form stores its halves from the accumulator layout by element (16 lanes: 32 contiguous bytes of one channel
// plane, the next group of the same workgroup continues the run).  No atomics, no workspace, no host synchronisation; the
// bits of a pixel depend on that pixel's 128 inputs only (MFMA columns are independent), not on N, the group or the grid.
#include <limits.h>

#include <type_traits>

#include "lgu_common.hpp"

namespace lgu {

constexpr int UM_CI = 128;                  // input channels
constexpr int UM_CO = 576;                  // output channels = 9 taps x 8 x 8 sub-pixels
constexpr int UM_THREADS = 256;
constexpr int UM_TAPS = 9;                  // row tiles per wave
constexpr int UM_PITCH = 2 * UM_CI + 16;    // bytes per staged pixel: 256 of channels + one 16-byte slot
constexpr int UM_BUF = 16 * UM_PITCH;       // one staged group

static_assert(LGU_UPMASK_WPACK_HALVES == UM_CO * UM_CI, "weight pack size");
static_assert(LGU_UPMASK_WPACK_HALVES == 36 * 4 * kWave * 8, "36 row tiles x 4 K steps of lane fragments");
static_assert(16 * 16 == UM_THREADS, "one (pixel, channel octet) per thread and group");

// The GEMM main loop both kernels share: h[k][i] = half(b_h + sum_c x_h[c] * w_h[co, c]) for the lane's channels
// co = 64 k + 16 q + 4 g + i of the staged pixel p (bs: the bias in LDS from channel 16 q + 4 g on).  Four K steps
// kc = 0..3 from zero, then the bias, then one rounding.
__device__ __forceinline__ void um_gemm(const unsigned char* __restrict__ xs, const f16x8 (&aw)[UM_TAPS][4],
                                        const _Float16* __restrict__ bs, int p, int g, f16x4 (&h)[UM_TAPS]) {
  f16x8 b[4];
#pragma unroll
  for (int kc = 0; kc < 4; kc++) b[kc] = *reinterpret_cast<const f16x8*>(xs + p * UM_PITCH + 64 * kc + 16 * g);
#pragma unroll
  for (int k = 0; k < UM_TAPS; k++) {
    f32x4 acc = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int kc = 0; kc < 4; kc++) acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(aw[k][kc], b[kc], acc, 0, 0, 0);
    const f16x4 bh = *reinterpret_cast<const f16x4*>(bs + 64 * k);
#pragma unroll
    for (int i = 0; i < 4; i++) h[k][i] = (_Float16)((float)bh[i] + acc[i]);
  }
}

// FUSED false: out = h (N,576,H,W) half.  FUSED true: x holds U frames, out = disps_up (N,8H,8W) float, rows ix[u].
template <bool XH, bool FUSED, bool HALFW>
__global__ __launch_bounds__(UM_THREADS, 2) void upmask_kernel(const void* __restrict__ xv, const f16x8* __restrict__ wpack,
                                                               const _Float16* __restrict__ bias, void* __restrict__ outv,
                                                               const float* __restrict__ disps, const long long* __restrict__ ix,
                                                               int N, int H, int W, int total, int groups, int per) {
  using XT = typename std::conditional<XH, _Float16, float>::type;
  __shared__ __attribute__((aligned(16))) unsigned char smem[2 * UM_BUF];
  __shared__ __attribute__((aligned(16))) _Float16 sbias[UM_CO];
  const int g0 = blockIdx.x * per;
  const int g1 = g0 + per < groups ? g0 + per : groups;
  if (g0 >= g1) return;
  const int tid = threadIdx.x, lane = tid & (kWave - 1), q = tid >> 6;
  const int p = lane & 15, g = lane >> 4;
  const int HW = H * W;

  // the wave's weight fragments stay in registers for all its groups; the bias waits in LDS (read by element: it is
  // served at element alignment), visible after the first group's barrier
  f16x8 aw[UM_TAPS][4];
#pragma unroll
  for (int k = 0; k < UM_TAPS; k++)
#pragma unroll
    for (int kc = 0; kc < 4; kc++) aw[k][kc] = wpack[((4 * k + q) * 4 + kc) * kWave + lane];
  for (int c = tid; c < UM_CO; c += UM_THREADS) sbias[c] = bias[c];
  const _Float16* bs = sbias + 16 * q + 4 * g;

  // staging: thread = (pixel sp of the group, channel octet so); a pixel past the end re-reads the last pixel (its
  // results are never stored), so every load is unconditional
  const int sp = tid & 15, so = tid >> 4;
  const XT* xb = static_cast<const XT*>(xv);
  XT raw[8];
  auto load_group = [&](int grp) {
    int gp = 16 * grp + sp;
    gp = gp < total ? gp : total - 1;
    const int n = gp / HW, pi = gp - n * HW;
    const XT* src = xb + ((size_t)n * UM_CI + 8 * so) * HW + pi;
#pragma unroll
    for (int ch = 0; ch < 8; ch++) raw[ch] = src[(size_t)ch * HW];
  };
  load_group(g0);

  for (int grp = g0; grp < g1; grp++) {
    unsigned char* buf = smem + ((grp - g0) & 1) * UM_BUF;
    f16x8 v;
#pragma unroll
    for (int ch = 0; ch < 8; ch++) v[ch] = (_Float16)raw[ch];
    *reinterpret_cast<f16x8*>(buf + sp * UM_PITCH + 16 * so) = v;
    // one barrier per group: the buffer written two groups later is this one, and a wave gets there only through the
    // next group's barrier, which every wave reaches after its reads of this group
    __syncthreads();
    if (grp + 1 < g1) load_group(grp + 1);

    f16x4 h[UM_TAPS];
    um_gemm(buf, aw, bs, p, g, h);

    const int gp = 16 * grp + p;
    if (gp >= total) continue;
    const int n = gp / HW, pi = gp - n * HW;
    if (!FUSED) {
      _Float16* dst = static_cast<_Float16*>(outv) + ((size_t)n * UM_CO + 16 * q + 4 * g) * HW + pi;
#pragma unroll
      for (int k = 0; k < UM_TAPS; k++)
#pragma unroll
        for (int i = 0; i < 4; i++) dst[(size_t)(64 * k + i) * HW] = h[k][i];
    } else {
      const long long row = ix[n];
      if (row < 0 || row >= N) continue;
      const int y = pi / W, x = pi - y * W;
      const float* d = disps + (size_t)row * HW;
      float nb[UM_TAPS];   // the disparity at (y + ky - 1, x + kx - 1), 0 outside the frame
#pragma unroll
      for (int k = 0; k < UM_TAPS; k++) {
        const int yy = y + k / 3 - 1, xx = x + k % 3 - 1;
        nb[k] = in_bounds(yy, xx, H, W) ? d[(size_t)yy * W + xx] : 0.0f;
      }
      // csrc/aggregate.hip's per-output rule on the lane's sub-pixels (a, b + i)
      f32x4 res;
#pragma unroll
      for (int i = 0; i < 4; i++) {
        float xk[UM_TAPS];
#pragma unroll
        for (int k = 0; k < UM_TAPS; k++) xk[k] = (float)h[k][i];
        float mx = xk[0];
#pragma unroll
        for (int k = 1; k < UM_TAPS; k++) mx = xk[k] > mx ? xk[k] : mx;
        float e[UM_TAPS];
        float s = 0.0f;
#pragma unroll
        for (int k = 0; k < UM_TAPS; k++) {
          e[k] = expf(xk[k] - mx);
          s = s + e[k];
        }
        float acc = 0.0f;
#pragma unroll
        for (int k = 0; k < UM_TAPS; k++) {
          float wk = e[k] / s;
          if (HALFW) wk = (float)(_Float16)wk;
          const float prod = wk * nb[k];
          acc = k == 0 ? prod : acc + prod;
        }
        res[i] = acc;
      }
      const int a = 2 * q + (g >> 1), b = 4 * (g & 1);
      float* o = static_cast<float*>(outv) + (size_t)row * 64 * HW + (size_t)(8 * y + a) * 8 * W + 8 * x + b;
      *reinterpret_cast<f32x4*>(o) = res;
    }
  }
}

static inline bool um_aligned(const void* p, int n) { return (reinterpret_cast<uintptr_t>(p) % n) == 0; }

template <bool XH, bool FUSED, bool HALFW>
static int um_launch(const void* x, const void* wpack, const void* bias, void* out, const float* disps, const long long* ix,
                     int N, int H, int W, int total, hipStream_t s) {
  const int groups = (total + 15) / 16;
  const int want = 2 * device_cu_count();
  const int per = (groups + want - 1) / want;
  const int blocks = (groups + per - 1) / per;
  hipLaunchKernelGGL((upmask_kernel<XH, FUSED, HALFW>), dim3(blocks), dim3(UM_THREADS), 0, s, x, static_cast<const f16x8*>(wpack),
                     static_cast<const _Float16*>(bias), out, disps, ix, N, H, W, total, groups, per);
  return launch_status();
}

}  // namespace lgu

extern "C" int lgu_upmask1x1_c128_h16(lgu_upmask_args a, void* stream) {
  using namespace lgu;
  if (a.N < 0 || a.H < 0 || a.W < 0 || (a.flags & ~LGU_UPMASK_X_HALF)) return LGU_E_BADARG;
  if (a.N == 0 || a.H == 0 || a.W == 0) return LGU_OK;
  if (!a.x || !a.wpack || !a.bias || !a.out) return LGU_E_BADARG;
  const bool xh = (a.flags & LGU_UPMASK_X_HALF) != 0;
  if (!um_aligned(a.x, xh ? 2 : 4) || !um_aligned(a.bias, 2) || !um_aligned(a.out, 2)) return LGU_E_BADARG;
  if (!um_aligned(a.wpack, 16)) return LGU_E_UNSUPPORTED;
  const long long total = (long long)a.N * a.H * a.W;
  if (total > INT_MAX - 16) return LGU_E_UNSUPPORTED;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  return xh ? um_launch<true, false, false>(a.x, a.wpack, a.bias, a.out, nullptr, nullptr, a.N, a.H, a.W, (int)total, s)
            : um_launch<false, false, false>(a.x, a.wpack, a.bias, a.out, nullptr, nullptr, a.N, a.H, a.W, (int)total, s);
}

extern "C" int lgu_upmask_upsample_f32(lgu_upmask_ups_args a, void* stream) {
  using namespace lgu;
  if (a.N < 0 || a.U < 0 || a.ht < 0 || a.wd < 0) return LGU_E_BADARG;
  if ((a.flags & ~(LGU_UPMASK_X_HALF | LGU_UPS_HALF_WEIGHTS)) != 0) return LGU_E_BADARG;
  if ((long long)a.ht * a.wd > (long long)INT_MAX / 576) return LGU_E_BADARG;
  if ((long long)a.U * a.ht * a.wd == 0 || a.N == 0) return LGU_OK;   // nothing to write
  if (!a.x || !a.wpack || !a.bias || !a.disps || !a.ix || !a.disps_up) return LGU_E_BADARG;
  const bool xh = (a.flags & LGU_UPMASK_X_HALF) != 0, halfw = (a.flags & LGU_UPS_HALF_WEIGHTS) != 0;
  if (!um_aligned(a.x, xh ? 2 : 4) || !um_aligned(a.bias, 2) || !um_aligned(a.disps, 4) || !um_aligned(a.ix, 8))
    return LGU_E_BADARG;
  if (!um_aligned(a.wpack, 16) || !um_aligned(a.disps_up, 16)) return LGU_E_UNSUPPORTED;
  const long long total = (long long)a.U * a.ht * a.wd;
  if (total > INT_MAX - 16) return LGU_E_UNSUPPORTED;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
#define LGU_UM_GO(XH, HW_) \
  um_launch<XH, true, HW_>(a.x, a.wpack, a.bias, a.disps_up, a.disps, a.ix, a.N, a.ht, a.wd, (int)total, s)
  if (xh) return halfw ? LGU_UM_GO(true, true) : LGU_UM_GO(true, false);
  return halfw ? LGU_UM_GO(false, true) : LGU_UM_GO(false, false);
#undef LGU_UM_GO
}
