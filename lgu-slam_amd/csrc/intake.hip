// intake.hip — the frame intake: a decoded camera frame to Droid.track's operands in one launch.  What the reference's
// streams do on the host with OpenCV before track sees a frame (demo.py:39-54, demo_depth.py:39-65,
// evaluation_scripts/test_tum.py:34-52, test_euroc.py:29-76) and motion_filter.py:56-57 after it: rectify (stage 1),
// resize (stage 2), crop (stage 3), the planar BGR bytes and the normalised RGB floats.  The definition is
// tests/intake_restatement.py (include/lgu_corr.h restates it): the map of stage 1 in double with every operation rounded
// on its own, coordinates quantised to 1/32 pixel, 5-bit weights and a 10-bit shift; stage 2 on the rounded BYTES of stage 1
// with 11-bit weights and a 22-bit shift.  Everything after the map is integer arithmetic, so the bytes are exact.
//
//   intake_tile_kernel    both stages: one workgroup per IT_W x IT_H output tile.  It works out the rectangle of stage-1
//                         pixels its resize taps fall into, computes each of them once into LDS (one packed dword per
//                         pixel), and after one barrier every lane blends its four taps from LDS.  A workgroup whose
//                         rectangle exceeds IT_MAXPIX computes its taps directly instead (same bytes).
//   intake_direct_kernel  <S1, S2>: every lane computes the stage-1 pixels it needs itself (four with stage 2, one
//                         without); without stage 1 they are raw pixels.  Serves the calls with a stage absent and the
//                         downscales whose rectangle does not fit.
//   intake_depth_kernel   the sensor disparity: only the points [3::8, 3::8] of the resized, cropped depth, in double.
// No atomics, no workgroup waits on another, one writer per output element: the same bits on every run.
#include "lgu_common.hpp"
#include "image_norm.hpp"

// The map has numpy's bits only if no product is fused into a sum: the build's -ffp-contract=off says so for every file;
// this says it for this one whatever the flags.
#pragma clang fp contract(off)

namespace lgu {

constexpr int IT_W = 32, IT_H = 8, IT_THREADS = IT_W * IT_H;
constexpr int IT_MAXPIX = 2048;                 // stage-1 pixels a tile keeps in LDS (8 KiB)
constexpr int CAM_DOUBLES = sizeof(lgu_intake_camera) / sizeof(double);
constexpr double Q_LIMIT = 1073741824.0;        // 2^30: |q| beyond it is far outside every frame

// floor(32 m + 0.5) as an int, clamped to [-2^30, 2^30]; a NaN fails the first comparison and becomes -2^30 (outside).
__device__ __forceinline__ int quantise32(double m) {
  double t = floor(32.0 * m + 0.5);
  t = t >= -Q_LIMIT ? t : -Q_LIMIT;
  t = t <= Q_LIMIT ? t : Q_LIMIT;
  return (int)t;
}

// The map of stage 1 at pixel (u, v) of the rectified image, c = the 22 doubles of the frame's camera (LDS).
__device__ __forceinline__ void rectify_map(const double* c, int u, int v, int* qx, int* qy) {
  const double* k = c;
  const double* kn = c + 4;
  const double* ir = c + 8;
  const double* d = c + 17;
  double x = ((double)u - kn[2]) / kn[0];
  double y = ((double)v - kn[3]) / kn[1];
  const double X = (ir[0] * x + ir[1] * y) + ir[2];
  const double Y = (ir[3] * x + ir[4] * y) + ir[5];
  const double W = (ir[6] * x + ir[7] * y) + ir[8];
  x = X / W;
  y = Y / W;
  const double x2 = x * x, y2 = y * y;
  const double r2 = x2 + y2;
  const double rad = 1.0 + r2 * (d[0] + r2 * (d[1] + r2 * d[4]));
  const double t = 2.0 * (x * y);
  const double xd = (x * rad + d[2] * t) + d[3] * (r2 + 2.0 * x2);
  const double yd = (y * rad + d[2] * (r2 + 2.0 * y2)) + d[3] * t;
  *qx = quantise32(xd * k[0] + k[2]);
  *qy = quantise32(yd * k[1] + k[3]);
}

// Pixel (y, x) of raw frame n as b | g << 8 | r << 16; 0 outside the frame.  C = 1 replicates the grey byte.
__device__ __forceinline__ unsigned raw_pixel(const unsigned char* __restrict__ raw, size_t frame, int y, int x, int h0, int w0,
                                              int C) {
  if (!in_range(y, h0) || !in_range(x, w0)) return 0u;
  const unsigned char* p = raw + frame + ((size_t)y * w0 + x) * C;
  if (C == 1) return (unsigned)p[0] * 0x010101u;
  return (unsigned)p[0] | ((unsigned)p[1] << 8) | ((unsigned)p[2] << 16);
}

// Pixel (v, u) of the stage-1 image of frame n, packed as raw_pixel's.
template <bool S1>
__device__ __forceinline__ unsigned stage1_pixel(const unsigned char* __restrict__ raw, size_t frame, const double* cam, int v,
                                                 int u, int h0, int w0, int C) {
  if (!S1) return raw_pixel(raw, frame, v, u, h0, w0, C);
  int qx, qy;
  rectify_map(cam, u, v, &qx, &qy);
  const int ix = qx >> 5, iy = qy >> 5;
  const unsigned ax = (unsigned)(qx & 31), ay = (unsigned)(qy & 31);
  // |ix|, |iy| <= 2^25: ix + 1 cannot wrap, and raw_pixel's range test takes every value
  const unsigned p00 = raw_pixel(raw, frame, iy, ix, h0, w0, C), p01 = raw_pixel(raw, frame, iy, ix + 1, h0, w0, C);
  const unsigned p10 = raw_pixel(raw, frame, iy + 1, ix, h0, w0, C), p11 = raw_pixel(raw, frame, iy + 1, ix + 1, h0, w0, C);
  const unsigned w00 = (32u - ax) * (32u - ay), w01 = ax * (32u - ay), w10 = (32u - ax) * ay, w11 = ax * ay;
  unsigned out = 0;
#pragma unroll
  for (int s = 0; s < 24; s += 8) {
    const unsigned sum = ((p00 >> s) & 255u) * w00 + ((p01 >> s) & 255u) * w01 + ((p10 >> s) & 255u) * w10 + ((p11 >> s) & 255u) * w11;
    out |= ((sum + 512u) >> 10) << s;
  }
  return out;
}

// One axis of stage 2 at output index o: the taps i0, i1 and the 11-bit weight k of i1.
__device__ __forceinline__ void resize_taps(int o, double scale, int n_in, int* i0, int* i1, unsigned* k) {
  const double f = ((double)o + 0.5) * scale - 0.5;
  const double fl = floor(f);
  int i = (int)fl;               // -1 <= f < n_in: the conversion is exact
  double a = f - fl;
  if (i < 0) {
    i = 0;
    a = 0.0;
  }
  if (i >= n_in - 1) {
    i = n_in - 1;
    a = 0.0;
  }
  *i0 = i;
  *i1 = i + 1 < n_in ? i + 1 : n_in - 1;
  *k = (unsigned)floor(2048.0 * a + 0.5);
}

__device__ __forceinline__ unsigned resize_blend(unsigned p00, unsigned p01, unsigned p10, unsigned p11, unsigned kx, unsigned ky) {
  const unsigned w00 = (2048u - kx) * (2048u - ky), w01 = kx * (2048u - ky), w10 = (2048u - kx) * ky, w11 = kx * ky;
  unsigned out = 0;
#pragma unroll
  for (int s = 0; s < 24; s += 8) {
    const unsigned sum = ((p00 >> s) & 255u) * w00 + ((p01 >> s) & 255u) * w01 + ((p10 >> s) & 255u) * w10 + ((p11 >> s) & 255u) * w11;
    out |= ((sum + (1u << 21)) >> 22) << s;   // sum <= 255 * 2^22: no overflow
  }
  return out;
}

// The three byte planes (BGR) and, with inputs, the three float planes (RGB) of output pixel (oy, ox) of frame n.
__device__ __forceinline__ void store_pixel(const lgu_intake_args& a, int n, int oy, int ox, unsigned px) {
  const size_t plane = (size_t)a.H * a.W;
  const size_t at = (size_t)n * 3 * plane + (size_t)oy * a.W + ox;
  unsigned char* img = static_cast<unsigned char*>(a.image) + at;
#pragma unroll
  for (int c = 0; c < 3; c++) img[c * plane] = (unsigned char)(px >> (8 * c));
  if (a.inputs) {
    float* inp = a.inputs + at;
#pragma unroll
    for (int c = 0; c < 3; c++) inp[c * plane] = image_normalize_value((unsigned char)(px >> (8 * (2 - c))), a.mean[c], a.std[c]);
  }
}

// The camera of frame n into LDS (the first CAM_DOUBLES threads); the caller's barrier publishes it.
__device__ __forceinline__ void load_camera(const lgu_intake_args& a, int n, double* cam) {
  const int t = threadIdx.x;
  if (t >= CAM_DOUBLES) return;
  if (a.cam_table) {
    cam[t] = reinterpret_cast<const double*>(a.cam_table + n)[t];
  } else {
    const lgu_intake_camera& c = a.cam[(a.ncam == 1 || n == 0) ? 0 : 1];
    cam[t] = t < 4 ? c.k[t] : (t < 8 ? c.kn[t - 4] : (t < 17 ? c.ir[t - 8] : c.d[t - 17]));
  }
}

__global__ __launch_bounds__(IT_THREADS) void intake_tile_kernel(const lgu_intake_args a) {
  __shared__ unsigned tile[IT_MAXPIX];
  __shared__ double cam[CAM_DOUBLES];
  const int n = blockIdx.z;
  const int ox0 = blockIdx.x * IT_W, oy0 = blockIdx.y * IT_H;
  const int tx = threadIdx.x % IT_W, ty = threadIdx.x / IT_W;
  const unsigned char* raw = static_cast<const unsigned char*>(a.raw);
  const size_t frame = (size_t)n * a.h0 * a.w0 * a.C;
  const double sy = (double)a.h0 / (double)a.h1, sx = (double)a.w0 / (double)a.w1;
  load_camera(a, n, cam);
  // the rectangle of stage-1 pixels: the taps are monotone in the output index, so the first output's i0 and the last
  // output's i1 bound it
  int r0, r1, c0, c1, unused;
  unsigned ku;
  const int oyl = (oy0 + IT_H < a.H ? oy0 + IT_H : a.H) - 1, oxl = (ox0 + IT_W < a.W ? ox0 + IT_W : a.W) - 1;
  resize_taps(a.top + oy0, sy, a.h0, &r0, &unused, &ku);
  resize_taps(a.top + oyl, sy, a.h0, &unused, &r1, &ku);
  resize_taps(a.left + ox0, sx, a.w0, &c0, &unused, &ku);
  resize_taps(a.left + oxl, sx, a.w0, &unused, &c1, &ku);
  const int rw = c1 - c0 + 1;
  const long long cnt = (long long)(r1 - r0 + 1) * rw;
  const bool fits = cnt <= IT_MAXPIX;      // uniform over the workgroup
  __syncthreads();
  if (fits) {
    for (int idx = threadIdx.x; idx < (int)cnt; idx += IT_THREADS) {
      const int dv = idx / rw, du = idx - dv * rw;
      tile[idx] = stage1_pixel<true>(raw, frame, cam, r0 + dv, c0 + du, a.h0, a.w0, a.C);
    }
    __syncthreads();
  }
  const int ox = ox0 + tx, oy = oy0 + ty;
  if (ox >= a.W || oy >= a.H) return;
  int y0, y1, x0, x1;
  unsigned ky, kx;
  resize_taps(a.top + oy, sy, a.h0, &y0, &y1, &ky);
  resize_taps(a.left + ox, sx, a.w0, &x0, &x1, &kx);
  unsigned p00, p01, p10, p11;
  if (fits) {   // r0 <= y0 <= y1 <= r1 and c0 <= x0 <= x1 <= c1 by monotonicity
    p00 = tile[(y0 - r0) * rw + (x0 - c0)];
    p01 = tile[(y0 - r0) * rw + (x1 - c0)];
    p10 = tile[(y1 - r0) * rw + (x0 - c0)];
    p11 = tile[(y1 - r0) * rw + (x1 - c0)];
  } else {
    p00 = stage1_pixel<true>(raw, frame, cam, y0, x0, a.h0, a.w0, a.C);
    p01 = stage1_pixel<true>(raw, frame, cam, y0, x1, a.h0, a.w0, a.C);
    p10 = stage1_pixel<true>(raw, frame, cam, y1, x0, a.h0, a.w0, a.C);
    p11 = stage1_pixel<true>(raw, frame, cam, y1, x1, a.h0, a.w0, a.C);
  }
  store_pixel(a, n, oy, ox, resize_blend(p00, p01, p10, p11, kx, ky));
}

template <bool S1, bool S2>
__global__ __launch_bounds__(IT_THREADS) void intake_direct_kernel(const lgu_intake_args a) {
  __shared__ double cam[CAM_DOUBLES];
  const int n = blockIdx.z;
  const int ox = blockIdx.x * IT_W + threadIdx.x % IT_W, oy = blockIdx.y * IT_H + threadIdx.x / IT_W;
  const unsigned char* raw = static_cast<const unsigned char*>(a.raw);
  const size_t frame = (size_t)n * a.h0 * a.w0 * a.C;
  if (S1) {
    load_camera(a, n, cam);
    __syncthreads();
  }
  if (ox >= a.W || oy >= a.H) return;
  unsigned px;
  if (S2) {
    const double sy = (double)a.h0 / (double)a.h1, sx = (double)a.w0 / (double)a.w1;
    int y0, y1, x0, x1;
    unsigned ky, kx;
    resize_taps(a.top + oy, sy, a.h0, &y0, &y1, &ky);
    resize_taps(a.left + ox, sx, a.w0, &x0, &x1, &kx);
    const unsigned p00 = stage1_pixel<S1>(raw, frame, cam, y0, x0, a.h0, a.w0, a.C);
    const unsigned p01 = stage1_pixel<S1>(raw, frame, cam, y0, x1, a.h0, a.w0, a.C);
    const unsigned p10 = stage1_pixel<S1>(raw, frame, cam, y1, x0, a.h0, a.w0, a.C);
    const unsigned p11 = stage1_pixel<S1>(raw, frame, cam, y1, x1, a.h0, a.w0, a.C);
    px = resize_blend(p00, p01, p10, p11, kx, ky);
  } else {
    px = stage1_pixel<S1>(raw, frame, cam, a.top + oy, a.left + ox, a.h0, a.w0, a.C);
  }
  store_pixel(a, n, oy, ox, px);
}

// One axis of the framework's bilinear interpolation without aligned corners at output index o.
__device__ __forceinline__ void interp_taps(int o, double scale, int n_in, int* i0, int* i1, double* l1) {
  double f = ((double)o + 0.5) * scale - 0.5;
  f = f > 0.0 ? f : 0.0;
  int i = (int)f;
  i = i < n_in - 1 ? i : n_in - 1;
  *i0 = i;
  *i1 = i + (i < n_in - 1 ? 1 : 0);
  *l1 = f - (double)i;
}

template <typename T>
__global__ __launch_bounds__(IT_THREADS) void intake_depth_kernel(const lgu_intake_depth_args a, int hs, int ws) {
  const long long total = (long long)a.N * hs * ws;
  const long long t = (long long)blockIdx.x * IT_THREADS + threadIdx.x;
  if (t >= total) return;
  const int j = (int)(t % ws), i = (int)((t / ws) % hs);
  const long long n = t / ((long long)ws * hs);
  const T* src = static_cast<const T*>(a.raw) + (size_t)n * a.h0 * a.w0;
  const double sy = (double)a.h0 / (double)a.h1, sx = (double)a.w0 / (double)a.w1;
  int y0, y1, x0, x1;
  double ly1, lx1;
  interp_taps(a.top + 3 + 8 * i, sy, a.h0, &y0, &y1, &ly1);
  interp_taps(a.left + 3 + 8 * j, sx, a.w0, &x0, &x1, &lx1);
  const double ly0 = 1.0 - ly1, lx0 = 1.0 - lx1;
  const double p00 = (double)src[(size_t)y0 * a.w0 + x0] * a.scale, p01 = (double)src[(size_t)y0 * a.w0 + x1] * a.scale;
  const double p10 = (double)src[(size_t)y1 * a.w0 + x0] * a.scale, p11 = (double)src[(size_t)y1 * a.w0 + x1] * a.scale;
  const double d = ly0 * (lx0 * p00 + lx1 * p01) + ly1 * (lx0 * p10 + lx1 * p11);
  a.out[t] = (float)(d > 0.0 ? 1.0 / d : d);
}

inline bool intake_sizes_ok(int N, int h0, int w0, int h1, int w1, int top, int left, int H, int W) {
  if (N < 0 || h0 < 0 || w0 < 0 || h1 < 0 || w1 < 0 || top < 0 || left < 0 || H < 0 || W < 0) return false;
  return (long long)top + H <= h1 && (long long)left + W <= w1;
}

}  // namespace lgu

extern "C" {

int lgu_intake_frame_u8(lgu_intake_args a, void* stream) {
  using namespace lgu;
  if (!intake_sizes_ok(a.N, a.h0, a.w0, a.h1, a.w1, a.top, a.left, a.H, a.W)) return LGU_E_BADARG;
  if ((a.C != 1 && a.C != 3) || a.path < 0 || a.path > 2) return LGU_E_BADARG;
  if (a.ncam != 0 && a.ncam != 1 && a.ncam != a.N) return LGU_E_BADARG;
  if (a.N == 0 || (long long)a.H * a.W == 0) return LGU_OK;
  if (a.h0 == 0 || a.w0 == 0 || !a.raw || !a.image) return LGU_E_BADARG;
  if (a.ncam > 2 && (!a.cam_table || (reinterpret_cast<uintptr_t>(a.cam_table) & 7) != 0)) return LGU_E_BADARG;
  if (a.ncam <= 2) a.cam_table = nullptr;
  const int gx = (a.W + IT_W - 1) / IT_W, gy = (a.H + IT_H - 1) / IT_H;
  if (gy > 65535 || a.N > 65535) return LGU_E_UNSUPPORTED;
  const bool s1 = a.ncam > 0, s2 = a.h1 != a.h0 || a.w1 != a.w0;
  // the largest rectangle a tile's taps span: floor((IT - 1) scale) + 3 pixels per axis
  const double sy = (double)a.h0 / (double)a.h1, sx = (double)a.w0 / (double)a.w1;
  const double rect = (floor((IT_H - 1) * sy) + 3.0) * (floor((IT_W - 1) * sx) + 3.0);
  const bool tile = s1 && s2 && (a.path == 1 || (a.path == 0 && rect <= (double)IT_MAXPIX));
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const dim3 grid(gx, gy, a.N), block(IT_THREADS);
  if (tile)
    hipLaunchKernelGGL(intake_tile_kernel, grid, block, 0, st, a);
  else if (s1 && s2)
    hipLaunchKernelGGL((intake_direct_kernel<true, true>), grid, block, 0, st, a);
  else if (s1)
    hipLaunchKernelGGL((intake_direct_kernel<true, false>), grid, block, 0, st, a);
  else if (s2)
    hipLaunchKernelGGL((intake_direct_kernel<false, true>), grid, block, 0, st, a);
  else
    hipLaunchKernelGGL((intake_direct_kernel<false, false>), grid, block, 0, st, a);
  return launch_status();
}

int lgu_intake_depth_f32(lgu_intake_depth_args a, void* stream) {
  using namespace lgu;
  if (!intake_sizes_ok(a.N, a.h0, a.w0, a.h1, a.w1, a.top, a.left, a.H, a.W)) return LGU_E_BADARG;
  const int hs = (a.H + 4) / 8, ws = (a.W + 4) / 8;   // len(range(3, H, 8))
  const long long total = (long long)a.N * hs * ws;
  if (total == 0) return LGU_OK;
  if (a.h0 == 0 || a.w0 == 0 || !a.raw || !a.out) return LGU_E_BADARG;
  const long long blocks = (total + IT_THREADS - 1) / IT_THREADS;
  if (blocks > 0x7fffffffLL) return LGU_E_UNSUPPORTED;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (a.src_u16)
    hipLaunchKernelGGL((intake_depth_kernel<unsigned short>), dim3((unsigned)blocks), dim3(IT_THREADS), 0, st, a, hs, ws);
  else
    hipLaunchKernelGGL((intake_depth_kernel<float>), dim3((unsigned)blocks), dim3(IT_THREADS), 0, st, a, hs, ws);
  return launch_status();
}

}  // extern "C"
