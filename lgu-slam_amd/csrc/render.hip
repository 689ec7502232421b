// render.hip — the offscreen view of the map: a z-buffered rasteriser of coloured points and of one wireframe frustum per
// keyframe, the drawing half of the reference's visualiser (droid_slam/visualization.py:36-51, 121-134, 144-153 and
// misc/renderoption.json: white background, point size 2).  The definition is tests/render_restatement.py; DESIGN.md
// section 3.27 states it in full.  Every float operation below rounds on its own (-ffp-contract=off).
//
// Frame buffer: one 64-bit key per pixel, all ones = empty.  A primitive offers (bits(z) << 32) | (r << 16) | (g << 8) | b
// with the float32 bit pattern of its positive camera-space z; a pixel keeps the minimum.  Positive floats order as their
// bit patterns: the nearest primitive wins, among equal depths the smaller packed colour.  The minimum does not depend on
// the order of points, launches or arrival: the same bytes on every run.
//
//   render_clear_kernel   the keys = all ones, 16 bytes per store
//   render_points_kernel  one thread per point (grid-stride above the grid cap): transform, reject, project, and one 64-bit
//                         atomic minimum per covered pixel of the point_size x point_size footprint
//   render_lines_kernel   one wave per camera: the ten segments of its frustum in turn, the lanes share a segment's samples,
//                         one atomic minimum per sample inside the image
//   render_resolve_kernel the keys to image (H,W,3) uint8 and depth (H,W) float, four pixels per thread where aligned
#include <float.h>
#include <limits.h>

#include "lgu_common.hpp"
#include "geom_pixel.hpp"

namespace lgu {

typedef unsigned long long u64;
typedef u64 u64x2 __attribute__((ext_vector_type(2)));

constexpr int RENDER_THREADS = 256;
constexpr u64 RENDER_EMPTY = ~0ull;
constexpr long long RENDER_MAX_PIXELS = 1ll << 28;
constexpr int RENDER_MAX_BLOCKS = 1 << 22;     // of the point kernel: 2^30 threads, beyond that a thread strides
constexpr float RENDER_MAX_SAMPLES = 1048576.0f;  // 2^20 per segment

// The camera actor, in this project's words.  Vertices in the camera's own frame (x right, y down, z ahead) before the
// scale: 0 the apex (the optical centre); 1-4 the base, a 2 x 2 square at depth 1.5, from the upper left corner clockwise
// as the image shows it; 5-7 the up-marker, a shallow wedge hanging from the middle half of the base's lower edge.
__constant__ float FRUSTUM_VERTS[8][3] = {{0.0f, 0.0f, 0.0f},  {-1.0f, -1.0f, 1.5f}, {1.0f, -1.0f, 1.5f}, {1.0f, 1.0f, 1.5f},
                                          {-1.0f, 1.0f, 1.5f}, {-0.5f, 1.0f, 1.5f},  {0.5f, 1.0f, 1.5f},  {0.0f, 1.2f, 1.5f}};
// Segments A -> B: the base's four edges, the four edges from the apex, the marker's two strokes.
constexpr int FRUSTUM_SEGMENTS = 10;
__constant__ int FRUSTUM_SEGS[FRUSTUM_SEGMENTS][2] = {{1, 2}, {2, 3}, {3, 4}, {4, 1}, {0, 1}, {0, 2}, {0, 3}, {0, 4}, {5, 7}, {7, 6}};

__device__ __forceinline__ bool finite3(const float* v) { return isfinite(v[0]) && isfinite(v[1]) && isfinite(v[2]); }

// Offer `key` to pixel `at`.  PRELOAD: a relaxed agent-scope load first (served from where the atomics execute, not from
// a wave's L1), the atomic only where the key would lower what is there.  The key in memory only ever decreases, so a
// skipped atomic could not have changed it: the same result either way.
template <bool PRELOAD>
__device__ __forceinline__ void offer(u64* __restrict__ keys, size_t at, u64 key) {
  if (PRELOAD && __hip_atomic_load(keys + at, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) <= key) return;
  atomicMin(keys + at, key);
}

// clamp(floorf(c * 255 + 0.5f), 0, 255), a NaN gives 0
__device__ __forceinline__ unsigned colour_byte(float c) {
  const float f = floorf(c * 255.0f + 0.5f);
  if (!(f >= 0.0f)) return 0u;
  return f > 255.0f ? 255u : (unsigned)f;
}

__global__ __launch_bounds__(RENDER_THREADS) void render_clear_kernel(u64* __restrict__ keys, long long n) {
  const long long i = ((long long)blockIdx.x * RENDER_THREADS + threadIdx.x) * 2;
  if (i + 1 < n) {
    const u64x2 ones = {RENDER_EMPTY, RENDER_EMPTY};
    *reinterpret_cast<u64x2*>(keys + i) = ones;   // keys is 16-byte aligned, i even
  } else if (i < n) {
    keys[i] = RENDER_EMPTY;
  }
}

template <bool U8, bool PRELOAD>
__global__ __launch_bounds__(RENDER_THREADS) void render_points_kernel(const float* __restrict__ points, const void* __restrict__ colors,
                                                                       const float* __restrict__ view,
                                                                       const float* __restrict__ intrinsics, u64* __restrict__ keys,
                                                                       long long P, int H, int W, int s, float near) {
  // uniform: the compiler keeps these in scalar registers
  const float t[3] = {view[0], view[1], view[2]};
  const float q[4] = {view[3], view[4], view[5], view[6]};
  const float fx = intrinsics[0], fy = intrinsics[1], cx = intrinsics[2], cy = intrinsics[3];
  const float shift = 1.0f - 0.5f * (float)s;
  const long long step = (long long)gridDim.x * RENDER_THREADS;
  for (long long p = (long long)blockIdx.x * RENDER_THREADS + threadIdx.x; p < P; p += step) {
    const float X[3] = {points[p * 3], points[p * 3 + 1], points[p * 3 + 2]};
    float Y[3];
    act_so3(q, X, Y);
    Y[0] = Y[0] + t[0];
    Y[1] = Y[1] + t[1];
    Y[2] = Y[2] + t[2];
    if (!finite3(Y) || !(Y[2] > near)) continue;
    const float u = fx * (Y[0] / Y[2]) + cx;
    const float v = fy * (Y[1] / Y[2]) + cy;
    const long long x0 = cvt_i32_sat(floorf(u + shift)), y0 = cvt_i32_sat(floorf(v + shift));  // 64-bit: x0 + s cannot wrap
    if (x0 >= W || y0 >= H || x0 + s <= 0 || y0 + s <= 0) continue;
    unsigned rgb;
    if (U8) {
      const unsigned char* c = static_cast<const unsigned char*>(colors) + p * 3;
      rgb = ((unsigned)c[0] << 16) | ((unsigned)c[1] << 8) | (unsigned)c[2];
    } else {
      const float* c = static_cast<const float*>(colors) + p * 3;
      rgb = (colour_byte(c[0]) << 16) | (colour_byte(c[1]) << 8) | colour_byte(c[2]);
    }
    const u64 key = ((u64)__float_as_uint(Y[2]) << 32) | rgb;
    const long long xlo = x0 < 0 ? 0 : x0, xhi = x0 + s < W ? x0 + s : W;
    const long long ylo = y0 < 0 ? 0 : y0, yhi = y0 + s < H ? y0 + s : H;
    for (long long y = ylo; y < yhi; y++)
      for (long long x = xlo; x < xhi; x++) offer<PRELOAD>(keys, (size_t)(y * W + x), key);
  }
}

// The line samples take the atomic alone: the load in front of it only lengthened the wave's serial walk (measured).
__global__ __launch_bounds__(kWave) void render_lines_kernel(const float* __restrict__ cameras, const float* __restrict__ view,
                                                              const float* __restrict__ intrinsics, u64* __restrict__ keys, int H,
                                                              int W, float near, float scale, unsigned rgb) {
  const float* cam = cameras + (size_t)blockIdx.x * 7;
  const float fx = intrinsics[0], fy = intrinsics[1], cx = intrinsics[2], cy = intrinsics[3];
  float tr[3], qr[4];
  rel_se3(cam, cam + 3, view, view + 3, tr, qr);  // the camera's frame -> the view's frame
  const int lane = threadIdx.x;
  for (int sg = 0; sg < FRUSTUM_SEGMENTS; sg++) {  // uniform over the wave
    float E[2][3];
    for (int e = 0; e < 2; e++) {
      const float* C = FRUSTUM_VERTS[FRUSTUM_SEGS[sg][e]];
      const float X[3] = {scale * C[0], scale * C[1], scale * C[2]};
      act_so3(qr, X, E[e]);
      E[e][0] = E[e][0] + tr[0];
      E[e][1] = E[e][1] + tr[1];
      E[e][2] = E[e][2] + tr[2];
    }
    if (!finite3(E[0]) || !finite3(E[1])) continue;
    const bool in_a = E[0][2] >= near, in_b = E[1][2] >= near;
    if (!in_a && !in_b) continue;
    if (!in_a || !in_b) {  // the end behind the near plane moves onto it, along A -> B
      const float tc = (near - E[0][2]) / (E[1][2] - E[0][2]);
      const float mx = E[0][0] + tc * (E[1][0] - E[0][0]), my = E[0][1] + tc * (E[1][1] - E[0][1]);
      float* M = in_a ? E[1] : E[0];
      M[0] = mx;
      M[1] = my;
      M[2] = near;
    }
    const float ua = fx * (E[0][0] / E[0][2]) + cx, va = fy * (E[0][1] / E[0][2]) + cy, wa = 1.0f / E[0][2];
    const float ub = fx * (E[1][0] / E[1][2]) + cx, vb = fy * (E[1][1] / E[1][2]) + cy, wb = 1.0f / E[1][2];
    const float du = ub - ua, dv = vb - va, dw = wb - wa;
    const float au = fabsf(du), av = fabsf(dv);
    if (!isfinite(au) || !isfinite(av)) continue;
    float n = ceilf(au > av ? au : av);
    if (n == 0.0f) n = 1.0f;
    if (n > RENDER_MAX_SAMPLES) continue;
    const int count = (int)n;
    for (int k = lane; k <= count; k += kWave) {
      const float tk = (float)k / n;
      const float u = ua + tk * du, v = va + tk * dv, w = wa + tk * dw;
      const float z = 1.0f / w;
      const float px = floorf(u + 0.5f), py = floorf(v + 0.5f);
      if (!(px >= 0.0f && px < (float)W && py >= 0.0f && py < (float)H)) continue;  // a NaN is outside
      const u64 key = ((u64)__float_as_uint(z) << 32) | rgb;
      offer<false>(keys, (size_t)(int)py * W + (int)px, key);
    }
  }
}

// image and depth of pixel i from its key
__device__ __forceinline__ void resolve_one(u64 key, unsigned bg, unsigned* rgb, float* z) {
  const bool empty = key == RENDER_EMPTY;
  *rgb = empty ? bg : (unsigned)(key & 0xffffffu);
  *z = empty ? __uint_as_float(0x7f800000u) : __uint_as_float((unsigned)(key >> 32));
}

__global__ __launch_bounds__(RENDER_THREADS) void render_resolve_kernel(const u64* __restrict__ keys, unsigned char* __restrict__ image,
                                                                        float* __restrict__ depth, long long n, unsigned bg,
                                                                        int aligned) {
  const long long i = ((long long)blockIdx.x * RENDER_THREADS + threadIdx.x) * 4;
  if (i >= n) return;
  if (aligned && i + 3 < n) {  // image 4-byte and depth 16-byte aligned: 12 image bytes as three dwords, four depths as one store
    const u64x2 k01 = *reinterpret_cast<const u64x2*>(keys + i), k23 = *reinterpret_cast<const u64x2*>(keys + i + 2);
    unsigned c[4];
    f32x4 z;
    float zz;
    resolve_one(k01[0], bg, &c[0], &zz); z[0] = zz;
    resolve_one(k01[1], bg, &c[1], &zz); z[1] = zz;
    resolve_one(k23[0], bg, &c[2], &zz); z[2] = zz;
    resolve_one(k23[1], bg, &c[3], &zz); z[3] = zz;
    // bytes in memory order: r0 g0 b0 r1 | g1 b1 r2 g2 | b2 r3 g3 b3, little endian
    const unsigned r0 = c[0] >> 16, g0 = (c[0] >> 8) & 255u, b0 = c[0] & 255u, r1 = c[1] >> 16, g1 = (c[1] >> 8) & 255u, b1 = c[1] & 255u;
    const unsigned r2 = c[2] >> 16, g2 = (c[2] >> 8) & 255u, b2 = c[2] & 255u, r3 = c[3] >> 16, g3 = (c[3] >> 8) & 255u, b3 = c[3] & 255u;
    unsigned* dst = reinterpret_cast<unsigned*>(image + i * 3);
    dst[0] = r0 | (g0 << 8) | (b0 << 16) | (r1 << 24);
    dst[1] = g1 | (b1 << 8) | (r2 << 16) | (g2 << 24);
    dst[2] = b2 | (r3 << 8) | (g3 << 16) | (b3 << 24);
    *reinterpret_cast<f32x4*>(depth + i) = z;
    return;
  }
  const long long end = i + 4 < n ? i + 4 : n;
  for (long long j = i; j < end; j++) {
    unsigned c;
    float z;
    resolve_one(keys[j], bg, &c, &z);
    image[j * 3] = (unsigned char)(c >> 16);
    image[j * 3 + 1] = (unsigned char)(c >> 8);
    image[j * 3 + 2] = (unsigned char)c;
    depth[j] = z;
  }
}

inline unsigned pack_rgb(const unsigned char* c) { return ((unsigned)c[0] << 16) | ((unsigned)c[1] << 8) | (unsigned)c[2]; }

}  // namespace lgu

extern "C" {

long long lgu_render_scratch_bytes(int H, int W) {
  if (H <= 0 || W <= 0) return 0;
  return (long long)H * W * 8;
}

int lgu_render_view(lgu_render_args a, void* stream) {
  using namespace lgu;
  if (a.H < 0 || a.W < 0 || a.npoints < 0 || a.ncam < 0 || a.point_size < 1 || a.point_size > 8) return LGU_E_BADARG;
  if (!(a.near > 0.0f) || a.near > FLT_MAX) return LGU_E_BADARG;  // NaN, inf, zero and negative
  if (!(a.camera_scale >= -FLT_MAX && a.camera_scale <= FLT_MAX)) return LGU_E_BADARG;
  const long long n = (long long)a.H * a.W;
  if (n > RENDER_MAX_PIXELS) return LGU_E_UNSUPPORTED;
  if (n == 0) return LGU_OK;
  if (!a.view || !a.intrinsics || !a.scratch || !a.image || !a.depth) return LGU_E_BADARG;
  if (a.npoints > 0 && (!a.points || !a.colors)) return LGU_E_BADARG;
  if (a.ncam > 0 && !a.cameras) return LGU_E_BADARG;
  if ((reinterpret_cast<uintptr_t>(a.scratch) & 15) != 0) return LGU_E_BADARG;
  u64* keys = static_cast<u64*>(a.scratch);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const bool preload = env_int("LGU_RENDER_PRELOAD", 1) != 0;  // measured: DESIGN.md section 3.27 (0: the atomic alone)
  int rc;
  hipLaunchKernelGGL(render_clear_kernel, dim3((unsigned)((n + 2 * RENDER_THREADS - 1) / (2 * RENDER_THREADS))), dim3(RENDER_THREADS), 0, st,
                     keys, n);
  if ((rc = launch_status())) return rc;
  if (a.npoints > 0) {
    int cap = env_int("LGU_RENDER_MAX_BLOCKS", RENDER_MAX_BLOCKS);  // tests: a small grid exercises the stride
    cap = cap < 1 ? 1 : (cap > RENDER_MAX_BLOCKS ? RENDER_MAX_BLOCKS : cap);
    const long long want = (a.npoints + RENDER_THREADS - 1) / RENDER_THREADS;
    const unsigned blocks = (unsigned)(want < cap ? want : cap);
    auto kern = a.color_u8 ? (preload ? render_points_kernel<true, true> : render_points_kernel<true, false>)
                           : (preload ? render_points_kernel<false, true> : render_points_kernel<false, false>);
    hipLaunchKernelGGL(kern, dim3(blocks), dim3(RENDER_THREADS), 0, st, a.points, a.colors, a.view, a.intrinsics, keys, a.npoints, a.H,
                       a.W, a.point_size, a.near);
    if ((rc = launch_status())) return rc;
  }
  if (a.ncam > 0) {
    hipLaunchKernelGGL(render_lines_kernel, dim3((unsigned)a.ncam), dim3(kWave), 0, st, a.cameras, a.view, a.intrinsics, keys, a.H, a.W, a.near,
                       a.camera_scale, pack_rgb(a.camera_color));
    if ((rc = launch_status())) return rc;
  }
  const int aligned = (reinterpret_cast<uintptr_t>(a.image) & 3) == 0 && (reinterpret_cast<uintptr_t>(a.depth) & 15) == 0;
  hipLaunchKernelGGL(render_resolve_kernel, dim3((unsigned)((n + 4 * RENDER_THREADS - 1) / (4 * RENDER_THREADS))), dim3(RENDER_THREADS), 0,
                     st, keys, a.image, a.depth, n, pack_rgb(a.background), aligned);
  return launch_status();
}

}  // extern "C"
