// lowmem_family.hpp — what the four files of the on-the-fly correlation family share (lowmem.hip, lowmem_tile.hip,
// lowmem_mfma.hip, lowmem_coop.hip): the launch block, the checks of the extern "C" arguments, the preconditions of the
// tiled kernels and the dispatchers that one file defines and another calls.
//
// Who serves a call (each step returns -1 for what it does not serve, and the next one is tried):
//   float maps  lowmem.hip entries      -> lowmem_mfma_dispatch_f32 -> lowmem_tile_dispatch -> wave-per-pixel kernels
//   half maps   lowmem_tile.hip entries -> lowmem_mfma_dispatch (-> lowmem_coop_dispatch first) -> VALU tile kernel
//   pyramids    lowmem_mfma.hip entries -> the matrix-core dispatcher of the element type, or LGU_E_UNSUPPORTED
#pragma once
#include <limits.h>

#include <initializer_list>

#include "lgu_common.hpp"

namespace lgu {

constexpr int LOWMEM_MAXL = 4;  // pyramid levels one launch can serve

// Launch parameters, and the one argument of the matrix-core kernels (the cooperative kernel reads it where it lies, in
// the kernarg segment).  L == 1: one operator call (lowMem_defSample / altcorr_forward).  L > 1: the per-level loop of
// AltCorrBlock.corr_fn (reference corr.py:192-213) in ONE launch: level l samples fmap2[l] at coords / 2^(lbase + l)
// with offset[l] and writes channels (lvl0 + l) * NT .. of the Ltot * NT concatenated output channels.
struct LowmemParams {
  const void* fmap1;  // element type = the kernel's T (half or float)
  const void* fmap2[LOWMEM_MAXL];
  float* offset[LOWMEM_MAXL];  // null = zero offsets for that level (altcorr)
  const float* coords;
  float* corr;
  int H2[LOWMEM_MAXL], W2[LOWMEM_MAXL];
  int L, B, S, H1, W1;
  // set by the launchers: pixel blocks (4 x 4 MT, one-wave kernel) or tiles (4 x 8, cooperative kernel) per row / column
  // of the image, edges dealt to XCDs, 16-byte output stores
  int tiles_x, tiles_y, xcd_map, vec_out;
  int lbase;       // pyramid level of fmap2[0]
  int lvl0, Ltot;  // (a pyramid call may be split into a launch for the levels with offsets and one for the others)
  // fmap2 storage.  0: channel-last (F,H2,W2,C), the operators' layout.  1: chunk-planar (F, C/EPL, H2, W2, EPL) with
  // EPL = 16 bytes of channels: the 16 x-adjacent positions an MFMA B fragment covers are then 256 CONTIGUOUS bytes per
  // 16-byte channel chunk, where channel-last puts them 2C bytes apart.  The vector L1 serves a load quad by quad
  // (4 lanes), one access per distinct 128-byte line in the quad: 64 accesses per fragment load channel-last, 16-20
  // chunk-planar — the access rate, not L2 bandwidth, is what bounds the sweep (AltCorrBlock keeps its pyramid in this form).
  int f2_chunked;
  // Work units of the cooperative kernel (set by its launcher).  The first n_fused workgroups serve ALL levels of their
  // (edge, tile) in one wave life; the remaining n_split (edge, tile) items are served level group by level group
  // (group k = levels gl0[k] .. gl0[k + 1] - 1), groups in launch order: n_fused is a whole number of rounds over the
  // device's workgroup slots, and the short units fill the last, partial round (launch_coop).
  int n_fused, n_split, ngroups, gl0[LOWMEM_MAXL + 1];
  const long long* ii;  // optional frame indices (device, int64): edge b reads fmap1[ii[b]] and fmap2[l][jj[b]]
  const long long* jj;  // straight from the frame buffers — no gathered per-edge copies; null = fmap*[b]
  // Several reference calls in one launch (lgu_lowmem_pyramid_calls_fwd_h16; cooperative kernel only): edge b samples
  // with offset row orow[b] — the first edge of ITS call — instead of row b*n.  Null = one call.  Values are clamped to
  // n_orow - 1 (no wild reads).
  const int* orow;
  int n_orow;
};

// The block of a single-level entry (lowMem_defSample / altcorr_forward).
inline LowmemParams single_level(const void* fmap1, const void* fmap2, const float* coords, float* offset, float* corr, int B,
                                 int S, int H1, int W1, int H2, int W2) {
  LowmemParams p = {};
  p.fmap1 = fmap1; p.fmap2[0] = fmap2; p.offset[0] = offset; p.coords = coords; p.corr = corr;
  p.H2[0] = H2; p.W2[0] = W2;
  p.L = 1; p.B = B; p.S = S; p.H1 = H1; p.W1 = W1;
  p.lvl0 = 0; p.Ltot = 1;
  return p;
}

// ---- the extern "C" arguments of the family ------------------------------------------------------------------------
// The reference indexes offset[b * n] (lowMem_defSample.cu:80-83): B edges x S samples need more than (B-1)*(S-1) rows.
constexpr long long kAnyOffsetRows = LLONG_MAX;  // NO of the entries that take no offsets
inline bool offset_rows_ok(int B, int S, long long NO) { return (long long)(B - 1) * (S - 1) < NO; }

// Non-null pointers, positive sizes (B = 0 is an empty call, not an error; H2 / W2 of all L levels) and the NO rule.
// What differs between the entries stays with them: the radius and channel counts each one answers
// LGU_E_UNSUPPORTED for, and the index and level arguments of the pyramid entries.
inline int lowmem_entry_args(std::initializer_list<const void*> ptrs, int B, int S, int H1, int W1, const int* H2, const int* W2,
                             int L, int C, int radius, long long NO) {
  for (const void* q : ptrs)
    if (!q) return LGU_E_BADARG;
  if (B < 0 || S < 1 || H1 < 1 || W1 < 1 || C < 1 || radius < 0) return LGU_E_BADARG;
  for (int l = 0; l < L; l++)
    if (H2[l] < 1 || W2[l] < 1) return LGU_E_BADARG;
  return offset_rows_ok(B, S, NO) ? LGU_OK : LGU_E_BADARG;
}

// ---- what the kernels ask of a launch ------------------------------------------------------------------------------
// The tiled kernels (VALU tile, one-wave and cooperative matrix-core): 16-byte channel loads of the maps; coords and
// offsets (null = none) go as 8-byte (x, y) pairs; S is the grid's y extent; offsets inside one edge are 32-bit; the
// kernels are instantiated for radius 1..3.
inline bool lowmem_tiled_serves(const LowmemParams& p, int C, int radius) {
  if (p.L < 1 || p.L > LOWMEM_MAXL || radius < 1 || radius > 3 || p.S > 65535) return false;
  uintptr_t al16 = reinterpret_cast<uintptr_t>(p.fmap1), al8 = reinterpret_cast<uintptr_t>(p.coords);
  for (int l = 0; l < p.L; l++) {
    al16 |= reinterpret_cast<uintptr_t>(p.fmap2[l]);
    al8 |= reinterpret_cast<uintptr_t>(p.offset[l]);
    if ((size_t)p.H2[l] * p.W2[l] * C >= (1u << 31)) return false;
  }
  return (al16 & 15) == 0 && (al8 & 7) == 0 && (size_t)p.H1 * p.W1 * C < (1u << 31);
}
// The matrix-core kernels also pack window coordinates into int16 pairs.
inline bool lowmem_matrix_serves(const LowmemParams& p, int C, int radius) {
  if (!lowmem_tiled_serves(p, C, radius)) return false;
  for (int l = 0; l < p.L; l++)
    if (p.H2[l] > 32767 || p.W2[l] > 32767) return false;
  return true;
}

// ---- dispatchers: LGU_OK or a HIP error after a launch, -1 when the kernel does not serve the block ----------------
// lowmem_coop.hip: half maps, C in {32, 64, 128}; four waves share the swept windows, all levels in one wave life
int lowmem_coop_dispatch(const LowmemParams& p, int C, int radius, hipStream_t st);
// lowmem_mfma.hip: one wave per pixel block.  Half maps (v_mfma_f32_16x16x32_f16, the cooperative kernel first) and
// float maps (v_mfma_f32_16x16x4_f32)
int lowmem_mfma_dispatch(const LowmemParams& p, int C, int radius, hipStream_t st);
int lowmem_mfma_dispatch_f32(const LowmemParams& p, int C, int radius, hipStream_t st);
// lowmem_tile.hip: VALU tile kernel, float maps, single level
int lowmem_tile_dispatch(const LowmemParams& p, int C, int radius, hipStream_t st);

}  // namespace lgu
