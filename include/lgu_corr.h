/*
 * lgu_corr.h — C ABI of the MI355X (gfx950) deformable correlation-sampling library.
 *
 * This is the drop-in boundary for LGU-SLAM's hot path: every entry point below
 * replaces one Python-visible operator of the reference's two CUDA extensions
 * (`defCorrSample`, reference offersample_LGS/droid.cpp:138-147, and the two
 * `altcorr_*` operators of `droid_backends`, reference src/droid.cpp:246-247).
 *
 * Conventions (all entry points):
 *   - every pointer is a DEVICE pointer into a dense, contiguous fp32 buffer owned by
 *     the caller (PyTorch's allocator in practice); the library never allocates,
 *     frees or retains memory;
 *   - the work is enqueued on `stream` (a hipStream_t passed as void*; NULL = the
 *     legacy default stream, which is what the reference launches on);
 *   - the return value is 0 on success, a hipError_t value if the launch failed, or
 *     one of the LGU_E_* codes below for arguments the kernels cannot serve;
 *     nothing throws; lgu_error_string() names any code;
 *   - re-entrant; no mutable global state beyond idempotent per-device launch caches ("this kernel may use > 64 KB of
 *     LDS on device d", the device's CU count: the same values whoever writes them) and one flag read when the library
 *     is loaded: the LGU_* debug environment variables that select superseded kernels for tests / A-B tools are
 *     honoured only if LGU_DEBUG_KNOBS=1 was set at load time — otherwise no entry point reads the environment;
 *   - alignment: every operand must be aligned to its element, and unless the entry says otherwise that is all it
 *     needs — the kernels then access it by element (or the host picks an element-wise kernel with the same
 *     arithmetic) and the result does not depend on its address.  Where an entry names a stricter alignment it also
 *     says what a contiguous operand below it gets: another kernel (and whether the bits change), LGU_E_UNSUPPORTED or
 *     LGU_E_BADARG — every entry decides that before it launches anything.  DESIGN.md section 4.1 has the table,
 *     operand by operand;
 *   - "fully written" outputs need no initialisation by the caller; "accumulated"
 *     outputs must be zero-filled by the caller before the call (the reference
 *     allocates them with torch::zeros / zeros_like).
 *
 * Index conventions follow the reference: tap index i moves in x (width), j in y
 * (height); rd = 2*radius+1.
 */
#ifndef LGU_CORR_H
#define LGU_CORR_H

#ifdef __cplusplus
extern "C" {
#endif

#define LGU_OK 0
#define LGU_E_BADARG 100001     /* null pointer / non-positive size / radius out of range */
#define LGU_E_UNSUPPORTED 100002 /* shape the kernels do not serve (e.g. C % 32 != 0) */

#define LGU_MAX_LEVELS 8
#define LGU_MAX_RADIUS 7

/* Library identification: "lgu_corr <semver> gfx950", followed by " [<extra compiler flags>]" for a non-default
 * (experiment) build. */
const char* lgu_version(void);
/* 1 if the library was loaded with LGU_DEBUG_KNOBS=1 in the environment (debug / A-B knobs live), else 0. */
int lgu_debug_knobs_enabled(void);
/* Static string for a code returned by any entry point (LGU_E_* or hipError_t). */
const char* lgu_error_string(int code);

/* ---- volume path -------------------------------------------------------------- */

/* defCorrSample.defCorr_index_forward   (reference offersample_LGS/droid.cpp:53-63,
 * defCorrSample_kernel.cu:25-91,165-196).
 *   volume (E,H1,W1,H2,W2)  coords (E,2,H1,W1)  offset (E,H1,W1,rd,rd,2) IN/OUT
 *   corr   (E,rd,rd,H1,W1)  fully written (masked taps are written as 0).
 * Side effect kept from the reference: offset[e][y][x][r][r][0:2] = 0.
 * Alignment (this entry and lgu_corridx_fwd_f32): the fast kernels (radius 1..3, W2 % 4 == 0) want volume, coords and
 * offset 16-byte aligned; otherwise the generic one-thread-per-output kernel runs, same arithmetic, same bits.  corr is
 * stored by element. */
int lgu_defcorr_fwd_f32(const float* volume, const float* coords, float* offset, float* corr,
                        int E, int H1, int W1, int H2, int W2, int radius, void* stream);

/* defCorrSample.defCorr_index_backward  (droid.cpp:65-77, defCorrSample_kernel.cu:93-162,198-231).
 *   corr_grad (E,rd,rd,H1,W1); volume_grad like volume — ACCUMULATED (caller zero-fills);
 *   offset_grad like offset — fully written (0 for masked taps). offset centre re-zeroed. */
int lgu_defcorr_bwd_f32(const float* volume, const float* coords, float* offset,
                        const float* corr_grad, float* volume_grad, float* offset_grad,
                        int E, int H1, int W1, int H2, int W2, int radius, void* stream);

/* defCorrSample.corr_index_forward      (droid.cpp:79-87, corrSample_kernel.cu:24-82,139-168). */
int lgu_corridx_fwd_f32(const float* volume, const float* coords, float* corr,
                        int E, int H1, int W1, int H2, int W2, int radius, void* stream);

/* defCorrSample.corr_index_backward     (droid.cpp:89-99, corrSample_kernel.cu:84-136,170-199).
 *   volume_grad ACCUMULATED (caller zero-fills). `volume` is accepted for signature
 *   fidelity and never read (the reference kernel does not read it either). */
int lgu_corridx_bwd_f32(const float* volume, const float* coords, const float* corr_grad,
                        float* volume_grad,
                        int E, int H1, int W1, int H2, int W2, int radius, void* stream);

/* defCorrSample.gaussianMask            (droid.cpp:100-110, gaussianAttn.cu:19-68,134-163).
 *   means, covs (E,H1,W1,2); volume, volume1 (E,H1,W1,H2,W2); volume1 fully written
 *   (zero outside the (2*radius+1)^2 window around floor(mean)).  volume and volume1 16-byte aligned and W2 % 4 == 0:
 *   16-byte accesses; otherwise one thread per element, same expression, same bits. */
int lgu_gaussmask_fwd_f32(const float* means, const float* covs, const float* volume,
                          float* volume1,
                          int E, int H1, int W1, int H2, int W2, int radius, void* stream);

/* defCorrSample.gaussianMask_backward   (droid.cpp:112-123, gaussianAttn.cu:72-131,165-200).
 *   means_grad, covs_grad (E,H1,W1,2) fully written. */
int lgu_gaussmask_bwd_f32(const float* means, const float* covs, const float* volume,
                          const float* volume1_grad, float* means_grad, float* covs_grad,
                          int E, int H1, int W1, int H2, int W2, int radius, void* stream);

/* Fused multi-level deformable sample = the body of CorrBlock.__call__
 * (reference droid_slam/modules/corr.py:88-109): L calls of defCorr_index_forward on the
 * L pyramid levels with coords / 2^l, written straight into the concatenated tensor
 *   out (E, L*rd*rd, H1, W1)   channel = l*rd*rd + i*rd + j     (corr.py:103,109).
 * volumes[l] (E,H1,W1,H2[l],W2[l]); offsets[l] (E,H1,W1,rd,rd,2) IN/OUT (centre zeroed) or
 * NULL = structurally zero offsets for that level (corr.py:132-135), nothing is read.
 * The pointer/size tables are HOST arrays of length L (copied at launch).
 * flags: LGU_PYR_PROBE fuses the uncertainty probe of corr.py:94-99 as well: the 3x3
 *   plain sample of level 1 at coords/2, its unbiased variance over the 9 taps,
 *   mask = sigmoid(var), offsets[1] *= mask written back (the reference's stateful
 *   update) before level 1 is sampled. Requires L >= 2 and offsets[1] != NULL.
 * Alignment: coords, every volumes[l] and every non-null offsets[l] 16-byte aligned (and W2[l] % 4 == 0 or LGU_PYR_TILED)
 * select the fast kernels; otherwise the generic kernel serves the plain row-major form (no flags) with the same
 * arithmetic and bits, and every flagged form is LGU_E_UNSUPPORTED.  `out` is stored by element in the planar and the
 * LGU_PYR_OUT_* forms.  The decision is taken for all levels before the first launch: a refused call has changed
 * nothing. */
#define LGU_PYR_PROBE 1
/* LGU_PYR_TILED: volumes[l] are in this library's tiled slice layout instead of the reference's row-major
 *   H2 x W2 slices: every (edge,pixel) slice is stored as 4 x 8 element tiles (one 128-byte line each), tiles
 *   row-major over the slice padded to multiples of (4, 8):
 *     pos(y, x) = ((y/4) * ceil(W2/8) + x/8) * 32 + (y%4) * 8 + x%8,   slice pitch = ceil(H2/4)*ceil(W2/8)*32 floats.
 *   HBM is fetched in whole 128-byte lines; a pixel's tap footprint touches ~40 % fewer lines in this layout.
 *   H2[l], W2[l] stay the LOGICAL sizes.  Produced by lgu_volume_pyramid_tiled_f32 / lgu_volume_retile_f32.
 *   Served for radius 3 (the production case); otherwise LGU_E_UNSUPPORTED.  Results are bit-identical to the
 *   reference layout. */
#define LGU_PYR_TILED 2
/* LGU_PYR_COORDS_LAST: coords is (E,H1,W1,2) with x, y interleaved — how factor_graph.py holds them — instead of the
 *   operator's (E,2,H1,W1) planes: saves the permute().contiguous() pass of corr.py:91 in front of every lookup.
 *   Served by the fast kernels (radius 1..3, 16-byte aligned operands); otherwise LGU_E_UNSUPPORTED. */
#define LGU_PYR_COORDS_LAST 4
/* LGU_PYR_OUT_NHWC: out is channel-last, (E, H1, W1, L*rd*rd) — the memory format the consumer of the lookup, the 1x1
 *   convolution of UpdateModule.corr_encoder (droid_net.py:76-80), prefers — instead of (E, L*rd*rd, H1, W1); same
 *   values.  LGU_PYR_OUT_F16 (with LGU_PYR_OUT_NHWC only, else LGU_E_BADARG): out holds IEEE half, each value the
 *   round-to-nearest-even of the fp32 result, i.e. exactly the cast autocast applies in front of that convolution
 *   (factor_graph.py wraps the update operator in autocast); `out` then points at E*H1*W1*L*rd*rd 2-byte elements.
 *   Served by the production kernel (LGU_PYR_TILED, radius 3); otherwise LGU_E_UNSUPPORTED. */
#define LGU_PYR_OUT_NHWC 8
#define LGU_PYR_OUT_F16 16
int lgu_defcorr_pyramid_fwd_f32(const float* const* volumes, const float* coords,
                                float* const* offsets, float* out,
                                int L, int E, int H1, int W1, const int* H2, const int* W2,
                                int radius, int flags, void* stream);

/* The same with a storage indirection for the volumes: edge e's slices are at slot edge_slot[e] (device array of E
 * int32) of the level buffers, which may hold more slots than E.  This is what lets the CorrBlock state container
 * implement `cat` (factor_graph.py:123) and `__getitem__` (:139) by editing a small index array instead of copying the
 * multi-GB pyramid as the reference's tensor concatenation / boolean indexing do.  Offsets, coords and out are indexed by e as before.
 * Served by the fast kernels; otherwise LGU_E_UNSUPPORTED. */
int lgu_defcorr_pyramid_slots_fwd_f32(const float* const* volumes, const int* edge_slot, const float* coords,
                                      float* const* offsets, float* out,
                                      int L, int E, int H1, int W1, const int* H2, const int* W2,
                                      int radius, int flags, void* stream);

/* The lookup with its consumer fused in: lgu_defcorr_pyramid_slots_fwd_f32 followed by the first layer of
 * UpdateModule.corr_encoder (reference droid_slam/droid_net.py:76-77,116: Conv2d(L*rd*rd, 128, 1) + ReLU, evaluated
 * under autocast: half inputs and weights, fp32 accumulation, half result) on the matrix cores, in the same launch:
 *   out (E, H1, W1, enc_n) IEEE half, channel-last = relu(W1 . half(samples) + b1) per pixel
 * so the L*rd*rd samples of a pixel never go to HBM.
 *   enc_w  half (enc_n, Kp): the convolution weight (enc_n, L*rd*rd, 1, 1) with every row zero-padded to
 *          Kp = ceil(L*rd*rd / 32) * 32 entries, 16-byte aligned;   enc_b  half (enc_n).
 * edge_slot may be NULL (slot e = edge e).  flags: LGU_PYR_TILED is required; LGU_PYR_PROBE and LGU_PYR_COORDS_LAST as
 * above; the LGU_PYR_OUT_* flags do not apply (LGU_E_BADARG).  Served for radius 3, enc_n = 128, zero-offset patterns
 * the sampler handles in one launch (none / all / levels >= 2); otherwise LGU_E_UNSUPPORTED.  Offsets get the same in-place side
 * effects as in the unfused entry.  enc_w and out 16-byte, enc_b 8-byte aligned, the rest as in the unfused entry; otherwise
 * LGU_E_UNSUPPORTED. */
int lgu_defcorr_pyramid_enc_fwd_f32(const float* const* volumes, const int* edge_slot, const float* coords,
                                    float* const* offsets, const void* enc_w, const void* enc_b, void* out,
                                    int L, int E, int H1, int W1, const int* H2, const int* W2,
                                    int radius, int enc_n, int flags, void* stream);

/* Tail of GaussianMask.gaussian_parameters (reference droid_slam/gaussianMask_cuda.py:69-83) after the two linear heads:
 *   mean_ofs, cov_raw (E, H*W, 2) fp32 or half (is_half: the heads ran under autocast; steps rounded to half like the
 *   framework's half kernels);  mean (E,H,W,2) fp32 = pixel grid (x, y) + mean_ofs;  cov (E,H,W,2) fp32 =
 *   sigmoid(per-sample standardised cov_raw) * 5 + 0.05;  det (E, H*W) = cov.x * cov.y in the input's dtype. */
int lgu_gaussian_params(const void* mean_ofs, const void* cov_raw, float* mean, float* cov, void* det,
                        int E, int H, int W, int is_half, float eps, void* stream);

/* The uncertainty mask of AltCorrBlock.corr_fn (reference droid_slam/modules/corr.py:203-207) applied in place:
 *   probe (E, T, H*W): the T = 9 plain level-1 samples of every pixel (altcorr_forward, radius 1);
 *   offset (E, H*W, C) IN/OUT: offset[e][p][:] *= sigmoid(unbiased variance of probe[e][:][p]). */
int lgu_probe_mask_scale_f32(const float* probe, float* offset, int E, int HW, int T, int C, void* stream);

/* The level-0 offset head of AltCorrBlock.corr_fn (reference droid_slam/modules/corr.py:174-189, :220:
 * ofsMap(cat(fmap[ii] * 4, fmap[jj] * 4).float()), a Conv2d(2C, Cout, 3, padding=1) evaluated in fp32) straight from the
 * stored half frame buffers, on the half matrix cores with fp32-accurate weights:
 *   frames (NF, H, W, C) half, channel-last (AltCorrBlock.pyramid[0], = fmap / 4);  ii, jj (E) int64 frame indices;
 *   wpack: the weight times 4 (exact), split into two half parts hi + lo (22 significant bits) and laid out in MFMA
 *          fragment order [9 taps][2C/32][hi, lo][7][64 lanes][8] (lgu_slam_amd.ops.pack_offset_conv builds it);
 *   bias (Cout) fp32;  out (E, Cout, H, W) fp32 fully written.
 * Half x half products are exact in fp32 and accumulation is fp32, so the result equals the fp32 convolution up to the
 * 2^-22 truncation of the weights (below that convolution's own summation noise).  frames_lo (may be NULL): a second
 * half part of the input, same layout — input = frames + frames_lo — for inputs that need up to 24 bits (the residual
 * head of :219-220 takes 2 x 2 averages of the frames; split as hi = half(x), lo = half(x - hi)).  C % 32 == 0,
 * Cout <= 112, frames, frames_lo, wpack and out 16-byte aligned (LDS-DMA of the weights, 16-byte loads of the frames, 16-byte
 * stores); otherwise LGU_E_UNSUPPORTED. */
int lgu_offset_conv_frames_h16(const void* frames, const void* frames_lo, const long long* ii, const long long* jj,
                               const void* wpack, const float* bias, float* out, int E, int H, int W, int C, int Cout,
                               void* stream);

/* The same heads through per-FRAME partial convolutions (csrc/offconv.hip).  The convolution is linear in its input
 * cat(frame ii, frame jj): conv(cat(a, b)) = conv_A(a) + conv_B(b), a frame is source / target of ~10 edges each, and one
 * AltCorrBlock serves every chunk of an update_lowmem pass (reference factor_graph.py:272-300): P_A[f] = conv_A(frames[f])
 * + bias and P_B[f] = conv_B(frames[f]) are computed once per frame and kept, an edge's output is P_A[ii] + P_B[jj].
 *   lgu_offset_heads_mark         claims, on the device, the frames of ii (half 0) / jj (half 1) whose partials are
 *                                 missing: done (2, NF) int32 flags (0 = missing, set to 1), worklist (>= 2E ints)
 *                                 receives frame * 2 + half per claimed frame, *count their number (zero before the first
 *                                 call; reset by the combine).
 *   lgu_offset_conv_worklist_h16  the partial convolutions of the worklist: wpack_a / wpack_b = the weight's two input halves
 *                                 packed like wpack above (C input channels each, C % 64 == 0), bias added to P_A only;
 *                                 PA, PB (NF, Cout, H, W) fp32; maxwork >= the worklist's possible length (sizes the grid).
 *   lgu_offset_heads_combine_f32  out[e] = PA[ii[e]] + PB[jj[e]] over rows of n floats (n % 4 == 0); *count_reset = 0.
 * frames, frames_lo, wpack_a, wpack_b, PA, PB and out 16-byte aligned, otherwise LGU_E_UNSUPPORTED. */
int lgu_offset_heads_mark(const long long* ii, const long long* jj, int E, int* done, int NF, int* worklist, int* count,
                          void* stream);
int lgu_offset_conv_worklist_h16(const void* frames, const void* frames_lo, const int* worklist, const int* count, int maxwork,
                                 const void* wpack_a, const void* wpack_b, const float* bias_a, float* PA, float* PB, int H,
                                 int W, int C, int Cout, void* stream);
int lgu_offset_heads_combine_f32(const float* PA, const float* PB, const long long* ii, const long long* jj, float* out, int E,
                                 int n, int* count_reset, void* stream);

/* Post-processing of the learned sampling offsets (reference droid_slam/modules/corr.py:117-135 and :217-235 with
 * per_Corr_Normalization, gaussianMask_cuda.py:26-33) in one pass:
 *   o0 (E,C,H,W), o1 (E,C,Hl,Wl): the outputs of the two offset convolutions (o1 still at the pooled resolution; the
 *   nearest-neighbour upsampling to (H,W) is an index map inside the kernel), fp32 or IEEE half (is_half);
 *   out0 = 4 tanh((o0 - mean) / sqrt(var + eps)),  out1 = (4 tanh((o1 - mean1) / sqrt(var1 + eps)) + out0) / 2,
 *   statistics per edge over (C,H,W), biased variance; both written as (E,H,W,C) fp32 — the (E,H,W,rd,rd,2) tensors
 *   the samplers take.  is_half = 1: every step is rounded to half as the framework's half kernels do; is_half = 2: the
 *   same for level 0, level 1 in fp32 — what autocast yields, which promotes the nearest upsampling to fp32.
 * scratch: lgu_offsets_finalize_scratch_bytes(E) bytes of device memory (partial sums; no initialisation needed), 8-byte
 * aligned (it holds doubles), else LGU_E_BADARG. */
long long lgu_offsets_finalize_scratch_bytes(int E);
int lgu_offsets_finalize(const void* o0, const void* o1, float* out0, float* out1, void* scratch,
                         int E, int C, int H, int W, int Hl, int Wl, int is_half, float eps, void* stream);
/* The same with the uncertainty mask of AltCorrBlock.corr_fn (reference corr.py:203-207) folded in: probe (E, T, H, W) fp32,
 * the T >= 2 plain level-1 samples of every pixel; out1 = level-1 offsets * sigmoid(unbiased variance over T) — bit for bit
 * lgu_offsets_finalize followed by lgu_probe_mask_scale_f32, without the extra read-modify-write pass over out1. */
int lgu_offsets_finalize_masked(const void* o0, const void* o1, const float* probe, int T, float* out0, float* out1,
                                void* scratch, int E, int C, int H, int W, int Hl, int Wl, int is_half, float eps,
                                void* stream);

/* Fused volume post-processing of CorrBlock.__init__ (reference droid_slam/gaussianMask_cuda.py:84-86
 * and droid_slam/modules/corr.py:79-86): in ONE pass over the raw all-pairs volume
 *   level0 = gaussianMask(means, covs, volume, radius) / (6.28*sqrt(covs.x*covs.y)) + volume
 *   level l = avg_pool2d(level l-1, 2, stride 2) over the target dims, l = 1..L-1
 * levels[l] (E,H1,W1,H2>>l,W2>>l) fully written; levels[0] may alias `volume` (in place).
 * `levels` is a HOST array of L device pointers.  Requires W2 % 4 == 0 and a slice pyramid
 * that fits LDS (<= 96 KiB), `volume` and levels[0] 16-byte aligned (the coarser levels are stored by element); otherwise
 * LGU_E_UNSUPPORTED and the caller composes the ops.  The same holds for the three entries below. */
int lgu_volume_pyramid_f32(const float* means, const float* covs, const float* volume, float* const* levels, int L,
                           int E, int H1, int W1, int H2, int W2, int radius, void* stream);

/* Same as lgu_volume_pyramid_f32 but every level is written in the tiled slice layout (LGU_PYR_TILED above).
 * levels[0] may alias `volume` when H2 % 4 == 0 and W2 % 8 == 0 (the slice is converted in place). */
int lgu_volume_pyramid_tiled_f32(const float* means, const float* covs, const float* volume, float* const* levels,
                                 int L, int E, int H1, int W1, int H2, int W2, int radius, void* stream);

/* The same over a HALF raw volume (what the all-pairs product of the half feature maps returns, corr.py:145-152): the
 * `.float()` of corr.py:64 becomes this kernel's load (exact) instead of a pass of its own over the volume.  Levels are
 * fp32 as above; tiled != 0 writes them in the tiled slice layout.  levels[0] cannot alias `volume`. */
int lgu_volume_pyramid_h16(const float* means, const float* covs, const void* volume, float* const* levels, int L,
                           int E, int H1, int W1, int H2, int W2, int radius, int tiled, void* stream);

/* The same builder with the determinant handed over: det (E*H1*W1) is what GaussianMask.forward computes as
 * `det = cov[:,:,0] * cov[:,:,1]` (gaussianMask_cuda.py:79), fp32 or IEEE half (det_half != 0).  Inside the reference's
 * autocast region (factor_graph.py:90) det IS a half tensor, and the denominator `6.28 * sqrt(det)` (:85) is rounded to half after
 * the square root and after the product; a half det reproduces those roundings, an fp32 det is the fp32 evaluation
 * (= lgu_volume_pyramid_f32 / _tiled_f32 / _h16, which form det = cov0 * cov1 themselves).  volume_half / tiled as above. */
int lgu_volume_pyramid_det(const float* means, const float* covs, const void* det, int det_half, const void* volume,
                           int volume_half, float* const* levels, int L, int E, int H1, int W1, int H2, int W2, int radius,
                           int tiled, void* stream);

/* CorrBlock.__init__'s volume, BUILT into the tiled pyramid (reference droid_slam/modules/corr.py:145-152 matmul of the
 * two feature maps / 4 each, :64 .float(), gaussianMask_cuda.py:84-86 Gaussian re-weighting and "/ denominator + corr",
 * corr.py:79-86 three average poolings) in ONE launch on the fp32 matrix cores: the raw all-pairs volume never reaches HBM.
 *   fmap1, fmap2 (E, C, H, W) fp32, the reference's NCHW maps (un-scaled: the kernel applies the / 16 exactly)
 *   means, covs (E, H, W, 2), det (E*H*W) fp32 / half (det_half) or NULL: as lgu_volume_pyramid_det
 *   levels[l] (E, H, W, <tiled slice of (H >> l, W >> l)>) fp32, fully written incl. the slices' zero padding; L must be 4
 * Served: H % 8 == 0, W in {16, 32, 64}, C % 16 == 0, fmap1, fmap2 and every levels[l] 16-byte aligned; anything else
 * LGU_E_UNSUPPORTED (callers take the library GEMM + lgu_volume_pyramid_*).  Equal to that composition up to the GEMM's
 * fp32 summation order. */
int lgu_volume_build_pyramid_f32(const float* fmap1, const float* fmap2, const float* means, const float* covs, const void* det,
                                 int det_half, float* const* levels, int L, int E, int C, int H, int W, int radius, void* stream);

/* The same for HALF feature maps (the reference under autocast, factor_graph.py:90: corr.py:145-152 is then a half GEMM —
 * exact half x half products, fp32 accumulation, one rounding of each sum to half, which this kernel applies before the
 * .float() of corr.py:64).
 *   feats (E, H, W, 2C) half, channel-last, the source map's C channels first then the target map's (un-scaled;
 *   CorrBlock's `t`, corr.py:57-62)
 *   workspace: E*H*W*2C halves of scratch, 16-byte aligned, distinct from feats (a first small launch re-orders the maps
 *   into MFMA fragment order there; contents afterwards unspecified)
 * Served: H % 8 == 0, W in {16, 32, 64}, C % 32 == 0, feats, workspace and every levels[l] 16-byte aligned.  Differs from
 * the library half GEMM + lgu_volume_pyramid_det only where a different fp32 summation order moves a sum across a half
 * rounding boundary (one half ulp of that raw product). */
int lgu_volume_build_pyramid_h16(const void* feats, void* workspace, const float* means, const float* covs, const void* det,
                                 int det_half, float* const* levels, int L, int E, int C, int H, int W, int radius, void* stream);

/* Layout conversion of `nslices` slices of H2 x W2 floats: to_tiled != 0: row-major -> tiled, else tiled -> row-major
 * (padding elements of the tiled form are written as 0).  src and dst must not overlap. */
int lgu_volume_retile_f32(const float* src, float* dst, long long nslices, int H2, int W2, int to_tiled, void* stream);

/* ---- low-memory (on-the-fly correlation) path ---------------------------------- */

/* The channel contraction of the two forward operators below runs on the matrix cores for radius 1..3 and
 * C in {16, 32, 64, 128} (v_mfma_f32_16x16x4_f32: exact fp32 products, fp32 fmaf-chain accumulation; the channel
 * summation order differs from the reference's, results agree to fp32 rounding, tests: 1e-5); other shapes take
 * VALU kernels.  The matrix-core and the tile-staged kernels read the feature maps 16 bytes and coords / offset 8 bytes
 * (one (x, y) pair) at a time: with fmap1 or fmap2 below 16-byte or coords or offset below 8-byte alignment the _f32
 * entries (lowMem_defSample, altcorr_forward: any contiguous tensor is served) take the wave-per-pixel kernel, which
 * accesses everything by element — another channel summation order, same 1e-5 — and the _h16 and pyramid entries, which
 * have no such kernel, return LGU_E_UNSUPPORTED.  corr / out: 16-byte stores when it is 16-byte aligned and W1 % 4 == 0,
 * element stores of the same values otherwise.
 *
 * defCorrSample.lowMem_defSample        (droid.cpp:124-136, lowMem_defSample.cu:27-134,137-168).
 *   fmap1 (B,H1,W1,C)  fmap2 (B,H2,W2,C)  coords (B,S,H1,W1,2) [x,y interleaved]
 *   offset (NO,H1,W1,rd,rd,2) IN/OUT — indexed with b*s exactly as the reference does
 *   (lowMem_defSample.cu:80-83), i.e. offset[0] for every b when S == 1;
 *   corr (B,S,rd,rd,H1,W1) fully written. Requires C % 32 == 0 and (B-1)*(S-1) < NO. */
int lgu_lowmem_defsample_fwd_f32(const float* fmap1, const float* fmap2, const float* coords,
                                 float* offset, float* corr,
                                 int B, int S, int H1, int W1, int H2, int W2, int C, int NO,
                                 int radius, void* stream);

/* droid_backends.altcorr_forward        (src/droid.cpp:193-203, src/altcorr_kernel.cu:27-149,290-319).
 *   corr (B,S,rd*rd,H1,W1), channel = ix*rd + iy, fully written. Requires C % 32 == 0. */
int lgu_altcorr_fwd_f32(const float* fmap1, const float* fmap2, const float* coords, float* corr,
                        int B, int S, int H1, int W1, int H2, int W2, int C,
                        int radius, void* stream);

/* droid_backends.altcorr_backward       (src/droid.cpp:205-217, src/altcorr_kernel.cu:152-286,321-356).
 *   fmap1_grad (B,H1,W1,C) fully written; fmap2_grad (B,H2,W2,C) ACCUMULATED with float
 *   atomics (caller zero-fills); coords_grad is never written by the reference and is
 *   not part of this ABI (the host shim returns zeros). */
int lgu_altcorr_bwd_f32(const float* fmap1, const float* fmap2, const float* coords,
                        const float* corr_grad, float* fmap1_grad, float* fmap2_grad,
                        int B, int S, int H1, int W1, int H2, int W2, int C,
                        int radius, void* stream);

/* Mixed-precision forms of the two low-memory forward operators: feature maps in IEEE half
 * (as droid_slam/depth_video.py stores them), everything else — coords, offsets, products,
 * sums, output — fp32.  The reference call sites (droid_slam/modules/corr.py:202,209) convert with
 * .float() and run the fp32 operator; these entries skip the conversion passes and, for
 * C in {32, 64, 128, 256}, run the channel contraction on the matrix cores
 * (v_mfma_f32_16x16x32_f16: half products are exact in fp32, accumulation is fp32), so the result
 * equals the _f32 entry on fmap.float() up to fp32 summation order (<= 1e-5; measured 2.4e-7).
 * Other C (multiples of 16) take a VALU kernel that is bit-identical to the _f32 entry.
 * Same shapes/side effects as the _f32 forms; radius in 1..3, otherwise LGU_E_UNSUPPORTED. */
int lgu_lowmem_defsample_fwd_h16(const void* fmap1_half, const void* fmap2_half, const float* coords,
                                 float* offset, float* corr,
                                 int B, int S, int H1, int W1, int H2, int W2, int C, int NO,
                                 int radius, void* stream);
int lgu_altcorr_fwd_h16(const void* fmap1_half, const void* fmap2_half, const float* coords, float* corr,
                        int B, int S, int H1, int W1, int H2, int W2, int C,
                        int radius, void* stream);

/* The per-level loop of AltCorrBlock.corr_fn (reference droid_slam/modules/corr.py:192-213) in ONE launch:
 *   for l in 0..L-1   out[:, :, l*rd*rd:(l+1)*rd*rd] =
 *       lowMem_defSample(fmap1[ii].float(), fmap2[l][jj].float(), coords / 2^(lbase+l), offsets[l], radius)
 * written straight into the concatenated tensor out (B,S,L*rd*rd,H1,W1) (what corr.py:211-213 builds for S == 1).
 *   fmap1 (F,H1,W1,C), fmap2[l] (F,H2[l],W2[l],C): the FRAME buffers of the pyramid; ii, jj: device arrays of B int64
 *   frame indices (corr.py:193-194 `self.pyramid[i][:, jj]`) read in place — no gathered per-edge copies.  ii == jj ==
 *   NULL: fmap1 / fmap2[l] are already per-edge, (B,...).
 *   coords (B,S,H1,W1,2) in level-0 units; lbase = pyramid level of fmap2[0] (the level-1 probe of corr.py:201-202 is
 *   this entry with L = 1, lbase = 1, offsets = {NULL}, radius = 1).
 *   offsets[l] (NO,H1,W1,rd,rd,2) IN/OUT with the reference's offset[b*s] indexing, or NULL = zero offsets.
 *   `fmap2`, `offsets`, `H2`, `W2` are HOST arrays of length L <= 4.
 * _h16: half feature maps (C in {32,64,128,256}); _f32: float feature maps, exact fp32 on v_mfma_f32_16x16x4_f32
 * (C in {16,32,64,128}); radius in 1..3; otherwise LGU_E_UNSUPPORTED (compose the per-level entries instead). */
int lgu_lowmem_pyramid_fwd_h16(const void* fmap1_half, const void* const* fmap2_half, const float* coords,
                               float* const* offsets, float* out,
                               int L, int lbase, int B, int S, int H1, int W1, const int* H2, const int* W2, int C, int NO,
                               int radius, const long long* ii, const long long* jj, void* stream);
int lgu_lowmem_pyramid_fwd_f32(const float* fmap1, const float* const* fmap2, const float* coords,
                               float* const* offsets, float* out,
                               int L, int lbase, int B, int S, int H1, int W1, const int* H2, const int* W2, int C, int NO,
                               int radius, const long long* ii, const long long* jj, void* stream);

/* The same with every fmap2[l] in this library's CHUNK-PLANAR form (F, C/k, H2l, W2l, k), k = 8 halves / 4 floats (16
 * bytes of channels); fmap1 stays channel-last.  Same results bit for bit (same products, same summation order); the
 * sweep's operand loads then read 256 contiguous bytes per 16 x-adjacent positions instead of 16 separate lines, which
 * is what bounds it.  AltCorrBlock keeps its feature pyramid in this form. */
int lgu_lowmem_pyramid_chunked_fwd_h16(const void* fmap1_half, const void* const* fmap2_half, const float* coords,
                                       float* const* offsets, float* out,
                                       int L, int lbase, int B, int S, int H1, int W1, const int* H2, const int* W2, int C, int NO,
                                       int radius, const long long* ii, const long long* jj, void* stream);
int lgu_lowmem_pyramid_chunked_fwd_f32(const float* fmap1, const float* const* fmap2, const float* coords,
                                       float* const* offsets, float* out,
                                       int L, int lbase, int B, int S, int H1, int W1, const int* H2, const int* W2, int C, int NO,
                                       int radius, const long long* ii, const long long* jj, void* stream);

/* SEVERAL calls of AltCorrBlock.corr_fn in ONE launch (the chunk loop of update_lowmem, reference
 * droid_slam/factor_graph.py:272-279, runs one corr_fn call per chunk of source frames only to bound memory).  The B
 * edges are the calls' edges back to back, one sample per pixel (S = 1); `offsets[l]` holds NO rows (NO = number of
 * calls), row k = the offsets of call k's FIRST edge — the only row the reference's sampler reads in a call:
 * offset[b*n] with n = 0 (offersample_LGS/lowMem_defSample.cu:80-83) — and off_row (device, B ints, values in [0, NO))
 * names each edge's call.  Edge b's results are, bit for bit, those of lgu_lowmem_pyramid_(chunked_)fwd_h16 over its
 * call alone.  coords (B,1,H1,W1,2), out (B,1,L*rd*rd,H1,W1).  chunked != 0: fmap2 levels in the chunk-planar form.
 * Half maps with C in {32,64,128}, radius 1..3 (the cooperative kernel); LGU_E_UNSUPPORTED otherwise — the caller
 * then issues the calls one by one.  Out-of-range off_row values are clamped to [0, NO) on the device. */
int lgu_lowmem_pyramid_calls_fwd_h16(const void* fmap1_half, const void* const* fmap2_half, const float* coords,
                                     float* const* offsets, float* out,
                                     int L, int lbase, int B, int H1, int W1, const int* H2, const int* W2, int C, int NO,
                                     const int* off_row, int radius, const long long* ii, const long long* jj, int chunked,
                                     void* stream);

/* ---- dense bundle adjustment: device kernels (first version) ---------------------------
 * The data-parallel kernels of droid_backends.ba (reference src/droid.cpp:88-107 -> src/droid_kernels.cu:1314-1434).
 * The reference's host driver copies every block to the CPU and solves with Eigen; here lgu-slam_amd/ba.py assembles
 * and solves the reduced camera system on the device and calls these for its operands.  All index arrays are int64
 * device arrays (the dtype the reference's tensors have).  Parity: the kernels are held to the reference's own kernels
 * (tests/test_droid_kernels_vs_reference_build.py); the assembly and solve, Eigen host code there, to oracle/ba_oracle.py.
 *
 * lgu_ba_build_f32        projective_transform_kernel (:176-425): per edge e = (ii[e] -> jj[e]): reprojection residual of
 *   targets (E,2,ht,wd) with weights (E,2,ht,wd), pose / depth Jacobians; Hs (4,E,6,6) = Hii,Hij,Hji,Hjj, vs (2,E,6),
 *   Eii, Eij (E,6,ht*wd), Cii, wi (E,ht*wd), all fully written.  poses (N,7) = t, q(xyzw); disps (N,ht,wd); intrinsics (4).
 *   An edge's pixels are split over lgu_ba_build_slices(E) workgroups (so that tens of edges still fill 256 CUs);
 *   `scratch` (device, E * slices * 90 floats) holds their partial sums, which a second kernel adds in slice order.
 * lgu_ba_accum_f32        accum_kernel (:854-874): out[j] = sum of inp rows idxs[ptrs[j] .. ptrs[j+1]), rows of D floats.
 * lgu_ba_depth_system_f32 the depth block of the normal equations in one pass (ba_cuda :1394-1398): for depth frame kx[j],
 *                         C = sum_{edges of the frame} Cii + m*0.05 + (1-m)*eta, w = sum wi - m*0.05*(disps - disps_sens),
 *                         m = (disps_sens > 0); writes Q = 1/C and w, both (K,ht*wd).  Segment tables as lgu_ba_accum_f32;
 *                         eta (eta_rows, ht*wd) with eta_rows in {1, K}.
 * lgu_ba_depth_update_f32 dz = Q (w - sum_{E entries of the frame} dw) (:1415) and disps[kx[j]] += dz (:933-946) in one pass.
 * lgu_ba_scatter_sum_f64  assembly of the reduced camera system (SparseBlock::update_lhs / update_rhs :1137-1179, on the CPU
 *                         in the reference): out[dst[j]] += sign * sum of inp rows idxs[ptrs[j] .. ptrs[j+1]) in double, rows of
 *                         D floats; one thread per output component, fixed summation order (bit-reproducible).
 * lgu_ba_eet_f32          EEt6x6_kernel (:1001-1056): S[b] = (E[idx[b][0]] * Q[idx[b][2]]) E[idx[b][1]]^T, idx (nblocks,3).
 * lgu_ba_ev_f32           Ev6x1_kernel (:1059-1093): v[n] = E[n] (Q[kk[n]] * w[kk[n]]), fully written.
 * lgu_ba_evt_f32          EvT6x1_kernel (:1095-1115): dw[n] = E[n]^T x[idx[n]], zero rows where idx[n] <= 0 or >= P
 *                         (the reference's condition, kept).
 * lgu_ba_solve_f64        SparseBlock::solve (:1206-1231), which the reference runs on the CPU with Eigen: damping
 *                         diag += ep + lm*diag, blocked Cholesky and both triangular solves in one workgroup with the
 *                         matrix in LDS.  A (6P x 6P, row-major double, symmetric), b (6P) double; x (P,6) float; x = 0
 *                         if the damped matrix is not positive definite.  6P <= 192 (the matrix lives in LDS as a packed lower triangle), otherwise LGU_E_UNSUPPORTED.
 * lgu_ba_solve_blocked_f64  the same solve for any window size (csrc/ba_chol.hip): blocked Cholesky over 32-column panels
 *                         (every workgroup factorises the diagonal block in LDS, one thread per row below it; 64 x 64 tiles
 *                         for the trailing update), the right-hand side carried as row 6P of the matrix, back substitution
 *                         in one workgroup.  A is OVERWRITTEN with the factor; work >= lgu_ba_solve_blocked_work_doubles(P)
 *                         doubles; x = 0 if not positive definite.
 * lgu_ba_pose_retr_f32    pose_retr_kernel (:898-931): poses[k] <- exp(dx[k-t0]) * poses[k], k in [t0, t1).
 * lgu_ba_disp_retr_f32    disp_retr_kernel (:933-946): disps[inds[b]] += dz[b]. */
int lgu_ba_build_f32(const float* targets, const float* weights, const float* poses, const float* disps,
                     const float* intrinsics, const long long* ii, const long long* jj,
                     float* Hs, float* vs, float* Eii, float* Eij, float* Cii, float* wi, float* scratch,
                     int E, int ht, int wd, void* stream);
int lgu_ba_build_slices(int E);
int lgu_ba_accum_f32(const float* inp, const long long* ptrs, const long long* idxs, float* out, int nout, int D, void* stream);
int lgu_ba_depth_system_f32(const float* Cii, const float* wi, const long long* ptrs, const long long* idxs, const long long* kx,
                            const float* disps, const float* disps_sens, const float* eta, int eta_rows, float* Q, float* w,
                            int K, int HW, void* stream);
int lgu_ba_depth_update_f32(const float* Q, const float* w, const float* dw, const long long* ptrs, const long long* idxs,
                            const long long* kx, float* dz, float* disps, int K, int HW, void* stream);
int lgu_ba_scatter_sum_f64(const float* inp, const long long* ptrs, const long long* idxs, const long long* dst, double* out,
                           int m, int D, double sign, void* stream);
int lgu_ba_eet_f32(const float* E, const float* Q, const long long* idx, float* S, int nblocks, int D, void* stream);
int lgu_ba_ev_f32(const float* E, const float* Q, const float* w, const long long* kk, float* v, int n, int D, void* stream);
int lgu_ba_evt_f32(const float* E, const float* x, const long long* idx, float* dw, int n, int D, int P, void* stream);
int lgu_ba_solve_f64(const double* A, const double* b, float* x, int P, double lm, double ep, void* stream);
long long lgu_ba_solve_blocked_work_doubles(int P);
int lgu_ba_solve_blocked_f64(double* A, const double* b, float* x, double* work, int P, double lm, double ep, void* stream);
/* lgu_ba_assemble_f64: the four scatter sums of one iteration, their zero-fills and the blocked -> dense permutation in one
 * launch: block d = bi * P + bj of the system = sum of Hs rows [hptr[d], hptr[d+1]) of hidx - sum of S rows (sptr, sidx;
 * S may be NULL: motion only), written to Ad (6P x 6P row-major, double); b (6P) likewise from vs / sv.  CSR tables cover
 * all P*P (resp. P) destinations.  An entry e < 0 of sidx stands for row -e - 1 of S TRANSPOSED (S_ca = S_ac^T: the caller
 * computes the Schur products for a <= c only); direct entries first in a segment.  Per-entry arithmetic and summation
 * order are those of lgu_ba_scatter_sum_f64 (direct rows, then transposed rows).
 * Alignment: every kernel of csrc/ba.hip accesses its operands by element; lgu_ba_solve_blocked_f64 alone loads A and work
 * 16 bytes at a time and returns LGU_E_BADARG for a misaligned one. */
int lgu_ba_assemble_f64(const float* Hs, const long long* hptr, const long long* hidx, const float* S, const long long* sptr,
                        const long long* sidx, const float* vs, const long long* vptr, const long long* vidx, const float* sv,
                        const long long* svptr, const long long* svidx, double* Ad, double* b, int P, void* stream);
int lgu_ba_pose_retr_f32(float* poses, const float* dx, int t0, int t1, void* stream);
int lgu_ba_disp_retr_f32(float* disps, const float* dz, const long long* inds, int n, int HW, void* stream);

/* ---- geometry entries of droid_backends (reference src/droid.cpp:237-249) ---------------------------------------
 * frame_distance, projmap, depth_filter and iproj of src/droid_kernels.cu.  poses (np,7) float = t, q(xyzw); disps
 * (nd,ht,wd) float; intrinsics (>= 4 floats) = fx, fy, cx, cy; index arrays are int64 device arrays.  Per-pixel values
 * follow the reference's fp32 operation order bit for bit.  A frame index is valid when 0 <= index < min(np, nd); no
 * kernel dereferences an invalid one (the reference reads out of bounds).  Every output element is written (the
 * reference's outputs are zero-filled first; these need no fill).  Launched on `stream`, no host synchronisation.
 *
 * lgu_frame_distance_f32  frame_distance_kernel (:518-658, host :1438-1460): dist[k] for the pair ii[k] -> jj[k]: per
 *   pixel, the flow magnitude under T_ij (weight beta) and under its translation alone (weight 1 - beta); a weight
 *   always counts to the total, to the valid weight and (times the magnitude) to the sum only where the point's depth
 *   > 0.25.  dist = 1000 if valid / (total + 1e-8) < 0.75 (in double), else sum / valid.  The pixels of a pair are
 *   summed in a fixed order that depends on (ht, wd) only: a pair's result does not depend on the batch it is in.
 *   NaN for a pair with an invalid index.
 * lgu_projmap_f32         projmap_kernel (:427-516, host :1463-1488): coords (num,ht,wd,3) = (u, v, 0), (u, v) replaced
 *   by the projection into jj[k] where the depth > 0.01 (double comparison); valid (num,ht,wd,1) = depth > 0.25.  A pair
 *   with an invalid index: coords (NaN, NaN, 0), valid 0.
 * lgu_depth_filter_f32    depth_filter_kernel (:661-776, host :1491-1515): counter (num,ht,wd), for each pixel of frame
 *   ix[b], the number of neighbours ix-1, ix-2, ix-3, ix+3, ix+4, ix+5 (valid ones only) in which the pixel projects
 *   with floor(u) in [0, wd-1) and floor(v) in [0, ht-1) and |1/d_proj - 1/d_corner| < thresh[b] in double for one of
 *   the four corners.  floor() converts to int as v_cvt_i32_f32 does (NaN -> 0, saturating).  A zero row for an
 *   invalid ix[b].
 * lgu_iproj_f32           iproj_kernel (:779-851, host :1518-1541): points (nd,ht,wd,3) = act_se3(poses[n], (x, y, 1, d))
 *   divided by d; NaN points for frames n >= np.
 * Sizes: num, np, nd, ht, wd >= 0 (num == 0 or an empty frame: nothing is launched), ht * wd < 2^31 / 3, otherwise
 * LGU_E_BADARG; more than 65535 * 256 pixels per frame: LGU_E_UNSUPPORTED (projmap, depth_filter, iproj). */
int lgu_frame_distance_f32(const float* poses, int np, const float* disps, int nd, int ht, int wd, const float* intrinsics,
                           const long long* ii, const long long* jj, int num, float beta, float* dist, void* stream);
int lgu_projmap_f32(const float* poses, int np, const float* disps, int nd, int ht, int wd, const float* intrinsics,
                    const long long* ii, const long long* jj, int num, float* coords, float* valid, void* stream);
int lgu_depth_filter_f32(const float* poses, int np, const float* disps, int nd, int ht, int wd, const float* intrinsics,
                         const long long* ix, const float* thresh, int num, float* counter, void* stream);
int lgu_iproj_f32(const float* poses, int np, const float* disps, int nd, int ht, int wd, const float* intrinsics,
                  float* points, void* stream);

/* ---- projective_transform and the motion features (reference droid_slam/geom/projective_ops.py:18-128,
 * factor_graph.py:210-212) -----------------------------------------------------------------------------------------
 * Reprojection, without a Lie-group library, of every pixel of frame ii[k] into frame jj[k], per batch b.
 * poses (B,np,7) float = t, q(xyzw), used as given (not normalised); disps (B,nd,ht,wd); intrinsics (B,ni,4) = fx, fy, cx, cy PER FRAME
 * (back-projection reads frame ii[k]'s row, projection frame jj[k]'s); ii, jj int64 device arrays of num entries, shared
 * by the batches.  Per pixel: X0 = ((u - cx) / fx, (v - cy) / fy, 1, disp); G_ij = G_j * G_i^-1, replaced by t =
 * (-0.1, 0, 0), q = identity where ii == jj (the stereo baseline); X1 = (R X0[0:3] + t disp, disp); Z = X1.z, replaced
 * by 1 where Z < 0.1f; d = 1 / Z; coords = (fx (X1.x d) + cx, fy (X1.y d) + cy[, disp d]); valid = X1.z > 0.2f (float
 * comparisons, 0.2f itself is invalid).  Values follow a fixed fp32 order, bit for bit the float32 restatement of the
 * tests.  An edge is valid when 0 <= ii[k], jj[k] < min(np, nd, ni); for another edge nothing is dereferenced and its
 * coordinates, Jacobians and motion channels are NaN, valid 0.  Every output element is written (no fill needed).
 * Launched on `stream`, no host synchronisation (graph-capturable).
 *
 * lgu_projective_transform_f32  coords (B,num,ht,wd,2), or 3 channels with LGU_REPROJ_DEPTH; valid (B,num,ht,wd), may
 *   be NULL.  LGU_REPROJ_JACOBIAN also writes Ji, Jj (B,num,ht,wd,2,6) and Jz (B,num,ht,wd,2,1): Jj = Jp Ja (tangent
 *   order translation, rotation), Ji = -(Jj Adj(G_ij)), Jz = Jp (t, 1); structural zeros of Jj are written as 0.
 *   coords (2 channels) and Jz must be 8-byte aligned, Ji and Jj 16-byte aligned (else LGU_E_UNSUPPORTED).
 * lgu_motion_features_f32  FactorGraph.update's motion features in one launch: coords1 (B,num,ht,wd,2) as above and
 *   motn (B,num,4,ht,wd) = clamp((x1 - u, y1 - v, tx - x1, ty - y1), -bound, bound) with target (B,num,ht,wd,2); the
 *   clamp keeps a NaN a NaN.  valid (B,num,ht,wd) may be NULL.  coords1 and target 8-byte aligned.
 * Sizes: B, num, np, nd, ni, ht, wd >= 0 (B, num == 0 or an empty frame: nothing is launched), ht * wd < 2^31 / 3, known
 * flag bits only, bound >= 0, otherwise LGU_E_BADARG; more than 65535 * 256 pixels per frame or B > 65535:
 * LGU_E_UNSUPPORTED. */
#define LGU_REPROJ_JACOBIAN 1
#define LGU_REPROJ_DEPTH 2
int lgu_projective_transform_f32(const float* poses, const float* disps, const float* intrinsics, const long long* ii,
                                 const long long* jj, int B, int np, int nd, int ni, int ht, int wd, int num, int flags,
                                 float* coords, float* valid, float* Ji, float* Jj, float* Jz, void* stream);
int lgu_motion_features_f32(const float* poses, const float* disps, const float* intrinsics, const long long* ii,
                            const long long* jj, const float* target, int B, int np, int nd, int ni, int ht, int wd, int num,
                            float bound, float* coords1, float* motn, float* valid, void* stream);

/* ---- GraphAgg's segment mean and the convex upsampling (reference droid_slam/droid_net.py:14-37, :53-69;
 * depth_video.py:124-128) --------------------------------------------------------------------------------------------
 * Launched on `stream`, no host synchronisation, no allocation (graph-capturable); no atomics: the bits do not depend on
 * the launch geometry.
 *
 * lgu_scatter_mean_f32 / lgu_scatter_mean_h16  the reference's scatter_mean(src, index, dim, dim_size=M) with a 1-D index
 *   (droid_net.py:64, GraphAgg.forward): src (outer,n,inner) float / IEEE half, index (n,) int64, out (outer,M,inner) of
 *   src's type, FULLY written.  out[o,m,i] = S / c with S the fp32 sum of src[o,j,i] over the j with index[j] == m,
 *   added in ascending j, c the number of those j; fp32 division, then rounded to nearest even for half.  An empty
 *   segment gives 0.  An index outside [0, M) matches no segment (never read as an address, never counted).
 *   16-byte loads and stores when inner is a multiple of 16 bytes and src / out are 16-byte aligned, any inner >= 1
 *   otherwise.  outer, n, inner, M >= 0, else LGU_E_BADARG; outer * M * inner == 0 launches nothing; n == 0 writes
 *   zeros (index may then be NULL); n > 65536, M > 65536 or outer > 65535: LGU_E_UNSUPPORTED.
 * lgu_cvx_upsample_f32  cvx_upsample(data, mask) with data width 1 (droid_net.py:15-29): data (B,ht,wd) float, mask
 *   (B,576,ht,wd) float or half (LGU_UPS_MASK_F16), out (B,8ht,8wd) float, FULLY written.  Mask channel k*64 + a*8 + b
 *   weighs the neighbour (y+ky-1, x+kx-1), k = ky*3 + kx (0 outside the frame), for the output pixel (8y+a, 8x+b).  Per
 *   output: m = max_k x_k; e_k = expf(x_k - m); s = sum e_k (ascending k); w_k = e_k / s; with LGU_UPS_HALF_WEIGHTS
 *   (only with LGU_UPS_MASK_F16, else LGU_E_BADARG) w_k is rounded to half and back, as the softmax of a half mask
 *   returns half weights (FactorGraph.update, autocast off); out = sum w_k * d_k, each product rounded to fp32, added
 *   in ascending k.
 * lgu_upsample_disps_f32  DepthVideo.upsample (depth_video.py:124-128) in one launch, in place: for u < U with
 *   0 <= ix[u] < N, disps_up[ix[u]] (8ht,8wd) = cvx_upsample of disps[ix[u]] (ht,wd) with mask[u] (576,ht,wd).  Only
 *   those rows of disps_up (N,8ht,8wd) are written; an ix[u] outside [0, N) writes nothing.  With duplicate entries in
 *   ix one of the rows wins, as with index_put (the reference passes unique indices).
 * Upsampling sizes: B, N, U, ht, wd >= 0, ht * wd <= INT_MAX / 576, known flag bits, otherwise LGU_E_BADARG; an empty
 * frame, B, U or N == 0 launches nothing; out / disps_up must be 16-byte aligned and the mask aligned to its element,
 * and more than 2^32 threads are LGU_E_UNSUPPORTED. */
#define LGU_UPS_MASK_F16 1
#define LGU_UPS_HALF_WEIGHTS 2
int lgu_scatter_mean_f32(const float* src, const long long* index, int outer, int n, long long inner, int M, float* out,
                         void* stream);
int lgu_scatter_mean_h16(const void* src, const long long* index, int outer, int n, long long inner, int M, void* out,
                         void* stream);
int lgu_cvx_upsample_f32(const float* data, const void* mask, int B, int ht, int wd, int flags, float* out, void* stream);
int lgu_upsample_disps_f32(const float* disps, int N, int ht, int wd, const long long* ix, int U, const void* mask,
                           int flags, float* disps_up, void* stream);

/* ---- KAN-bias GRU of the update operator (reference droid_slam/modules/gru_kanBias.py, modules/kan.py) ----------------
 * Reference configuration only: 128 hidden channels, 448 = 128 + 320 channels of net_inp, three KANLinear(128, 128,
 * grid_size=3, spline_order=3) heads (SiLU, standalone spline scaler).  _f32: float tensors (autocast off); _h16: IEEE
 * half tensors with the reference's autocast rounding points (each intermediate the composition returns as half is
 * rounded to half).  All tensors contiguous; launched on `stream`, no host synchronisation, no allocation, no atomics
 * (graph-capturable; the bits of an edge depend only on that edge's data and H*W).  E, HW >= 0, else LGU_E_BADARG;
 * E == 0 (or HW == 0 for gates / blend) launches nothing.
 *
 * lgu_kangru_context_*  glo[e,c] = mean_p r(r(s) * net[e,c,p]), s = sigmoid(r(W·net[e,:,p] + bias[c])) with r the
 *   rounding to the tensor type (the bias joins the fp32 sum before its one rounding, as the library convolution adds
 *   it): net (E,128,HW), weight (128,128), bias (128), glo (E,128).  The 1x1 convolution runs on the matrix cores with
 *   fp32 accumulation.  partial: fp32 workspace of E * ceil(HW / LGU_KANGRU_CTX_PIXELS) * 128 floats (per-(edge, pixel
 *   tile) sums, added in ascending tile order by a second launch and divided by HW).  HW == 0 with E > 0 is
 *   LGU_E_BADARG; E > 65535 or a weight not 16-byte aligned: LGU_E_UNSUPPORTED.
 * lgu_kan_heads_*  the three heads in one launch: out[h,e,:] = r(r(silu(x)·Wb[h]ᵀ) + r(B_h(x)·Ws[h]ᵀ)), x = glo[e,:]
 *   (E,128), out (3,E,128).  grid (3,128,10) float: each head's knots per input feature (need not be uniform); B_h(x)
 *   are the 6 cubic B-spline bases of each feature by the Cox–de Boor recursion in fp32, in the reference's operation
 *   order (NaN propagates, x outside the knots gives zero bases).  wpack (384, 896) of the tensor type: row h*128 + o =
 *   [base_weight[h][o,:] (128) | (spline_weight[h] * spline_scaler[h][...,None])[o].flatten() (768)], the product formed
 *   in fp32 and then rounded; 16-byte aligned, else LGU_E_UNSUPPORTED.
 * lgu_kangru_gates_*  z = r(sigmoid(r(cz + kz))) into z (E,128,HW), and r(r(sigmoid(r(cr + kr))) * net) IN PLACE over
 *   channels 0..127 of net_inp (E,448,HW); cz, cr, net (E,128,HW), kz, kr (E,128) broadcast over the pixels.
 * lgu_kangru_blend_*  out = r(r(r(1 - z) * net) + r(z * q)), q = r(tanh(r(cq + kq))): cq, z, net, out (E,128,HW), kq
 *   (E,128).
 * Alignment: gates and blend go 16 bytes at a time when HW is a multiple of that and every (E,128,HW) / (E,448,HW) operand is
 * 16-byte aligned, by element otherwise, and so does the context's load of net: same arithmetic, same bits.
 * sigmoid(v) = 1 / (1 + expf(-v)), silu(v) = v / (1 + expf(-v)), tanh = tanhf, all in fp32. */
#define LGU_KANGRU_CTX_PIXELS 256
int lgu_kangru_context_f32(const float* net, const float* weight, const float* bias, int E, int HW, float* partial,
                           float* glo, void* stream);
int lgu_kangru_context_h16(const void* net, const void* weight, const void* bias, int E, int HW, float* partial, void* glo,
                           void* stream);
int lgu_kan_heads_f32(const float* glo, const float* grid, const float* wpack, int E, float* out, void* stream);
int lgu_kan_heads_h16(const void* glo, const float* grid, const void* wpack, int E, void* out, void* stream);
int lgu_kangru_gates_f32(const float* cz, const float* cr, const float* kz, const float* kr, const float* net, int E,
                         int HW, float* z, float* net_inp, void* stream);
int lgu_kangru_gates_h16(const void* cz, const void* cr, const void* kz, const void* kr, const void* net, int E, int HW,
                         void* z, void* net_inp, void* stream);
int lgu_kangru_blend_f32(const float* cq, const float* kq, const float* z, const float* net, int E, int HW, float* out,
                         void* stream);
int lgu_kangru_blend_h16(const void* cq, const void* kq, const void* z, const void* net, int E, int HW, void* out,
                         void* stream);

/* ---- proximity edges of the factor graph (reference droid_slam/factor_graph.py:319-383, add_proximity_factors) -------
 * Window: rows i in [t0, t), columns j in [t1, t); dist holds one float per cell at f = (i - t0) * (t - t1) + (j - t1),
 * n = (t - t0) * (t - t1) cells.  known_ii / known_jj (num_known int64 device entries, may be NULL when num_known == 0)
 * are the edges the graph already has (ii, ii_bad, ii_inac in that order); any values are allowed, an edge outside the
 * window kills the cells of its diamond that fall inside.
 *   dead cell: i - rad < j, or d > 100, or j in [max(i - rad - 1, 0), i), or (stereo and i == j), or |di| + |dj| <=
 *     max(min(|i - j| - 2, nms), 0) around a known or an accepted edge (i, j);
 *   prefix: for i = t0 .. t-1: (i, i) if stereo, then (i, j), (j, i) for j = max(i - rad - 1, 0) .. i - 1;
 *   selection: live cells with d <= thresh (d widened to double) in ascending (d, f); a live one is accepted while
 *     len(edges) <= max_factors (the first failure ends the selection; max_factors < 0 accepts nothing), appends (i, j),
 *     (j, i) and kills its diamond.
 * Against the reference: equal distances are visited in ascending f (its argsort leaves the order open) and a NaN is
 * never selected (it would accept one).  Any float orders correctly (negative values included, -0 as +0).
 * Outputs: e_ii, e_jj (capacity int64 entries each, capacity >= lgu_proximity_capacity() = min(max(prefix,
 * max_factors + 2), prefix + 2 n)) and count (one device int) = the number of entries written; nothing is written at or
 * beyond count.  Launched on `stream`, no host synchronisation, no allocation (graph-capturable).
 * Rules: 0 <= t1 <= t0 <= t, t1 <= max(t0 - rad - 1, 0), rad >= 0, nms >= 0, num_known >= 0, prefix <= 2^30, else
 * LGU_E_BADARG; n > 2^24 or t > 2^30: LGU_E_UNSUPPORTED; n == 0 writes count = 0 only.
 *
 * lgu_proximity_select_small   everything in ONE launch of one workgroup, n <= LGU_PROXIMITY_SMALL_MAX (else
 *   LGU_E_UNSUPPORTED): marking, 63-bit keys, a bitonic sort of the keys in LDS, the prefix and the greedy pass.
 * lgu_proximity_keys           marking and key build for any n: work (lgu_proximity_work_bytes(), 4-byte aligned) becomes
 *   the bitmap of the known edges' diamonds (bit f), keys[f] (n int64) = (m(d) << 31) | f >= 0 with m the order-preserving
 *   32-bit image of d's bits, or INT64_MAX for a dead cell or d > thresh.  Three launches (the first clears work).
 * lgu_proximity_select_sorted  the prefix and the greedy pass over keys SORTED ascending as signed 64-bit integers (by any
 *   sort), one workgroup; work as lgu_proximity_keys left it (it is modified).  The greedy pass takes 64 keys at a time, one per
 *   lane: the lowest live lane is accepted, every lane drops its own candidate if it lies in the accepted diamond, the diamond
 *   goes into the bitmap (in LDS up to 512 000 cells, else in work) for later windows; it ends at the first INT64_MAX.
 *   Sequential depth: accepted edges + windows visited.
 * lgu_proximity_prefix_len / _capacity / _work_bytes: host helpers, -1 for arguments outside the rules.
 * Alignment: dist, the index arrays and keys by element; work is read and or-ed as 32-bit words: 4-byte aligned, else
 * LGU_E_BADARG. */
#define LGU_PROXIMITY_SMALL_MAX 4096
long long lgu_proximity_prefix_len(int t, int t0, int rad, int stereo);
long long lgu_proximity_capacity(int t, int t0, int t1, int rad, int stereo, long long max_factors);
long long lgu_proximity_work_bytes(int t, int t0, int t1);
int lgu_proximity_select_small(const float* dist, const long long* known_ii, const long long* known_jj, int num_known, int t,
                               int t0, int t1, int rad, int nms, double thresh, long long max_factors, int stereo,
                               long long* e_ii, long long* e_jj, long long capacity, int* count, void* stream);
int lgu_proximity_keys(const float* dist, const long long* known_ii, const long long* known_jj, int num_known, int t, int t0,
                       int t1, int rad, int nms, double thresh, int stereo, long long* keys, void* work, void* stream);
int lgu_proximity_select_sorted(const long long* sorted_keys, void* work, int t, int t0, int t1, int rad, int nms,
                                long long max_factors, int stereo, long long* e_ii, long long* e_jj, long long capacity,
                                int* count, void* stream);

/* ---- Lie groups: the SO3 / SE3 operations of lgu_slam_amd.lie (csrc/liegroup.hip) ---------------------------------------
 * float32, contiguous tensors.  group = LGU_LIE_SO3: an element is q = (x, y, z, w), 4 floats, tangent phi (3);
 * LGU_LIE_SE3: (t, q), 7 floats, tangent (tau, phi) (6), translation first.  Quaternions are used as given (not
 * normalised, not sign-flipped).  R(q) X = X + w (2 v x X) + v x (2 v x X); G H = (t_G + R_G t_H, q_G q_H) with the
 * Hamilton product; matrix = [[R, t], [0, 1]] row-major (16 floats).  exp(tau, phi) = (V tau, [sin(th/2) phi / th,
 * cos(th/2)]) equals the matrix exponential of [[ [phi]x, tau ], [0, 0]]; log is its inverse with |phi| <= pi (q and -q
 * give the same result); both use series at small angles, are finite at every angle, and exp(0) / log(identity) are
 * exact.  retr(G, a) = exp(a) G with the bits of exp followed by mul.
 * Per element (inv, mul, retr, exp, log, matrix): n elements, one thread each, ONE launch on `stream`; n == 0 launches
 * nothing; n < 0, an unknown group or a null pointer: LGU_E_BADARG; matrix needs a 16-byte aligned out.
 * Broadcast (act, adj): `rows` operand rows, row r uses group element r / g_div of the COMPACT tensor G (ng elements; an
 * expanded copy is never read).  act: width 3 rows p -> R p + t, width 4 rows (X, Y, Z, W) -> (R XYZ + t W, W).  adj:
 * rows of the tangent size, a -> Adj(G) a, or Adj(G)^T a with transpose = 1; SE3: Adj = [[R, [t]x R], [0, R]], SO3:
 * Adj = R.  16-byte global accesses when the operand and out are 16-byte aligned, any 4-byte alignment otherwise.  out
 * must not overlap the inputs.  rows == 0 launches nothing; rows, ng < 0, g_div < 1, (rows - 1) / g_div >= ng, another
 * width / transpose: LGU_E_BADARG; more than INT_MAX workgroups: LGU_E_UNSUPPORTED. */
#define LGU_LIE_SO3 0
#define LGU_LIE_SE3 1
int lgu_lie_inv_f32(int group, const float* G, int n, float* out, void* stream);
int lgu_lie_mul_f32(int group, const float* G, const float* H, int n, float* out, void* stream);
int lgu_lie_retr_f32(int group, const float* G, const float* a, int n, float* out, void* stream);
int lgu_lie_exp_f32(int group, const float* a, int n, float* out, void* stream);
int lgu_lie_log_f32(int group, const float* G, int n, float* out, void* stream);
int lgu_lie_matrix_f32(int group, const float* G, int n, float* out, void* stream);
int lgu_lie_act_f32(int group, const float* G, long long ng, const float* p, int width, long long rows, long long g_div,
                    float* out, void* stream);
int lgu_lie_adj_f32(int group, const float* G, long long ng, const float* a, int transpose, long long rows,
                    long long g_div, float* out, void* stream);

/* ---- feature encoder: fused instance norm + ReLU + residual, and the frame normalisation (csrc/instnorm.hip) ------------
 * Reference droid_slam/modules/extractor.py: BasicEncoder(output_dim=128, norm_fn='instance') builds its 15 norm sites as
 * nn.InstanceNorm2d(planes) (:28-32, :131: biased variance, eps 1e-5, no affine terms, no running statistics).
 * A plane is one (n, c) slice of a contiguous NCHW tensor, hw elements; a, b, out hold `planes` of them.
 *   IN(x) = (x - mean) * rstd,  mean = sum(x) / hw,  rstd = 1 / sqrt(sum((x - mean)^2) / hw + eps)
 * with the statistics in fp32 from the values as stored, the centred sum taken after the mean is final, every sum a
 * tree of depth <= log2(hw) + 4 on the single-launch path (beyond it a thread first adds its ceil(hw / (1024 V)) vector
 * sums in sequence, V = 16 / sizeof element; csrc/instnorm.hip), all arithmetic in fp32 and ONE rounding to the tensor
 * type at the store (_h16: IEEE half).
 *   mode 0  out = relu(IN(a))                  extractor.py:49-50, :188-189   (b is not read, may be NULL)
 *   mode 1  out = relu(b + relu(IN(a)))        :50, :55 with downsample None  (b added as it is)
 *   mode 2  out = relu(IN(b) + relu(IN(a)))    :50-55 with the 1x1 downsample branch and its norm3
 *   mode 3  out = IN(a)                        a bare InstanceNorm2d          (b is not read, may be NULL)
 * relu keeps a NaN.  out may be exactly a or exactly b; any other overlap is the caller's error.  No atomics: the bits
 * of a plane depend on its own values, hw and eps only.
 * hw <= lgu_instnorm_resident_limit(sizeof element) (6144 vectors of 16 bytes: 49152 halves, 24576 floats): ONE launch,
 *   one workgroup per plane, the plane (both planes in mode 2) held in registers between the statistics and the store.
 *   Operands need the alignment of one element only; the bits do not depend on the address.
 * Otherwise: a statistics launch (one workgroup per plane) and an apply launch; the 16 * planes bytes between them come
 *   from the stream-ordered allocator on `stream` (hipMallocAsync / hipFreeAsync), without host synchronisation.  Under
 *   stream capture these become allocation and free nodes of the graph, which needs a runtime that supports them; the
 *   single-launch path allocates nothing and captures as one kernel node.
 * planes == 0 launches nothing; hw < 1, planes < 0, an unknown mode, eps < 0, a null or misaligned operand:
 * LGU_E_BADARG; planes > INT_MAX or more than INT_MAX workgroups: LGU_E_UNSUPPORTED.
 *
 * lgu_image_normalize_u8  the frame upload of droid_slam/motion_filter.py:56-57 (image[:, [2,1,0]] / 255.0, sub_(MEAN),
 *   div_(STDV)): img (n,3,hw) uint8 BGR, out (n,3,hw) float32 RGB, out[n,c,i] = (float(img[n,2-c,i]) * r255 - mean[c])
 *   / std[c] in that order, r255 = (float)(1.0 / 255.0): on the device PyTorch divides a tensor by a Python number by
 *   multiplying with the reciprocal, which is what the reference's `/ 255.0` therefore computes (the correctly rounded
 *   quotient differs for 126 of the 256 byte values); the subtraction and the division by std are correctly rounded
 *   fp32 ops.  Bit-identical to those four PyTorch ops on the device.  mean, std: 3 host floats each.  n, hw >= 0 (0
 *   launches nothing), else LGU_E_BADARG. */
int lgu_instnorm_relu_f32(const float* a, const float* b, float* out, long planes, long hw, float eps, int mode,
                          void* stream);
int lgu_instnorm_relu_h16(const void* a, const void* b, void* out, long planes, long hw, float eps, int mode,
                          void* stream);
long lgu_instnorm_resident_limit(int elem_bytes); /* largest hw served by the single-launch path; 0 for another size */
int lgu_image_normalize_u8(const unsigned char* img, float* out, long n, long hw, const float mean[3], const float std[3],
                           void* stream);

/* ---- motion (flow) encoder: the 7x7 first layer with its ReLU, under float16 autocast (csrc/flowenc.hip) -----------------
 * Reference droid_slam/droid_net.py:82-84: flow_encoder = Conv2d(4, 128, 7, padding=3), ReLU(inplace=True), ... evaluated
 * under the float16 autocast of the update operator.  x (N,4,H,W) float32 planar, what lgu_motion_features_f32 writes;
 * out (N,128,H,W) IEEE half, NCHW contiguous, fully written and nothing outside it.  Rounding points:
 *   x_h = half(x), w_h = half(weight), b_h = half(bias)     round to nearest even (x_h in the kernel, the others in the pack)
 *   s   = b_h + sum over c, ky, kx of x_h * w_h             exact half x half products, fp32 accumulation, zero padding
 *   y   = relu(half(s))                                     ONE rounding; relu keeps a NaN
 * A NaN or infinite input reaches exactly the output pixels whose 7x7 window covers it.  No atomics, no workspace: the
 * bits of an image depend on that image, H and W only, not on N or on its position in the batch.
 * wpack: LGU_FLOW_CONV7_WPACK_HALVES halves laid out [7 window rows ky][8 channel tiles ct][64 lanes l][8 halves j], the B
 *   operand of v_mfma_f32_16x16x32_f16 as each lane loads it: element j of lane l is w_h[16 ct + (l & 15)][c][ky][kx] with
 *   k = 8 (l >> 4) + j, kx = k / 4, c = k % 4, and zero where kx == 7 (the padding slot that makes a window row one K step
 *   of 32).  16-byte aligned, otherwise LGU_E_UNSUPPORTED.  bias: 128 halves b_h.
 * x, bias and out are served at the alignment of their element: out is stored 8 bytes at a time where W % 4 == 0 and out
 *   is 8-byte aligned, by element otherwise, with the same arithmetic and the same bits.
 * Every N >= 0, H >= 1, W >= 1 is served; N == 0 launches nothing.  N < 0, H < 1, W < 1, a null operand or one below its
 * element's alignment: LGU_E_BADARG; more than INT_MAX workgroups (N * ceil(W / 64) * ceil(H / 8)): LGU_E_UNSUPPORTED.
 * The operands travel in one parameter block passed by value. */
#define LGU_FLOW_CONV7_WPACK_HALVES 28672
typedef struct {
  const float* x; const void* wpack; const void* bias; void* out;   /* bias: 128 halves */
  int N, H, W;
} lgu_flow_conv7_args;
int lgu_flow_conv7_relu_h16(lgu_flow_conv7_args args, void* stream);

/* ---- update operator: Conv2d(128, 64 | 128, 3, padding=1) + bias (+ ReLU) under float16 autocast (csrc/conv3.hip) ---------
 * Reference droid_slam/droid_net.py: corr_encoder[2], flow_encoder[2], delta[0], weight[0], GraphAgg.conv1 / conv2.
 * x (N,128,H,W) NCHW contiguous, float32, or IEEE half with LGU_CONV3_X_HALF; out (N,Cout,H,W) IEEE half, NCHW contiguous,
 * fully written and nothing outside it; Cout 64 or 128.  Rounding points:
 *   x_h = half(x), w_h = half(weight), b_h = half(bias)     round to nearest even (x_h in the kernel, and a half x is used
 *                                                           as it is; the others in the pack)
 *   s   = b_h + sum over c, ky, kx of x_h[c][y+ky-1][x+kx-1] * w_h[co][c][ky][kx]
 *                                                           exact half x half products, fp32 accumulation, zero padding
 *   y   = act(half(s))                                      ONE rounding; act = relu with LGU_CONV3_RELU (a NaN is kept),
 *                                                           the identity otherwise
 * The accumulator starts at b_h and takes its 36 K steps in a fixed order (ky, kx, then channel blocks of 32), whatever
 * the tile: the bits of an image depend on that image, H and W only, not on N or on its position in the batch.  A NaN or
 * infinite input reaches exactly its 3x3 neighbourhood.  No atomics, no workspace, no host synchronisation.
 * wpack: LGU_CONV3_WPACK_HALVES_<Cout> halves laid out [9 taps t = 3 ky + kx][4 channel blocks kc][Cout/16 channel tiles
 *   ct][64 lanes l][8 halves j], the B operand of v_mfma_f32_16x16x32_f16 as each lane loads it: element j of lane l is
 *   w_h[16 ct + (l & 15)][32 kc + 8 (l >> 4) + j][t / 3][t % 3].  Every slot holds a weight.  16-byte aligned, otherwise
 *   LGU_E_UNSUPPORTED.  bias: Cout halves b_h.
 * x, bias and out are served at the alignment of their element with the same bits: out is stored 16 bytes at a time
 *   where W % 8 == 0 and out is 16-byte aligned, by element otherwise.
 * Every N >= 0, H >= 1, W >= 1 is served; N == 0 launches nothing.  N < 0, H < 1, W < 1, an unknown flag, a null operand
 * or one below its element's alignment: LGU_E_BADARG; Cout outside {64, 128}, or more than INT_MAX workgroups (N * the
 * smaller of ceil(W / 64) * ceil(H / 2) and ceil(W / 32) * ceil(H / 4) by padded area): LGU_E_UNSUPPORTED, nothing written.
 * The operands travel in one parameter block passed by value. */
#define LGU_CONV3_WPACK_HALVES_128 147456
#define LGU_CONV3_WPACK_HALVES_64 73728
#define LGU_CONV3_X_HALF 1   /* flags: x holds IEEE half */
#define LGU_CONV3_RELU 2     /* flags: act = relu */
typedef struct {
  const void* x; const void* wpack; const void* bias; void* out;   /* bias: Cout halves */
  int N, H, W, Cout, flags;
} lgu_conv3_args;
int lgu_conv3x3_c128_h16(lgu_conv3_args args, void* stream);

/* ---- fan-out: G = 2 or 3 convolutions Conv2d(128, 128, 3, padding=1) + bias (+ ReLU) of ONE input in one launch
 * (csrc/conv3.hip).  Reference droid_slam/droid_net.py: delta[0], weight[0] and GraphAgg.conv1 all read the GRU's result.
 * x (N,128,H,W) as for lgu_conv3x3_c128_h16; wpack[g], bias[g], out[g] (g < G) one Cout-128 pack, its 128 bias halves and
 * an (N,128,H,W) half output of its own, fully written and nothing outside it; entries g >= G are not read.
 * out[g] has exactly the bits lgu_conv3x3_c128_h16 gives for x, wpack[g], bias[g] and the same flags: the tile of x is
 * staged once, every group takes the same 36 K steps from its own bias, and no sum depends on which other channels share
 * the launch.  A NaN of x reaches its 3x3 neighbourhood in every group, a NaN of bias[g] group g only.  No atomics, no
 * workspace, no host synchronisation.  The outputs must not overlap x or one another.
 * x, bias[g] and out[g] are served at the alignment of their element with the same bits: out is stored 8 bytes at a time
 *   where W % 4 == 0 and every out[g] is 8-byte aligned, by element otherwise.
 * N == 0: LGU_OK, nothing launched.  N < 0, H < 1, W < 1, an unknown flag, a null operand among the G groups or one below
 * its element's alignment: LGU_E_BADARG; G outside {2, 3}, a wpack[g] that is not 16-byte aligned or more than INT_MAX
 * workgroups (N * ceil(W / 32) * ceil(H / 4)): LGU_E_UNSUPPORTED, nothing written.  All refusals come before any launch.
 * The operands travel in one parameter block passed by value. */
typedef struct {
  const void* x; const void* wpack[3]; const void* bias[3]; void* out[3];   /* bias[g]: 128 halves */
  int N, H, W, G, flags;                                                  /* flags: LGU_CONV3_X_HALF, LGU_CONV3_RELU */
} lgu_conv3_fanout_args;
int lgu_conv3x3_fanout_c128_h16(lgu_conv3_fanout_args args, void* stream);

/* ---- update operator: the narrow heads Conv2d(128, 1 | 2, 3, padding=1) + bias (+ sigmoid | softplus) under float16 autocast
 * (csrc/heads.hip).  Reference droid_slam/droid_net.py: delta[2], weight[2] + Sigmoid, GraphAgg.eta + GradientClip + Softplus.
 * x (N,128,H,W) NCHW contiguous, float32, or IEEE half with LGU_HEAD_X_HALF; out (N,Cout,H,W) NCHW contiguous, IEEE half, or
 * float32 with LGU_HEAD_SOFTPLUS; fully written and nothing outside it; Cout 1 or 2.  Rounding points:
 *   x_h = half(x), w_h = half(weight), b_h = half(bias)     round to nearest even (x_h in the kernel, and a half x is used
 *                                                           as it is; the others in the pack)
 *   p_t = sum over c of x_h[c][y+ky-1][x+kx-1] * w_h[co][c][ky][kx]      t = 3 ky + kx; exact half x half products, fp32
 *                                                           accumulation from zero in four steps of 32 channels, zero padding
 *   s   = b_h + p_0 + p_1 + ... + p_8                        fp32, left to right
 *   h   = half(s)                                           ONE rounding
 *   y   = h                                                 no activation flag: half out
 *   y   = half(1 / (1 + exp(-h)))                           LGU_HEAD_SIGMOID: evaluated in fp32, half out
 *   y   = h > 20 ? h : log1p(exp(h))                        LGU_HEAD_SOFTPLUS (beta 1, threshold 20): fp32, float32 out
 * All three keep a NaN.  The order is the same whatever the tile: the bits of an image depend on that image, H and W only,
 * not on N or on its position in the batch.  A NaN or infinite input reaches exactly its 3x3 neighbourhood.  No atomics, no
 * workspace, no host synchronisation.
 * wpack: LGU_HEAD_WPACK_HALVES_<Cout> halves laid out [4 channel blocks kc][NT column tiles nt][64 lanes l][8 halves j] with
 *   NT = 1 (Cout 1) or 2 (Cout 2), the B operand of v_mfma_f32_16x16x32_f16 as each lane loads it: with the column
 *   q = 16 nt + (l & 15), element j of lane l is w_h[q % Cout][32 kc + 8 (l >> 4) + j][t / 3][t % 3] for the tap t = q / Cout
 *   where q < 9 Cout, and zero where q >= 9 Cout (7 of 16 columns at Cout 1, 14 of 32 at Cout 2).  16-byte aligned,
 *   otherwise LGU_E_UNSUPPORTED.  bias: Cout halves b_h.
 * x, bias and out are read and written by element: they are served at the alignment of their element with the same bits.
 * N == 0, H == 0 or W == 0: LGU_OK, nothing launched.  N, H or W < 0, an unknown flag, a null operand or one below its
 * element's alignment: LGU_E_BADARG; Cout outside {1, 2}, both activation flags, a wpack that is not 16-byte aligned or more
 * than INT_MAX workgroups (N * ceil(W / 32) * ceil(H / 4)): LGU_E_UNSUPPORTED, nothing written.
 * The operands travel in one parameter block passed by value. */
#define LGU_HEAD_X_HALF 1     /* flags: x holds IEEE half */
#define LGU_HEAD_SIGMOID 2    /* flags: act = sigmoid, half out */
#define LGU_HEAD_SOFTPLUS 4   /* flags: act = softplus, float32 out */
#define LGU_HEAD_WPACK_HALVES_1 2048
#define LGU_HEAD_WPACK_HALVES_2 4096
typedef struct {
  const void* x; const void* wpack; const void* bias; void* out;   /* bias: Cout halves */
  int N, H, W, Cout, flags;
} lgu_head_args;
int lgu_head3x3_c128_h16(lgu_head_args args, void* stream);

/* ---- the pair of two-channel heads in one launch, edge-major (csrc/heads.hip).  Reference droid_slam/droid_net.py:
 * delta[2] and weight[2] + Sigmoid, then view / permute / [..., :2] / contiguous; droid_slam/factor_graph.py:
 * coords1 + float32(delta) and float32(weight) (lines 224-225 and 290-291).
 * Head 0 reads x[0] with wpack[0], bias[0] and has no activation; head 1 reads x[1] with wpack[1], bias[1] and has the
 * sigmoid.  x[k] (N,128,H,W) as for lgu_head3x3_c128_h16 (both float32, or both half with LGU_HEAD_X_HALF), the packs those
 * of Cout 2.  h_k is what lgu_head3x3_c128_h16 gives for head k, bit for bit (same staging, K steps and nine-tap sum).
 *   without LGU_HEAD_PAIR_F32   out[k] (N,H,W,2) IEEE half: out[k][n][y][x][co] = h_k[n][co][y][x]; coords must be null
 *   with LGU_HEAD_PAIR_F32      out[k] (N,H,W,2) float32, coords (N,H,W,2) float32, not null:
 *                               out[0] = coords + float(h_0)   one fp32 addition; coords is read at that element only
 *                               out[1] = float(h_1)
 * Outputs are fully written and nothing outside them; a pixel's two channels are one 4-byte (half) or 8-byte (float32)
 * store, and coords is read 8 bytes at a time.  No atomics, no workspace, no host synchronisation.
 * x[k] and bias[k] are served at the alignment of their element with the same bits.
 * N == 0, H == 0 or W == 0: LGU_OK, nothing launched.  N, H or W < 0, an unknown flag, LGU_HEAD_PAIR_F32 without coords or
 * coords without it, a null operand or one below its element's alignment: LGU_E_BADARG; a wpack[k] that is not 16-byte
 * aligned, an out[k] or coords that is not aligned to a whole pixel (4 bytes half, 8 bytes float32) or more than INT_MAX
 * workgroups (2 * N * ceil(W / 32) * ceil(H / 4)): LGU_E_UNSUPPORTED, nothing written.  All refusals come before any launch.
 * The operands travel in one parameter block passed by value. */
#define LGU_HEAD_PAIR_F32 8   /* flags of lgu_head3x3_pair_c128_h16: float32 outputs, out[0] = coords + delta */
typedef struct {
  const void* x[2]; const void* wpack[2]; const void* bias[2]; void* out[2];   /* bias[k]: 2 halves */
  const void* coords;                                                          /* null without LGU_HEAD_PAIR_F32 */
  int N, H, W, flags;
} lgu_head_pair_args;
int lgu_head3x3_pair_c128_h16(lgu_head_pair_args args, void* stream);

/* ---- KAN-bias GRU: Conv2d(448, 128, 3, padding=1) x 3 with the gates and the blend, float16 autocast (csrc/gruconv.hip) ------
 * Reference droid_slam/modules/gru_kanBias.py: convz, convr, convq of KAN_bias_GRU(128, 320).  All tensors IEEE half.
 * Input: nseg (1..4) NCHW-contiguous tensors seg[i] (N,seg_ch[i],H,W), read as their concatenation along the channels
 * without that tensor existing; every seg_ch[i] a multiple of 32, their sum 448.  The split does not change a bit: one
 * segment of 448, [128,320] and [128,128,128,64] give the same output.  Rounding points:
 *   w_h = half(weight), b_h = half(bias)                    round to nearest even, in the pack
 *   s   = b_h + sum over c, ky, kx of x[c][y+ky-1][x+kx-1] * w_h[co][c][ky][kx]
 *                                                           exact half x half products, fp32 accumulation, zero padding
 *   c   = half(s)                                           ONE rounding, then by mode (r(v) = half(v) below):
 *   LGU_GRUCONV_PLAIN  Cout 128 or 256: out0 (N,Cout,H,W) = c.
 *   LGU_GRUCONV_ZR     Cout 256, the pack's outputs 0..127 convz, 128..255 convr; k0 = kz, k1 = kr (N,128), net (N,128,H,W):
 *                      out0 = z = r(sigmoid(r(c_z + kz))), out1 = rnet = r(r(sigmoid(r(c_r + kr))) * net), both
 *                      (N,128,H,W): the arithmetic of lgu_kangru_gates_h16 on c.
 *   LGU_GRUCONV_Q      Cout 128 (segment 0 is rnet); k0 = kq (N,128), z and net (N,128,H,W):
 *                      out0 = r(r(r(1 - z) * net) + r(z * r(tanh(r(c + kq))))): the arithmetic of lgu_kangru_blend_h16 on c.
 * The accumulator starts at b_h and takes its 126 K steps in ONE order, whatever the mode, the tile, N or the segment split:
 *   step = (c64 * 9 + t) * 2 + kc   c64 < 7: chunk of 64 channels; t = 3 ky + kx < 9: tap; kc < 2: block of 32 channels
 * covering channels 64 c64 + 32 kc .. + 32 of tap t.  The bits of an image depend on that image, H and W only, not on N
 * or on its position in the batch.  A NaN or infinite input reaches exactly its 3x3 neighbourhood.  No atomics, no
 * workspace, no host synchronisation.
 * wpack: LGU_GRUCONV_WPACK_HALVES_<Cout> halves laid out [126 steps][Cout/16 channel tiles ct][64 lanes l][8 halves j], the
 *   B operand of v_mfma_f32_16x16x32_f16 as each lane loads it: element j of lane l in step (c64, t, kc) is
 *   w_h[16 ct + (l & 15)][64 c64 + 32 kc + 8 (l >> 4) + j][t / 3][t % 3].  Every slot holds a weight.  16-byte aligned,
 *   otherwise LGU_E_UNSUPPORTED.  bias: Cout halves b_h.
 * Outputs are fully written and nothing outside them.  They must not overlap any input (other workgroups read the
 * segments' pixels as halo): rnet is a tensor of its own, never segment 0 of the same call.
 * Alignment: segments, bias, k0, k1, net, z and the outputs at element alignment (stores and the reads of net and z go
 * 16 bytes at a time when W % 8 == 0 and the mode's outputs, net and z are 16-byte aligned, by element otherwise: same
 * bits).  Refusals, all before any launch, nothing written.  LGU_E_BADARG: N < 0, H < 1, W < 1, an unknown mode, flags
 * other than 0, nseg outside 1..4, a null pointer among the mode's operands or one below its element's alignment.
 * LGU_E_UNSUPPORTED: a seg_ch[i] that is not a positive multiple of 32, a sum other than 448, a Cout that does not fit the
 * mode, a wpack that is not 16-byte aligned, H * W above 2^30, more than INT_MAX workgroups.  N == 0: LGU_OK without a launch.
 * The operands travel in one parameter block passed by value. */
#define LGU_GRUCONV_CIN 448
#define LGU_GRUCONV_STEPS 126
#define LGU_GRUCONV_MAX_SEGMENTS 4
#define LGU_GRUCONV_WPACK_HALVES_128 516096
#define LGU_GRUCONV_WPACK_HALVES_256 1032192
#define LGU_GRUCONV_PLAIN 0  /* mode */
#define LGU_GRUCONV_ZR 1     /* mode */
#define LGU_GRUCONV_Q 2      /* mode */
typedef struct {
  const void* seg[4];                              /* seg[i]: (N,seg_ch[i],H,W) half, i < nseg */
  const void* wpack; const void* bias;             /* bias: Cout halves */
  const void* k0; const void* k1;                  /* ZR: kz, kr; Q: kq, unused */
  const void* net; const void* z;                  /* ZR: net; Q: net, z */
  void* out0; void* out1;                          /* PLAIN: out; ZR: z, rnet; Q: the new net */
  int seg_ch[4]; int nseg;
  int N, H, W, Cout, mode, flags;                  /* flags: 0 */
} lgu_gruconv_args;
int lgu_gruconv3x3_c448_h16(lgu_gruconv_args args, void* stream);

/* ---- GraphAgg's upsampling mask, Conv2d(128, 576, 1) + bias under float16 autocast, alone and fused with the convex
 * upsampling of the disparity (csrc/upmask.hip).  Reference droid_slam/droid_net.py:50-51,67 and depth_video.py:124-128.
 * Rounding points of both entries:
 *   x_h = half(x), w_h = half(weight), b_h = half(bias)     round to nearest even (x_h in the kernel, and a half x is used
 *                                                           as it is; the others in the pack)
 *   p   = sum over c of x_h[c] * w_h[co][c]                 exact half x half products, fp32 accumulation from zero in four
 *                                                           steps of 32 channels (kc = 0..3)
 *   h   = half(b_h[co] + p)                                 one fp32 addition, ONE rounding to half; NaN is kept
 * The order depends on nothing but the pixel's own 128 inputs: not on N or U, the position in the batch or the launch
 * geometry.  Both entries run the same device function for h, so the fused entry sees the bits the plain one stores.
 * No atomics, no workspace, no allocation, no host synchronisation; launched on `stream`.
 *
 * lgu_upmask1x1_c128_h16  the layer.  x (N,128,H,W) NCHW contiguous, float32, or IEEE half with LGU_UPMASK_X_HALF; out
 *   (N,576,H,W) NCHW contiguous IEEE half, fully written and nothing outside it.  A NaN or infinite input reaches exactly
 *   its own pixel's 576 outputs.
 * lgu_upmask_upsample_f32  the layer, then DepthVideo.upsample, in one launch, in place: x (U,128,ht,wd) as above, disps
 *   (N,ht,wd) float, ix (U) int64, disps_up (N,8ht,8wd) float.  For u < U with 0 <= ix[u] < N, disps_up[ix[u]] =
 *   cvx_upsample of disps[ix[u]] with the mask h of x[u], by exactly the per-output rule of lgu_cvx_upsample_f32 above on
 *   a half mask: channel k*64 + a*8 + b weighs the neighbour (y+ky-1, x+kx-1) for the output pixel (8y+a, 8x+b); m = max_k
 *   h_k; e_k = expf(h_k - m); s = sum e_k (ascending k); w_k = e_k / s; with LGU_UPS_HALF_WEIGHTS w_k is rounded to half
 *   and back; out = sum w_k * d_k, each product rounded to fp32, added in ascending k; d_k = 0 outside the frame.  Only
 *   those rows of disps_up are written; an ix[u] outside [0, N) writes nothing; with duplicates in ix the result of those
 *   rows is unspecified among the candidates (the reference passes unique indices).  A NaN at one pixel of x reaches exactly
 *   that pixel's 8x8 outputs.  flags: LGU_UPMASK_X_HALF | LGU_UPS_HALF_WEIGHTS.
 * wpack: LGU_UPMASK_WPACK_HALVES halves laid out [36 row tiles mt][4 channel blocks kc][64 lanes l][8 halves j], the A
 *   operand of v_mfma_f32_16x16x32_f16 as each lane loads it: element j of lane l is w_h[16 mt + (l & 15)][32 kc + 8 (l >> 4)
 *   + j].  Every slot holds a weight.  16-byte aligned, otherwise LGU_E_UNSUPPORTED.  bias: 576 halves b_h.
 * x, bias, out, disps and ix are accessed by element and served at the alignment of their element with the same bits;
 * disps_up is stored 16 bytes at a time and must be 16-byte aligned, otherwise LGU_E_UNSUPPORTED.
 * Sizes: a negative size or an unknown flag: LGU_E_BADARG; for the fused entry ht * wd > INT_MAX / 576: LGU_E_BADARG (the
 * rule of the upsampling entries); an empty x (N, H, W, U, ht or wd == 0) or, fused, N == 0: LGU_OK, nothing launched; a
 * null operand or one below its element's alignment: LGU_E_BADARG; more than INT_MAX - 16 pixels in x: LGU_E_UNSUPPORTED.
 * Every refusal comes before any launch and writes nothing.  The operands travel in one parameter block passed by value. */
#define LGU_UPMASK_X_HALF 1   /* flags: x holds IEEE half */
#define LGU_UPMASK_COUT 576
#define LGU_UPMASK_WPACK_HALVES 73728
typedef struct {
  const void* x; const void* wpack; const void* bias; void* out;   /* bias: 576 halves */
  int N, H, W, flags;
} lgu_upmask_args;
typedef struct {
  const void* x; const void* wpack; const void* bias;              /* x: (U,128,ht,wd) */
  const float* disps; const long long* ix; float* disps_up;
  int U, N, ht, wd, flags;
} lgu_upmask_ups_args;
int lgu_upmask1x1_c128_h16(lgu_upmask_args args, void* stream);
int lgu_upmask_upsample_f32(lgu_upmask_ups_args args, void* stream);

/* ---- update operator: Conv2d(Cin, 128, 1) + bias (+ ReLU) under float16 autocast, 1 <= Cin <= 224 (csrc/conv1.hip).
 * Reference droid_slam/droid_net.py: corr_encoder[0] = Conv2d(196, 128, 1) + ReLU, the consumer of the correlation lookup.
 * x (N,Cin,H,W) NCHW contiguous, float32, or IEEE half with LGU_CONV1_X_HALF; out (N,128,H,W) NCHW contiguous IEEE half,
 * fully written and nothing outside it.  Rounding points:
 *   x_h = half(x), w_h = half(weight), b_h = half(bias)     round to nearest even (x_h in the kernel, and a half x is used
 *                                                           as it is; the others in the pack)
 *   p   = sum over c < Cin of x_h[c] * w_h[co][c]           exact half x half products, fp32 accumulation from zero in seven
 *                                                           steps of 32 channels (kc = 0..6, ascending; channels >= Cin
 *                                                           contribute exact zeros)
 *   h   = half(b_h[co] + p)                                 one fp32 addition, ONE rounding to half
 *   y   = h, or with LGU_CONV1_RELU: h < 0 ? 0 : h          a compare and select: NaN is kept
 * The bits of a pixel depend on that pixel's Cin inputs only: not on N, the position in the batch, the pixel's group or the
 * launch geometry.  A NaN or infinite input reaches exactly its own pixel's 128 outputs.  A channel >= Cin is never read:
 * its staged value is written as zero.  No atomics, no workspace, no allocation, no host synchronisation.
 * wpack: LGU_CONV1_WPACK_HALVES halves laid out [7 channel blocks kc][8 channel tiles ct][64 lanes l][8 halves j], the B
 *   operand of v_mfma_f32_16x16x32_f16 as each lane loads it: element j of lane l is w_h[16 ct + (l & 15)][c] with
 *   c = 32 kc + 8 (l >> 4) + j where c < Cin, and zero where c >= Cin.  16-byte aligned, otherwise LGU_E_UNSUPPORTED.
 *   bias: 128 halves b_h.
 * x, bias and out are served at the alignment of their element with the same bits (out is stored 8 bytes at a time when
 * H * W % 4 == 0 and it is 8-byte aligned, by element otherwise).
 * N, H or W < 0 or an unknown flag: LGU_E_BADARG; N, H or W == 0: LGU_OK, nothing launched; a null operand or one below
 * its element's alignment: LGU_E_BADARG; Cin outside 1..LGU_CONV1_MAX_CIN, a wpack that is not 16-byte aligned or more than
 * INT_MAX - 32 pixels: LGU_E_UNSUPPORTED.  Every refusal comes before any launch and writes nothing.  The operands travel
 * in one parameter block passed by value. */
#define LGU_CONV1_COUT 128
#define LGU_CONV1_MAX_CIN 224
#define LGU_CONV1_WPACK_HALVES 28672
#define LGU_CONV1_X_HALF 1   /* flags: x holds IEEE half */
#define LGU_CONV1_RELU 2     /* flags: act = relu */
typedef struct {
  const void* x; const void* wpack; const void* bias; void* out;   /* bias: 128 halves */
  int N, Cin, H, W, flags;
} lgu_conv1_args;
int lgu_conv1x1_o128_h16(lgu_conv1_args args, void* stream);

/* ---- the encoders' residual stages: Conv2d(Cin, Cout, 3, stride=s, padding=1) + bias with the norm-free tail of a
 * ResidualBlock as its epilogue and, with stride 2, the block's Conv2d(Cin, Cout, 1, stride=2) downsample branch in the same
 * launch, under float16 autocast (csrc/encconv.hip).  Reference droid_slam/modules/extractor.py: layer1..3 of BasicEncoder.
 * (Cin, Cout, s) is one of (32,32,1), (32,64,2), (64,64,1), (64,128,2), (128,128,1); anything else: LGU_E_UNSUPPORTED.
 * x (N,Cin,H,W) NCHW contiguous IEEE half; out, res and r (N,Cout,Ho,Wo) NCHW contiguous IEEE half with Ho = ceil(H / s),
 * Wo = ceil(W / s) (PyTorch's rule for k = 3, p = 1); out and r are fully written and nothing outside them, and overlap neither
 * x nor res nor one another.  Rounding points:
 *   w_h = half(weight), b_h = half(bias)                    round to nearest even, in the pack; x is half and used as it is
 *   s   = b_h + sum over ky, kx, c of x[c][s y+ky-1][s x+kx-1] * w_h[co][c][ky][kx]
 *                                                           exact half x half products, fp32 accumulation, zero padding:
 *                                                           a row or column outside the image, row H and column W of an
 *                                                           odd size included, contributes exact zeros
 *   y0  = half(s)                                           ONE rounding
 *   y   = y0                                                flags 0 (what an instance norm of the feature encoder reads)
 *       = y0 < 0 ? 0 : y0                                   LGU_ENCCONV_RELU: a compare and select, NaN is kept
 *       = relu(half(res + relu(y0)))                        LGU_ENCCONV_RESIDUAL: the add of two halves in fp32, ONE rounding,
 *                                                           PyTorch's bits of relu(x + relu(conv)) on half tensors
 *   r   = half(b'_h + sum over c of x[c][2 y][2 x] * w'_h[co][c])    the downsample branch (dpack, dbias, r all given; s = 2
 *                                                           only): the centre tap of the staged window, accumulators of its
 *                                                           own from b'_h over the channel blocks in ascending order, the
 *                                                           identity epilogue always; r does not depend on wpack or flags
 * The accumulator starts at b_h and takes its 9 Cin / 32 K steps in a fixed order, tap-major (ky, kx), then blocks of 32
 * channels, whatever the tile and the split of the output channels over workgroups: the bits of an image depend on that
 * image, H and W only, not on N or on its position in the batch, and out has the same bits with or without the branch.  A
 * NaN or infinite x reaches exactly the outputs whose window holds it, and its one pixel of r where its row and column are
 * even; a NaN of res reaches one element.  No atomics, no workspace, no host synchronisation.
 * wpack: 9 * Cin * Cout halves laid out [9 taps t = 3 ky + kx][Cin/32 channel blocks kc][Cout/16 channel tiles ct][64 lanes l]
 *   [8 halves j], the B operand of v_mfma_f32_16x16x32_f16 as each lane loads it: element j of lane l is
 *   w_h[16 ct + (l & 15)][32 kc + 8 (l >> 4) + j][t / 3][t % 3].  dpack: Cin * Cout halves [Cin/32 kc][Cout/16 ct][64 l][8 j],
 *   element j of lane l is w'_h[16 ct + (l & 15)][32 kc + 8 (l >> 4) + j].  Every slot of either holds a weight.  16-byte
 *   aligned, otherwise LGU_E_UNSUPPORTED.  bias, dbias: Cout halves.
 * x, res, bias, dbias, out and r are served at the alignment of their element with the same bits: res is loaded and out and
 *   r are stored 16 bytes at a time where Wo % 8 == 0 and the pointer is 16-byte aligned, by element otherwise.
 * Every N >= 0, H >= 1, W >= 1 is served; N == 0: LGU_OK, nothing launched.  N < 0, H < 1, W < 1, an unknown flag, both flags,
 * a null x, wpack, bias or out, res without LGU_ENCCONV_RESIDUAL or the flag without res, an incomplete (dpack, dbias, r), the
 * branch with s != 2, or an operand below its element's alignment: LGU_E_BADARG; another (Cin, Cout, s), a pack that is not
 * 16-byte aligned or more than INT_MAX workgroups (at most N * ceil(Wo / 32) * ceil(Ho / 2) * Cout / 32): LGU_E_UNSUPPORTED.  Every refusal comes before any launch and writes
 * nothing.  The operands travel in one parameter block passed by value. */
#define LGU_ENCCONV_RELU 1       /* flags: y = relu(y0) */
#define LGU_ENCCONV_RESIDUAL 2   /* flags: y = relu(half(res + relu(y0))) */
typedef struct {
  const void* x; const void* wpack; const void* bias; const void* res; void* out;   /* bias: Cout halves */
  const void* dpack; const void* dbias; void* r;                                    /* all three, or all null */
  int N, H, W, Cin, Cout, stride, flags;
} lgu_encconv_args;
int lgu_encconv3x3_h16(lgu_encconv_args args, void* stream);

/* ---- the encoders' stem: Conv2d(3, 32, 7, stride=2, padding=3) + bias with an optional ReLU, one launch, under float16
 * autocast (csrc/encends.hip).  Reference droid_slam/modules/extractor.py: conv1 of BasicEncoder (+ relu1 without a norm).
 * x (N,3,H,W) NCHW contiguous float32, or IEEE half with LGU_ENCSTEM_X_HALF; out (N,32,Ho,Wo) NCHW contiguous IEEE half with
 * Ho = ceil(H / 2), Wo = ceil(W / 2) (PyTorch's rule for k = 7, s = 2, p = 3), fully written and nothing outside it; it does
 * not overlap x.  Rounding points:
 *   x_h = half(x)                                           round to nearest even, in the kernel; a half x is used as it is
 *   w_h = half(weight), b_h = half(bias)                    in the pack
 *   s   = b_h + sum over ky, kx, c of x_h[c][2 y+ky-3][2 x+kx-3] * w_h[co][c][ky][kx]
 *                                                           exact half x half products, fp32 accumulation that starts at b_h
 *                                                           and takes the seven window rows in ascending ky; zero padding: a
 *                                                           row or column outside the image, the one just past an odd size
 *                                                           included, contributes exact zeros
 *   y0  = half(s)                                           ONE rounding
 *   y   = y0                                                flags without LGU_ENCSTEM_RELU (what an instance norm reads)
 *       = y0 < 0 ? 0 : y0                                   LGU_ENCSTEM_RELU: a compare and select, NaN is kept
 * The bits of an image depend on that image, H and W only, not on N, its position in the batch or the launch geometry.  A
 * NaN or infinite x reaches exactly the outputs whose 7x7 window holds it.  No atomics, no workspace, no host
 * synchronisation.
 * wpack: LGU_ENCSTEM_WPACK_HALVES = 7 * 2 * 64 * 8 halves laid out [7 window rows ky][2 channel tiles ct][64 lanes l][8 halves
 *   j], the B operand of v_mfma_f32_16x16x32_f16 as each lane loads it: a K step is one window row of 8 x-slots x 4
 *   channels, and element j of lane l is w_h[16 ct + (l & 15)][j & 3][ky][2 (l >> 4) + (j >> 2)] where the channel j & 3 is
 *   below 3 and the x-slot 2 (l >> 4) + (j >> 2) below 7, and ZERO in every other slot (the 4th channel and the 8th x-slot
 *   are padding of the K dimension; the kernel zeroes them in its A operand as well).  16-byte aligned, otherwise
 *   LGU_E_UNSUPPORTED.  bias: 32 halves.
 * x, bias and out are served at the alignment of their element with the same bits: out is stored 8 bytes at a time where
 *   Wo % 4 == 0 and the pointer is 8-byte aligned, by element otherwise.
 * Every N >= 0, H >= 1, W >= 1 is served; N == 0: LGU_OK, nothing launched.  N < 0, H < 1, W < 1, an unknown flag, a null
 * operand or one below its element's alignment: LGU_E_BADARG; Cin != 3 or Cout != 32, a pack that is not 16-byte aligned or
 * more than INT_MAX workgroups (N * ceil(Wo / 32) * ceil(Ho / 4)): LGU_E_UNSUPPORTED.  Every refusal comes before any launch
 * and writes nothing.  The operands travel in one parameter block passed by value. */
#define LGU_ENCSTEM_WPACK_HALVES 7168
#define LGU_ENCSTEM_X_HALF 1     /* flags: x holds IEEE half */
#define LGU_ENCSTEM_RELU 2       /* flags: y = relu(y0) */
typedef struct {
  const void* x; const void* wpack; const void* bias; void* out;   /* bias: 32 halves */
  int N, H, W, Cin, Cout, flags;
} lgu_encstem_args;
int lgu_encstem7x7_h16(lgu_encstem_args args, void* stream);

/* ---- the encoders' output layer: Conv2d(128, Cout, 1) + bias, Cout 128 (the feature encoder) or 256 (the context encoder),
 * one launch, under float16 autocast (csrc/encends.hip).  Reference droid_slam/modules/extractor.py: conv2 of BasicEncoder;
 * with LGU_ENCOUT_SPLIT also motion_filter.py:36-37, `net, inp = cnet(..).split([128,128], dim=2)`, `net.tanh()`, `inp.relu()`.
 * x (N,128,H,W) NCHW contiguous IEEE half.  Rounding points (those of lgu_upmask1x1_c128_h16):
 *   w_h = half(weight), b_h = half(bias)                    in the pack; x is half and used as it is
 *   p   = sum over c of x[c] * w_h[co][c]                   exact products; fp32 accumulation from ZERO in four steps of 32
 *                                                           channels, ascending
 *   h   = half(b_h + p)                                     one fp32 addition, ONE rounding; NaN is kept
 *   flags 0:           out (N,Cout,H,W) half = h; inp must be null
 *   LGU_ENCOUT_SPLIT:  Cout == 256 only.  out (N,128,H,W) half = net = half(tanhf(float(h[:128]))): the device library's
 *                      float tanh, one rounding, tanh(+-inf) = +-1, NaN kept; inp (N,128,H,W) half = h[128:] < 0 ? 0 :
 *                      h[128:], NaN kept.  out and inp overlap neither x nor one another.
 * The bits of a pixel depend on its own 128 inputs only: a NaN or infinite x reaches exactly its pixel's Cout outputs.  The
 * outputs are fully written and nothing outside them.  No atomics, no workspace, no host synchronisation.
 * wpack: 128 * Cout halves laid out [4 channel blocks kc][Cout/16 channel tiles ct][64 lanes l][8 halves j], the B operand of
 *   v_mfma_f32_16x16x32_f16 as each lane loads it: element j of lane l is w_h[16 ct + (l & 15)][32 kc + 8 (l >> 4) + j].
 *   Every slot holds a weight.  16-byte aligned, otherwise LGU_E_UNSUPPORTED.  bias: Cout halves.
 * x, bias, out and inp are served at the alignment of their element with the same bits: the outputs are stored 8 bytes at a
 *   time where H W % 4 == 0 and their pointers are 8-byte aligned, by element otherwise.
 * Every N >= 0, H >= 1, W >= 1 is served; N == 0: LGU_OK, nothing launched.  N < 0, H < 1, W < 1, an unknown flag,
 * LGU_ENCOUT_SPLIT with Cout != 256, a null x, wpack, bias or out, inp without the flag or the flag without inp, or an operand
 * below its element's alignment: LGU_E_BADARG; Cin != 128, another Cout, a pack that is not 16-byte aligned, H W above
 * INT_MAX - 64 or more than INT_MAX workgroups (N * ceil(H W / 64) * Cout / 64): LGU_E_UNSUPPORTED.  Every refusal comes before
 * any launch and writes nothing.  The operands travel in one parameter block passed by value. */
#define LGU_ENCOUT_SPLIT 1       /* flags: out = tanh(h[:128]), inp = relu(h[128:]) */
typedef struct {
  const void* x; const void* wpack; const void* bias; void* out; void* inp;   /* bias: Cout halves; inp: SPLIT only */
  int N, H, W, Cin, Cout, flags;
} lgu_encout_args;
int lgu_encout1x1_c128_h16(lgu_encout_args args, void* stream);

/* ---- the feature encoder's instance norms folded into its residual-stage convolutions (csrc/encconv.hip, csrc/encstats.hpp).
 * Reference droid_slam/modules/extractor.py:49-55: relu(norm1(conv1 x)), relu(norm2(conv2 .)), relu(x + .) of a ResidualBlock
 * with norm_fn='instance' (InstanceNorm2d without affine terms or running statistics, biased variance).  The producer
 * convolution adds exact sums of its stored half outputs to per-plane accumulators (EMIT); the consumer convolution
 * normalises while it stages its input (the prologue) and, where the staged tensor is a residual later, writes it out once
 * (keep).  The bits are NOT those of lgu_instnorm_relu_h16 (whose statistics are fp32 tree sums): the folded route is opt-in.
 *
 * Exact plane statistics.  A finite half h is m 2^(k-24) with integers 0 <= m < 2048, 0 <= k <= 29, so xi = h 2^24 is an
 * integer, |xi| < 2^40, and xi^2 = m^2 << 2k is below 2^80.  The accumulator of a plane (n, c) is R slots of four 64-bit
 * integers, a tensor (N,C,R,4) int64, ZERO on entry (accumulated into a caller-zeroed buffer, the rule of volume_grad) and
 * 8-byte aligned, R = lgu_encstats_replicas() (8):
 *   S1  = sum xi (two's complement)   LO = sum (xi^2 mod 2^40)   HI = sum (xi^2 >> 40)   BAD = number of non-finite values
 * A workgroup reduces its tile over lanes first and issues one integer atomic add per channel and word (vector-memory
 * atomics, global_atomic_add_x2; BAD only where it is not zero) into slot = (its tile index) mod R.  Integer sums do not
 * depend on their order: summed over the R slots the four words are exact and the same for every schedule, tile choice and R.
 * Planes of more than 2^22 pixels: LGU_E_UNSUPPORTED (each word stays below 2^62 up to there).
 *
 * Mean and rstd: ONE device function, used by the prologue and by lgu_encstats_finalize; double arithmetic, every step
 * rounded once, in this order (IEEE division and square root, no contraction; the same lines in numpy give the same bits):
 *   S1, LO, HI, BAD = integer sums over the R slots
 *   a    = double(S1)                      q   = double(HI) * 2^40 + double(LO)           cnt = pixels per plane
 *   mean = float(a / (cnt * 2^24))         var = max((q - (a * a) / cnt) / (cnt * 2^48), 0)
 *   rstd = float(1 / sqrt(var + double(eps)))
 *   BAD != 0: mean = rstd = NaN            (PyTorch's instance norm makes such a plane NaN)
 * lgu_encstats_finalize({acc, mean_rstd, planes, cnt, eps}, stream) writes (planes,2) float32 {mean, rstd} from acc
 * (planes,R,4); like every layer entry it takes its operands in one parameter block passed by value.  planes == 0: LGU_OK, nothing launched.  planes < 0, cnt < 1, eps < 0 or NaN, a null pointer, acc below
 * 8-byte or mean_rstd below 4-byte alignment: LGU_E_BADARG; cnt > 2^22: LGU_E_UNSUPPORTED.
 *
 * lgu_encconv3x3_norm_h16: x, wpack, bias, out, dpack, dbias, r, N, H, W, Cin, Cout, stride as lgu_encconv3x3_h16, with the
 * identity epilogue always.  mode names the prologue, applied to every staged pixel INSIDE the image; a pixel outside the
 * image is zero AFTER the prologue (the padding belongs to the normalised tensor):
 *   IN(v; mu, rho) = (float(v) - mu) * rho       an fp32 subtraction, then an fp32 product, no contraction
 *   relu(v)        = v < 0 ? 0 : v               a NaN is kept
 *   LGU_ENCNORM_NONE      h = x                                                      (EMIT only)
 *   LGU_ENCNORM_NORM      h = half(relu(IN(x; mu_x, rho_x)))                         extractor.py:49-50
 *   LGU_ENCNORM_RES       h = half(relu(float(y) + relu(IN(x; mu_x, rho_x))))        :50, :55, no downsample
 *   LGU_ENCNORM_RES_NORM  h = half(relu(IN(y; mu_y, rho_y) + relu(IN(x; mu_x, rho_x))))   :50-55, with downsample.1
 * (mu_x, rho_x) per plane of x from stats_x (N,Cin,R,4) with cnt = H W and eps, (mu_y, rho_y) from stats_y; y (N,Cin,H,W)
 * half.  ONE rounding to half; the add is an fp32 add of its own.  h is what the convolution (and on a strided launch the
 * 1x1 branch) then sees: from there on out and r have the bits of lgu_encconv3x3_h16 on h with flags 0.  Each workgroup fills
 * a (mean, rstd) table in LDS from the accumulators at its start; the producer is an earlier launch on the same stream, no
 * workgroup waits on another and there are no fences.
 * keep (N,Cin,H,W) half, with a prologue only: h is also written there, each pixel once, by the workgroup of channel group 0
 *   whose output tile (TY rows from y0, TX columns from x0) owns it: input rows [s y0, s (y0 + TY)), columns [s x0, s (x0 +
 *   TX)), clipped to the image.  keep overlaps no operand (other workgroups read their halo).  Fully written, nothing outside.
 * LGU_ENCNORM_EMIT: the sums of the stored half output over its pixels (y < Ho, x < Wo only) are added to stats_out
 *   (N,Cout,R,4), and on a launch with the branch those of r to stats_r.  Emitting changes no bit of out or r.
 * The bits of out, r and keep depend on the image, its accumulators, H and W only: not on N, the batch position or the tile.
 * A plane with BAD != 0 makes h NaN over that whole plane (for RES_NORM also y's plane), and with it every output that
 * reads it.
 * Refusals and alignment follow lgu_encconv3x3_h16; further LGU_E_BADARG: mode outside 0..3, an unknown flag, eps < 0 or NaN,
 * LGU_ENCNORM_NONE without LGU_ENCNORM_EMIT (that call is lgu_encconv3x3_h16), stats_x / y / stats_y not exactly those the
 * mode reads, keep without a prologue, stats_out not given exactly with EMIT, stats_r not given exactly with EMIT and the
 * branch, an accumulator below 8-byte alignment; H W > 2^22: LGU_E_UNSUPPORTED.  Every refusal comes before any launch and
 * writes nothing.  The operands travel in one parameter block passed by value; lgu_encconv_args is unchanged. */
#define LGU_ENCNORM_NONE 0
#define LGU_ENCNORM_NORM 1
#define LGU_ENCNORM_RES 2
#define LGU_ENCNORM_RES_NORM 3
#define LGU_ENCNORM_EMIT 1       /* flags: add the sums of out (and r) to stats_out (and stats_r) */
typedef struct {
  const void* x; const void* wpack; const void* bias; void* out;      /* bias: Cout halves */
  const void* dpack; const void* dbias; void* r;                      /* all three, or all null */
  const void* y; const void* stats_x; const void* stats_y;            /* what the mode reads, null otherwise */
  void* keep;                                                         /* or null */
  void* stats_out; void* stats_r;                                     /* EMIT (stats_r: with the branch), null otherwise */
  float eps;
  int N, H, W, Cin, Cout, stride, mode, flags;
} lgu_encconv_norm_args;
int lgu_encconv3x3_norm_h16(lgu_encconv_norm_args args, void* stream);
typedef struct {
  const void* acc; void* mean_rstd;   /* (planes,R,4) int64 in, (planes,2) float32 out */
  long planes, cnt;
  float eps;
} lgu_encstats_args;
int lgu_encstats_finalize(lgu_encstats_args args, void* stream);
int lgu_encstats_replicas(void);

/* ---- the Gaussian mask's parameter head: Linear(256, 16) + Tanh, then Linear(16, 2) twice, in one launch
 * (csrc/gausshead.hip).  Reference droid_slam/gaussianMask_cuda.py:69-73: tt = mapA(x), meanMap(tt), covMap(tt); what follows
 * them (:74-83) is lgu_gaussian_params.  x (E,H,W,256) channel-last contiguous; mean_ofs (E,H,W,2), cov_raw (E,H*W,2) and,
 * where the pointer is not null, hidden (E,H,W,16) = tt: fully written, nothing outside them; they overlap neither x nor
 * one another.  Per pixel p, with W2 = [Wm; Wc] (4,16) and b2 = [bm; bc] (4):
 *   half mode (flags without LGU_GAUSSHEAD_FP32): what float16 autocast evaluates.  x float32, or IEEE half with
 *   LGU_GAUSSHEAD_X_HALF; parameters and outputs IEEE half.  Rounding points:
 *     x_h = half(x), W_h = half(W), b_h = half(b)           round to nearest even (x_h in the load, a half x is used as it
 *                                                           is; the parameters in the pack)
 *     s1  = sum over c of x_h[p][c] * W1_h[k][c]            exact products, fp32 accumulation from zero in a fixed order (8
 *                                                           steps of 32 channels, ascending)
 *     u   = half(b1_h[k] + s1)                              one fp32 addition, ONE rounding
 *     tt  = half(tanhf(float(u)))                           the device library's float tanh, ONE rounding; NaN is kept
 *     s2  = sum over k of tt[k] * W2_h[o][k]                exact products, fp32 accumulation from zero (one step of 16)
 *     out = half(b2_h[o] + s2)                              one fp32 addition, ONE rounding; o = 0,1: mean_ofs, 2,3: cov_raw
 *   fp32 mode (LGU_GAUSSHEAD_FP32; not with LGU_GAUSSHEAD_X_HALF): x, parameters and outputs float32, no half rounding:
 *     s1  = fp32 fused multiply-add chains on the fp32 matrix cores (v_mfma_f32_16x16x4_f32, one rounding per term): the
 *           channels 16 m + 4 g + i in the order g, i, m for even m and for odd m, the two chains added once
 *     tt  = tanhf(b1[k] + s1),  out = b2[o] + (the chain over k = 0..15)
 * The bits of a pixel depend on its own 256 inputs only: not on E, the pixel's position, its tile or the launch geometry.
 * A NaN or infinite input reaches exactly its own pixel's 4 outputs and 16 hidden values.  No atomics, no workspace, no
 * LDS, no host synchronisation.
 * wpack: LGU_GAUSSHEAD_WPACK_ELEMS = 256 * 16 + 64 * 4 elements (half, or float32 in fp32 mode), bias: LGU_GAUSSHEAD_BIAS_ELEMS
 *   = 20 elements of the same type, [b1 (16); bm (2); bc (2)].  With lane l, r = l & 15, g = l >> 4:
 *   half: wpack[(kc * 64 + l) * 8 + j] = W1_h[r][32 kc + 8 g + j] (kc < 8, j < 8): the A operand of v_mfma_f32_16x16x32_f16;
 *         wpack[4096 + 4 l + j] = W2_h[r][4 g + j] for r < 4 and ZERO for r >= 4 (j < 4): the A operand of
 *         v_mfma_f32_16x16x16_f16.
 *   fp32: wpack[s * 64 + l] = W1[r][16 (s >> 2) + 4 g + (s & 3)] (s < 64); wpack[4096 + 64 i + l] = W2[r][4 g + i] for r < 4
 *         and ZERO for r >= 4 (i < 4): the A operands of v_mfma_f32_16x16x4_f32, one K step each.
 * x and wpack must be 16-byte aligned, otherwise LGU_E_UNSUPPORTED; bias and the outputs are served at the alignment of
 * their element with the same bits (they are accessed by element).
 * The layer sizes are fixed (256 in, 16 hidden, 2 + 2 out: LGU_GAUSSHEAD_CIN, LGU_GAUSSHEAD_HIDDEN) and the block
 * carries no size: the Python layer refuses any other layer before it gets here.  E, H or W < 0, an unknown flag or both
 * flags: LGU_E_BADARG; E, H or W == 0: LGU_OK, nothing launched; a null x, wpack, bias, mean_ofs or cov_raw, or bias or an
 * output below its element's alignment: LGU_E_BADARG; more than INT_MAX - 16 pixels: LGU_E_UNSUPPORTED.  Every refusal comes
 * before any launch and writes nothing.  The operands travel in one parameter block passed by value. */
#define LGU_GAUSSHEAD_CIN 256
#define LGU_GAUSSHEAD_HIDDEN 16
#define LGU_GAUSSHEAD_WPACK_ELEMS 4352
#define LGU_GAUSSHEAD_BIAS_ELEMS 20
#define LGU_GAUSSHEAD_X_HALF 1   /* flags: x holds IEEE half (half mode only) */
#define LGU_GAUSSHEAD_FP32 2     /* flags: fp32 mode */
typedef struct {
  const void* x; const void* wpack; const void* bias;
  void* mean_ofs; void* cov_raw; void* hidden;              /* hidden: or null */
  int E, H, W, flags;
} lgu_gausshead_args;
int lgu_gaussian_head(lgu_gausshead_args args, void* stream);

/* ---- the map export: the filtered, coloured point cloud of a set of keyframes, compacted on the device (csrc/cloud.hip).
 * Reference droid_slam/visualization.py:92-129: iproj under the inverted poses, depth_filter, the per-frame disparity floor
 * and the boolean index per frame.  poses (np,7), disps (nd,ht,wd), intrinsics, ix (num) int64 and thresh (num) as the
 * geometry entries above take them; floor (num) float: the per-entry disparity floor.  For entry b and pixel k (row-major)
 * of frame ix[b]:
 *   count = what lgu_depth_filter_f32 writes for that pixel (one shared definition, csrc/geom_pixel.hpp; an ix[b] outside
 *           [0, min(np, nd)) counts 0)
 *   keep  = count >= min_count && disps[ix[b]][k] > floor[b]        (float comparison; an invalid ix[b] keeps nothing,
 *           whatever min_count)
 *   point = what lgu_iproj_f32 writes for that pixel (the same shared definition) under the inverse of poses[ix[b]], the
 *           inverse formed once per workgroup as conj(q), uv = 2 (v x t), w = v x uv, -((t + q.w uv) + w) with every product
 *           and sum rounded on its own, except a cross product's a1 b2 - a2 b1 = fma(a1, b2, -(a2 b1)), as the framework's
 *           cross product evaluates it: the bits of the pure-framework inverse the callers of lgu_iproj_f32 use
 *   colour[c] = float(images[ix[b]][2 - c][phase + stride i][phase + stride j]) * r255 with lgu_image_normalize_u8's r255,
 *           or with color_u8 the byte itself; images (ni,3,H,W) uint8 BGR, or null: no colours
 * Kept pixels are written densely, entries in ix order and pixels ascending inside an entry: entry b owns the rows
 * offsets[b] : offsets[b + 1] of points (cap,3) float and colors (cap,3) float or uint8.  A row >= cap is not written;
 * offsets (num + 1) int64 always holds the true totals.  The order comes from the launch boundaries (no atomics, no
 * workgroup waits on another): the same bits on every run.
 *
 * lgu_cloud_decide_f32   two launches: count, keep and the 64-lane ballot words of keep into scratch; then one workgroup forms
 *   the exclusive prefix of the kept counts and writes offsets.  Reads poses .. floor, min_count; writes scratch, offsets.
 * lgu_cloud_write_f32    one launch: every kept lane ranks itself from the ballot words and the prefix in scratch and stores its
 *   point and colour.  Takes the scratch of a lgu_cloud_decide_f32 call with the same num, ht, wd, ix; reads poses, disps,
 *   intrinsics, ix, images; writes points and colors below cap.  cap == 0: nothing is launched.
 * scratch: lgu_cloud_scratch_bytes(num, ht, wd) bytes of device memory, 8-byte aligned like offsets (else LGU_E_BADARG); it
 * needs no initialisation.  Sizes as the geometry entries' (num == 0 or an empty frame: nothing is launched; more than
 * 65535 * 256 pixels per frame: LGU_E_UNSUPPORTED).  With images: ni >= min(np, nd), stride >= 1, phase >= 0, phase + stride
 * (ht - 1) < H and phase + stride (wd - 1) < W, else LGU_E_BADARG.  Launched on `stream`, no host synchronisation.  The
 * operands travel in one parameter block passed by value. */
typedef struct {
  const float* poses; const float* disps; const float* intrinsics;
  const long long* ix; const float* thresh; const float* floor;        /* thresh, floor: the decision pass only */
  const void* images;                                                  /* or null */
  void* scratch; long long* offsets;                                   /* offsets: the decision pass only */
  float* points; void* colors; long long cap;                          /* the write pass only; colors: or null */
  int np, nd, ht, wd, num, min_count;
  int ni, H, W, stride, phase, color_u8;
} lgu_cloud_args;
long long lgu_cloud_scratch_bytes(int num, int ht, int wd);
int lgu_cloud_decide_f32(lgu_cloud_args args, void* stream);
int lgu_cloud_write_f32(lgu_cloud_args args, void* stream);

/* ---- the frame intake: rectify, resize, crop and normalise a decoded camera frame in one launch (csrc/intake.hip).
 * What the reference's streams do on the host before Droid.track (demo.py:39-54, demo_depth.py:39-65,
 * evaluation_scripts/test_tum.py:34-52, test_euroc.py:29-76) and motion_filter.py:56-57 after it.  The definition is
 * tests/intake_restatement.py; DESIGN.md section 3.26 states it in full.
 *   raw (N,h0,w0,C) uint8, C = 3 (BGR, interleaved as decoders deliver it) or 1 (grey, replicated)
 *   stage 1, present when ncam > 0: pixel (u,v) of the rectified image (h0,w0) reads raw at the camera's map, in double
 *     with every operation rounded on its own (no contraction): x = (u - kn[2]) / kn[0], y = (v - kn[3]) / kn[1];
 *     (X,Y,W) = ((ir[3r] x + ir[3r+1] y) + ir[3r+2]); x = X / W, y = Y / W; r2 = x x + y y;
 *     rad = 1 + r2 (d[0] + r2 (d[1] + r2 d[4])); t = 2 (x y); xd = (x rad + d[2] t) + d[3] (r2 + 2 (x x));
 *     yd = (y rad + d[2] (r2 + 2 (y y))) + d[3] t; m = (xd k[0] + k[2], yd k[1] + k[3]).  q = floor(32 m + 0.5) per axis,
 *     clamped to [-2^30, 2^30] (a NaN to -2^30); taps (q >> 5, (q >> 5) + 1) with weights (32 - (q & 31), q & 31), a tap
 *     outside the raw frame contributes 0; byte = (sum + 512) >> 10 per channel
 *   stage 2, present when (h1,w1) != (h0,w0): per axis f = (o + 0.5) (n_in / n_out) - 0.5 in double, i0 = floor(f),
 *     a = f - i0; i0 < 0: i0 = 0, a = 0; i0 >= n_in - 1: i0 = n_in - 1, a = 0; i1 = min(i0 + 1, n_in - 1);
 *     k = floor(2048 a + 0.5); byte = (sum of the four stage-1 BYTES with weights (2048 - k, k) per axis + 2^21) >> 22
 *   stage 3: the rectangle (top, left, H, W) of the (h1,w1) image
 *   image (N,3,H,W) uint8 BGR planar; inputs (N,3,H,W) float RGB or null: lgu_image_normalize_u8's value of image, the
 *     same device function (csrc/image_norm.hpp), with mean[3], std[3] RGB
 * Cameras: ncam = 0 (no stage 1), 1 (shared by the batch) or N (one per frame).  Up to 2 travel in the block (cam);
 * more as a device table cam_table (ncam entries, 8-byte aligned), else LGU_E_BADARG.  lgu_intake_camera is 22 doubles:
 * k = fx, fy, cx, cy of the raw camera; kn = the same of the rectified camera; ir = the inverse of the rectifying
 * rotation, row-major; d = k1, k2, p1, p2, k3.
 * path: 0 picks the kernel (the LDS tile when both stages are present and the tile's stage-1 rectangle fits, else the
 * direct kernel); 1 asks for the tile kernel (a workgroup whose rectangle does not fit computes directly), 2 for the
 * direct kernel.  The bytes do not depend on it.
 * Negative sizes, C not 1 or 3, a crop outside (h1,w1), an empty raw frame behind a non-empty output, ncam not 0 | 1 | N,
 * a null raw or image, an unknown path: LGU_E_BADARG.  N == 0 or H W == 0 launches nothing.  More than 65535 frames or
 * tile rows: LGU_E_UNSUPPORTED.  No atomics; the same bits on every run.  Operands at element alignment.
 *
 * lgu_intake_depth_f32  the sensor disparity of depth_video.py:64-66 from the raw depth image: for the points [3::8, 3::8]
 * of the (top, left, H, W) rectangle of the depth resized to (h1,w1) as the framework's bilinear interpolation without
 * aligned corners does (f = max((o + 0.5) (n_in / n_out) - 0.5, 0), i0 = floor(f), i1 = i0 + (i0 < n_in - 1), l1 = f - i0,
 * l0 = 1 - l1): d = ly0 (lx0 p00 + lx1 p01) + ly1 (lx0 p10 + lx1 p11) with p = double(raw) * scale, in double;
 * out = float(d > 0 ? 1 / d : d).  raw (N,h0,w0) uint16 (src_u16) or float; out (N, (H + 4) / 8, (W + 4) / 8) float.
 * Refusals as above (an empty raw behind a non-empty output, a crop outside: LGU_E_BADARG). */
typedef struct {
  double k[4]; double kn[4]; double ir[9]; double d[5];
} lgu_intake_camera;
typedef struct {
  const void* raw; void* image; float* inputs;                         /* inputs: or null */
  const lgu_intake_camera* cam_table;                                  /* ncam > 2 only */
  lgu_intake_camera cam[2];
  float mean[3]; float std[3];
  int N, h0, w0, C, h1, w1, top, left, H, W, ncam, path;
} lgu_intake_args;
typedef struct {
  const void* raw; float* out; double scale;
  int N, h0, w0, h1, w1, top, left, H, W, src_u16;
} lgu_intake_depth_args;
int lgu_intake_frame_u8(lgu_intake_args args, void* stream);
int lgu_intake_depth_f32(lgu_intake_depth_args args, void* stream);

/* ---- the offscreen view of the map: coloured points and one wireframe frustum per keyframe, z-buffered (csrc/render.hip).
 * The drawing half of the reference's visualiser: the point actors and camera actors of droid_slam/visualization.py:36-51,
 * 121-134 in the window of :144-153 with misc/renderoption.json (white background, point size 2).  The definition is
 * tests/render_restatement.py; DESIGN.md section 3.27 states it in full.  It is this project's own definition of the view:
 * it was never compared with an Open3D render.
 *   points (npoints,3) float, world coordinates; colors (npoints,3) RGB, float in [0,1] or with color_u8 the bytes
 *   view (7) float, world-to-camera t, q(xyzw); intrinsics: fx, fy, cx, cy of the output image; cameras (ncam,7) float,
 *   world-to-camera, or null with ncam == 0
 *   image (H,W,3) uint8 RGB; depth (H,W) float: the camera-space z of the winning primitive, +inf on background
 * Frame buffer: one 64-bit key per pixel in scratch, all ones = empty.  A primitive offers (bits(z) << 32) | (r << 16) |
 * (g << 8) | b with the float bit pattern of its positive z; a pixel keeps the minimum (64-bit atomic minimum): the nearest
 * wins, among equal depths the smaller packed colour, whatever the order of points, launches or arrival.
 * Every float operation rounds on its own.
 *   point:  Y = act_so3(q, P) + t (the shared definition of csrc/se3.hpp); skipped unless x, y, z are finite and z > near;
 *           u = fx (x / z) + cx, v = fy (y / z) + cy; x0 = int(floor(u + (1 - 0.5 s))) saturating (NaN: 0), y0 likewise, s =
 *           point_size; the pixels x0 .. x0 + s - 1 by y0 .. y0 + s - 1 inside the image are offered the key.  A float
 *           colour becomes the byte clamp(floor(c 255 + 0.5), 0, 255), a NaN 0.
 *   frustum of camera k: (tr, qr) = rel_se3(cameras[k], view); eight vertices (an apex, a 2 x 2 base at depth 1.5, an
 *           up-marker on the base's lower edge) times camera_scale, V = act_so3(qr, X) + tr; ten segments A -> B (the base's
 *           four edges, the four apex edges, the marker's two strokes).  A segment with a non-finite coordinate or both ends
 *           with !(z >= near) is skipped; one end with !(z >= near) is replaced by A + tc (B - A), tc = (near - A.z) / (B.z -
 *           A.z), with z = near exactly.  Ends are projected as points are, w = 1 / z; n = ceil(max(|ub - ua|, |vb - va|)),
 *           1 if 0; a non-finite n or n > 2^20 skips the segment.  Sample k = 0 .. n: tk = float(k) / n, u = ua + tk (ub -
 *           ua), v and w likewise, z = 1 / w; it offers (bits(z), camera_color) to pixel (floor(u + 0.5), floor(v + 0.5)) if
 *           inside the image.
 *   resolve: an empty pixel gets background and +inf, any other the key's three bytes and the float of its high word.
 * Launches: clear, points (npoints > 0), lines (ncam > 0, one wave per camera), resolve; all on `stream`, no host
 * synchronisation.  scratch: lgu_render_scratch_bytes(H, W) = 8 H W bytes of device memory (0 for an empty or negative
 * size), 16-byte aligned (else LGU_E_BADARG); it needs no initialisation.  Other operands at element alignment.
 * Negative sizes, point_size outside 1..8, a near that is not finite and positive, a non-finite camera_scale, a null operand
 * that the sizes need: LGU_E_BADARG.  H W > 2^28: LGU_E_UNSUPPORTED.  H W == 0: nothing is launched.  Every refusal comes
 * before any launch.  The operands travel in one parameter block passed by value. */
typedef struct {
  const float* points; const void* colors; const float* view; const float* intrinsics;
  const float* cameras;                                                /* or null */
  void* scratch; unsigned char* image; float* depth;
  long long npoints;
  float near, camera_scale;
  int ncam, H, W, point_size, color_u8;
  unsigned char background[3]; unsigned char camera_color[3];
} lgu_render_args;
long long lgu_render_scratch_bytes(int H, int W);
int lgu_render_view(lgu_render_args args, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LGU_CORR_H */
