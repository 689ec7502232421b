// defcorr_lean.hpp — what defcorr.hip calls in defcorr_lean.hip.
#pragma once
#include "lgu_common.hpp"

namespace lgu {

// The production configuration of the fused pyramid sampler (radius 3, 4 levels, offsets on levels 0-1, planar output).
// Returns LGU_E_UNSUPPORTED for anything else: pyramid_forward (defcorr.hip) then takes the general kernel.
int lean_pyramid_forward(const float* const* volumes, const float* coords, float* const* offsets, float* out, int E,
                         int H1, int W1, const int* H2, const int* W2, int flags, const int* edge_slot, hipStream_t st);

}  // namespace lgu
