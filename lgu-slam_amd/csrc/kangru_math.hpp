// kangru_math.hpp — the scalar pieces of the KAN-bias GRU's element-wise arithmetic, shared by kangru.hip (the gates and
// the blend as streaming kernels) and gruconv.hip (the same arithmetic as the epilogue of the 448-channel convolution):
// one definition, so the two compute the same bits.  Built with -ffp-contract=off.
#pragma once
#include "lgu_common.hpp"

namespace lgu {

// rounds an fp32 value to T and back: the identity for fp32, round-to-nearest-even to half otherwise
template <typename T> __device__ __forceinline__ float rnd(float v) { return (float)(T)v; }
__device__ __forceinline__ float kg_sigmoid(float v) { return 1.0f / (1.0f + expf(-v)); }

}  // namespace lgu
