// image_norm.hpp — the frame normalisation of droid_slam/motion_filter.py:56-57 for one byte: the one device definition
// behind lgu_image_normalize_u8 (instnorm.hip) and the `inputs` of lgu_intake_frame_u8 (intake.hip).
#pragma once

namespace lgu {

// The product is what the reference's `/ 255.0` is on the device: a tensor divided by a Python number is multiplied by
// the reciprocal, formed in double and rounded to fp32 once (it equals the correctly rounded quotient for 130 of the 256
// byte values only).  The subtraction and the division by std are the tensor-tensor ops: IEEE.
constexpr float IMG_INV255 = (float)(1.0 / 255.0);

__device__ __forceinline__ float image_normalize_value(unsigned char px, float m, float sd) {
  return ((float)px * IMG_INV255 - m) / sd;
}

}  // namespace lgu
