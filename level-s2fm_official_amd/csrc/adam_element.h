// The element update of torch.optim.Adam (amsgrad = False, maximize = False) in fp32, with the scalars formed as adam.hip's header
// describes.  Shared by the fused Adam step (adam.hip) and the classical bundle adjustment's update kernel (bundle_adjust.hip);
// tests/test_hip_fused_adam.py holds it to a float64 Adam element by element.
#pragma once

#include "ls2fm_device.h"

namespace {

struct AdamHyper { float step_size, bc2_sqrt, w1, beta2, one_minus_beta2, eps, weight_decay; };

__device__ __forceinline__ void adam_one(float& p, float g, float& m, float& v, const AdamHyper& h) {
    if (h.weight_decay != 0.f) g = fmaf(h.weight_decay, p, g);
    m = h.w1 < 0.5f ? m + h.w1 * (g - m) : g - (g - m) * (1.0f - h.w1);       // torch lerp
    v = v * h.beta2 + (h.one_minus_beta2 * g) * g;
    const float denom = sqrtf(v) / h.bc2_sqrt + h.eps;
    p = p - h.step_size * (m / denom);
}

}  // namespace
