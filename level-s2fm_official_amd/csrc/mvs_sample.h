// What csrc/mvs_sweep.hip and csrc/mvs_patchmatch.hip both say of THE SWEEP RULE (include/ls2fm.h): the pose of a (reference,
// source) pair, step 3's bilinear sample, the correctly rounded root, and the arguments every entry point of the two refuses.
#pragma once

#include "ls2fm_device.h"
#include "raster_project.h"

#include <cmath>

__device__ __forceinline__ float finite_or_nan(float v) { return fabsf(v) < INFINITY ? v : NAN; }

// the correctly rounded fp32 square root.  __fsqrt_rn lowers to the bare v_sqrt_f32 here (1 ulp), so the root is taken in fp64
// (correctly rounded: csrc/mesh_colors.hip relies on it too) and rounded to fp32: 53 >= 2 * 24 + 2 bits leave no double rounding
__device__ __forceinline__ float sqrt_rn(float v) { return (float)__dsqrt_rn((double)v); }

// the pose of entry `pair` of a [.., 3, 4] array with the intrinsics of view `view`: uniform over the wave, scalar loads
__device__ __forceinline__ View load_pair(const float* __restrict__ rel, int64_t pair, const float* __restrict__ intr, int view) {
    View w;
    const float* p = rel + pair * 12;
#pragma unroll
    for (int k = 0; k < 12; ++k) w.p[k] = p[k];
    const float* q = intr + (int64_t)view * 4;
    w.fx = q[0]; w.fy = q[1]; w.cx = q[2]; w.cy = q[3];
    return w;
}

// STEP 3 of THE SWEEP RULE: the bilinear sample of one image at the projection p, NaN when the tap (`tap_ok`) or the sample is
// invalid or the result not finite.  kSkip: an invalid sample returns before its loads (the sweep: a lane has one or two samples
// per fill).  Without it there is no branch: an invalid sample reads the image's first four pixels and is discarded, so the
// loads of several taps can be in flight at once (PatchMatch; the image is at least 2 x 2 there, the caller's pixel has a window).
template <bool kSkip>
__device__ __forceinline__ float sample(const float* __restrict__ img, int height, int width, const Projected& p, bool tap_ok = true) {
#pragma clang fp contract(off)
    const float x = __fsub_rn(p.u, 0.5f), y = __fsub_rn(p.v, 0.5f);
    const float x0 = floorf(x), y0 = floorf(y);
    // every comparison is false for a NaN; |u|, |v| <= 65536 by usable, so x0 and y0 convert
    const bool ok = tap_ok && p.usable && x0 >= 0.0f && x0 <= (float)(width - 2) && y0 >= 0.0f && y0 <= (float)(height - 2);
    if (kSkip && !ok) return NAN;
    const float tx = __fsub_rn(x, x0), ty = __fsub_rn(y, y0);
    const float* q = img + (kSkip || ok ? (int64_t)(int)y0 * width + (int)x0 : (int64_t)0);
    const float b00 = q[0], b10 = q[1], b01 = q[width], b11 = q[width + 1];
    const float r0 = __fadd_rn(b00, __fmul_rn(tx, __fsub_rn(b10, b00)));
    const float r1 = __fadd_rn(b01, __fmul_rn(tx, __fsub_rn(b11, b01)));
    const float b = finite_or_nan(__fadd_rn(r0, __fmul_rn(ty, __fsub_rn(r1, r0))));
    return kSkip || ok ? b : NAN;
}

static inline bool finite_not_negative(float v) { return v >= 0.0f && v < INFINITY; }

// what every entry point refuses before n_refs = 0 returns; the sweep adds its plane count, PatchMatch its tap step
static inline bool mvs_shape_ok(int32_t n_views, int32_t height, int32_t width, int32_t n_refs, int32_t n_sources, int32_t half_width,
                                float near, float min_var, int32_t min_sources) {
    return raster_image_ok(n_views, height, width) && raster_image_ok(n_refs, height, width) && raster_near_ok(near) && n_sources >= 1 &&
           n_sources <= LS2FM_MVS_MAX_SOURCES && half_width >= 1 && half_width <= LS2FM_MVS_MAX_HALF_WIDTH && finite_not_negative(min_var) &&
           min_sources >= 1 && min_sources <= n_sources;
}
