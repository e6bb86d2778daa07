// The expressions csrc/mvs_patchmatch.hip shares with THE SWEEP RULE (include/ls2fm.h), stated for that file alone -- the pose of a
// (reference, source) pair, step 3's bilinear sample, the correctly rounded root -- and THE DRAWS of the PatchMatch rules.
// csrc/mvs_sweep.hip keeps its own statement of the first three: its code object stays what it was.
#pragma once

#include "ls2fm_device.h"
#include "raster_project.h"

#include <cmath>

__device__ __forceinline__ float pm_finite_or_nan(float v) { return fabsf(v) < INFINITY ? v : NAN; }

// the correctly rounded fp32 square root: the fp64 root (correctly rounded) rounded to fp32; 53 >= 2 * 24 + 2 bits leave no
// double rounding
__device__ __forceinline__ float pm_sqrt_rn(float v) { return (float)__dsqrt_rn((double)v); }

// the pose of entry `pair` of a [.., 3, 4] array with the intrinsics of view `view`: uniform over the wave, scalar loads
__device__ __forceinline__ View pm_load_pair(const float* __restrict__ rel, int64_t pair, const float* __restrict__ intr, int view) {
    View w;
    const float* p = rel + pair * 12;
#pragma unroll
    for (int k = 0; k < 12; ++k) w.p[k] = p[k];
    const float* q = intr + (int64_t)view * 4;
    w.fx = q[0]; w.fy = q[1]; w.cx = q[2]; w.cy = q[3];
    return w;
}

// STEP 3 of THE SWEEP RULE: the bilinear sample of one image at the projection p, NaN when the tap (`tap_ok`) or the sample is
// invalid or the result not finite.  Without a branch: an invalid sample reads the image's first four pixels and is discarded, so
// the loads of several taps can be in flight at once.  The image is at least 2 x 2 (the caller's pixel has a window).
__device__ __forceinline__ float pm_sample(const float* __restrict__ img, int height, int width, const Projected& p, bool tap_ok) {
#pragma clang fp contract(off)
    const float x = __fsub_rn(p.u, 0.5f), y = __fsub_rn(p.v, 0.5f);
    const float x0 = floorf(x), y0 = floorf(y);
    // every comparison is false for a NaN; |u|, |v| <= 65536 by usable, so x0 and y0 convert
    const bool ok = tap_ok && p.usable && x0 >= 0.0f && x0 <= (float)(width - 2) && y0 >= 0.0f && y0 <= (float)(height - 2);
    const float tx = __fsub_rn(x, x0), ty = __fsub_rn(y, y0);
    const float* q = img + (ok ? (int64_t)(int)y0 * width + (int)x0 : (int64_t)0);
    const float b00 = q[0], b10 = q[1], b01 = q[width], b11 = q[width + 1];
    const float r0 = __fadd_rn(b00, __fmul_rn(tx, __fsub_rn(b10, b00)));
    const float r1 = __fadd_rn(b01, __fmul_rn(tx, __fsub_rn(b11, b01)));
    return ok ? pm_finite_or_nan(__fadd_rn(r0, __fmul_rn(ty, __fsub_rn(r1, r0)))) : NAN;
}

// THE DRAWS
__device__ __forceinline__ uint32_t pm_mix(uint32_t x) {
    x ^= x >> 16; x *= LS2FM_MVS_MIX_A;
    x ^= x >> 15; x *= LS2FM_MVS_MIX_B;
    return x ^ (x >> 15);
}

__device__ __forceinline__ float pm_draw(uint32_t key, uint32_t j) { return __fmul_rn((float)(pm_mix(key + j) >> 8), 0x1p-24f); }

// 2 u - 1: exact, u is a multiple of 2^-24 below 1
__device__ __forceinline__ float pm_signed(float u) { return __fsub_rn(__fmul_rn(2.0f, u), 1.0f); }

struct Normal {
    float x, y, z;
};

__device__ __forceinline__ Normal pm_normalise(float x, float y, float z) {
#pragma clang fp contract(off)
    const float root = pm_sqrt_rn(__fadd_rn(__fadd_rn(__fmul_rn(x, x), __fmul_rn(y, y)), __fmul_rn(z, z)));
    return {__fdiv_rn(x, root), __fdiv_rn(y, root), __fdiv_rn(z, root)};
}

// g = ((n_x xn) + (n_y yn)) + n_z
__device__ __forceinline__ float pm_g(const Normal& n, float xn, float yn) {
#pragma clang fp contract(off)
    return __fadd_rn(__fadd_rn(__fmul_rn(n.x, xn), __fmul_rn(n.y, yn)), n.z);
}
