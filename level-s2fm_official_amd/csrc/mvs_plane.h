// What csrc/mvs_patchmatch.hip alone adds to csrc/mvs_sample.h: THE DRAWS of the PatchMatch rules, and a plane's normal with its
// normalisation and its g.
#pragma once

#include "mvs_sample.h"

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
    const float root = sqrt_rn(__fadd_rn(__fadd_rn(__fmul_rn(x, x), __fmul_rn(y, y)), __fmul_rn(z, z)));
    return {__fdiv_rn(x, root), __fdiv_rn(y, root), __fdiv_rn(z, root)};
}

// g = ((n_x xn) + (n_y yn)) + n_z
__device__ __forceinline__ float pm_g(const Normal& n, float xn, float yn) {
#pragma clang fp contract(off)
    return __fadd_rn(__fadd_rn(__fmul_rn(n.x, xn), __fmul_rn(n.y, yn)), n.z);
}
