// shade_fwd: per-sample field evaluation + per-ray compositing of Renderer.forward on the matrix cores.
//
//   workgroup = one ray (its N samples are the N dimension of every GEMM), wave = CT 16-column tiles of consecutive samples
//   (CT = 2: 32 samples per wave and 4 waves/SIMD for rays of up to 256 samples; CT = 4 beyond).
//   Everything is kept TRANSPOSED, [feature x sample], so that the accumulator tile of one v_mfma_f32_16x16x4_f32
//   (lane 16 g + jl holds rows 4 g + r, column jl) is directly the B operand of the next GEMM over that feature
//   dimension (k-slot g <-> row 4 g + r): the whole chain
//        A1 = W0' U          (64 x 36) x (36 x S)     U = [32 encoding channels ; p / rescale ; 1]  (bias folded in)
//        H  = softplus_100(A1), S1 = softplus'
//        F  = W1[1..16] H    (16 x 64) x (64 x S)     sdf row W1[0] H: 16 FMAs per lane + 2 cross-lane adds
//        R  = W0'^T (S1 . w1_0)   (48 x 64) x (64 x S)  -> analytic normal n = kappa (dU/dp)^T R      
//        [second field: A1, H, F only]
//   runs out of registers with no LDS staging; the MFMA-ordered weight copies come from prep_weights (L2-resident, one
//   coalesced 256-B load per operand).  The per-sample scalars (sdf, normal, colour) are then transposed through LDS to
//   one-thread-per-sample order for the transmittance scan (Renderer.py:33-49).
// fp32 MFMA = exact fp32 products and sums (no reduced-precision path); only the summation order differs from the
// scalar-FMA oracle.
//
// Shared by the training forward's kernel (shade_fwd.hip) and the image render's (render_image.hip); the kernel body is
// shade_fwd_body.inc.
#pragma once

#include "render_common.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

// No issue-priority hooks here: with four waves per SIMD, raising a wave's priority inside the hidden-block loop or around its MFMA
// clusters measured nothing or worse (profiles/r06_notes.md sections 9 and 13); neither did a scheduling barrier behind that loop.
// The per-sample outputs (sdf, normal, colour, the CT = 2 feature blocks: what shade_bwd reads back ~100 us later, and the caller's
// [R, N] tensors) leave with non-temporal stores (section 12).
__device__ __forceinline__ f32x4 mfma4(float a, float b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

// sum over the four 16-lane groups (g = 0..3) of a wave: every lane ends with the total
__device__ __forceinline__ float sum_over_groups(float v) {
    v += __shfl_xor(v, 16, 64);
    v += __shfl_xor(v, 32, 64);
    return v;
}

}  // namespace
