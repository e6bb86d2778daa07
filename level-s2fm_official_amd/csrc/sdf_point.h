// Point evaluation shared by the kernels of sdf_eval.hip and trace_image.hip: one level's gather, the hash encoding of a world
// point, the LDS copy of the geometry MLP's weights and the signed SDF (SDF.infer_sdf, models/SDF.py:55-78).  Every evaluator
// of the field is built from these (and render_common.h's layer0_preact / geometry_forward), which is why they agree bit for bit.
#pragma once

#include "render_common.h"

// weight preparation (render_fwd.hip) and the normal query on prepared weights (sdf_eval.hip), shared with trace_image.hip
int ls2fm_launch_prep_sdf(const ls2fm_params* params, int n_levels, Packed* out, hipStream_t stream, int32_t* zero_word = nullptr);
int ls2fm_launch_prep_render(const ls2fm_params* params, int n_levels, int n_levels2, int dual, Packed* out, hipStream_t stream);
int ls2fm_launch_sdf_normals(const ls2fm_field_desc* field, const ls2fm_grid_desc* grid, const Packed* pk, const float* table,
                             const float* p, int64_t n, int64_t n_query, float* sdf, float* normal, hipStream_t s);

namespace {

// position in the unit cube of the scene box: what the hash grid is indexed with
__device__ __forceinline__ void unit_cube(const FieldC& fc, const float p[3], float x[3]) {
#pragma unroll
    for (int a = 0; a < 3; ++a) x[a] = (p[a] - fc.bmin[a]) / (fc.bmax[a] - fc.bmin[a]);
}

// level l at unit-cube position x: the cell, its eight corner values, and the trilinear value as ONE fmaf chain per feature over
// the corners k = 0 .. 7 from zero (the order every consumer of the encoding shares)
__device__ __forceinline__ void gather_level(const LevelSet& lv, const float* __restrict__ table, int l, const float x[3],
                                             Cell& c, float2 (&v)[8], float& y0, float& y1) {
    locate(x, lv.scale[l], lv.res[l], lv.size[l], lv.offset[l], lv.hashed[l], c);
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = *reinterpret_cast<const float2*>(table + 2ull * c.idx[k]);
    y0 = 0.f;
    y1 = 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const float wt = corner_weight(c.w, k);
        y0 = fmaf(wt, v[k].x, y0);
        y1 = fmaf(wt, v[k].y, y1);
    }
}

__device__ __forceinline__ void gather_level(const LevelSet& lv, const float* __restrict__ table, int l, const float x[3],
                                             float& y0, float& y1) {
    Cell c;
    float2 v[8];
    gather_level(lv, table, l, x, c, v, y0, y1);
}

// hash-encode a world point into u[35] = [p / rescale, e(x)]
__device__ __forceinline__ void encode_point(const LevelSet& lv, const FieldC& fc, const float* __restrict__ table,
                                             const float p[3], float (&u)[kInMax]) {
    float x[3];
    unit_cube(fc, p, x);
#pragma unroll
    for (int a = 0; a < 3; ++a) u[a] = p[a] / fc.rescale;
#pragma unroll
    for (int l = 0; l < LS2FM_MAX_LEVELS; ++l) {
        float y0 = 0.f, y1 = 0.f;
        if (l < lv.n_levels) gather_level(lv, table, l, x, y0, y1);
        u[3 + 2 * l] = y0;
        u[4 + 2 * l] = y1;
    }
}

__device__ __forceinline__ float signed_sdf(const FieldC& fc, int bg_sdf, float bg_rad, float f0, const float p[3],
                                            bool* bg_selected) {
    float sdf = fc.inside ? f0 / fc.scale_mlp : -f0 / fc.scale_mlp;
    *bg_selected = false;
    if (bg_sdf) {
        const float other = bg_rad - sqrtf(p[0] * p[0] + p[1] * p[1] + p[2] * p[2]);
        if (other < sdf) { sdf = other; *bg_selected = true; }
    }
    return sdf;
}

// ---- the 16-lanes-per-point kernels read the layer-0 rows and the layer-1 columns from LDS
constexpr int kW0Stride = 36;           // W0[j][0..34], b0[j] : 16-byte aligned rows, 2-way bank conflicts at most
constexpr int kW1Stride = kOut;         // 17: odd, the 16 lanes' feature weights of one unit are conflict-free

// 256 threads copy W0 | b0 of every unit into s_w0 (rows of kW0Stride) and the first w1_stride layer-1 weights of every unit into
// s_w1 (1: the sdf row alone; kW1Stride: all 17 rows); the caller synchronises
__device__ __forceinline__ void stage_weights(const float* __restrict__ rec, float* __restrict__ s_w0, float* __restrict__ s_w1,
                                              int w1_stride) {
    for (int q = threadIdx.x; q < kHidden * kW0Stride; q += 256) s_w0[q] = rec[(q / kW0Stride) * kRecStride + q % kW0Stride];
    for (int q = threadIdx.x; q < kHidden * w1_stride; q += 256) s_w1[q] = rec[(q / w1_stride) * kRecStride + kRecW1 + q % w1_stride];
}

// ---- the field's value at p, three ways.  One lane: the whole chain -- 16 levels of dependent gathers and 3.3 k scalar-operand
// FMAs -- in that lane (throughput: no redundant lanes).
__device__ __forceinline__ float lane_sdf(const LevelSet& lv, const FieldC& fc, int bg_sdf, float bg_rad,
                                          const float* __restrict__ rec, const float* __restrict__ table, const float p[3]) {
    float u[kInMax], f[kOut], dummy[kInMax];
    encode_point(lv, fc, table, p, u);
    geometry_forward<false>(rec, u, f, dummy);
    bool bg;
    return signed_sdf(fc, bg_sdf, bg_rad, f[0], p, &bg);
}

// One lane: the analytic normal d sdf / d p (SDF.gradient, not normalised) from r = W0^T (s' w1_0) of geometry_forward<true>: a
// second gather pass contracting the hash Jacobian with r, levels and corners in index order; the background sphere's normal
// where signed_sdf selected it.  These are the statements of sdf_eval_kernel<true> (sdf_eval.hip), which keeps them inline: called
// from there, the same statements cost that kernel 18 more VGPRs (120 for 102), and nothing measured says that is free.
// tests/test_hip_radiance_points.py holds the two to the same bits with the thread-per-point kernel forced.
__device__ __forceinline__ void lane_normal(const LevelSet& lv, const FieldC& fc, const float* __restrict__ table, const float p[3],
                                            const float (&rr)[kInMax], bool bg, float (&nrm)[3]) {
    float acc[3] = {0.f, 0.f, 0.f};
    float x[3];
    unit_cube(fc, p, x);
#pragma unroll
    for (int l = 0; l < LS2FM_MAX_LEVELS; ++l) {
        if (l < lv.n_levels) {
            Cell c;
            locate(x, lv.scale[l], lv.res[l], lv.size[l], lv.offset[l], lv.hashed[l], c);
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const float2 v = *reinterpret_cast<const float2*>(table + 2ull * c.idx[k]);
                const float m = fmaf(v.x, rr[3 + 2 * l], v.y * rr[4 + 2 * l]) * lv.scale[l];
#pragma unroll
                for (int a = 0; a < 3; ++a) acc[a] = fmaf(corner_dweight(c.w, k, a), m, acc[a]);
            }
        }
    }
    const float len = sqrtf(p[0] * p[0] + p[1] * p[1] + p[2] * p[2]);
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float n = fc.kappa * (rr[a] / fc.rescale + acc[a] * fc.inv_ext[a]);
        nrm[a] = bg ? -p[a] / len : n;
    }
}

// f += w[J] * (lane J of this lane's 16-lane row).h for J = 0 .. 15, one fmaf chain; the broadcast is a DPP row_share operand
// (full-rate VALU), not an LDS permute
template <int J>
__device__ __forceinline__ float row_chain(const float* __restrict__ w, float h, float f) {
    if constexpr (J < 16) {
        const float hv = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(h), 0x150 + J, 0xF, 0xF, false));
        return row_chain<J + 1>(w, h, fmaf(w[J], hv, f));
    } else {
        return f;
    }
}

// A 16-lane group (lanes gbase .. gbase + 15 of the wave, jl = lane - gbase): lane jl gathers level jl, the 35 inputs are exchanged
// by shuffles, the lane evaluates hidden units jl, jl + 16, jl + 32, jl + 48 from the LDS copy of W0 and every lane of the group
// forms the sdf row in geometry_forward's order (j = 0 .. 63, one fmaf chain): a ~10x shorter step than one lane's.
__device__ __forceinline__ float group_sdf(const LevelSet& lv, const FieldC& fc, int bg_sdf, float bg_rad,
                                           const float* __restrict__ table, const float* __restrict__ s_w0,
                                           const float* __restrict__ s_w1, float b1_0, const float p[3], int jl, int gbase) {
    float x[3];
    unit_cube(fc, p, x);
    float y0 = 0.f, y1 = 0.f;
    if (jl < lv.n_levels) gather_level(lv, table, jl, x, y0, y1);
    float u[kInMax];
#pragma unroll
    for (int a = 0; a < 3; ++a) u[a] = p[a] / fc.rescale;
#pragma unroll
    for (int l = 0; l < LS2FM_MAX_LEVELS; ++l) {
        u[3 + 2 * l] = __shfl(y0, gbase + l, 64);
        u[4 + 2 * l] = __shfl(y1, gbase + l, 64);
    }
    float h[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) h[q] = softplus100_value(layer0_preact(s_w0 + (jl + 16 * q) * kW0Stride, u));
    float f0 = b1_0;
#pragma unroll
    for (int q = 0; q < 4; ++q) f0 = row_chain<0>(s_w1 + 16 * q, h[q], f0);
    bool bg;
    return signed_sdf(fc, bg_sdf, bg_rad, f0, p, &bg);
}

__device__ __forceinline__ float lane_bcast(float v, int src) {
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), src));
}

template <int J>
__device__ __forceinline__ float wave_chain(float w1_me, float h, float f) {
    if constexpr (J < kHidden) {
        const float hv = lane_bcast(h, J);
        const float wv = lane_bcast(w1_me, J);
        return wave_chain<J + 1>(w1_me, h, fmaf(wv, hv, f));
    } else {
        return f;
    }
}

// A whole wave: lane j owns hidden unit j with its W0 row | b0 in registers (w) and its sdf-row weight (w1_me), lanes 0-15 gather
// the 16 levels, the 32 encoding values are broadcast as scalars (v_readlane) and the sdf row is the same j = 0 .. 63 fmaf chain
// fed by v_readlane.
__device__ __forceinline__ float wave_sdf(const LevelSet& lv, const FieldC& fc, int bg_sdf, float bg_rad,
                                          const float* __restrict__ table, const float (&w)[kInMax + 1], float w1_me, float b1_0,
                                          const float p[3], int lane) {
    float x[3];
    unit_cube(fc, p, x);
    float y0 = 0.f, y1 = 0.f;
    if (lane < lv.n_levels) gather_level(lv, table, lane, x, y0, y1);
    float u[kInMax];
#pragma unroll
    for (int a = 0; a < 3; ++a) u[a] = p[a] / fc.rescale;
#pragma unroll
    for (int l = 0; l < LS2FM_MAX_LEVELS; ++l) {
        u[3 + 2 * l] = lane_bcast(y0, l);
        u[4 + 2 * l] = lane_bcast(y1, l);
    }
    const float h = softplus100_value(layer0_preact(w, u));
    const float f0 = wave_chain<0>(w1_me, h, b1_0);
    bool bg;
    return signed_sdf(fc, bg_sdf, bg_rad, f0, p, &bg);
}

}  // namespace
