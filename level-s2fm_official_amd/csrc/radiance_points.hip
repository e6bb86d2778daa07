// The radiance field at free points: per point p (and view direction v) exactly what Renderer.forward_composed forms per sample
// (models/Renderer.py:105-117) -- sdf and features of the SDF field, its analytic normal g (not normalised), the Fourier view
// embedding, the second field's features (dual field), and the radiance decoder on [p, g, view, features] -- without a ray, a
// composite or a graph.  ls2fm_radiance_points, behind ls2fm.mesh_colors.field_colors: the colour of a mesh vertex.
//
// Decomposition: ONE LANE PER POINT, two launches.  prep_weights (render_fwd.hip, all three tasks: both geometry MLPs' packed
// records and the collapsed decoder Wc, bc) and then radiance_points_kernel, whose lane runs sdf_eval_kernel<true>'s chain --
// encode_point, geometry_forward<true>, signed_sdf, lane_normal (sdf_point.h / render_common.h) -- so sdf and g carry the bits of
// ls2fm_sdf_eval on the same points, then encode_point + geometry_forward<false> on the second table, and the decoder as one
// fmaf chain per colour channel.  The weights are wave-uniform scalar loads; nothing is staged in LDS and no lane talks to
// another.  What bounds it: at a mesh's vertex count (10^5 .. 10^6 points) the 2 x 128 dependent 8-byte gathers per point,
// which is the regime where ls2fm_sdf_eval itself takes one lane per point; below a few thousand points the launch is one
// lane's latency chain (~3.3 k dependent FMAs per MLP) however few the points.  The transposed MFMA chain of shade_fwd.h reads
// its encodings from rows a gather pass left in HBM; a point evaluator would need that pass and its workspace for a call that
// runs once per extracted mesh.
#include "sdf_point.h"

namespace {

constexpr int kThreads = 256;          // LS2FM_RADIANCE_POINTS_TILE: the points of one workgroup

static_assert(kThreads == LS2FM_RADIANCE_POINTS_TILE, "the header states the tile of points");

template <bool DUAL>
__global__ void __launch_bounds__(kThreads)
radiance_points_kernel(LevelSet lv, LevelSet lv2, FieldC fc, const Packed* __restrict__ pk, const float* __restrict__ table,
                       const float* __restrict__ table2, const float* __restrict__ pts, const float* __restrict__ dirs, int64_t n,
                       float* __restrict__ rgb_out, float* __restrict__ normal_out, float* __restrict__ sdf_out) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const float p[3] = {pts[i * 3], pts[i * 3 + 1], pts[i * 3 + 2]};
    float nrm[3], z[3];
    {   // the SDF field: sdf_eval_kernel<true>'s chain
        float u[kInMax], f[kOut], rr[kInMax];
        encode_point(lv, fc, table, p, u);
        geometry_forward<true>(pk->sdf, u, f, rr);
        bool bg;
        const float sdf = signed_sdf(fc, 0, 0.f, f[0], p, &bg);
        if (sdf_out) sdf_out[i] = sdf;
        lane_normal(lv, fc, table, p, rr, bg, nrm);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            float acc = pk->bc[k];
#pragma unroll
            for (int o = 0; o < LS2FM_FEAT; ++o) acc = fmaf(pk->wc[k][33 + o], f[1 + o], acc);
            z[k] = acc;
        }
    }
    if (DUAL) {
        float u[kInMax], f[kOut], dummy[kInMax];
        encode_point(lv2, fc, table2, p, u);
        geometry_forward<false>(pk->geo, u, f, dummy);
#pragma unroll
        for (int k = 0; k < 3; ++k)
#pragma unroll
            for (int o = 0; o < LS2FM_FEAT; ++o) z[k] = fmaf(pk->wc[k][49 + o], f[1 + o], z[k]);
    }
    float d[3];
    if (dirs) {
        d[0] = dirs[i * 3]; d[1] = dirs[i * 3 + 1]; d[2] = dirs[i * 3 + 2];
    } else {          // the surface seen head-on: -normalize(g), torch.nn.functional.normalize's clamp
        const float len = fmaxf(sqrtf(nrm[0] * nrm[0] + nrm[1] * nrm[1] + nrm[2] * nrm[2]), 1e-12f);
#pragma unroll
        for (int a = 0; a < 3; ++a) d[a] = -(nrm[a] / len);
    }
#pragma unroll
    for (int c = 0; c < kView; ++c) {
        const float e = view_component(d, c);
#pragma unroll
        for (int k = 0; k < 3; ++k) z[k] = fmaf(pk->wc[k][6 + c], e, z[k]);
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
#pragma unroll
        for (int a = 0; a < 3; ++a) z[k] = fmaf(pk->wc[k][a], p[a], z[k]);
#pragma unroll
        for (int a = 0; a < 3; ++a) z[k] = fmaf(pk->wc[k][3 + a], nrm[a], z[k]);
        rgb_out[i * 3 + k] = 1.0f / (1.0f + expf(-z[k]));
    }
    if (normal_out) {
#pragma unroll
        for (int a = 0; a < 3; ++a) normal_out[i * 3 + a] = nrm[a];
    }
}

// what the kernel serves: ls2fm_render_fwd's refusals that concern a point
int points_config(const ls2fm_field_desc* field, const ls2fm_grid_desc* g1, const ls2fm_grid_desc* g2, const ls2fm_params* params) {
    if (!field || !params || !grid_desc_ok(g1) || (field->dual_field && !grid_desc_ok(g2))) return LS2FM_ERR_INVALID_ARGUMENT;
    if (!params->sdf_table || !params->sdf_mlp[0].weight_v || !params->sdf_mlp[1].weight_v || !params->rad_mlp[0].weight_v ||
        !params->rad_mlp[1].weight_v || !params->rad_mlp[2].weight_v || !params->beta)
        return LS2FM_ERR_INVALID_ARGUMENT;
    if (field->dual_field && (!params->rad_table || !params->geo_mlp[0].weight_v || !params->geo_mlp[1].weight_v))
        return LS2FM_ERR_INVALID_ARGUMENT;
    if (field->bg_sdf) return LS2FM_ERR_UNSUPPORTED;          // min(sdf, bg_rad - |p|): the composed form
    return LS2FM_OK;
}

}  // namespace

extern "C" int64_t ls2fm_radiance_points_workspace_bytes(void) { return (int64_t)((sizeof(Packed) + 255) / 256 * 256); }

extern "C" int ls2fm_radiance_points(const ls2fm_field_desc* field, const ls2fm_grid_desc* sdf_grid, const ls2fm_grid_desc* rad_grid,
                                     const ls2fm_params* params, const float* points, const float* view_dirs, int64_t n, float* rgb,
                                     float* normal, float* sdf, void* workspace, void* stream) {
    const int st = points_config(field, sdf_grid, rad_grid, params);
    if (st != LS2FM_OK) return st;
    LS2FM_CHECK_ARG(n >= 0 && n < ((int64_t)1 << 31) * kThreads);
    if (n == 0) return LS2FM_OK;
    LS2FM_CHECK_ARG(points && rgb);
    if (!workspace) return LS2FM_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    const int dual = field->dual_field ? 1 : 0;
    Packed* pk = (Packed*)workspace;
    const int r = ls2fm_launch_prep_render(params, sdf_grid->n_levels, dual ? rad_grid->n_levels : 0, dual, pk, s);
    if (r != LS2FM_OK) return r;
    const FieldC fc = make_field_c(field);
    const unsigned blocks = (unsigned)((n + kThreads - 1) / kThreads);
    if (dual)
        radiance_points_kernel<true><<<blocks, kThreads, 0, s>>>(make_level_set(sdf_grid), make_level_set(rad_grid), fc, pk,
                                                                 params->sdf_table, params->rad_table, points, view_dirs, n, rgb,
                                                                 normal, sdf);
    else
        radiance_points_kernel<false><<<blocks, kThreads, 0, s>>>(make_level_set(sdf_grid), make_level_set(sdf_grid), fc, pk,
                                                                  params->sdf_table, nullptr, points, view_dirs, n, rgb, normal, sdf);
    return ls2fm_launch_status();
}
