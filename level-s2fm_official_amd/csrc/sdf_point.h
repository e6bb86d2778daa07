// Point evaluation shared by the tracing kernels of sdf_eval.hip and trace_image.hip: the hash encoding of a world point and
// the signed SDF (SDF.infer_sdf, models/SDF.py:55-78).  Both files compile it to the same instructions.
#pragma once

#include "render_common.h"

namespace {

// hash-encode a world point into u[35] = [p / rescale, e(x)]
__device__ __forceinline__ void encode_point(const LevelSet& lv, const FieldC& fc, const float* __restrict__ table,
                                             const float p[3], float (&u)[kInMax]) {
    float x[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        x[a] = (p[a] - fc.bmin[a]) / (fc.bmax[a] - fc.bmin[a]);
        u[a] = p[a] / fc.rescale;
    }
#pragma unroll
    for (int l = 0; l < LS2FM_MAX_LEVELS; ++l) {
        float y0 = 0.f, y1 = 0.f;
        if (l < lv.n_levels) {
            Cell c;
            locate(x, lv.scale[l], lv.res[l], lv.size[l], lv.offset[l], lv.hashed[l], c);
            float2 v[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) v[k] = *reinterpret_cast<const float2*>(table + 2ull * c.idx[k]);
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const float wt = corner_weight(c.w, k);
                y0 = fmaf(wt, v[k].x, y0);
                y1 = fmaf(wt, v[k].y, y1);
            }
        }
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

}  // namespace
