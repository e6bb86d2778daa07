// One observation of the re-projection term: a point x[3] through a world-to-camera pose [3][4] and the 3 x 3 K against its key point
// uv_obs[2] (sdf: the point's SDF value for the on-surface mask, or null).  Shared by the BA re-projection term (reproject.hip) and
// the classical bundle adjustment (bundle_adjust.hip), so both round alike:
//      x_c = R x + t ;  u = K x_c ;  uv = u_xy / (u_z + 1e-6) ;  err = || uv - key point ||
#pragma once

#include "ls2fm_device.h"

namespace {

struct Camera3 { float k[9]; };

struct Obs {                       // forward quantities of one observation
    float xc[3], u[3], e[2], err, inv;
    bool on;
};

__device__ __forceinline__ Obs project(const float* __restrict__ x, const float* __restrict__ pose, const Camera3& K,
                                       const float* __restrict__ uv_obs, const float* __restrict__ sdf, float bound) {
    Obs o;
#pragma unroll
    for (int a = 0; a < 3; ++a)
        o.xc[a] = fmaf(pose[4 * a + 2], x[2], fmaf(pose[4 * a + 1], x[1], pose[4 * a] * x[0])) + pose[4 * a + 3];
#pragma unroll
    for (int a = 0; a < 3; ++a) o.u[a] = fmaf(K.k[3 * a + 2], o.xc[2], fmaf(K.k[3 * a + 1], o.xc[1], K.k[3 * a] * o.xc[0]));
    o.inv = 1.0f / (o.u[2] + 1e-6f);
    const float uv0 = o.u[0] * o.inv, uv1 = o.u[1] * o.inv;
    o.e[0] = uv0 - uv_obs[0];
    o.e[1] = uv1 - uv_obs[1];
    o.err = sqrtf(fmaf(o.e[1], o.e[1], o.e[0] * o.e[0]));
    o.on = (sdf == nullptr || fabsf(sdf[0]) < bound) && !isinf(uv0) && !isinf(uv1);
    return o;
}

bool load_intrinsic(const float* host_k, Camera3* out) {
    if (!host_k) return false;
    for (int q = 0; q < 9; ++q) out->k[q] = host_k[q];
    return true;
}

}  // namespace
