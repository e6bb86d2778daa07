// A view's pose and intrinsics, and the camera point / projection / usable / in-the-image part of the RASTERISATION RULE of
// include/ls2fm.h, stated once for csrc/rasterize.hip (faces, mask votes) and csrc/mesh_colors.hip (vertex colours): a vertex
// lands on the same pixel in all of them because they run these very expressions.
#pragma once

#include "ls2fm_device.h"

// pose rows and intrinsics of one view.  The view index is uniform over the wave wherever this is called, so these are scalar
// loads into scalar registers.
struct View {
    float p[12];
    float fx, fy, cx, cy;
};

__device__ __forceinline__ View load_view(const float* __restrict__ poses, const float* __restrict__ intr, int view) {
    View w;
    const float* p = poses + (int64_t)view * 12;
#pragma unroll
    for (int k = 0; k < 12; ++k) w.p[k] = p[k];
    const float* q = intr + (int64_t)view * 4;
    w.fx = q[0]; w.fy = q[1]; w.cx = q[2]; w.cy = q[3];
    return w;
}

struct Projected {
    float x, y, z;         // the camera point
    float u, v;            // the image point
    bool usable;
};

// camera point, projection and the usable rule.  Spelled with the rounded-operation intrinsics and compiled with contraction
// off for this function, so the result does not depend on the build's -ffp-contract flag.
__device__ __forceinline__ Projected project(const View& w, float x, float y, float z, float near) {
#pragma clang fp contract(off)
    float c[3];
#pragma unroll
    for (int r = 0; r < 3; ++r)
        c[r] = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(w.p[4 * r], x), __fmul_rn(w.p[4 * r + 1], y)), __fmul_rn(w.p[4 * r + 2], z)),
                         w.p[4 * r + 3]);
    Projected o;
    o.x = c[0]; o.y = c[1]; o.z = c[2];
    o.u = __fadd_rn(__fmul_rn(w.fx, __fdiv_rn(c[0], c[2])), w.cx);
    o.v = __fadd_rn(__fmul_rn(w.fy, __fdiv_rn(c[1], c[2])), w.cy);
    // every comparison is false for a NaN; c_z = +inf fails the first
    o.usable = fabsf(c[2]) < INFINITY && c[2] >= near && fabsf(o.u) <= 65536.0f && fabsf(o.v) <= 65536.0f;
    return o;
}

// IN THE IMAGE: usable, 0 <= u < width and 0 <= v < height as fp32 comparisons; the pixel is (floor(u), floor(v)).  width and
// height are at most 32768, so their fp32 values are exact, and 0 <= u < width gives floor(u) in [0, width - 1]; v likewise.
__device__ __forceinline__ bool pixel_of(const Projected& p, int height, int width, int& px, int& py) {
    if (!(p.usable && p.u >= 0.0f && p.u < (float)width && p.v >= 0.0f && p.v < (float)height)) return false;
    px = (int)floorf(p.u);
    py = (int)floorf(p.v);
    return true;
}

static inline bool raster_image_ok(int32_t n_views, int32_t height, int32_t width) {
    return n_views >= 0 && height >= 1 && height <= 32768 && width >= 1 && width <= 32768 &&
           (int64_t)n_views * height * width < ((int64_t)1 << 40);
}

static inline bool raster_near_ok(float near) { return near > 0.0f && near < INFINITY; }
