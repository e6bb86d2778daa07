// Vertex colours of a mesh from photographs: a per-vertex blend of the views that see the vertex, with a z-test against the
// rasteriser's depth maps of that same mesh (ls2fm_mesh_vertex_colors, ls2fm_mesh_vertex_colors_finish): the primitives under
// ls2fm.mesh_colors.photo_colors.  include/ls2fm.h states the VERTEX COLOUR RULE; tests/mesh_colors_restate.py repeats it in numpy.
//
// One lane takes one vertex and walks the views in index order, so a vertex's sums are one fixed chain of fp64 additions: no
// atomics, and nothing about the launch shows in the bits.  The running sums live in caller-owned state that the kernel loads,
// extends and stores, so views may arrive in chunks (one rasterisation per chunk) and give the bits of one call.  The view is
// uniform over the wave: its pose and intrinsics are scalar loads.  The pixel, the camera point and the usable rule are the
// expressions of csrc/raster_project.h, the ones the depth maps were drawn with.
#include "ls2fm_device.h"
#include "raster_project.h"

#include <cmath>

namespace {

constexpr int kThreads = 256;          // LS2FM_MESH_COLORS_THREADS

static_assert(kThreads == LS2FM_MESH_COLORS_THREADS, "the header states the workgroup size");

// one bilinear tap pair along x, then the blend along y: every operation one rounded fp64 operation
__device__ __forceinline__ double lerp(double a, double b, double t) {
#pragma clang fp contract(off)
    return __dadd_rn(a, __dmul_rn(t, __dsub_rn(b, a)));
}

template <int C>
__global__ void __launch_bounds__(kThreads)
vertex_colors(const float* __restrict__ verts, const float* __restrict__ normals, int64_t n_verts, const float* __restrict__ poses,
              const float* __restrict__ intr, int n_views, int height, int width, float near, const float* __restrict__ images,
              const float* __restrict__ depth, const uint8_t* __restrict__ masks, float depth_tol, int power,
              double* __restrict__ sums, int32_t* __restrict__ count) {
#pragma clang fp contract(off)
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n_verts) return;
    const float x = verts[3 * i], y = verts[3 * i + 1], z = verts[3 * i + 2];
    double n[3] = {0.0, 0.0, 0.0};
    if (normals) {
        n[0] = (double)normals[3 * i]; n[1] = (double)normals[3 * i + 1]; n[2] = (double)normals[3 * i + 2];
    }
    double acc[C + 1];
#pragma unroll
    for (int c = 0; c <= C; ++c) acc[c] = sums[(C + 1) * i + c];
    int seen = count[i];
    const int64_t hw = (int64_t)height * width;
    for (int view = 0; view < n_views; ++view) {
        const View w = load_view(poses, intr, view);
        const Projected p = project(w, x, y, z, near);
        int px, py;
        if (!pixel_of(p, height, width, px, py)) continue;
        const int64_t at = (int64_t)view * hw + (int64_t)py * width + px;
        if (masks && masks[at] == 0) continue;
        // visible: c_z <= d + depth_tol d in fp32; an empty pixel (+inf) and a NaN depth fail
        const float d = depth[at];
        if (!(fabsf(d) < INFINITY && p.z <= __fadd_rn(d, __fmul_rn(depth_tol, d)))) continue;
        double wt = 1.0;
        if (normals) {
            const double cx = (double)p.x, cy = (double)p.y, cz = (double)p.z;
            double m[3];
#pragma unroll
            for (int r = 0; r < 3; ++r)
                m[r] = __dadd_rn(__dadd_rn(__dmul_rn((double)w.p[4 * r], n[0]), __dmul_rn((double)w.p[4 * r + 1], n[1])),
                                 __dmul_rn((double)w.p[4 * r + 2], n[2]));
            const double dot = __dadd_rn(__dadd_rn(__dmul_rn(m[0], cx), __dmul_rn(m[1], cy)), __dmul_rn(m[2], cz));
            const double mm = __dsqrt_rn(__dadd_rn(__dadd_rn(__dmul_rn(m[0], m[0]), __dmul_rn(m[1], m[1])), __dmul_rn(m[2], m[2])));
            const double cc = __dsqrt_rn(__dadd_rn(__dadd_rn(__dmul_rn(cx, cx), __dmul_rn(cy, cy)), __dmul_rn(cz, cz)));
            const double cosine = __ddiv_rn(-dot, __dmul_rn(mm, cc));
            if (!(cosine > 0.0 && cosine < (double)INFINITY)) continue;
            for (int k = 0; k < power; ++k) wt = __dmul_rn(wt, cosine);
        }
        // bilinear sample about the pixel centres, the four taps clamped to the image
        const double sx = __dsub_rn((double)p.u, 0.5), sy = __dsub_rn((double)p.v, 0.5);
        const double fx0 = floor(sx), fy0 = floor(sy);
        const double tx = __dsub_rn(sx, fx0), ty = __dsub_rn(sy, fy0);
        const int x0 = min(max((int)fx0, 0), width - 1), x1 = min(max((int)fx0 + 1, 0), width - 1);
        const int y0 = min(max((int)fy0, 0), height - 1), y1 = min(max((int)fy0 + 1, 0), height - 1);
        const float* img = images + (int64_t)view * hw * C;
        const float* q00 = img + ((int64_t)y0 * width + x0) * C;
        const float* q10 = img + ((int64_t)y0 * width + x1) * C;
        const float* q01 = img + ((int64_t)y1 * width + x0) * C;
        const float* q11 = img + ((int64_t)y1 * width + x1) * C;
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const double r0 = lerp((double)q00[c], (double)q10[c], tx);
            const double r1 = lerp((double)q01[c], (double)q11[c], tx);
            acc[c] = __dadd_rn(acc[c], __dmul_rn(wt, lerp(r0, r1, ty)));
        }
        acc[C] = __dadd_rn(acc[C], wt);
        ++seen;
    }
#pragma unroll
    for (int c = 0; c <= C; ++c) sums[(C + 1) * i + c] = acc[c];
    count[i] = seen;
}

struct Fill { float c[4]; };

__global__ void __launch_bounds__(kThreads)
vertex_colors_finish(const double* __restrict__ sums, const int32_t* __restrict__ count, int64_t n_verts, int channels,
                     const float* __restrict__ fallback, Fill fill, float* __restrict__ color) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n_verts) return;
    const bool seen = count[i] > 0;
    const double total = sums[(channels + 1) * i + channels];
    for (int c = 0; c < channels; ++c) {
        float v = fill.c[c];
        if (seen) v = (float)__ddiv_rn(sums[(channels + 1) * i + c], total);
        else if (fallback) v = fallback[channels * i + c];
        color[channels * i + c] = v;
    }
}

bool verts_ok(int64_t n_verts) { return n_verts >= 0 && n_verts < ((int64_t)1 << 31) * kThreads; }

}  // namespace

extern "C" int ls2fm_mesh_vertex_colors(const float* verts, const float* normals, int64_t n_verts, const float* poses,
                                        const float* intr, int32_t n_views, int32_t height, int32_t width, int32_t channels,
                                        const float* images, const float* depth, const uint8_t* masks, float near, float depth_tol,
                                        int32_t power, double* sums, int32_t* count, void* stream) {
    LS2FM_CHECK_ARG(verts_ok(n_verts) && raster_image_ok(n_views, height, width) && raster_near_ok(near) && channels >= 1 &&
                    channels <= 4 && power >= 0 && power <= 8 && depth_tol >= 0.0f && depth_tol < INFINITY);
    if (n_verts == 0 || n_views == 0) return LS2FM_OK;
    LS2FM_CHECK_ARG(verts && poses && intr && images && depth && sums && count);
    const unsigned blocks = (unsigned)((n_verts + kThreads - 1) / kThreads);
    hipStream_t s = (hipStream_t)stream;
#define LS2FM_COLORS_LAUNCH(C)                                                                                                    \
    vertex_colors<C><<<blocks, kThreads, 0, s>>>(verts, normals, n_verts, poses, intr, n_views, height, width, near, images, depth, \
                                                 masks, depth_tol, power, sums, count)
    switch (channels) {
        case 1: LS2FM_COLORS_LAUNCH(1); break;
        case 2: LS2FM_COLORS_LAUNCH(2); break;
        case 3: LS2FM_COLORS_LAUNCH(3); break;
        default: LS2FM_COLORS_LAUNCH(4); break;
    }
#undef LS2FM_COLORS_LAUNCH
    return ls2fm_launch_status();
}

extern "C" int ls2fm_mesh_vertex_colors_finish(const double* sums, const int32_t* count, int64_t n_verts, int32_t channels,
                                               const float* fallback, const float* fill, float* color, void* stream) {
    LS2FM_CHECK_ARG(verts_ok(n_verts) && channels >= 1 && channels <= 4);
    if (n_verts == 0) return LS2FM_OK;
    LS2FM_CHECK_ARG(sums && count && color && (fallback || fill));
    Fill f = {{0.0f, 0.0f, 0.0f, 0.0f}};
    if (fill)
        for (int c = 0; c < channels; ++c) f.c[c] = fill[c];          // on the host: `channels` floats, read before the call returns
    vertex_colors_finish<<<(unsigned)((n_verts + kThreads - 1) / kThreads), kThreads, 0, (hipStream_t)stream>>>(
        sums, count, n_verts, channels, fallback, f, color);
    return ls2fm_launch_status();
}
