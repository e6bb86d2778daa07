// TSDF fusion of posed depth maps into a dense volume (ls2fm_tsdf_integrate): the primitive under ls2fm.fusion.integrate.
// include/ls2fm.h states the FUSION RULE; tests/fusion_restate.py repeats it in numpy.
//
// One lane takes one lattice point and walks the call's views in index order with the point's tsdf and weight in registers: the
// state is loaded once and stored once per call, and a point's running average is one fixed chain of rounded fp32 operations --
// no atomics, and nothing about the launch shows in the bits.  A workgroup takes a brick of kBrickX x kBrickY x kBrickZ points,
// consecutive lanes along axis 2 (the fastest), so a wave's state loads and stores are one 256-byte row.  The view is uniform
// over the wave: its pose and intrinsics are scalar loads.  The camera point, the projection, the usable rule and the pixel are
// the expressions of csrc/raster_project.h, the ones ls2fm_rasterize draws its depth maps with.  A wave whose 64 points all miss
// a view's image (or lie behind its near plane) leaves that view at the branch after the projection.
#include "lattice.h"
#include "ls2fm_device.h"
#include "raster_project.h"

#include <cmath>

namespace {

constexpr int kBrickX = 2, kBrickY = 2, kBrickZ = 64;      // LS2FM_TSDF_BRICK_X / _Y / _Z
constexpr int kThreads = kBrickX * kBrickY * kBrickZ;

static_assert(kBrickX == LS2FM_TSDF_BRICK_X && kBrickY == LS2FM_TSDF_BRICK_Y && kBrickZ == LS2FM_TSDF_BRICK_Z,
              "the header states the brick");
static_assert(kBrickZ == 64, "one wave per row of the brick");

__global__ void __launch_bounds__(kThreads)
tsdf_integrate(float* __restrict__ tsdf, float* __restrict__ weight, int64_t nx, int64_t ny, int64_t nz, int64_t bricks_y,
               int64_t bricks_z, LatticeFrame lat, float trunc, const float* __restrict__ depth, const float* __restrict__ poses,
               const float* __restrict__ intr, const float* __restrict__ view_weight, int n_views, int height, int width, float near,
               float max_depth, float max_weight) {
#pragma clang fp contract(off)
    const int64_t brick = blockIdx.x;
    const int64_t bz = brick % bricks_z, by = (brick / bricks_z) % bricks_y, bx = brick / (bricks_z * bricks_y);
    const int t = threadIdx.x;
    const int64_t iz = bz * kBrickZ + (t % kBrickZ);
    const int64_t iy = by * kBrickY + (t / kBrickZ) % kBrickY;
    const int64_t ix = bx * kBrickX + t / (kBrickZ * kBrickY);
    if (ix >= nx || iy >= ny || iz >= nz) return;
    const int64_t at = (ix * ny + iy) * nz + iz;
    const float x = lattice_coord(ix, lat, 0), y = lattice_coord(iy, lat, 1), z = lattice_coord(iz, lat, 2);
    float T = tsdf[at], W = weight[at];
    const int64_t hw = (int64_t)height * width;
    for (int view = 0; view < n_views; ++view) {
        const float w = view_weight ? view_weight[view] : 1.0f;
        if (!(w > 0.0f)) continue;                                   // wave-uniform; false for a NaN
        const View cam = load_view(poses, intr, view);
        const Projected p = project(cam, x, y, z, near);
        int px, py;
        if (!pixel_of(p, height, width, px, py)) continue;
        const float d = depth[(int64_t)view * hw + (int64_t)py * width + px];
        if (!(fabsf(d) < INFINITY && d > 0.0f && d <= max_depth)) continue;
        const float s = __fsub_rn(d, p.z);
        if (s < -trunc) continue;
        const float val = fminf(1.0f, __fdiv_rn(s, trunc));
        const float Wn = __fadd_rn(W, w);
        T = __fdiv_rn(__fadd_rn(__fmul_rn(W, T), __fmul_rn(w, val)), Wn);
        W = fminf(Wn, max_weight);
    }
    tsdf[at] = T;
    weight[at] = W;
}

}  // namespace

extern "C" int ls2fm_tsdf_integrate(float* tsdf, float* weight, int64_t nx, int64_t ny, int64_t nz, const float* origin, float voxel,
                                    float trunc, const float* depth, const float* poses, const float* intr, const float* view_weight,
                                    int32_t n_views, int32_t height, int32_t width, float near, float max_depth, float max_weight,
                                    void* stream) {
    LS2FM_CHECK_ARG(lattice_ok(nx, ny, nz, 0, voxel) && raster_image_ok(n_views, height, width) && raster_near_ok(near) &&
                    trunc > 0.0f && trunc < INFINITY && max_depth > 0.0f && max_weight > 0.0f);
    if (nx == 0 || ny == 0 || nz == 0 || n_views == 0) return LS2FM_OK;
    const int64_t bricks_x = (nx + kBrickX - 1) / kBrickX, bricks_y = (ny + kBrickY - 1) / kBrickY, bricks_z = (nz + kBrickZ - 1) / kBrickZ;
    // the three factors are at most 2^23 each: the products below stay in int64
    LS2FM_CHECK_ARG(bricks_x * bricks_y < ((int64_t)1 << 31) && bricks_x * bricks_y * bricks_z < ((int64_t)1 << 31));
    LatticeFrame lat;
    LS2FM_CHECK_ARG(tsdf && weight && depth && poses && intr && lattice_frame(origin, voxel, &lat));
    tsdf_integrate<<<(unsigned)(bricks_x * bricks_y * bricks_z), kThreads, 0, (hipStream_t)stream>>>(
        tsdf, weight, nx, ny, nz, bricks_y, bricks_z, lat, trunc, depth, poses, intr, view_weight, n_views, height, width, near, max_depth,
        max_weight);
    return ls2fm_launch_status();
}
