// Fusion of per-view depth and normal maps into one oriented, coloured cloud (ls2fm_mvs_fuse_mark, ls2fm_mvs_fuse_emit): the
// primitives under ls2fm.mvs.fuse_depths.  include/ls2fm.h states THE FUSION RULE; tests/fuse_restate.py repeats it in numpy,
// ls2fm.mvs.fuse_depths_torch as torch ops.
//
// Two launches with the caller's prefix sum between them, the pattern of csrc/mesh_simplify.hip: `mark` walks every pixel's
// partners (steps 1 and 2 of the rule) and writes its support; `emit` repeats the walk of the pixels with support > 0, this time
// summing the contributors, and writes the pixel's row.  The walk is written once, walk(); what a consistent partner adds is the
// one thing the two kernels differ in.  One lane per pixel; a workgroup is a tile of kTileW x kTileH = 32 x 8 pixels of one view,
// so the view, its source list and the pair poses are uniform (scalar loads through load_pair, as in mvs_filter) and a wave, two
// rows of 32 pixels, finds its dependent gathers of the partners' depth, normal and colour in few cache lines: measured against
// 16 x 16, 64 x 4, 8 x 32 and mvs_filter's linear run of 256 pixels, the fastest of the five for the two launches together
// (tools/time_fuse.py, profiles/fuse_time.json).  No atomics, no workspace, no LDS, nothing read back.
#include "mvs_sample.h"

namespace {

constexpr int kThreads = 256;
#ifdef LS2FM_MVS_FUSE_AB_TILE_W    // a variant build of tools/time_fuse.py (tools/build_variant.sh): another tile, 256 x 1 is a linear run
constexpr int kTileW = LS2FM_MVS_FUSE_AB_TILE_W, kTileH = kThreads / kTileW;
#else
constexpr int kTileW = LS2FM_MVS_FUSE_TILE_W, kTileH = LS2FM_MVS_FUSE_TILE_H;
#endif
constexpr int kChannels = LS2FM_MVS_FUSE_MAX_CHANNELS;

static_assert(kTileW * kTileH == kThreads, "one lane per pixel of the tile");

// the maps and settings both kernels take
struct Maps {
    const float* depth;
    const float* normal;           // NULL: no normal test
    const int32_t* sources;
    const float* rel;
    const float* rel_back;
    const float* intr;
    int n_views, height, width, n_sources;
    float near, max_reproj, rel_depth, cos2;
};

// the camera point of a pixel centre at depth d: step 1 (and 5) of THE CONSISTENCY RULE
__device__ __forceinline__ void lift(float fx, float fy, float cx, float cy, int px, int py, float d, float& uc, float& vc, float& X, float& Y) {
#pragma clang fp contract(off)
    uc = __fadd_rn((float)px, 0.5f);
    vc = __fadd_rn((float)py, 0.5f);
    X = __fmul_rn(__fdiv_rn(__fsub_rn(uc, cx), fx), d);
    Y = __fmul_rn(__fdiv_rn(__fsub_rn(vc, cy), fy), d);
}

__device__ __forceinline__ float dot3(float ax, float ay, float az, float bx, float by, float bz) {
#pragma clang fp contract(off)
    return __fadd_rn(__fadd_rn(__fmul_rn(ax, bx), __fmul_rn(ay, by)), __fmul_rn(az, bz));
}

// Steps 1 and 2 of THE FUSION RULE for the pixel (px, py) of view r, whose depth d is finite and positive: add(sv, at, Xs, Ys, ds)
// is called for every consistent partner in source order -- the pixel `at` of view sv, its camera point (Xs, Ys, ds).  -> support
template <class Add>
__device__ __forceinline__ int walk(const Maps& m, int r, int px, int py, float d, Add&& add) {
#pragma clang fp contract(off)
    const int64_t hw = (int64_t)m.height * m.width;
    const float* k = m.intr + (int64_t)r * 4;
    float uc, vc, X, Y;
    lift(k[0], k[1], k[2], k[3], px, py, d, uc, vc, X, Y);
    const float reproj2 = __fmul_rn(m.max_reproj, m.max_reproj), dz = __fmul_rn(m.rel_depth, d);
    float nx = 0.0f, ny = 0.0f, nz = 0.0f, rr = 0.0f;
    if (m.normal) {
        const float* n = m.normal + ((int64_t)r * hw + (int64_t)py * m.width + px) * 3;
        nx = n[0]; ny = n[1]; nz = n[2];
        rr = dot3(nx, ny, nz, nx, ny, nz);
    }
    int count = 0;
    bool owner = true;
    for (int s = 0; s < m.n_sources; ++s) {
        const int sv = m.sources[(int64_t)r * m.n_sources + s];
        if (sv < 0 || sv >= m.n_views || sv == r) continue;          // uniform over the workgroup
        const int64_t pair = (int64_t)r * m.n_sources + s;
        const View there = load_pair(m.rel, pair, m.intr, sv);
        const Projected p = project(there, X, Y, d, m.near);
        int sx, sy;
        if (!pixel_of(p, m.height, m.width, sx, sy)) continue;
        const int64_t at = (int64_t)sy * m.width + sx;
        const float ds = m.depth[(int64_t)sv * hw + at];
        if (!(fabsf(ds) < INFINITY && ds > 0.0f)) continue;
        float us, vs, Xs, Ys;
        lift(there.fx, there.fy, there.cx, there.cy, sx, sy, ds, us, vs, Xs, Ys);
        const View back = load_pair(m.rel_back, pair, m.intr, r);
        const Projected q = project(back, Xs, Ys, ds, m.near);
        const float du = __fsub_rn(q.u, uc), dv = __fsub_rn(q.v, vc);
        const float e = __fadd_rn(__fmul_rn(du, du), __fmul_rn(dv, dv));
        if (!(q.usable && e <= reproj2 && fabsf(__fsub_rn(q.z, d)) <= dz)) continue;
        if (m.normal) {
            const float* n = m.normal + ((int64_t)sv * hw + at) * 3;
            const float sx_ = n[0], sy_ = n[1], sz_ = n[2];
            const float tx = dot3(back.p[0], back.p[1], back.p[2], sx_, sy_, sz_);
            const float ty = dot3(back.p[4], back.p[5], back.p[6], sx_, sy_, sz_);
            const float tz = dot3(back.p[8], back.p[9], back.p[10], sx_, sy_, sz_);
            const float a = dot3(nx, ny, nz, tx, ty, tz);
            const float ss = dot3(tx, ty, tz, tx, ty, tz);
            if (!(a > 0.0f && __fmul_rn(a, a) >= __fmul_rn(m.cos2, __fmul_rn(rr, ss)))) continue;
        }
        ++count;
        owner = owner && sv > r;
        add(sv, at, Xs, Ys, ds);
    }
    return owner ? 1 + count : 0;
}

// the pixel of this lane: a workgroup is one tile of one view
__device__ __forceinline__ bool lane_pixel(int tiles_x, int tiles_y, int width, int height, int& view, int& px, int& py) {
    const int tile = blockIdx.x, t = threadIdx.x;
    view = tile / (tiles_x * tiles_y);
    px = (tile % tiles_x) * kTileW + t % kTileW;
    py = ((tile / tiles_x) % tiles_y) * kTileH + t / kTileW;
    return px < width && py < height;
}

__global__ void __launch_bounds__(kThreads)
mvs_fuse_mark(const Maps m, int view_begin, int tiles_x, int tiles_y, uint8_t* __restrict__ support) {
    int view, px, py;
    if (!lane_pixel(tiles_x, tiles_y, m.width, m.height, view, px, py)) return;
    const int r = view_begin + view;
    const int64_t at = ((int64_t)r * m.height + py) * m.width + px;
    const float d = m.depth[at];
    int count = 0;
    if (fabsf(d) < INFINITY && d > 0.0f) count = walk(m, r, px, py, d, [](int, int64_t, float, float, float) {});
    support[at] = (uint8_t)count;
}

// the running sums of one row, in fp64
struct Sums {
    double p[3], n[3], c[kChannels];
};

// one contributor: the pixel `at` of view v with the camera point (X, Y, d)
__device__ __forceinline__ void contribute(Sums& sum, const Maps& m, const float* __restrict__ colour, int n_channels,
                                           const float* __restrict__ cam_to_world, int v, int64_t at, float X, float Y, float d) {
#pragma clang fp contract(off)
    const int64_t hw = (int64_t)m.height * m.width;
    const float* w = cam_to_world + (int64_t)v * 12;                  // uniform: scalar loads
    const double x = (double)X, y = (double)Y, z = (double)d;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const double wi = __dadd_rn(__dadd_rn(__dadd_rn(__dmul_rn((double)w[4 * i], x), __dmul_rn((double)w[4 * i + 1], y)),
                                              __dmul_rn((double)w[4 * i + 2], z)), (double)w[4 * i + 3]);
        sum.p[i] = __dadd_rn(sum.p[i], wi);
    }
    if (m.normal) {
        const float* n = m.normal + ((int64_t)v * hw + at) * 3;
        const double a = (double)n[0], b = (double)n[1], c = (double)n[2];
        double g[3];
#pragma unroll
        for (int i = 0; i < 3; ++i)
            g[i] = __dadd_rn(__dadd_rn(__dmul_rn((double)w[4 * i], a), __dmul_rn((double)w[4 * i + 1], b)), __dmul_rn((double)w[4 * i + 2], c));
        const double l = __dsqrt_rn(__dadd_rn(__dadd_rn(__dmul_rn(g[0], g[0]), __dmul_rn(g[1], g[1])), __dmul_rn(g[2], g[2])));
#pragma unroll
        for (int i = 0; i < 3; ++i) sum.n[i] = __dadd_rn(sum.n[i], __ddiv_rn(g[i], l));
    }
    if (colour) {
        const float* c = colour + ((int64_t)v * hw + at) * n_channels;
#pragma unroll
        for (int i = 0; i < kChannels; ++i)
            if (i < n_channels) sum.c[i] = __dadd_rn(sum.c[i], (double)c[i]);
    }
}

__global__ void __launch_bounds__(kThreads)
mvs_fuse_emit(const Maps m, const float* __restrict__ colour, int n_channels, const float* __restrict__ cam_to_world, int view_begin,
              int tiles_x, int tiles_y, const uint8_t* __restrict__ support, const int64_t* __restrict__ row, int64_t n_rows,
              float* __restrict__ points, float* __restrict__ normals, float* __restrict__ colours, int64_t* __restrict__ pixel) {
#pragma clang fp contract(off)
    int view, px, py;
    if (!lane_pixel(tiles_x, tiles_y, m.width, m.height, view, px, py)) return;
    const int r = view_begin + view;
    const int64_t in_view = (int64_t)py * m.width + px;
    const int64_t at = (int64_t)r * m.height * m.width + in_view;
    const int have = support[at];
    if (have == 0) return;
    const int64_t out = row[(int64_t)view * m.height * m.width + in_view];
    if (out < 0 || out >= n_rows) return;
    const float d = m.depth[at];
    const float* k = m.intr + (int64_t)r * 4;
    float uc, vc, X, Y;
    lift(k[0], k[1], k[2], k[3], px, py, d, uc, vc, X, Y);
    Sums sum;
#pragma unroll
    for (int i = 0; i < 3; ++i) sum.p[i] = sum.n[i] = 0.0;
#pragma unroll
    for (int i = 0; i < kChannels; ++i) sum.c[i] = 0.0;
    contribute(sum, m, colour, n_channels, cam_to_world, r, in_view, X, Y, d);
    const int found = walk(m, r, px, py, d, [&](int sv, int64_t there, float Xs, float Ys, float ds) {
        contribute(sum, m, colour, n_channels, cam_to_world, sv, there, Xs, Ys, ds);
    });
    const double n = (double)found;                                   // = support: the walk is the one `mark` ran
#pragma unroll
    for (int i = 0; i < 3; ++i) points[out * 3 + i] = (float)__ddiv_rn(sum.p[i], n);
    if (m.normal) {
        const double l = __dsqrt_rn(__dadd_rn(__dadd_rn(__dmul_rn(sum.n[0], sum.n[0]), __dmul_rn(sum.n[1], sum.n[1])), __dmul_rn(sum.n[2], sum.n[2])));
#pragma unroll
        for (int i = 0; i < 3; ++i) normals[out * 3 + i] = (float)__ddiv_rn(sum.n[i], l);
    }
    if (colour) {
#pragma unroll
        for (int i = 0; i < kChannels; ++i)
            if (i < n_channels) colours[out * n_channels + i] = (float)__ddiv_rn(sum.c[i], n);
    }
    pixel[out] = at;
}

// what both entry points refuse of the arguments they share; -> the workgroups of the range, or -1
int64_t fuse_workgroups(int32_t n_views, int32_t height, int32_t width, int32_t n_sources, float near, float max_reproj, float rel_depth,
                        float cos2, int32_t view_begin, int32_t view_end, int64_t& tiles_x, int64_t& tiles_y) {
    if (!(raster_image_ok(n_views, height, width) && raster_near_ok(near) && n_sources >= 1 && n_sources <= LS2FM_MVS_MAX_SOURCES &&
          finite_not_negative(max_reproj) && finite_not_negative(rel_depth) && cos2 >= 0.0f && cos2 <= 1.0f && view_begin >= 0 &&
          view_begin <= view_end && view_end <= n_views))
        return -1;
    tiles_x = (width + kTileW - 1) / kTileW;
    tiles_y = (height + kTileH - 1) / kTileH;
    const int64_t groups = tiles_x * tiles_y * (view_end - view_begin);
    return groups < ((int64_t)1 << 31) ? groups : -1;
}

}  // namespace

extern "C" int ls2fm_mvs_fuse_mark(const float* depth, const float* normal, int32_t n_views, int32_t height, int32_t width,
                                   const int32_t* sources, int32_t n_sources, const float* rel, const float* rel_back, const float* intr,
                                   float near, float max_reproj, float rel_depth, float cos2, int32_t view_begin, int32_t view_end,
                                   uint8_t* support, void* stream) {
    int64_t tiles_x = 0, tiles_y = 0;
    const int64_t groups = fuse_workgroups(n_views, height, width, n_sources, near, max_reproj, rel_depth, cos2, view_begin, view_end,
                                           tiles_x, tiles_y);
    LS2FM_CHECK_ARG(groups >= 0);
    if (groups == 0) return LS2FM_OK;
    LS2FM_CHECK_ARG(depth && sources && rel && rel_back && intr && support);
    const Maps m = {depth, normal, sources, rel, rel_back, intr, n_views, height, width, n_sources, near, max_reproj, rel_depth, cos2};
    mvs_fuse_mark<<<(unsigned)groups, kThreads, 0, (hipStream_t)stream>>>(m, view_begin, (int)tiles_x, (int)tiles_y, support);
    return ls2fm_launch_status();
}

extern "C" int ls2fm_mvs_fuse_emit(const float* depth, const float* normal, const float* colour, int32_t n_channels, int32_t n_views,
                                   int32_t height, int32_t width, const int32_t* sources, int32_t n_sources, const float* rel,
                                   const float* rel_back, const float* intr, const float* cam_to_world, float near, float max_reproj,
                                   float rel_depth, float cos2, int32_t view_begin, int32_t view_end, const uint8_t* support,
                                   const int64_t* row, int64_t n_rows, float* points, float* normals, float* colours, int64_t* pixel,
                                   void* stream) {
    int64_t tiles_x = 0, tiles_y = 0;
    const int64_t groups = fuse_workgroups(n_views, height, width, n_sources, near, max_reproj, rel_depth, cos2, view_begin, view_end,
                                           tiles_x, tiles_y);
    LS2FM_CHECK_ARG(groups >= 0 && n_rows >= 0);
    LS2FM_CHECK_ARG(colour ? n_channels >= 1 && n_channels <= kChannels : n_channels == 0);
    LS2FM_CHECK_ARG((normal != nullptr) == (normals != nullptr) && (colour != nullptr) == (colours != nullptr));
    if (groups == 0 || n_rows == 0) return LS2FM_OK;
    LS2FM_CHECK_ARG(depth && sources && rel && rel_back && intr && cam_to_world && support && row && points && pixel);
    const Maps m = {depth, normal, sources, rel, rel_back, intr, n_views, height, width, n_sources, near, max_reproj, rel_depth, cos2};
    mvs_fuse_emit<<<(unsigned)groups, kThreads, 0, (hipStream_t)stream>>>(m, colour, n_channels, cam_to_world, view_begin, (int)tiles_x,
                                                                          (int)tiles_y, support, row, n_rows, points, normals, colours, pixel);
    return ls2fm_launch_status();
}
