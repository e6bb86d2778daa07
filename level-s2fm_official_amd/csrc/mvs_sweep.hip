// Plane-sweep multi-view stereo (ls2fm_mvs_sweep) and the geometric-consistency filter of its depth maps (ls2fm_mvs_filter): the
// primitives under ls2fm.mvs.plane_sweep and ls2fm.mvs.filter_depths.  include/ls2fm.h states THE SWEEP RULE and THE CONSISTENCY
// RULE; tests/mvs_restate.py repeats both in numpy, ls2fm.mvs.plane_sweep_torch / filter_depths_torch as torch ops.
//
// Sweep: one workgroup of 256 lanes takes one (reference, 16 x 16 tile).  The reference tile with its halo of w pixels goes to LDS
// once, and every pixel's window mean and variance are formed once, before the plane and source loops.  Per (plane, source) the
// lanes share out the (16 + 2 w)^2 halo pixels: each warps its pixels onto the plane, projects them into the source
// (csrc/raster_project.h, unchanged) and samples it bilinearly (csrc/mvs_sample.h, the one statement csrc/mvs_patchmatch.hip
// uses too) into LDS -- a warped sample is formed once per tile, not once per window that holds it.  After a barrier every lane
// runs its own window from LDS.  A sample that is invalid or not finite is stored as NaN: a window's sum in tap order is NaN
// exactly when one of its taps is (finite taps can overflow to an infinity, never to a NaN), so "any tap invalid" costs one
// comparison per window.  The LDS rows are kRow = 48 floats apart: a 32-lane half of a wave reads two tile rows of 16 consecutive
// floats, and 48 = 16 mod 32 puts them on disjoint banks.  The running best score, the scores before and after it and its plane
// stay in registers over the planes.  The pose P_rs, the intrinsics and the plane depth are uniform over the workgroup: scalar
// loads.  No atomics, no workspace, nothing read back.
#include "mvs_sample.h"

namespace {

constexpr int kTile = 16;                  // LS2FM_MVS_TILE
constexpr int kThreads = kTile * kTile;
constexpr int kRow = 48;                   // floats between LDS rows: >= kTile + 2 * LS2FM_MVS_MAX_HALF_WIDTH, = 16 mod 32
constexpr int kFilterThreads = 256;

static_assert(kTile == LS2FM_MVS_TILE, "the header states the tile");
static_assert(kRow >= kTile + 2 * LS2FM_MVS_MAX_HALF_WIDTH && kRow % 32 == 16, "rows of a half-wave on disjoint banks");

typedef float Pair __attribute__((ext_vector_type(2)));

template <int HW>
__global__ void __launch_bounds__(kThreads)
mvs_sweep(const float* __restrict__ images, int n_views, int height, int width, const int32_t* __restrict__ refs,
          const int32_t* __restrict__ sources, int n_sources, const float* __restrict__ depths, int n_planes,
          const float* __restrict__ rel, const float* __restrict__ intr, float near, float min_var, int min_sources, int tiles_x,
          int tiles_y, float* __restrict__ out_depth, float* __restrict__ out_score, int32_t* __restrict__ out_plane) {
#pragma clang fp contract(off)
    constexpr int kSide = kTile + 2 * HW, kHalo = kSide * kSide, kPer = (kHalo + kThreads - 1) / kThreads;
    constexpr int kWin = 2 * HW + 1;
    constexpr float kTaps = (float)(kWin * kWin);
    __shared__ float ref_t[kSide * kRow];
    __shared__ float src_t[kSide * kRow];
    const int t = threadIdx.x;
    const int tile = blockIdx.x;
    const int tile_x = tile % tiles_x, tile_y = (tile / tiles_x) % tiles_y, r = tile / (tiles_x * tiles_y);
    const int64_t hw = (int64_t)height * width;
    const int lx = t % kTile, ly = t / kTile;
    const int px = tile_x * kTile + lx, py = tile_y * kTile + ly;
    const bool in_image = px < width && py < height;
    const int64_t at = (int64_t)r * hw + (int64_t)py * width + px;
    const int rv = refs[r];
    if (rv < 0 || rv >= n_views) {                                   // uniform over the workgroup, before any barrier
        if (in_image) { out_depth[at] = NAN; out_score[at] = NAN; out_plane[at] = -1; }
        return;
    }
    const float* ref_img = images + (int64_t)rv * hw;
    const float fx = intr[(int64_t)rv * 4], fy = intr[(int64_t)rv * 4 + 1], cx = intr[(int64_t)rv * 4 + 2], cy = intr[(int64_t)rv * 4 + 3];

    // the halo pixels of this lane: the reference taps to LDS, the normalised coordinates of STEP 2 to registers
    float xn[kPer], yn[kPer];
    bool live[kPer];
#pragma unroll
    for (int j = 0; j < kPer; ++j) {
        const int h = t + j * kThreads;
        const int hy = h / kSide, hx = h % kSide;
        const int qx = tile_x * kTile - HW + hx, qy = tile_y * kTile - HW + hy;
        live[j] = h < kHalo && qx >= 0 && qx < width && qy >= 0 && qy < height;
        xn[j] = __fdiv_rn(__fsub_rn(__fadd_rn((float)qx, 0.5f), cx), fx);
        yn[j] = __fdiv_rn(__fsub_rn(__fadd_rn((float)qy, 0.5f), cy), fy);
        if (h < kHalo) ref_t[hy * kRow + hx] = live[j] ? finite_or_nan(ref_img[(int64_t)qy * width + qx]) : NAN;
    }
    __syncthreads();

    // STEP 1: the window's mean and variance, once per pixel
    const float* a_win = ref_t + ly * kRow + lx;
    const float* b_win = src_t + ly * kRow + lx;
    bool pixel_ok = in_image && px >= HW && px <= width - 1 - HW && py >= HW && py <= height - 1 - HW;
    float ma = 0.0f, va = 0.0f;
    if (pixel_ok) {
        float sum = 0.0f;
#pragma unroll
        for (int i = 0; i < kWin; ++i)
#pragma unroll
            for (int j = 0; j < kWin; ++j) sum = __fadd_rn(sum, a_win[i * kRow + j]);
        ma = __fdiv_rn(sum, kTaps);
#pragma unroll
        for (int i = 0; i < kWin; ++i)
#pragma unroll
            for (int j = 0; j < kWin; ++j) {
                const float da = __fsub_rn(a_win[i * kRow + j], ma);
                va = __fadd_rn(va, __fmul_rn(da, da));
            }
        pixel_ok = sum == sum && !(va < min_var);
    }

    float best = NAN, before = NAN, after = NAN, previous = NAN;
    int best_k = -1;
    for (int k = 0; k < n_planes; ++k) {
        const float d = depths[(int64_t)r * n_planes + k];
        float total = 0.0f;
        int count = 0;
        for (int s = 0; s < n_sources; ++s) {
            const int sv = sources[(int64_t)r * n_sources + s];
            if (sv < 0 || sv >= n_views) continue;                   // uniform: every lane of the workgroup skips the barriers
            const View cam = load_pair(rel, (int64_t)r * n_sources + s, intr, sv);
            const float* src_img = images + (int64_t)sv * hw;
            // STEPS 2 and 3 for this lane's halo pixels
#pragma unroll
            for (int j = 0; j < kPer; ++j) {
                const int h = t + j * kThreads;
                if (h < kHalo) {
                    float b = NAN;
                    if (live[j]) b = sample<true>(src_img, height, width, project(cam, __fmul_rn(xn[j], d), __fmul_rn(yn[j], d), d, near));
                    src_t[(h / kSide) * kRow + h % kSide] = b;
                }
            }
            __syncthreads();
            // STEP 4
            if (pixel_ok) {
                float sum = 0.0f;
#pragma unroll
                for (int i = 0; i < kWin; ++i)
#pragma unroll
                    for (int j = 0; j < kWin; ++j) sum = __fadd_rn(sum, b_win[i * kRow + j]);
                if (sum == sum) {
                    const float mb = __fdiv_rn(sum, kTaps);
                    // vb and cov side by side: one packed product and one packed sum per tap, each lane of the pair rounded as alone
                    Pair acc = {0.0f, 0.0f};
#pragma unroll
                    for (int i = 0; i < kWin; ++i)
#pragma unroll
                        for (int j = 0; j < kWin; ++j) {
                            const float da = __fsub_rn(a_win[i * kRow + j], ma), db = __fsub_rn(b_win[i * kRow + j], mb);
                            const Pair lhs = {db, da}, rhs = {db, db};
                            acc = acc + lhs * rhs;
                        }
                    const float vb = acc.x, cov = acc.y;
                    if (!(vb < min_var)) {
                        total = __fadd_rn(total, __fdiv_rn(cov, sqrt_rn(__fmul_rn(va, vb))));
                        ++count;
                    }
                }
            }
            __syncthreads();                                         // the next fill overwrites src_t
        }
        // STEPS 5 and 6
        const float score = count >= min_sources ? __fdiv_rn(total, (float)count) : NAN;
        if (score == score && (best_k < 0 || score > best)) {
            best = score; best_k = k; before = previous; after = NAN;
        } else if (k == best_k + 1) {
            after = score;
        }
        previous = score;
    }
    if (!in_image) return;
    // STEP 7
    float depth = NAN;
    if (best_k >= 0) {
        const float* dr = depths + (int64_t)r * n_planes;
        const float d0 = dr[best_k];
        depth = d0;
        const float den = __fadd_rn(__fsub_rn(before, __fmul_rn(2.0f, best)), after);
        if (best_k > 0 && best_k < n_planes - 1 && den < 0.0f) {    // a NaN neighbour makes den a NaN: false
            const float off = __fdiv_rn(__fmul_rn(0.5f, __fsub_rn(before, after)), den);
            const float step = off >= 0.0f ? __fsub_rn(dr[best_k + 1], d0) : __fsub_rn(d0, dr[best_k - 1]);
            depth = __fadd_rn(d0, __fmul_rn(off, step));
        }
    }
    out_depth[at] = depth;
    out_score[at] = best;
    out_plane[at] = best_k;
}

__global__ void __launch_bounds__(kFilterThreads)
mvs_filter(const float* __restrict__ depth, int n_views, int height, int width, const int32_t* __restrict__ sources, int n_sources,
           const float* __restrict__ rel, const float* __restrict__ rel_back, const float* __restrict__ intr, float near,
           float max_reproj, float rel_depth, int min_consistent, int blocks_per_view, uint8_t* __restrict__ out_count,
           float* __restrict__ out_depth) {
#pragma clang fp contract(off)
    const int r = blockIdx.x / blocks_per_view;                      // uniform: a workgroup stays inside one view
    const int64_t hw = (int64_t)height * width;
    const int64_t pixel = (int64_t)(blockIdx.x % blocks_per_view) * kFilterThreads + threadIdx.x;
    if (pixel >= hw) return;
    const int py = (int)(pixel / width), px = (int)(pixel % width);
    const float d = depth[(int64_t)r * hw + pixel];
    int count = 0;
    if (fabsf(d) < INFINITY && d > 0.0f) {
        const float* k = intr + (int64_t)r * 4;
        const float uc = __fadd_rn((float)px, 0.5f), vc = __fadd_rn((float)py, 0.5f);
        const float X = __fmul_rn(__fdiv_rn(__fsub_rn(uc, k[2]), k[0]), d), Y = __fmul_rn(__fdiv_rn(__fsub_rn(vc, k[3]), k[1]), d);
        const float reproj2 = __fmul_rn(max_reproj, max_reproj), dz = __fmul_rn(rel_depth, d);
        for (int s = 0; s < n_sources; ++s) {
            const int sv = sources[(int64_t)r * n_sources + s];
            if (sv < 0 || sv >= n_views) continue;
            const int64_t pair = (int64_t)r * n_sources + s;
            const View there = load_pair(rel, pair, intr, sv);
            const Projected p = project(there, X, Y, d, near);
            int sx, sy;
            if (!pixel_of(p, height, width, sx, sy)) continue;
            const float ds = depth[(int64_t)sv * hw + (int64_t)sy * width + sx];
            if (!(fabsf(ds) < INFINITY && ds > 0.0f)) continue;
            const float Xs = __fmul_rn(__fdiv_rn(__fsub_rn(__fadd_rn((float)sx, 0.5f), there.cx), there.fx), ds);
            const float Ys = __fmul_rn(__fdiv_rn(__fsub_rn(__fadd_rn((float)sy, 0.5f), there.cy), there.fy), ds);
            const View back = load_pair(rel_back, pair, intr, r);
            const Projected q = project(back, Xs, Ys, ds, near);
            const float du = __fsub_rn(q.u, uc), dv = __fsub_rn(q.v, vc);
            const float e = __fadd_rn(__fmul_rn(du, du), __fmul_rn(dv, dv));
            if (q.usable && e <= reproj2 && fabsf(__fsub_rn(q.z, d)) <= dz) ++count;
        }
    }
    out_count[(int64_t)r * hw + pixel] = (uint8_t)count;
    out_depth[(int64_t)r * hw + pixel] = count >= min_consistent ? d : NAN;
}

typedef void (*SweepKernel)(const float*, int, int, int, const int32_t*, const int32_t*, int, const float*, int, const float*,
                            const float*, float, float, int, int, int, float*, float*, int32_t*);

}  // namespace

extern "C" int ls2fm_mvs_sweep(const float* images, int32_t n_views, int32_t height, int32_t width, const int32_t* refs, int32_t n_refs,
                               const int32_t* sources, int32_t n_sources, const float* depths, int32_t n_planes, const float* rel,
                               const float* intr, int32_t half_width, float near, float min_var, int32_t min_sources, float* depth,
                               float* score, int32_t* plane, void* stream) {
    LS2FM_CHECK_ARG(mvs_shape_ok(n_views, height, width, n_refs, n_sources, half_width, near, min_var, min_sources) && n_planes >= 1 &&
                    n_planes <= LS2FM_MVS_MAX_PLANES);
    if (n_refs == 0) return LS2FM_OK;
    LS2FM_CHECK_ARG(n_views >= 1 && images && refs && sources && depths && rel && intr && depth && score && plane);
    const int64_t tiles_x = (width + kTile - 1) / kTile, tiles_y = (height + kTile - 1) / kTile;
    LS2FM_CHECK_ARG(tiles_x * tiles_y * n_refs < ((int64_t)1 << 31));
    static const SweepKernel kernels[LS2FM_MVS_MAX_HALF_WIDTH] = {mvs_sweep<1>, mvs_sweep<2>, mvs_sweep<3>, mvs_sweep<4>, mvs_sweep<5>};
    kernels[half_width - 1]<<<(unsigned)(tiles_x * tiles_y * n_refs), kThreads, 0, (hipStream_t)stream>>>(
        images, n_views, height, width, refs, sources, n_sources, depths, n_planes, rel, intr, near, min_var, min_sources, (int)tiles_x,
        (int)tiles_y, depth, score, plane);
    return ls2fm_launch_status();
}

extern "C" int ls2fm_mvs_filter(const float* depth, int32_t n_views, int32_t height, int32_t width, const int32_t* sources,
                                int32_t n_sources, const float* rel, const float* rel_back, const float* intr, float near,
                                float max_reproj, float rel_depth, int32_t min_consistent, uint8_t* count, float* filtered,
                                void* stream) {
    LS2FM_CHECK_ARG(raster_image_ok(n_views, height, width) && raster_near_ok(near) && n_sources >= 1 &&
                    n_sources <= LS2FM_MVS_MAX_SOURCES && finite_not_negative(max_reproj) && finite_not_negative(rel_depth) &&
                    min_consistent >= 0);
    if (n_views == 0) return LS2FM_OK;
    LS2FM_CHECK_ARG(depth && sources && rel && rel_back && intr && count && filtered);
    const int64_t blocks_per_view = ((int64_t)height * width + kFilterThreads - 1) / kFilterThreads;
    LS2FM_CHECK_ARG(blocks_per_view * n_views < ((int64_t)1 << 31));
    mvs_filter<<<(unsigned)(blocks_per_view * n_views), kFilterThreads, 0, (hipStream_t)stream>>>(
        depth, n_views, height, width, sources, n_sources, rel, rel_back, intr, near, max_reproj, rel_depth, min_consistent,
        (int)blocks_per_view, count, filtered);
    return ls2fm_launch_status();
}
