// PatchMatch stereo with slanted planes: THE PLANE SCORE (ls2fm_mvs_plane_score) and THE PATCHMATCH STEP (ls2fm_mvs_patchmatch_step)
// of include/ls2fm.h, the primitives under ls2fm.mvs.plane_score, patch_match_step and patch_match.  tests/patchmatch_restate.py
// repeats both rules in numpy, ls2fm.mvs.plane_score_torch / patch_match_step_torch as torch ops.
//
// One workgroup of 256 lanes takes one (reference, 16 x 32 tile); every lane owns one pixel of a colour (the step: the colour of
// the call; the score: both, one after the other).  The reference tile with its halo of w pixels and the lift of its columns and
// rows go to LDS once; every pixel's window mean and variance are formed once.  A hypothesis is a plane of the lane's own, so no
// warped sample is shared between lanes (the sweep's LDS exchange has nothing to exchange here): per (candidate, source) a lane
// warps its n taps along its plane, projects them (csrc/raster_project.h, unchanged) and samples the source by plain global loads
// -- neighbouring lanes hit neighbouring texels.  NCC is the rule's two-pass form, so the n samples of one source wait for their
// mean: in a column of LDS of the lane's own (b_t[tap][lane], consecutive lanes on consecutive banks, no barrier: nobody else
// reads it), not in registers, and a_i - ma is read again from the tile per tap.  An invalid sample is stored as NaN, and the
// window's sum in tap order is NaN exactly when one of its taps is.  The candidate, source and window-row loops are loops -- one
// inlined score per kernel -- and a row of taps is unrolled with no branch in a tap (an invalid tap loads the image's first pixels
// and discards them), so that the divisions and the four loads of up to 11 taps overlap: 10.6 -> 7.5 ms per half-step at w = 3
// against one tap at a time behind a branch, the same bits.  Pose rows, intrinsics and the source list are uniform over the
// workgroup: scalar loads.  No atomics, no workspace, nothing read back.  The step reads only pixels of the other colour besides
// its own, so it is free of races in place.
#include "mvs_plane.h"

namespace {

constexpr int kTileH = LS2FM_MVS_PM_TILE_H, kTileW = LS2FM_MVS_PM_TILE_W;
constexpr int kThreads = 256;
constexpr int kCandidates = 12;            // 8 neighbours, 3 perturbations, 1 fresh hypothesis
static_assert(kTileH * kTileW == 2 * kThreads, "one lane per pixel of a colour");

struct Scene {
    const float* images;
    const int32_t* sources;                // this reference's row
    const float* rel;                      // this reference's row of poses
    const float* intr;
    int n_views, height, width, n_sources, min_sources;
    float near, min_var;
};

template <int HW, int T>
struct Tile {
    static constexpr int kAxis = 2 * HW / T + 1, kTaps = kAxis * kAxis;
    static constexpr int kCols = kTileW + 2 * HW, kRows = kTileH + 2 * HW;
    static constexpr int kRow = kCols | 1;                             // odd: the rows of a wave spread over the banks
    float ref[kRows * kRow];
    float xn[kCols], yn[kRows];
    float b[kTaps * kThreads];
};

// the halo to LDS: reference pixels (NaN outside the image or not finite) and the lift of the columns and rows
template <int HW, int T>
__device__ __forceinline__ void fill_tile(Tile<HW, T>& s, const float* __restrict__ ref_img, const float* __restrict__ k, int height,
                                          int width, int x0, int y0) {
#pragma clang fp contract(off)
    using L = Tile<HW, T>;
    const int t = threadIdx.x;
    for (int h = t; h < L::kRows * L::kCols; h += kThreads) {
        const int hy = h / L::kCols, hx = h % L::kCols;
        const int qx = x0 - HW + hx, qy = y0 - HW + hy;
        const bool live = qx >= 0 && qx < width && qy >= 0 && qy < height;
        s.ref[hy * L::kRow + hx] = live ? finite_or_nan(ref_img[(int64_t)qy * width + qx]) : NAN;
    }
    if (t < L::kCols) s.xn[t] = __fdiv_rn(__fsub_rn(__fadd_rn((float)(x0 - HW + t), 0.5f), k[2]), k[0]);
    if (t >= 64 && t < 64 + L::kRows) s.yn[t - 64] = __fdiv_rn(__fsub_rn(__fadd_rn((float)(y0 - HW + t - 64), 0.5f), k[3]), k[1]);
    __syncthreads();
}

// STEP 0 of THE PLANE SCORE for the pixel whose window starts at a_win: false when the pixel is invalid
template <int HW, int T>
__device__ __forceinline__ bool window_stats(const float* a_win, float min_var, float& ma, float& va) {
#pragma clang fp contract(off)
    using L = Tile<HW, T>;
    float sum = 0.0f;
    for (int i = 0; i < L::kAxis; ++i)
        for (int j = 0; j < L::kAxis; ++j) sum = __fadd_rn(sum, a_win[i * T * L::kRow + j * T]);
    ma = __fdiv_rn(sum, (float)L::kTaps);
    va = 0.0f;
    for (int i = 0; i < L::kAxis; ++i)
        for (int j = 0; j < L::kAxis; ++j) {
            const float da = __fsub_rn(a_win[i * T * L::kRow + j * T], ma);
            va = __fadd_rn(va, __fmul_rn(da, da));
        }
    return sum == sum && !(va < min_var);
}

// THE PLANE SCORE, steps 1 to 6, of (d, n) at the pixel at (lx, ly) of the tile, whose window is valid with (ma, va)
template <int HW, int T>
__device__ __forceinline__ float plane_score(const Scene& sc, Tile<HW, T>& s, int lx, int ly, float ma, float va, float d, const Normal& n) {
#pragma clang fp contract(off)
    using L = Tile<HW, T>;
    const float g_p = pm_g(n, s.xn[lx + HW], s.yn[ly + HW]);
    if (!(fabsf(d) < INFINITY && d > 0.0f && fabsf(n.x) < INFINITY && fabsf(n.y) < INFINITY && fabsf(n.z) < INFINITY && g_p < 0.0f)) return NAN;
    const float h = __fmul_rn(g_p, d);
    const float* a_win = s.ref + ly * L::kRow + lx;
    const float* xn_win = s.xn + lx;
    const float* yn_win = s.yn + ly;
    float* b_mine = s.b + threadIdx.x;
    const int64_t hw = (int64_t)sc.height * sc.width;
    float total = 0.0f;
    int count = 0;
    for (int src = 0; src < sc.n_sources; ++src) {
        const int sv = sc.sources[src];
        if (sv < 0 || sv >= sc.n_views) continue;
        const View cam = load_pair(sc.rel, src, sc.intr, sv);
        const float* src_img = sc.images + (int64_t)sv * hw;
        float sum = 0.0f;
        for (int i = 0; i < L::kAxis; ++i) {
            const float yq = yn_win[i * T];
            // a row of taps at a time, each tap free of branches: their divisions and loads overlap
            float row[L::kAxis];
#pragma unroll
            for (int j = 0; j < L::kAxis; ++j) {
                const float xq = xn_win[j * T];
                const float g_q = pm_g(n, xq, yq);
                const float d_q = __fdiv_rn(h, g_q);
                row[j] = sample<false>(src_img, sc.height, sc.width, project(cam, __fmul_rn(xq, d_q), __fmul_rn(yq, d_q), d_q, sc.near),
                                       g_q < 0.0f && fabsf(d_q) < INFINITY);
            }
#pragma unroll
            for (int j = 0; j < L::kAxis; ++j) {
                b_mine[(i * L::kAxis + j) * kThreads] = row[j];
                sum = __fadd_rn(sum, row[j]);
            }
        }
        if (sum == sum) {
            const float mb = __fdiv_rn(sum, (float)L::kTaps);
            float vb = 0.0f, cov = 0.0f;
            for (int i = 0; i < L::kAxis; ++i)
                for (int j = 0; j < L::kAxis; ++j) {
                    const float da = __fsub_rn(a_win[i * T * L::kRow + j * T], ma);
                    const float db = __fsub_rn(b_mine[(i * L::kAxis + j) * kThreads], mb);
                    vb = __fadd_rn(vb, __fmul_rn(db, db));
                    cov = __fadd_rn(cov, __fmul_rn(da, db));
                }
            if (!(vb < sc.min_var)) {
                total = __fadd_rn(total, __fdiv_rn(cov, sqrt_rn(__fmul_rn(va, vb))));
                ++count;
            }
        }
    }
    return count >= sc.min_sources ? __fdiv_rn(total, (float)count) : NAN;
}

struct Args {
    const float* images;
    const int32_t* refs;
    const int32_t* sources;
    const float* rel;
    const float* intr;
    int n_views, height, width, n_sources, min_sources, tiles_x, tiles_y;
    float near, min_var;
};

__device__ __forceinline__ Scene scene_of(const Args& a, int r) {
    Scene sc;
    sc.images = a.images;
    sc.sources = a.sources + (int64_t)r * a.n_sources;
    sc.rel = a.rel + (int64_t)r * a.n_sources * 12;
    sc.intr = a.intr;
    sc.n_views = a.n_views; sc.height = a.height; sc.width = a.width; sc.n_sources = a.n_sources; sc.min_sources = a.min_sources;
    sc.near = a.near; sc.min_var = a.min_var;
    return sc;
}

// the lane's pixel of `colour` in the tile: row t / 16, and of that row's columns of the colour the (t % 16)-th.  The tile's origin
// is even in both axes, so the pixel's colour is that of its place in the tile.
__device__ __forceinline__ void lane_pixel(int colour, int& lx, int& ly) {
    const int t = threadIdx.x;
    ly = t / (kTileW / 2);
    lx = 2 * (t % (kTileW / 2)) + ((ly ^ colour) & 1);
}

template <int HW, int T>
__global__ void __launch_bounds__(kThreads)
mvs_plane_score(Args a, const float* __restrict__ depth, const float* __restrict__ normal, float* __restrict__ score) {
    __shared__ Tile<HW, T> s;
    const int tile = blockIdx.x;
    const int tile_x = tile % a.tiles_x, tile_y = (tile / a.tiles_x) % a.tiles_y, r = tile / (a.tiles_x * a.tiles_y);
    const int64_t hw = (int64_t)a.height * a.width;
    const int rv = a.refs[r];
    const bool view_ok = rv >= 0 && rv < a.n_views;                    // uniform over the workgroup
    if (view_ok) fill_tile(s, a.images + (int64_t)rv * hw, a.intr + (int64_t)rv * 4, a.height, a.width, tile_x * kTileW, tile_y * kTileH);
    const Scene sc = scene_of(a, r);
    for (int colour = 0; colour < 2; ++colour) {
        int lx, ly;
        lane_pixel(colour, lx, ly);
        const int px = tile_x * kTileW + lx, py = tile_y * kTileH + ly;
        if (px >= a.width || py >= a.height) continue;
        const int64_t at = (int64_t)r * hw + (int64_t)py * a.width + px;
        float out = NAN, ma, va;
        if (view_ok && px >= HW && px <= a.width - 1 - HW && py >= HW && py <= a.height - 1 - HW &&
            window_stats<HW, T>(s.ref + ly * Tile<HW, T>::kRow + lx, a.min_var, ma, va)) {
            const Normal n = {normal[at * 3], normal[at * 3 + 1], normal[at * 3 + 2]};
            out = plane_score(sc, s, lx, ly, ma, va, depth[at], n);
        }
        score[at] = out;
    }
}

template <int HW, int T>
__global__ void __launch_bounds__(kThreads)
mvs_patchmatch_step(Args a, int colour, uint32_t iteration, uint32_t seed, float rho_d, float rho_n, float sigma,
                    const float* __restrict__ d_min, const float* __restrict__ d_max, float* depth, float* normal, float* score) {
#pragma clang fp contract(off)
    __shared__ Tile<HW, T> s;
    const int tile = blockIdx.x;
    const int tile_x = tile % a.tiles_x, tile_y = (tile / a.tiles_x) % a.tiles_y, r = tile / (a.tiles_x * a.tiles_y);
    const int64_t hw = (int64_t)a.height * a.width;
    const int rv = a.refs[r];
    if (rv < 0 || rv >= a.n_views) return;                             // uniform over the workgroup, before any barrier
    const float* k = a.intr + (int64_t)rv * 4;
    fill_tile(s, a.images + (int64_t)rv * hw, k, a.height, a.width, tile_x * kTileW, tile_y * kTileH);
    int lx, ly;
    lane_pixel(colour, lx, ly);
    const int px = tile_x * kTileW + lx, py = tile_y * kTileH + ly;
    if (!(px >= HW && px <= a.width - 1 - HW && py >= HW && py <= a.height - 1 - HW)) return;     // no barrier below
    float ma, va;
    // a pixel whose window is invalid scores NaN for every candidate: it keeps its incumbent
    if (!window_stats<HW, T>(s.ref + ly * Tile<HW, T>::kRow + lx, a.min_var, ma, va)) return;
    const Scene sc = scene_of(a, r);
    const int64_t base = (int64_t)r * hw, at = base + (int64_t)py * a.width + px;
    float best_d = depth[at], best_s = score[at];
    Normal best_n = {normal[at * 3], normal[at * 3 + 1], normal[at * 3 + 2]};
    const float xn_p = s.xn[lx + HW], yn_p = s.yn[ly + HW];
    const uint32_t key = pm_mix(pm_mix(pm_mix(pm_mix(seed + LS2FM_MVS_MIX_SALT) + (uint32_t)rv) + iteration) + (uint32_t)(py * a.width + px));
    const float fx = k[0], fy = k[1], cx = k[2], cy = k[3];
    for (int c = 0; c < kCandidates; ++c) {
        float cd = NAN;
        Normal cn = best_n;
        bool active = false;
        if (c < 8) {
            // 1. a neighbour's plane, met by this pixel's ray
            const int far = c < 4 ? 1 : 3, which = c & 3;
            const int mx = px + (which == 1 ? -far : which == 2 ? far : 0), my = py + (which == 0 ? -far : which == 3 ? far : 0);
            if (mx >= 0 && mx < a.width && my >= 0 && my < a.height) {
                const int64_t m = base + (int64_t)my * a.width + mx;
                const float d_m = depth[m];
                if (fabsf(d_m) < INFINITY && d_m > 0.0f) {
                    cn = {normal[m * 3], normal[m * 3 + 1], normal[m * 3 + 2]};
                    const float xn_m = __fdiv_rn(__fsub_rn(__fadd_rn((float)mx, 0.5f), cx), fx);
                    const float yn_m = __fdiv_rn(__fsub_rn(__fadd_rn((float)my, 0.5f), cy), fy);
                    cd = __fdiv_rn(__fmul_rn(pm_g(cn, xn_m, yn_m), d_m), pm_g(cn, xn_p, yn_p));
                    active = true;
                }
            }
        } else if (c < 11) {
            // 2. to 4. perturbations about the incumbent, when there is one
            active = best_s == best_s;
            const uint32_t j = c == 8 ? 0u : c == 9 ? 1u : 3u;
            cd = c == 9 ? best_d : __fmul_rn(best_d, __fadd_rn(1.0f, __fmul_rn(rho_d, pm_signed(pm_draw(key, j)))));
            if (c != 8) {
                const uint32_t jn = c == 9 ? 1u : 4u;
                cn = pm_normalise(__fadd_rn(best_n.x, __fmul_rn(rho_n, pm_signed(pm_draw(key, jn)))),
                                  __fadd_rn(best_n.y, __fmul_rn(rho_n, pm_signed(pm_draw(key, jn + 1)))), best_n.z);
            }
        } else {
            // 5. a fresh hypothesis
            active = true;
            const float i0 = __fdiv_rn(1.0f, d_min[r]), i1 = __fdiv_rn(1.0f, d_max[r]);
            cd = __fdiv_rn(1.0f, __fadd_rn(i0, __fmul_rn(pm_draw(key, 6), __fsub_rn(i1, i0))));
            cn = pm_normalise(__fmul_rn(sigma, pm_signed(pm_draw(key, 7))), __fmul_rn(sigma, pm_signed(pm_draw(key, 8))), -1.0f);
        }
        if (!active) continue;
        const float sco = plane_score(sc, s, lx, ly, ma, va, cd, cn);
        if (sco == sco && (!(best_s == best_s) || sco > best_s)) {
            best_d = cd; best_n = cn; best_s = sco;
        }
    }
    depth[at] = best_d;
    normal[at * 3] = best_n.x; normal[at * 3 + 1] = best_n.y; normal[at * 3 + 2] = best_n.z;
    score[at] = best_s;
}

typedef void (*ScoreKernel)(Args, const float*, const float*, float*);
typedef void (*StepKernel)(Args, int, uint32_t, uint32_t, float, float, float, const float*, const float*, float*, float*, float*);

}  // namespace

#define PM_KERNELS(name) \
    {name<1, 1>, name<1, 2>, name<2, 1>, name<2, 2>, name<3, 1>, name<3, 2>, name<4, 1>, name<4, 2>, name<5, 1>, name<5, 2>}

extern "C" int ls2fm_mvs_plane_score(const float* images, int32_t n_views, int32_t height, int32_t width, const int32_t* refs,
                                     int32_t n_refs, const int32_t* sources, int32_t n_sources, const float* rel, const float* intr,
                                     int32_t half_width, int32_t tap_step, float near, float min_var, int32_t min_sources,
                                     const float* depth, const float* normal, float* score, void* stream) {
    LS2FM_CHECK_ARG(mvs_shape_ok(n_views, height, width, n_refs, n_sources, half_width, near, min_var, min_sources) &&
                    (tap_step == 1 || tap_step == 2));
    if (n_refs == 0) return LS2FM_OK;
    LS2FM_CHECK_ARG(n_views >= 1 && images && refs && sources && rel && intr && depth && normal && score);
    const int64_t tiles_x = (width + kTileW - 1) / kTileW, tiles_y = (height + kTileH - 1) / kTileH;
    LS2FM_CHECK_ARG(tiles_x * tiles_y * n_refs < ((int64_t)1 << 31));
    const Args a = {images, refs, sources, rel, intr, n_views, height, width, n_sources, min_sources, (int)tiles_x, (int)tiles_y, near, min_var};
    static const ScoreKernel kernels[2 * LS2FM_MVS_MAX_HALF_WIDTH] = PM_KERNELS(mvs_plane_score);
    kernels[2 * (half_width - 1) + tap_step - 1]<<<(unsigned)(tiles_x * tiles_y * n_refs), kThreads, 0, (hipStream_t)stream>>>(
        a, depth, normal, score);
    return ls2fm_launch_status();
}

extern "C" int ls2fm_mvs_patchmatch_step(const float* images, int32_t n_views, int32_t height, int32_t width, const int32_t* refs,
                                         int32_t n_refs, const int32_t* sources, int32_t n_sources, const float* rel, const float* intr,
                                         int32_t half_width, int32_t tap_step, float near, float min_var, int32_t min_sources,
                                         int32_t colour, int32_t iteration, uint32_t seed, float rho_d, float rho_n, float sigma,
                                         const float* d_min, const float* d_max, float* depth, float* normal, float* score,
                                         void* stream) {
    LS2FM_CHECK_ARG(mvs_shape_ok(n_views, height, width, n_refs, n_sources, half_width, near, min_var, min_sources) &&
                    (tap_step == 1 || tap_step == 2) && (colour == 0 || colour == 1) && iteration >= 0 && finite_not_negative(rho_d) &&
                    finite_not_negative(rho_n) && finite_not_negative(sigma));
    if (n_refs == 0) return LS2FM_OK;
    LS2FM_CHECK_ARG(n_views >= 1 && images && refs && sources && rel && intr && d_min && d_max && depth && normal && score);
    const int64_t tiles_x = (width + kTileW - 1) / kTileW, tiles_y = (height + kTileH - 1) / kTileH;
    LS2FM_CHECK_ARG(tiles_x * tiles_y * n_refs < ((int64_t)1 << 31));
    const Args a = {images, refs, sources, rel, intr, n_views, height, width, n_sources, min_sources, (int)tiles_x, (int)tiles_y, near, min_var};
    static const StepKernel kernels[2 * LS2FM_MVS_MAX_HALF_WIDTH] = PM_KERNELS(mvs_patchmatch_step);
    kernels[2 * (half_width - 1) + tap_step - 1]<<<(unsigned)(tiles_x * tiles_y * n_refs), kThreads, 0, (hipStream_t)stream>>>(
        a, colour, (uint32_t)iteration, seed, rho_d, rho_n, sigma, d_min, d_max, depth, normal, score);
    return ls2fm_launch_status();
}
