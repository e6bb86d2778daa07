// Image undistortion and key-point (un)distortion (ls2fm_undistort_images, ls2fm_camera_points): the primitives under
// ls2fm.undistort.  include/ls2fm.h states THE DISTORTION RULE and THE UNDISTORTION RULE, csrc/camera_model.h holds the former's
// expressions for both kernels; tests/undistort_restate.py repeats them in numpy, ls2fm.undistort as torch ops.
//
// undistort_images: one lane per output pixel; a workgroup is a tile of kTileW x kTileH output pixels of one view, so the view's 12
// camera words and the output's 4 are uniform (scalar loads).  A distortion moves a pixel by a smooth field, so the source taps of a
// tile are a slightly bent tile of the photograph: the gathers of a wave fall in as many cache lines as its rows.  Tiles timed on
// 49 x 1200 x 1600 x 3 (tools/time_undistort.py, profiles/undistort_time.json).  No LDS, no atomics, no workspace, nothing read back.
// camera_points: one lane per point, fp64; the lane bisects view_start for its view; the Newton loop runs `iters` trips for every lane.
#include "camera_model.h"

namespace {

using namespace camera_model;

constexpr int kThreads = 256;
#ifdef LS2FM_UNDISTORT_AB_TILE_W    // a variant build of tools/time_undistort.py (tools/build_variant.sh): another tile, 256 x 1 is a linear run
constexpr int kTileW = LS2FM_UNDISTORT_AB_TILE_W, kTileH = kThreads / kTileW;
#else
constexpr int kTileW = LS2FM_UNDISTORT_TILE_W, kTileH = LS2FM_UNDISTORT_TILE_H;
#endif
constexpr int kPointThreads = LS2FM_CAMERA_POINTS_THREADS;

static_assert(kTileW * kTileH == kThreads, "one lane per pixel of the tile");

struct Fill {
    float c[4];
};

// the two columns (or rows) and the weight of a bilinear sample at the image coordinate u, 0 <= u < size: step 4 of the rule
__device__ __forceinline__ void taps(float u, int size, int& i0, int& i1, float& t) {
#pragma clang fp contract(off)
    const float x = __fsub_rn(u, 0.5f);
    const float x0 = floorf(x);                       // in [-1, size - 1]
    t = __fsub_rn(x, x0);
    const int i = (int)x0;
    i0 = min(max(i, 0), size - 1);
    i1 = min(max(i + 1, 0), size - 1);
}

template <int C, bool kBilinear>
__global__ void __launch_bounds__(kThreads)
undistort_images(const float* __restrict__ images, int src_height, int src_width, const float* __restrict__ cam,
                 const float* __restrict__ out_intr, int height, int width, int tiles_x, int tiles_y, const Fill fill,
                 float* __restrict__ out, uint8_t* __restrict__ valid) {
#pragma clang fp contract(off)
    const int tile = blockIdx.x, t = threadIdx.x;
    const int view = tile / (tiles_x * tiles_y);                  // uniform
    const int px = (tile % tiles_x) * kTileW + t % kTileW;
    const int py = ((tile / tiles_x) % tiles_y) * kTileH + t / kTileW;
    if (px >= width || py >= height) return;
    const Camera<float> c = load_camera(cam, (int64_t)view);
    const float* k = out_intr + (int64_t)view * 4;
    const float xn = __fdiv_rn(__fsub_rn(__fadd_rn((float)px, 0.5f), k[2]), k[0]);
    const float yn = __fdiv_rn(__fsub_rn(__fadd_rn((float)py, 0.5f), k[3]), k[1]);
    float xd, yd, u, v;
    distort(c, xn, yn, xd, yd);
    to_image(c, xd, yd, u, v);
    // IN THE IMAGE: every comparison is false for a NaN, and a value inside the bounds is finite
    const bool ok = u >= 0.0f && u < (float)src_width && v >= 0.0f && v < (float)src_height;
    float s[C];
#pragma unroll
    for (int i = 0; i < C; ++i) s[i] = fill.c[i];
    if (ok) {
        const float* img = images + (int64_t)view * src_height * src_width * C;
        if (kBilinear) {
            int x0, x1, y0, y1;
            float tx, ty;
            taps(u, src_width, x0, x1, tx);
            taps(v, src_height, y0, y1, ty);
            const float* a00 = img + ((int64_t)y0 * src_width + x0) * C;
            const float* a10 = img + ((int64_t)y0 * src_width + x1) * C;
            const float* a01 = img + ((int64_t)y1 * src_width + x0) * C;
            const float* a11 = img + ((int64_t)y1 * src_width + x1) * C;
#pragma unroll
            for (int i = 0; i < C; ++i) {
                const float r0 = __fadd_rn(a00[i], __fmul_rn(tx, __fsub_rn(a10[i], a00[i])));
                const float r1 = __fadd_rn(a01[i], __fmul_rn(tx, __fsub_rn(a11[i], a01[i])));
                s[i] = __fadd_rn(r0, __fmul_rn(ty, __fsub_rn(r1, r0)));
            }
        } else {
            const int x0 = min((int)floorf(u), src_width - 1), y0 = min((int)floorf(v), src_height - 1);
            const float* a = img + ((int64_t)y0 * src_width + x0) * C;
#pragma unroll
            for (int i = 0; i < C; ++i) s[i] = a[i];
        }
    }
    const int64_t at = ((int64_t)view * height + py) * width + px;
#pragma unroll
    for (int i = 0; i < C; ++i) out[at * C + i] = s[i];
    if (valid) valid[at] = ok ? 1 : 0;
}

__global__ void __launch_bounds__(kPointThreads)
camera_points(const double* __restrict__ uv, int64_t n_points, const int32_t* __restrict__ view_start, int n_views,
              const double* __restrict__ cam, const double* __restrict__ out_intr, int direction, int iters,
              double* __restrict__ uv_out, double* __restrict__ residual) {
#pragma clang fp contract(off)
    const int64_t row = (int64_t)blockIdx.x * kPointThreads + threadIdx.x;
    if (row >= n_points) return;
    // the last view whose start is at or before the row; the trip count depends on n_views alone
    int lo = 0, hi = n_views;
    while (hi - lo > 1) {
        const int mid = lo + (hi - lo) / 2;
        if ((int64_t)view_start[mid] <= row) lo = mid; else hi = mid;
    }
    if (!((int64_t)view_start[lo] <= row && row < (int64_t)view_start[lo + 1])) return;
    const Camera<double> c = load_camera(cam, (int64_t)lo);
    const double* k = out_intr + (int64_t)lo * 4;
    const double fx_o = k[0], fy_o = k[1], cx_o = k[2], cy_o = k[3];
    const double u = uv[2 * row], v = uv[2 * row + 1];
    double ou, ov, res = 0.0;
    if (direction == LS2FM_CAMERA_DISTORT) {
        const double x = quot(sub(u, cx_o), fx_o), y = quot(sub(v, cy_o), fy_o);
        double xd, yd;
        distort(c, x, y, xd, yd);
        to_image(c, xd, yd, ou, ov);
    } else {
        const double xd = quot(sub(u, c.cx), c.fx), yd = quot(sub(v, c.cy), c.fy);
        double x = xd, y = yd, fx_, fy_;
        bool live = true;
        for (int it = 0; it < iters; ++it) {
            const Radial<double> o = distort(c, x, y, fx_, fy_);
            double ja, jb, jc, jd;
            jacobian(c, o, x, y, ja, jb, jc, jd);
            const double ex = sub(fx_, xd), ey = sub(fy_, yd);
            const double det = sub(mul(ja, jd), mul(jb, jc));
            live = live && det != 0.0 && fabs(det) < INFINITY;        // false for a NaN
            if (live) {
                x = sub(x, quot(sub(mul(jd, ex), mul(jb, ey)), det));
                y = sub(y, quot(sub(mul(ja, ey), mul(jc, ex)), det));
            }
        }
        distort(c, x, y, fx_, fy_);
        const double px = mul(c.fx, sub(fx_, xd)), py = mul(c.fy, sub(fy_, yd));
        res = add(mul(px, px), mul(py, py));
        ou = add(mul(fx_o, x), cx_o);
        ov = add(mul(fy_o, y), cy_o);
    }
    uv_out[2 * row] = ou;
    uv_out[2 * row + 1] = ov;
    if (residual) residual[row] = res;
}

bool size_ok(int32_t n) { return n >= 1 && n <= 32768; }

}  // namespace

extern "C" int ls2fm_undistort_images(const float* images, int32_t n_views, int32_t src_height, int32_t src_width, int32_t channels,
                                      const float* cam, const float* out_intr, int32_t height, int32_t width, int32_t mode,
                                      const float* fill, float* out, uint8_t* valid, void* stream) {
    LS2FM_CHECK_ARG(n_views >= 0 && size_ok(src_height) && size_ok(src_width) && size_ok(height) && size_ok(width) &&
                    (int64_t)n_views * src_height * src_width < ((int64_t)1 << 40) &&
                    (int64_t)n_views * height * width < ((int64_t)1 << 40) && channels >= 1 && channels <= 4 &&
                    (mode == LS2FM_UNDISTORT_BILINEAR || mode == LS2FM_UNDISTORT_NEAREST));
    const int64_t tiles_x = (width + kTileW - 1) / kTileW, tiles_y = (height + kTileH - 1) / kTileH;
    const int64_t groups = tiles_x * tiles_y * n_views;
    LS2FM_CHECK_ARG(groups < ((int64_t)1 << 31));
    if (n_views == 0) return LS2FM_OK;
    LS2FM_CHECK_ARG(images && cam && out_intr && fill && out);
    Fill f = {{0.0f, 0.0f, 0.0f, 0.0f}};
    for (int c = 0; c < channels; ++c) f.c[c] = fill[c];            // on the host: `channels` floats, read before the call returns
    hipStream_t s = (hipStream_t)stream;
#define LS2FM_UNDISTORT_LAUNCH(C)                                                                                                  \
    if (mode == LS2FM_UNDISTORT_BILINEAR)                                                                                          \
        undistort_images<C, true><<<(unsigned)groups, kThreads, 0, s>>>(images, src_height, src_width, cam, out_intr, height, width, \
                                                                       (int)tiles_x, (int)tiles_y, f, out, valid);                \
    else                                                                                                                           \
        undistort_images<C, false><<<(unsigned)groups, kThreads, 0, s>>>(images, src_height, src_width, cam, out_intr, height, width, \
                                                                        (int)tiles_x, (int)tiles_y, f, out, valid)
    switch (channels) {
        case 1: LS2FM_UNDISTORT_LAUNCH(1); break;
        case 2: LS2FM_UNDISTORT_LAUNCH(2); break;
        case 3: LS2FM_UNDISTORT_LAUNCH(3); break;
        default: LS2FM_UNDISTORT_LAUNCH(4); break;
    }
#undef LS2FM_UNDISTORT_LAUNCH
    return ls2fm_launch_status();
}

extern "C" int ls2fm_camera_points(const double* uv, int64_t n_points, const int32_t* view_start, int32_t n_views, const double* cam,
                                   const double* out_intr, int32_t direction, int32_t iters, double* uv_out, double* residual,
                                   void* stream) {
    LS2FM_CHECK_ARG(n_points >= 0 && n_points < ((int64_t)1 << 31) && n_views >= 0 &&
                    (direction == LS2FM_CAMERA_DISTORT || direction == LS2FM_CAMERA_UNDISTORT) && iters >= 0 &&
                    iters <= LS2FM_CAMERA_MAX_ITERS);
    if (n_points == 0) return LS2FM_OK;
    LS2FM_CHECK_ARG(n_views >= 1 && uv && view_start && cam && out_intr && uv_out);
    const int64_t groups = (n_points + kPointThreads - 1) / kPointThreads;
    camera_points<<<(unsigned)groups, kPointThreads, 0, (hipStream_t)stream>>>(uv, n_points, view_start, n_views, cam, out_intr, direction,
                                                                              iters, uv_out, residual);
    return ls2fm_launch_status();
}
