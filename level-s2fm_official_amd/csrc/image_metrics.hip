// Image-quality metrics of rendered views against photographs (ls2fm.image_metrics): the squared error and SSIM over the valid
// region, batched over views, in fp64.  include/ls2fm.h states the rule and the summation order; tests/image_metrics_restate.py
// repeats both in numpy.
//
// Two launches, nothing read back, no atomic of any kind:
//   image_compare_tiles   one workgroup of 256 lanes per (view, tile of 16 x 16 pixels).  The tile plus its halo of n - 1 pixels to
//                         the right and below, all channels of both images, is read once into LDS as fp32.  Per channel: the row
//                         pass forms the five products of every loaded pixel once (a lane owns two neighbouring outputs of a
//                         row, so a product serves both) and writes the five row-blurred moments into LDS in fp64; the column
//                         pass reads them back, one window centre per lane, and evaluates the SSIM expression; the squared
//                         error of the lane's own pixel comes from the same LDS tile.  block_sum (wave_ops.h) per workgroup,
//                         one partial row (sse, ssim_sum) and two counts per (view, tile) into the workspace.
//   image_compare_finish  one workgroup per view: the view's rows added in tile order, the counts added.
// Tile (ty, tx) owns the PIXELS (16 ty + ly, 16 tx + lx) for the squared error and the window CENTRES of the same indices
// (y, x) -- centre pixel (y + r, x + r) -- for SSIM; lane 16 ly + lx takes both.  A tap sum starts from -0.0, so that its
// first addition returns w[0] v[0] bit for bit.  When the fp32 tile of all channels does not fit beside the moments (large
// windows with several channels: from n = 23 with four), the tile is read one channel at a time: the same values take the same
// operations.
#include "ls2fm_device.h"
#include "workspace.h"

namespace {

constexpr int kT = LS2FM_IMAGE_TILE;
constexpr int kThreads = kT * kT;                 // one lane per pixel / centre of the tile
constexpr int kMaxTaps = LS2FM_IMAGE_MAX_TAPS;
constexpr int kMoments = 5;                       // E[x], E[y], E[xx], E[yy], E[xy]
constexpr size_t kLdsBudget = 63 * 1024;          // dynamic LDS of image_compare_tiles (64 KiB less its static arrays)
constexpr int kMaxGridY = 65535;
constexpr int kFinishThreads = 256;
constexpr int kStage = 1024;                     // partial rows staged through LDS at a time by image_compare_finish
static_assert(kThreads == 256 && kT % 2 == 0, "lane = 16 ly + lx; the row pass takes two outputs per lane");

struct Taps { double w[kMaxTaps]; };

size_t tile_lds_bytes(int n_taps, int group) {
    const size_t side = (size_t)(kT + n_taps - 1);
    return kMoments * side * kT * sizeof(double) + 2 * side * side * group * sizeof(float);
}

// channels read into LDS together: all of them, or one at a time when they do not fit
int channel_group(int n_taps, int channels) { return tile_lds_bytes(n_taps, channels) <= kLdsBudget ? channels : 1; }

int64_t tiles_of(int height, int width) { return (int64_t)((height + kT - 1) / kT) * ((width + kT - 1) / kT); }

struct ImageWs {
    double* rows;              // [n_views][tiles][2]: sse, ssim_sum
    long long* counts;         // [n_views][tiles][2]: count, ssim_count
};

size_t image_layout(int64_t n_views, int64_t tiles, void* base, ImageWs* w) {
    Workspace ws(base, 256);
    double* rows = ws.take<double>((size_t)(n_views * tiles * 2));
    long long* counts = ws.take<long long>((size_t)(n_views * tiles * 2));
    if (w) *w = {rows, counts};
    return ws.bytes();
}

// NT: the number of taps at compile time for the two usual windows (11, 7) -- the tap loops unroll and the taps stay in scalar
// registers -- or 0: n_rt taps, one scalar load per tap.  The operations and their order are the same.
template <int NT>
__global__ void __launch_bounds__(kThreads)
image_compare_tiles(const float* __restrict__ a, const float* __restrict__ b, const uint8_t* __restrict__ mask, int view0, int H, int W,
                    int C, int G, Taps taps, int n_rt, double c1, double c2, int tiles_x, double* __restrict__ rows_out,
                    long long* __restrict__ counts_out, double* __restrict__ ssim_map) {
#pragma clang fp contract(off)
    const int n = NT ? NT : n_rt;
    constexpr int kUnroll = NT ? NT + 1 : 1;                 // of the tap loops
    extern __shared__ double s_dyn[];
    __shared__ double s_red[(kThreads / 64) * 2];
    __shared__ long long s_cnt[(kThreads / 64) * 2];
    const int tid = threadIdx.x;
    const int view = view0 + (int)blockIdx.y, tile = (int)blockIdx.x;
    const int ty = tile / tiles_x, tx = tile - ty * tiles_x;
    const int y0 = ty * kT, x0 = tx * kT;
    const int side = kT + n - 1, row_len = side * G, r = (n - 1) / 2;
    const int plane = side * kT;
    double* tmp = s_dyn;                                     // [5][side][kT]   row-blurred moments of one channel
    float* in_a = (float*)(tmp + kMoments * plane);          // [side][side][G] the tile and its halo, G channels
    float* in_b = in_a + side * row_len;
    const int64_t view_px = (int64_t)view * H * W;
    const int ly = tid / kT, lx = tid % kT;
    const int py = y0 + ly, px = x0 + lx;
    const int OH = H - n + 1, OW = W - n + 1;
    const bool centre = py < OH && px < OW;
    const bool pix_on = py < H && px < W && (!mask || mask[view_px + (int64_t)py * W + px] != 0);
    const bool ctr_on = centre && (!mask || mask[view_px + (int64_t)(py + r) * W + (px + r)] != 0);
    double acc[2] = {0.0, 0.0};                              // this lane's sse and ssim terms, channels in order
    for (int c0 = 0; c0 < C; c0 += G) {
        // a wave per row, the lanes along the row's floats: contiguous in memory when all channels are read (G == C)
        const int in_row = G == C ? (W - x0) * C : W - x0;   // the row's floats that lie inside the image
        for (int ry = tid >> 6; ry < side; ry += kThreads / 64) {
            const int gy = y0 + ry;
            const int64_t row_at = (view_px + (int64_t)gy * W + x0) * C;
            for (int j = tid & 63; j < row_len; j += 64) {
                float va = 0.f, vb = 0.f;                    // outside the image: read by no centre and no pixel
                if (gy < H && j < in_row) {
                    const int64_t at = row_at + (G == C ? j : j * C + c0);
                    va = a[at];
                    vb = b[at];
                }
                in_a[ry * row_len + j] = va;
                in_b[ry * row_len + j] = vb;
            }
        }
        __syncthreads();
        for (int g = 0; g < G; ++g) {
            // rows: lane -> (row ry, outputs xo and xo + 1); loaded column xo + k is tap k of the first and tap k - 1 of the second
            for (int i = tid; i < side * (kT / 2); i += kThreads) {
                const int ry = i / (kT / 2), xo = 2 * (i % (kT / 2));
                const float* ra = in_a + ry * row_len + xo * G + g;
                const float* rb = in_b + ry * row_len + xo * G + g;
                double m0[kMoments], m1[kMoments];
#pragma unroll
                for (int q = 0; q < kMoments; ++q) m0[q] = m1[q] = -0.0;
#pragma unroll kUnroll
                for (int k = 0; k <= n; ++k) {
                    const double da = (double)ra[k * G], db = (double)rb[k * G];
                    const double p[kMoments] = {da, db, da * da, db * db, da * db};
                    if (k < n) {
                        const double w = taps.w[k];
#pragma unroll
                        for (int q = 0; q < kMoments; ++q) m0[q] = m0[q] + w * p[q];
                    }
                    if (k > 0) {
                        const double w = taps.w[k - 1];
#pragma unroll
                        for (int q = 0; q < kMoments; ++q) m1[q] = m1[q] + w * p[q];
                    }
                }
#pragma unroll
                for (int q = 0; q < kMoments; ++q) {
                    tmp[q * plane + ry * kT + xo] = m0[q];
                    tmp[q * plane + ry * kT + xo + 1] = m1[q];
                }
            }
            __syncthreads();
            const double d = (double)in_a[ly * row_len + lx * G + g] - (double)in_b[ly * row_len + lx * G + g];
            const double e = d * d;
            acc[0] = acc[0] + (pix_on ? e : 0.0);
            if (centre) {
                double m[kMoments];
#pragma unroll
                for (int q = 0; q < kMoments; ++q) m[q] = -0.0;
#pragma unroll kUnroll
                for (int k = 0; k < n; ++k) {
                    const double w = taps.w[k];
#pragma unroll
                    for (int q = 0; q < kMoments; ++q) m[q] = m[q] + w * tmp[q * plane + (ly + k) * kT + lx];
                }
                const double mx = m[0], my = m[1];
                const double vx = m[2] - mx * mx, vy = m[3] - my * my, cxy = m[4] - mx * my;
                const double s = ((2.0 * mx * my + c1) * (2.0 * cxy + c2)) / ((mx * mx + my * my + c1) * (vx + vy + c2));
                if (ssim_map) ssim_map[(((int64_t)view * OH + py) * OW + px) * C + (c0 + g)] = s;
                acc[1] = acc[1] + (ctr_on ? s : 0.0);
            }
            __syncthreads();                                 // tmp and the tile are written again
        }
    }
    block_sum<2, kThreads>(acc, s_red);
    const long long n_pix = wave_sum((long long)(pix_on ? C : 0)), n_ctr = wave_sum((long long)(ctr_on ? C : 0));
    if ((tid & 63) == 0) {
        s_cnt[(tid >> 6) * 2] = n_pix;
        s_cnt[(tid >> 6) * 2 + 1] = n_ctr;
    }
    __syncthreads();
    if (tid < 2) {
        long long total = 0;
#pragma unroll
        for (int w = 0; w < kThreads / 64; ++w) total += s_cnt[w * 2 + tid];
        const int64_t row = (int64_t)view * gridDim.x + tile;
        counts_out[row * 2 + tid] = total;
        rows_out[row * 2 + tid] = acc[tid];
    }
}

// one workgroup per view: lane 0 adds the view's sse entries in tile order, lane 1 its ssim sums, from rows staged through LDS
// kStage at a time (a stage costs one round trip to memory; the additions are one dependent chain); the counts are integers
__global__ void __launch_bounds__(kFinishThreads)
image_compare_finish(const double* __restrict__ rows, const long long* __restrict__ counts, int tiles, double* __restrict__ sse,
                     long long* __restrict__ count, double* __restrict__ ssim_sum, long long* __restrict__ ssim_count) {
    __shared__ double s_stage[kStage * 2];
    __shared__ long long s_cnt[(kFinishThreads / 64) * 2];
    const int tid = threadIdx.x;
    const int64_t first = (int64_t)blockIdx.x * tiles;
    double acc = 0.0;
    long long n_pix = 0, n_ctr = 0;
    for (int base = 0; base < tiles; base += kStage) {
        const int nn = min(kStage, tiles - base);
        // rows past the last tile are +0.0: adding them changes no bit (the sum starts from +0.0 and is never -0.0)
        for (int e = tid; e < kStage * 2; e += kFinishThreads) s_stage[e] = e < nn * 2 ? rows[(first + base) * 2 + e] : 0.0;
        for (int t = tid; t < nn; t += kFinishThreads) {
            n_pix += counts[(first + base + t) * 2];
            n_ctr += counts[(first + base + t) * 2 + 1];
        }
        __syncthreads();
        if (tid < 2) {
#pragma unroll 16
            for (int t = 0; t < kStage; ++t) acc = acc + s_stage[t * 2 + tid];
        }
        __syncthreads();
    }
    n_pix = wave_sum(n_pix);
    n_ctr = wave_sum(n_ctr);
    if ((tid & 63) == 0) {
        s_cnt[(tid >> 6) * 2] = n_pix;
        s_cnt[(tid >> 6) * 2 + 1] = n_ctr;
    }
    __syncthreads();
    if (tid < 2) {
        long long total = 0;
#pragma unroll
        for (int w = 0; w < kFinishThreads / 64; ++w) total += s_cnt[w * 2 + tid];
        (tid == 0 ? count : ssim_count)[blockIdx.x] = total;
        (tid == 0 ? sse : ssim_sum)[blockIdx.x] = acc;
    }
}

bool shape_ok(int32_t n_views, int32_t height, int32_t width, int32_t channels, int32_t n_taps) {
    if (n_views < 1 || channels < 1 || channels > 4) return false;
    if (n_taps < 1 || n_taps > kMaxTaps || (n_taps & 1) == 0) return false;
    if (height < n_taps || width < n_taps) return false;
    return (int64_t)height * width * channels < ((int64_t)1 << 31);
}

bool constant_ok(double v) { return v >= 0.0 && v < (double)INFINITY; }       // a NaN fails both comparisons

}  // namespace

extern "C" int64_t ls2fm_image_compare_workspace_bytes(int32_t n_views, int32_t height, int32_t width, int32_t channels,
                                                       int32_t n_taps) {
    if (!shape_ok(n_views, height, width, channels, n_taps)) return (int64_t)LS2FM_ERR_INVALID_ARGUMENT;
    return (int64_t)image_layout(n_views, tiles_of(height, width), nullptr, nullptr);
}

extern "C" int ls2fm_image_compare(const float* a, const float* b, const uint8_t* mask, int32_t n_views, int32_t height, int32_t width,
                                   int32_t channels, const double* taps, int32_t n_taps, double c1, double c2, double* sse,
                                   int64_t* count, double* ssim_sum, int64_t* ssim_count, double* ssim_map, void* workspace,
                                   int64_t workspace_bytes, void* stream) {
    LS2FM_CHECK_ARG(a && b && taps && sse && count && ssim_sum && ssim_count);
    LS2FM_CHECK_ARG(shape_ok(n_views, height, width, channels, n_taps));
    LS2FM_CHECK_ARG(constant_ok(c1) && constant_ok(c2));
    const int64_t tiles = tiles_of(height, width);
    ImageWs w;
    if (!workspace || workspace_bytes < (int64_t)image_layout(n_views, tiles, nullptr, nullptr)) return LS2FM_ERR_WORKSPACE;
    image_layout(n_views, tiles, workspace, &w);
    hipStream_t st = (hipStream_t)stream;
    Taps t;
    for (int k = 0; k < kMaxTaps; ++k) t.w[k] = k < n_taps ? taps[k] : 0.0;
    const int group = channel_group(n_taps, channels);
    const size_t lds = tile_lds_bytes(n_taps, group);
    const int tiles_x = (width + kT - 1) / kT;
    auto* tiles_kernel = n_taps == 11 ? image_compare_tiles<11> : n_taps == 7 ? image_compare_tiles<7> : image_compare_tiles<0>;
    for (int v0 = 0; v0 < n_views; v0 += kMaxGridY)
        tiles_kernel<<<dim3((unsigned)tiles, (unsigned)std::min(n_views - v0, kMaxGridY)), kThreads, lds, st>>>(
            a, b, mask, v0, height, width, channels, group, t, n_taps, c1, c2, tiles_x, w.rows, w.counts, ssim_map);
    image_compare_finish<<<(unsigned)n_views, kFinishThreads, 0, st>>>(w.rows, w.counts, (int)tiles, sse, (long long*)count, ssim_sum,
                                                                      (long long*)ssim_count);
    return ls2fm_launch_status();
}
