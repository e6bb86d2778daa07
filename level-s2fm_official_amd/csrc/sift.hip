// Batched SIFT feature extraction (include/ls2fm.h, "SIFT feature extraction"): what `colmap feature_extractor` writes into its
// `keypoints` and `descriptors` tables (preparation/main.py:91) -- VLFeat-style DoG SIFT with COLMAP's default options, restated
// from the published algorithm -- for all views of a call.  tests/sift_restate.py repeats every rule in numpy.
//
//   sift_base_kernel      input -> the first octave's base image (2x linear up-sampling for first_octave = -1, a copy for 0)
//   sift_blur_kernel      one Gaussian level from the previous one: a 64 x 32 tile with its halo is read into LDS once, blurred
//                         along rows, then along columns, written once; the DoG plane is formed from the new level and the
//                         centre of the tile that is still in LDS
//   sift_down_kernel      every second pixel of level s = S - 1 -> the first level of the next octave
//   sift_detect_kernel    strict 3 x 3 x 3 extrema, the quadratic fit (at most 5 rounds), the acceptance tests; accepted
//                         candidates are appended through one INTEGER counter per view
//   sift_rank_kernel      the append order is not the output order: every candidate counts the keys below its own (keys are
//                         unique per view) and moves to that place
//   sift_orient_kernel    one wave per candidate: 36-bin histogram, six smoothing passes, the first two peaks in bin order
//   sift_select_kernel    the cap: rows of larger scale (ties: earlier rows) counted per candidate -> rows kept
//   sift_scan_kernel      one workgroup per view: exclusive scan of the rows kept -> output row of every candidate, counts
//   sift_describe_kernel  one wave per output row: 4 x 4 x 8 trilinear histogram, the two normalisations, uint8 in UBC order
//
// No floating-point atomic anywhere.  Histogram bins are summed in 2^-40 fixed point with 64-bit INTEGER adds in LDS: each fp32
// contribution times 2^40 is an exact integer, integer addition is associative, so a bin holds the same bits in whatever order
// the lanes arrive; everything else is per-thread arithmetic or a butterfly reduction in a fixed order.  A view's rows depend on
// that view's pixels alone, so a rerun, another batch around it or another chunking return the same bits.
#include "ls2fm_device.h"
#include "workspace.h"

#include <algorithm>
#include <cmath>
#include <vector>

namespace {

constexpr int kS = 3;                  // octave_resolution (the only one built)
constexpr int kLevels = kS + 3;        // Gaussian levels s = -1 .. S + 1 at index l = s + 1
constexpr int kDog = kLevels - 1;
constexpr int kPlanes = kLevels + kDog;
constexpr int kMaxOct = 4;
constexpr int kMinSide = 8;
constexpr int kThreads = 256;
constexpr int kTileX = 64, kTileY = 32;
constexpr int kMaxRadius = 16;         // the widest step (s = S + 1, sigma 3.09) has radius 13
constexpr int kTapStride = 2 * kMaxRadius + 1;
constexpr int kCandCap = 32768;        // candidates per view before the orientation step
constexpr int kMaxSide = 8192;         // input side: 14 bits per axis in the sort key at octave -1
constexpr int64_t kDefaultWorkspace = (int64_t)2 << 30;
constexpr float kTwoPi = 6.283185307179586f;
constexpr float kFix = 1099511627776.0f;          // 2^40
constexpr float kUnfix = 1.0f / 1099511627776.0f;

struct Img {
    int64_t pix;             // first pixel of the view in `pixels`
    int64_t base;            // workspace offsets in floats: the base image, then the octaves' planes (6 levels, 5 DoG)
    int64_t oct[kMaxOct];
    int32_t w, h, bw, bh;
    int32_t ow[kMaxOct], oh[kMaxOct];
    int32_t n_oct, view;
};

struct Cand {
    uint32_t key;            // octave << 30 | level << 28 | y cell << 14 | x cell  (the cell of the extremum)
    float x, y, s;           // refined, in octave units
};

struct Opts {
    int first_octave, max_features, max_orientations, upright, normalization;
    float peak, peak08, edge;
};

struct Chunk {
    int v0 = 0, v1 = 0, cap = 0;
    int max_base = 0, max_oct_pixels[kMaxOct] = {0, 0, 0, 0}, max_tiles[kMaxOct] = {0, 0, 0, 0}, n_oct = 0;
    std::vector<Img> imgs;
    int64_t floats = 0;
};

struct Ws {
    Img* imgs;
    float* taps;
    int32_t* cand_count;
    Cand* raw;
    Cand* sorted;
    float* scale;
    int32_t* n_ori;
    float* angles;
    int32_t* kept;
    int32_t* out_start;
    float* planes;
};

size_t ws_layout(int n_img, int cap, int64_t floats, char* base, Ws* w) {
    Workspace ws(base, 256);
    const size_t rows = (size_t)n_img * (size_t)cap;
    Ws t;
    t.imgs = ws.take<Img>((size_t)n_img);
    t.taps = ws.take<float>((size_t)kLevels * kTapStride);
    t.cand_count = ws.take<int32_t>((size_t)n_img);
    t.raw = ws.take<Cand>(rows);
    t.sorted = ws.take<Cand>(rows);
    t.scale = ws.take<float>(rows);
    t.n_ori = ws.take<int32_t>(rows);
    t.angles = ws.take<float>(2 * rows);
    t.kept = ws.take<int32_t>(rows);
    t.out_start = ws.take<int32_t>(rows);
    t.planes = ws.take<float>((size_t)floats);
    if (w) *w = t;
    return ws.bytes();
}

int check_opts(const ls2fm_sift_opts* o) {
    LS2FM_CHECK_ARG(o != nullptr);
    LS2FM_CHECK_ARG(o->first_octave == -1 || o->first_octave == 0);
    LS2FM_CHECK_ARG(o->num_octaves >= 1 && o->max_num_features >= 1 && o->max_num_orientations >= 1);
    LS2FM_CHECK_ARG(o->normalization == LS2FM_SIFT_L1_ROOT || o->normalization == LS2FM_SIFT_L2);
    LS2FM_CHECK_ARG(std::isfinite(o->peak_threshold) && o->peak_threshold >= 0.0 && std::isfinite(o->edge_threshold) && o->edge_threshold > 0.0);
    LS2FM_CHECK_ARG(o->max_workspace_bytes >= 0);
    if (o->octave_resolution != kS || o->num_octaves > kMaxOct || o->max_num_orientations > 2 ||
        o->max_num_features > LS2FM_MATCH_MAX_DESCRIPTORS)
        return LS2FM_ERR_UNSUPPORTED;
    return LS2FM_OK;
}

// the views of a call in chunks whose workspace stays under the limit (a chunk always holds at least one view)
int make_chunks(const int32_t* heights, const int32_t* widths, int32_t n_images, const ls2fm_sift_opts* o, std::vector<Chunk>* chunks,
                size_t* bytes) {
    const int st = check_opts(o);
    if (st != LS2FM_OK) return st;
    LS2FM_CHECK_ARG(heights && widths && n_images >= 1);
    bool big = false;
    for (int v = 0; v < n_images; ++v) {
        LS2FM_CHECK_ARG(heights[v] >= 16 && widths[v] >= 16);
        big = big || heights[v] > kMaxSide || widths[v] > kMaxSide;
    }
    if (big) return LS2FM_ERR_UNSUPPORTED;
    const int64_t limit = o->max_workspace_bytes > 0 ? o->max_workspace_bytes : kDefaultWorkspace;
    chunks->clear();
    size_t worst = 0;
    Chunk cur;
    auto close = [&]() { worst = std::max(worst, ws_layout((int)cur.imgs.size(), cur.cap, cur.floats, nullptr, nullptr)); chunks->push_back(cur); };
    for (int v = 0; v < n_images; ++v) {
        Img g{};
        g.w = widths[v]; g.h = heights[v]; g.view = v;
        const int up = o->first_octave == -1 ? 2 : 1;
        g.bw = g.w * up; g.bh = g.h * up;
        int64_t floats = (int64_t)g.bw * g.bh;
        int ow = g.bw, oh = g.bh;
        for (int k = 0; k < o->num_octaves && std::min(ow, oh) >= kMinSide; ++k) {
            g.ow[k] = ow; g.oh[k] = oh; g.n_oct = k + 1;
            floats += (int64_t)kPlanes * ow * oh;
            ow >>= 1; oh >>= 1;
        }
        const int cap = (int)std::min<int64_t>(kCandCap, (((int64_t)g.bw * g.bh / 4 + 255) / 256) * 256);
        if (!cur.imgs.empty()) {
            const size_t with = ws_layout((int)cur.imgs.size() + 1, std::max(cur.cap, cap), cur.floats + floats, nullptr, nullptr);
            if ((int64_t)with > limit || cur.imgs.size() >= 65535) { close(); cur = Chunk(); }
        }
        if (cur.imgs.empty()) cur.v0 = v;
        int64_t at = cur.floats;
        g.base = at; at += (int64_t)g.bw * g.bh;
        for (int k = 0; k < g.n_oct; ++k) {
            g.oct[k] = at; at += (int64_t)kPlanes * g.ow[k] * g.oh[k];
            cur.max_oct_pixels[k] = std::max(cur.max_oct_pixels[k], g.ow[k] * g.oh[k]);
            cur.max_tiles[k] = std::max(cur.max_tiles[k], ((g.ow[k] + kTileX - 1) / kTileX) * ((g.oh[k] + kTileY - 1) / kTileY));
        }
        cur.floats = at;
        cur.cap = std::max(cur.cap, cap);
        cur.max_base = std::max(cur.max_base, g.bw * g.bh);
        cur.n_oct = std::max(cur.n_oct, g.n_oct);
        cur.v1 = v + 1;
        cur.imgs.push_back(g);
    }
    close();
    *bytes = worst;
    return LS2FM_OK;
}

// normalised taps of radius ceil(4 sigma), computed in double and rounded once
int make_taps(double sigma, float* out) {
    const int r = (int)std::ceil(4.0 * sigma);
    double g[kTapStride], sum = 0.0;
    for (int k = -r; k <= r; ++k) { g[k + r] = std::exp(-0.5 * (k / sigma) * (k / sigma)); sum += g[k + r]; }
    for (int k = 0; k < kTapStride; ++k) out[k] = k <= 2 * r ? (float)(g[k] / sum) : 0.f;
    return r;
}

__global__ void __launch_bounds__(kThreads) sift_base_kernel(const float* __restrict__ pixels, const Img* __restrict__ imgs,
                                                             float* __restrict__ planes, int upsample) {
    const Img& g = imgs[blockIdx.y];
    const int i = (int)blockIdx.x * kThreads + threadIdx.x;
    if (i >= g.bw * g.bh) return;
    const int Y = i / g.bw, X = i - Y * g.bw;
    const float* src = pixels + g.pix;
    float v;
    if (upsample) {
        const int y = Y >> 1, x = X >> 1, x1 = min(x + 1, g.w - 1), y1 = min(y + 1, g.h - 1);
        const bool ox = X & 1, oy = Y & 1;
        const float a = ox ? 0.5f * (src[(int64_t)y * g.w + x] + src[(int64_t)y * g.w + x1]) : src[(int64_t)y * g.w + x];
        v = a;
        if (oy) {
            const float b = ox ? 0.5f * (src[(int64_t)y1 * g.w + x] + src[(int64_t)y1 * g.w + x1]) : src[(int64_t)y1 * g.w + x];
            v = 0.5f * (a + b);
        }
    } else {
        v = src[i];
    }
    planes[g.base + i] = v;
}

// level `level` of octave `oct` from the previous level (the base image for the first level of the first octave)
__global__ void __launch_bounds__(kThreads) sift_blur_kernel(const Img* __restrict__ imgs, float* __restrict__ planes,
                                                             const float* __restrict__ taps, int radius, int oct, int level) {
    __shared__ float in[kTileY + 2 * kMaxRadius][kTileX + 2 * kMaxRadius];
    __shared__ float tmp[kTileY + 2 * kMaxRadius][kTileX];
    __shared__ float wl[kTapStride];
    const Img& g = imgs[blockIdx.y];
    if (oct >= g.n_oct) return;
    const int ow = g.ow[oct], oh = g.oh[oct];
    const int tiles_x = (ow + kTileX - 1) / kTileX, tiles_y = (oh + kTileY - 1) / kTileY;
    const int t = (int)blockIdx.x;
    if (t >= tiles_x * tiles_y) return;
    const int ty0 = (t / tiles_x) * kTileY, tx0 = (t % tiles_x) * kTileX;
    const int64_t plane = (int64_t)ow * oh;
    const float* src = level == 0 ? planes + g.base : planes + g.oct[oct] + (int64_t)(level - 1) * plane;
    float* dst = planes + g.oct[oct] + (int64_t)level * plane;
    const int tid = threadIdx.x, r = radius, n_taps = 2 * r + 1;
    if (tid < kTapStride) wl[tid] = taps[tid];
    const int rows = kTileY + 2 * r, cols = kTileX + 2 * r;
    for (int i = tid; i < rows * cols; i += kThreads) {
        const int ry = i / cols, rx = i - ry * cols;
        const int gy = min(max(ty0 - r + ry, 0), oh - 1), gx = min(max(tx0 - r + rx, 0), ow - 1);
        in[ry][rx] = src[(int64_t)gy * ow + gx];
    }
    __syncthreads();
    for (int i = tid; i < rows * kTileX; i += kThreads) {
        const int ry = i >> 6, x = i & 63;
        float acc = 0.f;
        for (int k = 0; k < n_taps; ++k) acc = acc + wl[k] * in[ry][x + k];
        tmp[ry][x] = acc;
    }
    __syncthreads();
    for (int i = tid; i < kTileY * kTileX; i += kThreads) {
        const int y = i >> 6, x = i & 63;
        float acc = 0.f;
        for (int k = 0; k < n_taps; ++k) acc = acc + wl[k] * tmp[y + k][x];
        const int gy = ty0 + y, gx = tx0 + x;
        if (gy < oh && gx < ow) {
            dst[(int64_t)gy * ow + gx] = acc;
            if (level > 0) planes[g.oct[oct] + (int64_t)(kLevels + level - 1) * plane + (int64_t)gy * ow + gx] = acc - in[y + r][x + r];
        }
    }
}

__global__ void __launch_bounds__(kThreads) sift_down_kernel(const Img* __restrict__ imgs, float* __restrict__ planes, int oct) {
    const Img& g = imgs[blockIdx.y];
    if (oct >= g.n_oct) return;
    const int ow = g.ow[oct], oh = g.oh[oct], pw = g.ow[oct - 1];
    const int i = (int)blockIdx.x * kThreads + threadIdx.x;
    if (i >= ow * oh) return;
    const int y = i / ow, x = i - y * ow;
    const float* src = planes + g.oct[oct - 1] + (int64_t)kS * g.ow[oct - 1] * g.oh[oct - 1];      // index S = level s = S - 1
    planes[g.oct[oct] + i] = src[(int64_t)(2 * y) * pw + 2 * x];
}

struct Fit {
    float b0, b1, b2, val, dxx, dyy, dxy;
};

// the 3-D quadratic fit around (x, y) of DoG plane d; every product and sum rounds on its own (no contraction), in the order
// tests/sift_restate.py writes them
__device__ __forceinline__ Fit quadratic_fit(const float* __restrict__ dog, int64_t plane, int ow, int d, int y, int x) {
    const float* c = dog + (int64_t)d * plane + (int64_t)y * ow + x;
    const float* lo = c - plane;
    const float* hi = c + plane;
    const float v0 = c[0];
    const float Dx = 0.5f * (c[1] - c[-1]);
    const float Dy = 0.5f * (c[ow] - c[-ow]);
    const float Ds = 0.5f * (hi[0] - lo[0]);
    const float two = v0 + v0;
    const float Dxx = (c[1] + c[-1]) - two;
    const float Dyy = (c[ow] + c[-ow]) - two;
    const float Dss = (hi[0] + lo[0]) - two;
    const float Dxy = 0.25f * ((c[ow + 1] + c[-ow - 1]) - (c[ow - 1] + c[-ow + 1]));
    const float Dxs = 0.25f * ((hi[1] + lo[-1]) - (hi[-1] + lo[1]));
    const float Dys = 0.25f * ((hi[ow] + lo[-ow]) - (hi[-ow] + lo[ow]));
    const float c00 = Dyy * Dss - Dys * Dys;
    const float c01 = Dxs * Dys - Dxy * Dss;
    const float c02 = Dxy * Dys - Dxs * Dyy;
    const float c11 = Dxx * Dss - Dxs * Dxs;
    const float c12 = Dxy * Dxs - Dxx * Dys;
    const float c22 = Dxx * Dyy - Dxy * Dxy;
    const float det = (Dxx * c00 + Dxy * c01) + Dxs * c02;
    Fit f;
    f.b0 = f.b1 = f.b2 = 0.f;
    if (det != 0.f) {
        f.b0 = -(((c00 * Dx + c01 * Dy) + c02 * Ds) / det);
        f.b1 = -(((c01 * Dx + c11 * Dy) + c12 * Ds) / det);
        f.b2 = -(((c02 * Dx + c12 * Dy) + c22 * Ds) / det);
    }
    f.val = v0 + 0.5f * ((Dx * f.b0 + Dy * f.b1) + Ds * f.b2);
    f.dxx = Dxx; f.dyy = Dyy; f.dxy = Dxy;
    return f;
}

__global__ void __launch_bounds__(kThreads) sift_detect_kernel(const Img* __restrict__ imgs, const float* __restrict__ planes, int oct,
                                                               Opts o, int cap, Cand* __restrict__ raw, int32_t* __restrict__ cand_count) {
    const Img& g = imgs[blockIdx.y];
    if (oct >= g.n_oct) return;
    const int ow = g.ow[oct], oh = g.oh[oct];
    const int iw = ow - 2, ih = oh - 2;
    const int i = (int)blockIdx.x * kThreads + threadIdx.x;
    if (i >= kS * iw * ih) return;
    const int d = 1 + i / (iw * ih);
    const int rem = i - (d - 1) * (iw * ih);
    const int y0 = 1 + rem / iw, x0 = 1 + rem % iw;
    const int64_t plane = (int64_t)ow * oh;
    const float* dog = planes + g.oct[oct] + (int64_t)kLevels * plane;
    const float* c = dog + (int64_t)d * plane + (int64_t)y0 * ow + x0;
    const float v = c[0];
    if (!(fabsf(v) > o.peak08)) return;
    bool is_max = true, is_min = true;
    for (int ds = -1; ds <= 1; ++ds)
        for (int dy = -1; dy <= 1; ++dy)
            for (int dx = -1; dx <= 1; ++dx) {
                if (ds == 0 && dy == 0 && dx == 0) continue;
                const float n = c[(int64_t)ds * plane + dy * ow + dx];
                is_max = is_max && v > n;
                is_min = is_min && v < n;
            }
    if (!(is_max || is_min)) return;
    int x = x0, y = y0;
    Fit f;
    for (int round = 0; round < 5; ++round) {
        f = quadratic_fit(dog, plane, ow, d, y, x);
        const int dx = (f.b0 > 0.6f && x < ow - 2 ? 1 : 0) - (f.b0 < -0.6f && x > 1 ? 1 : 0);
        const int dy = (f.b1 > 0.6f && y < oh - 2 ? 1 : 0) - (f.b1 < -0.6f && y > 1 ? 1 : 0);
        if ((dx == 0 && dy == 0) || round == 4) break;        // the fifth fit is used where it stands
        x += dx; y += dy;
    }
    const float xn = (float)x + f.b0, yn = (float)y + f.b1, sn = (float)(d - 1) + f.b2;
    const float r = o.edge, tr = f.dxx + f.dyy, det2 = f.dxx * f.dyy - f.dxy * f.dxy;
    const float si = floorf(sn + 0.5f);
    const bool good = fabsf(f.b0) < 1.5f && fabsf(f.b1) < 1.5f && fabsf(f.b2) < 1.5f && fabsf(f.val) > o.peak && det2 > 0.f &&
                      (tr * tr) * r < ((r + 1.0f) * (r + 1.0f)) * det2 && xn >= 0.f && xn <= (float)(ow - 1) && yn >= 0.f &&
                      yn <= (float)(oh - 1) && si >= 0.f && si <= (float)(kS - 1);
    if (!good) return;
    const int at = atomicAdd(&cand_count[blockIdx.y], 1);      // integer counter: the order it leaves is undone by sift_rank_kernel
    if (at < cap) {
        Cand k;
        k.key = ((uint32_t)oct << 30) | ((uint32_t)(d - 1) << 28) | ((uint32_t)y0 << 14) | (uint32_t)x0;
        k.x = xn; k.y = yn; k.s = sn;
        raw[(int64_t)blockIdx.y * cap + at] = k;
    }
}

__global__ void __launch_bounds__(kThreads) sift_rank_kernel(const int32_t* __restrict__ cand_count, int cap, const uint4* __restrict__ raw,
                                                             uint4* __restrict__ sorted) {
    __shared__ uint32_t keys[kThreads];
    const int n = min(cand_count[blockIdx.y], cap);
    if ((int)blockIdx.x * kThreads >= n) return;
    const int tid = threadIdx.x, i = (int)blockIdx.x * kThreads + tid;
    const uint4* mine = raw + (int64_t)blockIdx.y * cap;        // a Cand as four words: key, x, y, s
    const uint32_t key = mine[min(i, n - 1)].x;
    int rank = 0;
    for (int t0 = 0; t0 < n; t0 += kThreads) {
        __syncthreads();
        keys[tid] = t0 + tid < n ? mine[t0 + tid].x : 0xffffffffu;
        __syncthreads();
        const int m = min(kThreads, n - t0);
        for (int j = 0; j < m; ++j) rank += keys[j] < key ? 1 : 0;
    }
    if (i < n) sorted[(int64_t)blockIdx.y * cap + rank] = mine[i];
}

// gradient of level L at (x, y), 1 <= x <= w - 2, 1 <= y <= h - 2 -> modulus and angle in [0, 2 pi)
__device__ __forceinline__ void gradient(const float* __restrict__ L, int ow, int x, int y, float& mod, float& ang) {
    const float* p = L + (int64_t)y * ow + x;
    const float gx = 0.5f * (p[1] - p[-1]);
    const float gy = 0.5f * (p[ow] - p[-ow]);
    mod = sqrtf(gx * gx + gy * gy);
    ang = atan2f(gy, gx);
    if (ang < 0.f) ang = ang + kTwoPi;
}

__device__ __forceinline__ const float* level_of(const Img& g, const float* planes, const Cand& c, int& oct, int& ow, int& oh) {
    oct = (int)(c.key >> 30);
    ow = g.ow[oct]; oh = g.oh[oct];
    const int si = (int)floorf(c.s + 0.5f);
    return planes + g.oct[oct] + (int64_t)(si + 1) * ow * oh;
}

__global__ void __launch_bounds__(64) sift_orient_kernel(const Img* __restrict__ imgs, const float* __restrict__ planes,
                                                         const int32_t* __restrict__ cand_count, int cap, Opts o,
                                                         const Cand* __restrict__ sorted, float* __restrict__ scale,
                                                         int32_t* __restrict__ n_ori, float* __restrict__ angles) {
    __shared__ unsigned long long hist[36];
    __shared__ float sm[2][36];
    const int n = min(cand_count[blockIdx.y], cap);
    const int j = (int)blockIdx.x;
    if (j >= n) return;
    const Img& g = imgs[blockIdx.y];
    const int64_t row = (int64_t)blockIdx.y * cap + j;
    const Cand c = sorted[row];
    int oct, ow, oh;
    const float* L = level_of(g, planes, c, oct, ow, oh);
    const int lane = threadIdx.x;
    const float sigma = 2.0158737f * exp2f(c.s / 3.0f);            // sigma0 = 1.6 * 2^(1/3)
    const float step = oct + o.first_octave < 0 ? 0.5f : (float)(1 << (oct + o.first_octave));
    if (lane == 0) scale[row] = sigma * step;
    if (o.upright) {
        if (lane == 0) { n_ori[row] = 1; angles[2 * row] = 0.f; }
        return;
    }
    if (lane < 36) hist[lane] = 0ull;
    __syncthreads();
    const float sw = 1.5f * sigma;
    const int W = max((int)floorf(3.0f * sw), 1);
    const int xi = (int)floorf(c.x + 0.5f), yi = (int)floorf(c.y + 0.5f);
    const int y_lo = max(-W, 1 - yi), y_hi = min(W, oh - 2 - yi), x_lo = max(-W, 1 - xi), x_hi = min(W, ow - 2 - xi);
    const int nx = x_hi - x_lo + 1, ny = y_hi - y_lo + 1;
    const int total = nx > 0 && ny > 0 ? nx * ny : 0;
    const float limit = (float)(W * W) + 0.6f, denom = 2.0f * sw * sw;
    for (int i = lane; i < total; i += 64) {
        const int ry = i / nx, rx = i - ry * nx;
        const int px = xi + x_lo + rx, py = yi + y_lo + ry;
        const float dx = (float)px - c.x, dy = (float)py - c.y;
        const float r2 = dx * dx + dy * dy;
        if (!(r2 < limit)) continue;
        float mod, ang;
        gradient(L, ow, px, py, mod, ang);
        const float wgt = expf(-(r2 / denom)) * mod;
        const float fbin = ang * (36.0f / kTwoPi);
        const float b = floorf(fbin - 0.5f);
        const float rb = (fbin - b) - 0.5f;
        const int bi = (int)b;
        atomicAdd(&hist[(bi + 36) % 36], (unsigned long long)((wgt * (1.0f - rb)) * kFix));
        atomicAdd(&hist[(bi + 1) % 36], (unsigned long long)((wgt * rb) * kFix));
    }
    __syncthreads();
    if (lane < 36) sm[0][lane] = (float)(long long)hist[lane] * kUnfix;
    __syncthreads();
    int cur = 0;
    for (int pass = 0; pass < 6; ++pass) {
        if (lane < 36) sm[cur ^ 1][lane] = ((sm[cur][(lane + 35) % 36] + sm[cur][lane]) + sm[cur][(lane + 1) % 36]) * (1.0f / 3.0f);
        cur ^= 1;
        __syncthreads();
    }
    const float h0 = lane < 36 ? sm[cur][lane] : 0.f;
    const float hm = lane < 36 ? sm[cur][(lane + 35) % 36] : 0.f;
    const float hp = lane < 36 ? sm[cur][(lane + 1) % 36] : 0.f;
    const float top = wave_max(h0);
    const bool peak = lane < 36 && h0 > 0.8f * top && h0 > hm && h0 > hp;
    const unsigned long long mask = __ballot(peak);
    const int before = __popcll(mask & ((1ull << lane) - 1ull));
    if (peak && before < o.max_orientations) {
        const float di = -0.5f * (hp - hm) / ((hp + hm) - (h0 + h0));
        angles[2 * row + before] = (kTwoPi / 36.0f) * (((float)lane + di) + 0.5f);
    }
    if (lane == 0) n_ori[row] = min(__popcll(mask), o.max_orientations);
}

// rows kept per candidate under the cap: the rows of larger scale (equal scale: of earlier candidates) come first
__global__ void __launch_bounds__(kThreads) sift_select_kernel(const int32_t* __restrict__ cand_count, int cap, int max_features,
                                                               const float* __restrict__ scale, const int32_t* __restrict__ n_ori,
                                                               int32_t* __restrict__ kept) {
    __shared__ float sc[kThreads];
    __shared__ int no[kThreads];
    const int n = min(cand_count[blockIdx.y], cap);
    if ((int)blockIdx.x * kThreads >= n) return;
    const int tid = threadIdx.x, j = (int)blockIdx.x * kThreads + tid;
    const int64_t base = (int64_t)blockIdx.y * cap;
    const float mine = scale[base + min(j, n - 1)];
    int before = 0;
    for (int t0 = 0; t0 < n; t0 += kThreads) {
        __syncthreads();
        sc[tid] = t0 + tid < n ? scale[base + t0 + tid] : 0.f;
        no[tid] = t0 + tid < n ? n_ori[base + t0 + tid] : 0;
        __syncthreads();
        const int m = min(kThreads, n - t0);
        for (int i = 0; i < m; ++i) before += (sc[i] > mine || (sc[i] == mine && t0 + i < j)) ? no[i] : 0;
    }
    if (j < n) kept[base + j] = min(max(max_features - before, 0), n_ori[base + j]);
}

__global__ void __launch_bounds__(kThreads) sift_scan_kernel(const Img* __restrict__ imgs, const int32_t* __restrict__ cand_count, int cap,
                                                             const int32_t* __restrict__ kept, int32_t* __restrict__ out_start,
                                                             int32_t* __restrict__ counts) {
    __shared__ int buf[2][kThreads];
    const int found = cand_count[blockIdx.x];
    const int n = min(found, cap);
    const int tid = threadIdx.x;
    const int64_t base = (int64_t)blockIdx.x * cap;
    int running = 0;
    for (int t0 = 0; t0 < n; t0 += kThreads) {
        const int v = t0 + tid < n ? kept[base + t0 + tid] : 0;
        int cur = 0;
        __syncthreads();
        buf[0][tid] = v;
        __syncthreads();
        for (int off = 1; off < kThreads; off <<= 1) {
            buf[cur ^ 1][tid] = buf[cur][tid] + (tid >= off ? buf[cur][tid - off] : 0);
            cur ^= 1;
            __syncthreads();
        }
        if (t0 + tid < n) out_start[base + t0 + tid] = running + buf[cur][tid] - v;
        running += buf[cur][kThreads - 1];
    }
    if (tid == 0) counts[imgs[blockIdx.x].view] = found > cap ? -1 : running;
}

__global__ void __launch_bounds__(64) sift_describe_kernel(const Img* __restrict__ imgs, const float* __restrict__ planes,
                                                           const int32_t* __restrict__ cand_count, int cap, Opts o,
                                                           const Cand* __restrict__ sorted, const float* __restrict__ scale,
                                                           const float* __restrict__ angles, const int32_t* __restrict__ kept,
                                                           const int32_t* __restrict__ out_start, float* __restrict__ keypoints,
                                                           uint8_t* __restrict__ descriptors, int32_t* __restrict__ keys) {
    __shared__ unsigned long long hist[128];
    const int n = min(cand_count[blockIdx.y], cap);
    const int j = (int)blockIdx.x >> 1, k = (int)blockIdx.x & 1;
    if (j >= n) return;
    const int64_t row = (int64_t)blockIdx.y * cap + j;
    if (k >= kept[row]) return;
    const Img& g = imgs[blockIdx.y];
    const Cand c = sorted[row];
    int oct, ow, oh;
    const float* L = level_of(g, planes, c, oct, ow, oh);
    const int lane = threadIdx.x;
    const float sigma = 2.0158737f * exp2f(c.s / 3.0f);
    const float angle = angles[2 * row + k];
    hist[lane] = 0ull;
    hist[lane + 64] = 0ull;
    __syncthreads();
    const float sbp = 3.0f * sigma;
    const int W = (int)floorf(3.5355339f * sbp + 0.5f);              // sqrt(2) * (4 + 1) / 2 bins
    const int xi = (int)floorf(c.x + 0.5f), yi = (int)floorf(c.y + 0.5f);
    const int y_lo = max(-W, 1 - yi), y_hi = min(W, oh - 2 - yi), x_lo = max(-W, 1 - xi), x_hi = min(W, ow - 2 - xi);
    const int nx = x_hi - x_lo + 1, ny = y_hi - y_lo + 1;
    const int total = nx > 0 && ny > 0 ? nx * ny : 0;
    const float ct = cosf(angle), st = sinf(angle);
    for (int i = lane; i < total; i += 64) {
        const int ry = i / nx, rx = i - ry * nx;
        const int px = xi + x_lo + rx, py = yi + y_lo + ry;
        float mod, ang;
        gradient(L, ow, px, py, mod, ang);
        const float dx = (float)px - c.x, dy = (float)py - c.y;
        float th = ang - angle;
        if (th < 0.f) th = th + kTwoPi;
        if (th >= kTwoPi) th = th - kTwoPi;
        const float nxf = (ct * dx + st * dy) / sbp;
        const float nyf = (ct * dy - st * dx) / sbp;
        const float nt = th * (8.0f / kTwoPi);
        const float win = expf(-((nxf * nxf + nyf * nyf) / 8.0f)) * mod;
        const float bx = floorf(nxf - 0.5f), by = floorf(nyf - 0.5f), bt = floorf(nt);
        const float rxf = (nxf - bx) - 0.5f, ryf = (nyf - by) - 0.5f, rt = nt - bt;
        const int bxi = (int)bx, byi = (int)by, bti = (int)bt;
#pragma unroll
        for (int ex = 0; ex < 2; ++ex)
#pragma unroll
            for (int ey = 0; ey < 2; ++ey) {
                const int cx = bxi + ex, cy = byi + ey;
                if (cx < -2 || cx >= 2 || cy < -2 || cy >= 2) continue;
                const float wxy = (win * (ex ? rxf : 1.0f - rxf)) * (ey ? ryf : 1.0f - ryf);
#pragma unroll
                for (int et = 0; et < 2; ++et) {
                    const float v = wxy * (et ? rt : 1.0f - rt);
                    atomicAdd(&hist[((bti + et) & 7) + 8 * (cx + 2) + 32 * (cy + 2)], (unsigned long long)(v * kFix));
                }
            }
    }
    __syncthreads();
    float d0 = (float)(long long)hist[lane] * kUnfix, d1 = (float)(long long)hist[lane + 64] * kUnfix;
#pragma unroll
    for (int pass = 0; pass < 2; ++pass) {
        const float nrm = fmaxf(sqrtf(wave_sum(d0 * d0 + d1 * d1)), 1e-30f);
        d0 = d0 / nrm; d1 = d1 / nrm;
        if (pass == 0) { d0 = fminf(d0, 0.2f); d1 = fminf(d1, 0.2f); }
    }
    if (o.normalization == LS2FM_SIFT_L1_ROOT) {
        const float sum = fmaxf(wave_sum(d0 + d1), 1e-30f);
        d0 = sqrtf(d0 / sum); d1 = sqrtf(d1 / sum);
    } else {
        const float nrm = fmaxf(sqrtf(wave_sum(d0 * d0 + d1 * d1)), 1e-30f);
        d0 = d0 / nrm; d1 = d1 / nrm;
    }
    const int64_t out = (int64_t)g.view * o.max_features + out_start[row] + k;
    uint8_t* dst = descriptors + out * 128;
    const int t = lane & 7, cell = lane >> 3;                      // VLFeat index 8 cell + t -> UBC index 8 cell + (8 - t) % 8
    const int ubc = 8 * cell + ((8 - t) & 7);
    dst[ubc] = (uint8_t)fminf(floorf(512.0f * d0 + 0.5f), 255.0f);
    dst[ubc + 64] = (uint8_t)fminf(floorf(512.0f * d1 + 0.5f), 255.0f);
    if (lane == 0) {
        const float step = oct + o.first_octave < 0 ? 0.5f : (float)(1 << (oct + o.first_octave));
        float* kp = keypoints + out * 4;
        kp[0] = c.x * step + 0.5f; kp[1] = c.y * step + 0.5f; kp[2] = scale[row]; kp[3] = angle;
        if (keys) { keys[2 * out] = (int32_t)c.key; keys[2 * out + 1] = k; }
    }
}

unsigned blocks_for(int64_t n) { return (unsigned)std::max<int64_t>((n + kThreads - 1) / kThreads, 1); }

}  // namespace

extern "C" int64_t ls2fm_sift_workspace_bytes(const int32_t* heights, const int32_t* widths, int32_t n_images, const ls2fm_sift_opts* opts) {
    std::vector<Chunk> chunks;
    size_t bytes = 0;
    const int st = make_chunks(heights, widths, n_images, opts, &chunks, &bytes);
    if (st != LS2FM_OK) return st;
    return (int64_t)bytes;
}

extern "C" int ls2fm_sift_extract(const float* pixels, const int64_t* image_offset, const int32_t* heights, const int32_t* widths,
                                  int32_t n_images, const ls2fm_sift_opts* opts, float* keypoints, uint8_t* descriptors, int32_t* counts,
                                  void* workspace, void* stream) {
    std::vector<Chunk> chunks;
    size_t bytes = 0;
    const int st = make_chunks(heights, widths, n_images, opts, &chunks, &bytes);
    if (st != LS2FM_OK) return st;
    LS2FM_CHECK_ARG(pixels && image_offset && keypoints && descriptors && counts);
    for (int v = 0; v < n_images; ++v) LS2FM_CHECK_ARG(image_offset[v] >= 0);
    LS2FM_CHECK_ARG(opts->debug_levels == nullptr || n_images == 1);
    if (!workspace || ((uintptr_t)workspace & 255) != 0) return LS2FM_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    Opts o;
    o.first_octave = opts->first_octave; o.max_features = opts->max_num_features; o.max_orientations = opts->max_num_orientations;
    o.upright = opts->upright != 0; o.normalization = opts->normalization;
    o.peak = (float)opts->peak_threshold; o.peak08 = (float)(0.8 * opts->peak_threshold); o.edge = (float)opts->edge_threshold;
    // blur steps in double: the first level from the base image, then level l from l - 1
    float taps[kLevels][kTapStride];
    int radius[kLevels];
    double sig[kLevels];
    const double sigma0 = 1.6 * std::pow(2.0, 1.0 / kS), base_blur = 0.5 * std::pow(2.0, -(double)opts->first_octave);
    for (int l = 0; l < kLevels; ++l) sig[l] = sigma0 * std::pow(2.0, (double)(l - 1) / kS);
    for (int l = 0; l < kLevels; ++l) {
        const double prev = l == 0 ? base_blur : sig[l - 1];
        radius[l] = make_taps(std::sqrt(sig[l] * sig[l] - prev * prev), taps[l]);
        if (radius[l] > kMaxRadius) return LS2FM_ERR_UNSUPPORTED;
    }
    for (Chunk& ch : chunks) {
        const int n_img = (int)ch.imgs.size();
        for (Img& g : ch.imgs) g.pix = image_offset[g.view];
        Ws w;
        ws_layout(n_img, ch.cap, ch.floats, (char*)workspace, &w);
        // host tables from pageable memory: the runtime stages the copy before this returns; nothing is read back
        if (hipMemcpyAsync(w.imgs, ch.imgs.data(), sizeof(Img) * (size_t)n_img, hipMemcpyHostToDevice, s) != hipSuccess ||
            hipMemcpyAsync(w.taps, taps, sizeof(taps), hipMemcpyHostToDevice, s) != hipSuccess ||
            hipMemsetAsync(w.cand_count, 0, sizeof(int32_t) * (size_t)n_img, s) != hipSuccess)
            return ls2fm_launch_status();
        const dim3 block(kThreads);
        sift_base_kernel<<<dim3(blocks_for(ch.max_base), n_img), block, 0, s>>>(pixels, w.imgs, w.planes, opts->first_octave == -1);
        for (int k = 0; k < ch.n_oct; ++k) {
            if (k > 0) sift_down_kernel<<<dim3(blocks_for(ch.max_oct_pixels[k]), n_img), block, 0, s>>>(w.imgs, w.planes, k);
            for (int l = k > 0 ? 1 : 0; l < kLevels; ++l)
                sift_blur_kernel<<<dim3((unsigned)ch.max_tiles[k], n_img), block, 0, s>>>(w.imgs, w.planes, w.taps + l * kTapStride, radius[l], k, l);
            sift_detect_kernel<<<dim3(blocks_for((int64_t)kS * ch.max_oct_pixels[k]), n_img), block, 0, s>>>(w.imgs, w.planes, k, o, ch.cap, w.raw,
                                                                                                          w.cand_count);
        }
        const unsigned cand_blocks = (unsigned)(ch.cap / kThreads);
        sift_rank_kernel<<<dim3(cand_blocks, n_img), block, 0, s>>>(w.cand_count, ch.cap, (const uint4*)w.raw, (uint4*)w.sorted);
        sift_orient_kernel<<<dim3((unsigned)ch.cap, n_img), dim3(64), 0, s>>>(w.imgs, w.planes, w.cand_count, ch.cap, o, w.sorted, w.scale, w.n_ori,
                                                                           w.angles);
        sift_select_kernel<<<dim3(cand_blocks, n_img), block, 0, s>>>(w.cand_count, ch.cap, o.max_features, w.scale, w.n_ori, w.kept);
        sift_scan_kernel<<<dim3((unsigned)n_img), block, 0, s>>>(w.imgs, w.cand_count, ch.cap, w.kept, w.out_start, counts);
        sift_describe_kernel<<<dim3((unsigned)(2 * ch.cap), n_img), dim3(64), 0, s>>>(w.imgs, w.planes, w.cand_count, ch.cap, o, w.sorted, w.scale,
                                                                                   w.angles, w.kept, w.out_start, keypoints, descriptors, opts->debug_keys);
        if (opts->debug_levels) {
            const Img& g = ch.imgs[0];
            int64_t at = 0;
            for (int k = 0; k < g.n_oct; ++k) {
                const int64_t nfl = (int64_t)kLevels * g.ow[k] * g.oh[k];
                if (hipMemcpyAsync(opts->debug_levels + at, w.planes + g.oct[k], sizeof(float) * (size_t)nfl, hipMemcpyDeviceToDevice, s) != hipSuccess)
                    return ls2fm_launch_status();
                at += nfl;
            }
        }
        const int lst = ls2fm_launch_status();
        if (lst != LS2FM_OK) return lst;
    }
    return LS2FM_OK;
}
