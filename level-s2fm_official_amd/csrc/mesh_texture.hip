// Texture atlases of a mesh: from texels to surface points (ls2fm_texture_texels) and from a rasterisation back to colours
// (ls2fm_texture_render): the primitives under ls2fm.texture.  include/ls2fm.h states THE ATLAS RULE and THE TEXTURE RENDER RULE;
// tests/texture_restate.py repeats them in numpy.
//
// The atlas is per-face charts, two to a square cell, the cells Morton-packed by class in descending size.  A texel finds its
// face by arithmetic alone: its Morton code against the class starts (a table of at most LS2FM_TEXTURE_MAX_CLASSES entries in
// the kernel arguments: scalar registers), a shift for the cell, the half of the cell for the slot, one load of order[slot].  No
// search structure, no atomic, no workspace.  Every fp32 step is one rounded operation, so the texel's point is a pure function
// of the mesh and the packing, and row bands leave the bits of one call.
#include "ls2fm_device.h"

#include <cmath>

namespace {

constexpr int kTile = 16;              // LS2FM_TEXTURE_TILE
constexpr int kThreads = kTile * kTile;
constexpr int kMaxClasses = 8;         // LS2FM_TEXTURE_MAX_CLASSES
constexpr int kRenderThreads = 256;
constexpr int kRenderRowBits = 20;     // blockIdx.x counts 2^20 workgroups, blockIdx.y the rest

static_assert(kTile == LS2FM_TEXTURE_TILE && kMaxClasses == LS2FM_TEXTURE_MAX_CLASSES, "the header states the tile and the table size");

// the packing, by value.  Class c holds the Morton codes [start[c], start[c + 1]) and the slots [slot[c], slot[c + 1]).
struct Classes {
    int32_t n;
    int32_t log2_pitch[kMaxClasses];
    uint32_t start[kMaxClasses + 1];
    int32_t slot[kMaxClasses + 1];
};

// bit b of v to bit 2 b, for v < 2^16
__device__ __forceinline__ uint32_t spread(uint32_t v) {
    v = (v | (v << 8)) & 0x00FF00FFu;
    v = (v | (v << 4)) & 0x0F0F0F0Fu;
    v = (v | (v << 2)) & 0x33333333u;
    v = (v | (v << 1)) & 0x55555555u;
    return v;
}

__global__ void __launch_bounds__(kThreads)
texture_texels(const float* __restrict__ verts, int64_t n_verts, const int32_t* __restrict__ faces, int64_t n_faces, const int32_t* __restrict__ order,
               const int32_t* __restrict__ rot, Classes cls, int gutter, int size, int row_begin, int row_end,
               int32_t* __restrict__ face_out, float* __restrict__ point, float* __restrict__ normal, float* __restrict__ uv) {
#pragma clang fp contract(off)
    // tiles are aligned to the atlas, not to the band: the lanes of a tile share a cell once the pitch reaches the tile
    const int x = (int)blockIdx.x * kTile + ((int)threadIdx.x & (kTile - 1));
    const int y = (row_begin & ~(kTile - 1)) + (int)blockIdx.y * kTile + ((int)threadIdx.x >> 4);
    if (x >= size || y < row_begin || y >= row_end) return;
    const int64_t at = (int64_t)(y - row_begin) * size + x;
    const uint32_t m = spread((uint32_t)x) | (spread((uint32_t)y) << 1);
    int c = -1;
#pragma unroll
    for (int i = 0; i < kMaxClasses; ++i)
        if (i < cls.n && m >= cls.start[i]) c = i;
    bool owned = false;
    int k = 0, slot = 0, i = 0, j = 0;
    if (c >= 0) {                                            // cls.n >= 1 and start[0] == 0: always
        k = cls.log2_pitch[c];
        const int p = 1 << k;
        const uint32_t cell = (m - cls.start[c]) >> (2 * k);
        i = x & (p - 1);
        j = y & (p - 1);
        const bool second = i + j > p - 1;                   // chart B: chart A turned by 180 degrees about the cell's centre
        if (second) { i = p - 1 - i; j = p - 1 - j; }
        // the cell lies in its class and the slot holds a face: an odd last slot leaves its chart B unowned.  A cell past the
        // class's last has m >= start[c + 1]; only the last class of the table can meet one (the unused tail of the atlas).
        const int64_t s = (int64_t)cls.slot[c] + 2 * (int64_t)cell + (second ? 1 : 0);
        owned = m < cls.start[c + 1] && s < cls.slot[c + 1];
        slot = owned ? (int)s : 0;
    }
    float X[3] = {NAN, NAN, NAN}, N[3] = {NAN, NAN, NAN};
    int f = -1;
    if (owned) {
        f = order[slot];
        if (f < 0 || f >= n_faces) { f = -1; owned = false; }       // not a permutation: the texel stays unowned, nothing is read
    }
    if (owned) {
        const int r = min(max(rot[f], 0), 2);
        const int32_t* fv = faces + 3 * (int64_t)f;
        const int64_t ia = fv[r], ib = fv[r == 2 ? 0 : r + 1], ic = fv[r == 0 ? 2 : r - 1];
        const bool in_range = ia >= 0 && ia < n_verts && ib >= 0 && ib < n_verts && ic >= 0 && ic < n_verts;
        const int L = (1 << k) - 2 * gutter - 3;
        if (in_range) {
            const float s = __fdiv_rn((float)(i - gutter), (float)L), t = __fdiv_rn((float)(j - gutter), (float)L);
            float d1[3], d2[3];
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                const float va = verts[3 * ia + a];
                d1[a] = __fsub_rn(verts[3 * ib + a], va);
                d2[a] = __fsub_rn(verts[3 * ic + a], va);
                X[a] = __fadd_rn(__fadd_rn(va, __fmul_rn(s, d1[a])), __fmul_rn(t, d2[a]));
            }
            N[0] = __fsub_rn(__fmul_rn(d1[1], d2[2]), __fmul_rn(d1[2], d2[1]));
            N[1] = __fsub_rn(__fmul_rn(d1[2], d2[0]), __fmul_rn(d1[0], d2[2]));
            N[2] = __fsub_rn(__fmul_rn(d1[0], d2[1]), __fmul_rn(d1[1], d2[0]));
        }
        if (uv) {
            // a chart corner's texel writes that corner: q in the chart's order is vertex (r + q) mod 3 of the face
            const int q = (i == gutter && j == gutter) ? 0 : (i == gutter + L && j == gutter) ? 1 : (i == gutter && j == gutter + L) ? 2 : -1;
            if (q >= 0) {
                const int corner = r + q >= 3 ? r + q - 3 : r + q;
                float* o = uv + 6 * (int64_t)f + 2 * corner;
                o[0] = __fadd_rn((float)x, 0.5f);
                o[1] = __fadd_rn((float)y, 0.5f);
            }
        }
    }
    face_out[at] = f;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        point[3 * at + a] = X[a];
        normal[3 * at + a] = N[a];
    }
}

struct Background { float c[4]; };

// one axis of the bilinear sample about the texel centres: the two taps clamped to the texture, and the fraction
__device__ __forceinline__ void taps(float u, int size, int& t0, int& t1, float& frac) {
#pragma clang fp contract(off)
    const float s = __fsub_rn(u, 0.5f);
    const float u0 = floorf(s);
    frac = __fsub_rn(s, u0);
    // as a float first, so that the conversion is defined for every input: a NaN becomes -1 (fmaxf returns its other operand)
    const int b = (int)fminf(fmaxf(u0, -1.0f), (float)size);
    t0 = min(max(b, 0), size - 1);
    t1 = min(max(b + 1, 0), size - 1);
}

template <int C>
__global__ void __launch_bounds__(kRenderThreads)
texture_render(const int32_t* __restrict__ face_id, const float* __restrict__ bary, int64_t n_pixels, const float* __restrict__ uv,
               int64_t n_faces, const float* __restrict__ texture, int size, Background bg, float* __restrict__ out) {
#pragma clang fp contract(off)
    const int64_t at = ((((int64_t)blockIdx.y << kRenderRowBits) | blockIdx.x) * kRenderThreads) + threadIdx.x;
    if (at >= n_pixels) return;
    const int64_t f = face_id[at];
    float v[C];
#pragma unroll
    for (int c = 0; c < C; ++c) v[c] = bg.c[c];
    if (f >= 0 && f < n_faces) {
        const float w0 = bary[3 * at], w1 = bary[3 * at + 1], w2 = bary[3 * at + 2];
        const float* q = uv + 6 * f;
        const float x = __fadd_rn(__fadd_rn(__fmul_rn(w0, q[0]), __fmul_rn(w1, q[2])), __fmul_rn(w2, q[4]));
        const float y = __fadd_rn(__fadd_rn(__fmul_rn(w0, q[1]), __fmul_rn(w1, q[3])), __fmul_rn(w2, q[5]));
        int x0, x1, y0, y1;
        float tx, ty;
        taps(x, size, x0, x1, tx);
        taps(y, size, y0, y1, ty);
        const float* b00 = texture + ((int64_t)y0 * size + x0) * C;
        const float* b10 = texture + ((int64_t)y0 * size + x1) * C;
        const float* b01 = texture + ((int64_t)y1 * size + x0) * C;
        const float* b11 = texture + ((int64_t)y1 * size + x1) * C;
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const float r0 = __fadd_rn(b00[c], __fmul_rn(tx, __fsub_rn(b10[c], b00[c])));
            const float r1 = __fadd_rn(b01[c], __fmul_rn(tx, __fsub_rn(b11[c], b01[c])));
            v[c] = __fadd_rn(r0, __fmul_rn(ty, __fsub_rn(r1, r0)));
        }
    }
#pragma unroll
    for (int c = 0; c < C; ++c) out[C * at + c] = v[c];
}

bool size_ok(int32_t size) { return size >= 4 && size <= 32768 && (size & (size - 1)) == 0; }

// the table as the kernel takes it, from the classes' pitches and face counts; false for a table the rule does not admit
bool make_classes(int64_t n_faces, int32_t n_classes, const int32_t* log2_pitch, const int64_t* count, int32_t gutter, int32_t size,
                  Classes& out) {
    if (n_classes < 1 || n_classes > kMaxClasses || !log2_pitch || !count || gutter < 0 || gutter > 64) return false;
    int64_t at = 0, slot = 0;
    const int64_t area = (int64_t)size * size;
    out.n = n_classes;
    for (int c = 0; c < kMaxClasses; ++c) {
        const bool live = c < n_classes;
        if (live) {
            const int32_t k = log2_pitch[c];
            if (k < 2 || k > 15 || (1 << k) < 2 * gutter + 4) return false;
            if (c > 0 && k >= log2_pitch[c - 1]) return false;                   // descending
            if (count[c] < 0 || count[c] > n_faces) return false;
        }
        out.log2_pitch[c] = live ? log2_pitch[c] : 2;
        out.start[c] = (uint32_t)at;
        out.slot[c] = (int32_t)slot;
        if (live) {
            at += ((count[c] + 1) / 2) << (2 * log2_pitch[c]);
            slot += count[c];
            if (at > area || slot > n_faces) return false;                       // the atlas holds the cells
        }
    }
    out.start[kMaxClasses] = (uint32_t)at;
    out.slot[kMaxClasses] = (int32_t)slot;
    // start[c + 1] and slot[c + 1] of the last live class are the totals: the entries behind it repeat them
    return slot == n_faces;
}

}  // namespace

extern "C" int ls2fm_texture_texels(const float* verts, int64_t n_verts, const int32_t* faces, int64_t n_faces, const int32_t* order,
                                    const int32_t* rot, int32_t n_classes, const int32_t* class_log2_pitch, const int64_t* class_count,
                                    int32_t gutter, int32_t size, int32_t row_begin, int32_t row_end, int32_t* face, float* point,
                                    float* normal, float* uv, void* stream) {
    LS2FM_CHECK_ARG(n_verts >= 0 && n_faces >= 0 && n_faces < ((int64_t)1 << 31) && size_ok(size) && row_begin >= 0 &&
                    row_begin <= row_end && row_end <= size);
    Classes cls;
    LS2FM_CHECK_ARG(make_classes(n_faces, n_classes, class_log2_pitch, class_count, gutter, size, cls));
    if (row_begin == row_end) return LS2FM_OK;
    LS2FM_CHECK_ARG(face && point && normal && (n_faces == 0 || (faces && order && rot)) && (n_verts == 0 || verts));
    const int first = row_begin & ~(kTile - 1);
    const dim3 grid((unsigned)((size + kTile - 1) / kTile), (unsigned)((row_end - first + kTile - 1) / kTile));
    texture_texels<<<grid, kThreads, 0, (hipStream_t)stream>>>(verts, n_verts, faces, n_faces, order, rot, cls, gutter, size, row_begin, row_end,
                                                               face, point, normal, uv);
    return ls2fm_launch_status();
}

extern "C" int ls2fm_texture_render(const int32_t* face_id, const float* bary, int32_t n_views, int32_t height, int32_t width,
                                    const float* uv, int64_t n_faces, const float* texture, int32_t size, int32_t channels,
                                    const float* background, float* out, void* stream) {
    LS2FM_CHECK_ARG(n_views >= 0 && height >= 1 && height <= 32768 && width >= 1 && width <= 32768 &&
                    (int64_t)n_views * height * width < ((int64_t)1 << 40) && n_faces >= 0 && n_faces < ((int64_t)1 << 31) &&
                    size_ok(size) && channels >= 1 && channels <= 4);
    if (n_views == 0) return LS2FM_OK;
    LS2FM_CHECK_ARG(face_id && bary && texture && background && out && (n_faces == 0 || uv));
    Background bg = {{0.0f, 0.0f, 0.0f, 0.0f}};
    for (int c = 0; c < channels; ++c) bg.c[c] = background[c];      // on the host: `channels` floats, read before the call returns
    const int64_t n_pixels = (int64_t)n_views * height * width;
    const int64_t blocks = (n_pixels + kRenderThreads - 1) / kRenderThreads;
    const int64_t row = (int64_t)1 << kRenderRowBits;
    const dim3 grid((unsigned)(blocks < row ? blocks : row), (unsigned)((blocks + row - 1) / row));
    hipStream_t s = (hipStream_t)stream;
#define LS2FM_TEXTURE_LAUNCH(C) \
    texture_render<C><<<grid, kRenderThreads, 0, s>>>(face_id, bary, n_pixels, uv, n_faces, texture, size, bg, out)
    switch (channels) {
        case 1: LS2FM_TEXTURE_LAUNCH(1); break;
        case 2: LS2FM_TEXTURE_LAUNCH(2); break;
        case 3: LS2FM_TEXTURE_LAUNCH(3); break;
        default: LS2FM_TEXTURE_LAUNCH(4); break;
    }
#undef LS2FM_TEXTURE_LAUNCH
    return ls2fm_launch_status();
}
