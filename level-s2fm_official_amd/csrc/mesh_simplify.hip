// Mesh simplification by vertex clustering with quadric error metrics (ls2fm.simplify; Lindstrom 2000): every cell of an absolute
// lattice of side `cell` keeps one vertex, placed where the quadrics of the faces that touch the cell are smallest.
// include/ls2fm.h states THE CLUSTERING RULE; tests/simplify_restate.py repeats it in numpy.
//
// The calls, with torch's stable sorts and prefix sums between them (plumbing, as ls2fm.metrics.voxel_downsample's):
//   ls2fm_mesh_simplify_keys    simplify_vertex_keys   one lane per vertex: the 63-bit cell key, the bad count
//                               simplify_face_classes  one lane per face: invalid / collapsed / surviving, the surviving count
//     -- sort the vertex keys --
//   ls2fm_mesh_simplify_mark    simplify_vertex_heads  one lane per sorted vertex: the position of its cell's first sorted vertex
//                               simplify_corners       one lane per face: the contributing corners' cells, the output cells marked
//     -- sort the corner cells, prefix sum of the marks --
//   ls2fm_mesh_simplify_index   simplify_vertex_index  vertex_map and the list of output cells
//                               simplify_face_index    the surviving faces in output indices
//     -- duplicate faces, the one host read of the counts --
//   ls2fm_mesh_simplify_place   simplify_sums          ONE WAVE per output cell: the hot path.  Lane l takes entries l, l + 64, ...
//                                                      of the cell's vertex segment and of its corner segment, the face quadric
//                                                      formed in registers from three gathered vertices; wave_sum ends it
//                               simplify_solve         one lane per output cell: the 3 x 3 solve, the placement
//   ls2fm_mesh_simplify_emit    simplify_emit_faces    the kept faces to their places
// No floating-point atomic: the only atomics are the two integer counts.
#include <cstdint>

#include "lm_math.h"
#include "ls2fm_device.h"
#include "workspace.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kBits = 21;                              // per axis of the key, as ls2fm.metrics.voxel_downsample packs it
constexpr int kBias = 1 << (kBits - 1);
constexpr int64_t kInvalidKey = -1;                    // every cell's key is >= 0: an invalid vertex sorts in front of them all
constexpr int32_t kNoCell = INT32_MAX;                 // a corner that does not contribute sorts behind every cell
constexpr int kQ = LS2FM_SIMPLIFY_SUMS;                // 13 sums before the colour channels
constexpr int kMaxChannels = 4;
enum { FACE_INVALID = 0, FACE_COLLAPSED = 1, FACE_SURVIVES = 2 };

unsigned blocks_of(int64_t n) { return (unsigned)((n + kThreads - 1) / kThreads); }
bool counts_ok(int64_t n_verts, int64_t n_faces) {
    return n_verts >= 0 && n_verts < ((int64_t)1 << 31) && n_faces >= 0 && 3 * n_faces < ((int64_t)1 << 31);
}
bool cell_ok(float cell) { return cell > 0.0f && cell < INFINITY; }

struct SimplifyWs {
    int32_t* vert_head;        // [n_verts]  position in the sorted vertex list of the first vertex of the vertex's cell, -1 invalid
    int32_t* out_head;         // [n_verts]  the first n_out entries: that position for output cell r
};

size_t simplify_layout(int64_t n_verts, void* base, SimplifyWs* w) {
    Workspace ws(base, 256);
    int32_t* vert_head = ws.take<int32_t>((size_t)n_verts);
    int32_t* out_head = ws.take<int32_t>((size_t)n_verts);
    if (w) *w = {vert_head, out_head};
    return ws.bytes();
}

// first position i of the ascending a[0 .. n) with a[i] >= x
template <typename T>
__device__ __forceinline__ int64_t lower_bound(const T* __restrict__ a, int64_t n, T x) {
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (a[mid] < x) lo = mid + 1; else hi = mid;
    }
    return lo;
}

__global__ void __launch_bounds__(kThreads)
simplify_vertex_keys(const float* __restrict__ verts, int n_verts, double cell, int64_t* __restrict__ vert_key, int64_t* counts) {
    const int64_t v = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (v >= n_verts) return;
    const float x[3] = {verts[3 * v], verts[3 * v + 1], verts[3 * v + 2]};
    int64_t key = kInvalidKey;
    if (isfinite(x[0]) && isfinite(x[1]) && isfinite(x[2])) {
        bool fits = true;
        int64_t packed = 0;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const double k = floor((double)x[a] / cell);
            fits = fits && k >= -(double)kBias && k < (double)kBias;
            packed = (packed << kBits) | (fits ? (int64_t)k + kBias : 0);
        }
        if (fits) key = packed;
        else atomicAdd((unsigned long long*)&counts[1], 1ull);
    }
    vert_key[v] = key;
}

__global__ void __launch_bounds__(kThreads)
simplify_face_classes(const int64_t* __restrict__ vert_key, const int32_t* __restrict__ faces, int n_faces,
                      uint8_t* __restrict__ face_class, int64_t* counts) {
    const int64_t f = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    int cls = FACE_INVALID;
    if (f < n_faces) {
        const int64_t ka = vert_key[faces[3 * f]], kb = vert_key[faces[3 * f + 1]], kc = vert_key[faces[3 * f + 2]];
        if (ka != kInvalidKey && kb != kInvalidKey && kc != kInvalidKey)
            cls = ka != kb && kb != kc && ka != kc ? FACE_SURVIVES : FACE_COLLAPSED;
        if (face_class) face_class[f] = (uint8_t)cls;
    }
    const int n = wave_sum(cls == FACE_SURVIVES ? 1 : 0);
    if ((threadIdx.x & 63) == 0 && n) atomicAdd((unsigned long long*)&counts[0], (unsigned long long)n);
}

__global__ void __launch_bounds__(kThreads)
simplify_vertex_heads(const int64_t* __restrict__ sorted_key, const int64_t* __restrict__ sorted_vert, int n_verts,
                      int32_t* __restrict__ vert_head) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n_verts) return;
    const int64_t key = sorted_key[i], v = sorted_vert[i];
    if (v < 0 || v >= n_verts) return;                 // a permutation has none
    vert_head[v] = key == kInvalidKey ? -1 : (int32_t)lower_bound(sorted_key, (int64_t)n_verts, key);
}

__global__ void __launch_bounds__(kThreads)
simplify_corners(const int32_t* __restrict__ vert_head, const int32_t* __restrict__ faces, const uint8_t* __restrict__ face_class,
                 int n_faces, int n_verts, int32_t* __restrict__ corner_head, int32_t* __restrict__ head_used) {
    const int64_t f = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (f >= n_faces) return;
    const int cls = face_class[f];
    int32_t h[3] = {kNoCell, kNoCell, kNoCell};
    if (cls != FACE_INVALID) {
#pragma unroll
        for (int k = 0; k < 3; ++k) h[k] = vert_head[faces[3 * f + k]];
    }
    const bool in_range = h[0] >= 0 && h[0] < n_verts && h[1] >= 0 && h[1] < n_verts && h[2] >= 0 && h[2] < n_verts;
    corner_head[3 * f] = h[0];
    corner_head[3 * f + 1] = h[1] == h[0] ? kNoCell : h[1];
    corner_head[3 * f + 2] = h[2] == h[0] || h[2] == h[1] ? kNoCell : h[2];
    if (cls == FACE_SURVIVES && in_range) {            // in_range: always, for a sorted_vert that is a permutation
#pragma unroll
        for (int k = 0; k < 3; ++k) head_used[h[k]] = 1;          // every writer stores the same value
    }
}

// lane i as a vertex: its vertex_map entry; lane i as a sorted position: the output cell that starts there
__global__ void __launch_bounds__(kThreads)
simplify_vertex_index(const int32_t* __restrict__ vert_head, const int32_t* __restrict__ head_used, const int32_t* __restrict__ head_rank,
                      int n_verts, int32_t* __restrict__ vertex_map, int32_t* __restrict__ out_head) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n_verts) return;
    const int32_t h = vert_head[i];
    vertex_map[i] = h >= 0 && h < n_verts && head_used[h] ? head_rank[h] - 1 : -1;
    const int32_t rank = head_rank[i];                 // the inclusive prefix sum of head_used: in [1, n_verts] where head_used is set
    if (head_used[i] && rank >= 1 && rank <= n_verts) out_head[rank - 1] = (int32_t)i;
}

__global__ void __launch_bounds__(kThreads)
simplify_face_index(const int32_t* __restrict__ vertex_map, const int32_t* __restrict__ faces, const uint8_t* __restrict__ face_class,
                    int n_faces, int32_t* __restrict__ face_index) {
    const int64_t f = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (f >= n_faces) return;
    const bool on = face_class[f] == FACE_SURVIVES;
#pragma unroll
    for (int k = 0; k < 3; ++k) face_index[3 * f + k] = on ? vertex_map[faces[3 * f + k]] : -1;
}

// the centre of the cell of `key`: (k + 0.5) cell, k + 0.5 exact, one rounding
__device__ __forceinline__ void cell_centre(int64_t key, double cell, double (&g)[3]) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const int k = (int)((key >> (kBits * (2 - a))) & ((1 << kBits) - 1)) - kBias;
        g[a] = ((double)k + 0.5) * cell;
    }
}

// one wave per output cell.  Lane l adds entries l, l + 64, l + 128, ... of the cell's segment of the sorted vertex list and then of
// the sorted corner list, each quantity into a running sum of its own that starts at +0; wave_sum (the xor butterfly 32 ... 1) adds
// the 64 lanes.  sums [n_out][13 + channels], count [n_out].
__global__ void __launch_bounds__(kThreads)
simplify_sums(const float* __restrict__ verts, const float* __restrict__ colors, int channels, const int32_t* __restrict__ faces,
              double cell, const int64_t* __restrict__ sorted_key, const int64_t* __restrict__ sorted_vert, int64_t n_verts,
              const int32_t* __restrict__ sorted_corner_head, const int64_t* __restrict__ sorted_corner, int64_t n_corners,
              const int32_t* __restrict__ out_head, int n_out, double* __restrict__ sums, int32_t* __restrict__ count) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63;
    // the wave's cell and its head position are the same in every lane: said so, they live in scalar registers and the binary
    // search over the sorted corners below is one search per wave, not 64
    const int64_t r = (int64_t)blockIdx.x * kWaves + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (r >= n_out) return;                                        // the whole wave
    const int32_t hp = __builtin_amdgcn_readfirstlane(out_head[r]);
    if (hp < 0 || hp >= n_verts) return;                           // never, for the out_head ls2fm_mesh_simplify_index wrote
    const int64_t key = sorted_key[hp];
    double g[3];
    cell_centre(key, cell, g);
    double acc[kQ + kMaxChannels];
#pragma unroll
    for (int q = 0; q < kQ + kMaxChannels; ++q) acc[q] = 0.0;
    int m = 0;
    for (int64_t base = hp;; base += 64) {
        const int64_t i = base + lane;
        const bool in = i < n_verts && sorted_key[i] == key;
        if (in) {
            const int64_t v = min(max(sorted_vert[i], (int64_t)0), n_verts - 1);
#pragma unroll
            for (int a = 0; a < 3; ++a) acc[10 + a] += (double)verts[3 * v + a] - g[a];
#pragma unroll
            for (int c = 0; c < kMaxChannels; ++c)
                if (c < channels) acc[kQ + c] += (double)colors[v * channels + c];
            ++m;
        }
        if (__ballot(in) != ~0ull) break;
    }
    for (int64_t base = lower_bound(sorted_corner_head, n_corners, hp);; base += 64) {
        const int64_t i = base + lane;
        const bool in = i < n_corners && sorted_corner_head[i] == hp;
        if (in) {
            const int64_t f = min(max(sorted_corner[i], (int64_t)0), n_corners - 1) / 3;
            double p[3][3];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const int64_t v = faces[3 * f + k];
#pragma unroll
                for (int a = 0; a < 3; ++a) p[k][a] = (double)verts[3 * v + a] - g[a];
            }
            double u[3], w[3];
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                u[a] = p[1][a] - p[0][a];
                w[a] = p[2][a] - p[0][a];
            }
            const double n[3] = {u[1] * w[2] - u[2] * w[1], u[2] * w[0] - u[0] * w[2], u[0] * w[1] - u[1] * w[0]};
            const double d = (n[0] * p[0][0] + n[1] * p[0][1]) + n[2] * p[0][2];
            acc[0] += n[0] * n[0];
            acc[1] += n[0] * n[1];
            acc[2] += n[0] * n[2];
            acc[3] += n[1] * n[1];
            acc[4] += n[1] * n[2];
            acc[5] += n[2] * n[2];
            acc[6] += d * n[0];
            acc[7] += d * n[1];
            acc[8] += d * n[2];
            acc[9] += d * d;
        }
        if (__ballot(in) != ~0ull) break;
    }
    const int ns = kQ + channels;
#pragma unroll
    for (int q = 0; q < kQ + kMaxChannels; ++q)
        if (q < ns) acc[q] = wave_sum(acc[q]);                     // uniform: a mesh without colours sums 13 quantities, not 17
    m = wave_sum(m);
    if (lane != 0) return;
#pragma unroll
    for (int q = 0; q < kQ + kMaxChannels; ++q)
        if (q < ns) sums[r * ns + q] = acc[q];
    count[r] = m;
}

__global__ void __launch_bounds__(kThreads)
simplify_solve(const double* __restrict__ sums, const int32_t* __restrict__ count, int channels, double cell, int mean_only, double reg,
               const int64_t* __restrict__ sorted_key, const int32_t* __restrict__ out_head, int n_verts, int n_out, float* __restrict__ out_verts,
               float* __restrict__ out_colors) {
#pragma clang fp contract(off)
    const int64_t r = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (r >= n_out) return;
    const int ns = kQ + channels;
    const double* s = sums + r * ns;
    const double m = (double)count[r];
    double g[3], x[3];
    const int32_t hp = out_head[r];
    if (hp < 0 || hp >= n_verts) return;
    cell_centre(sorted_key[hp], cell, g);
#pragma unroll
    for (int a = 0; a < 3; ++a) x[a] = s[10 + a] / m;
    const double t = (s[0] + s[3]) + s[5];
    if (!mean_only && t != 0.0 && isfinite(t)) {
        const double lam = reg * t;
        const double sys[9] = {s[0], s[1], s[2], s[3], s[4], s[5], -(s[6] + lam * x[0]), -(s[7] + lam * x[1]), -(s[8] + lam * x[2])};
        const double one[3] = {1.0, 1.0, 1.0};
        double y[3];
        const double half = cell / 2.0;
        if (lm_math::chol_solve(sys, lam, one, y) && fabs(y[0]) <= half && fabs(y[1]) <= half && fabs(y[2]) <= half) {
#pragma unroll
            for (int a = 0; a < 3; ++a) x[a] = y[a];
        }
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) out_verts[3 * r + a] = (float)(g[a] + x[a]);
#pragma unroll
    for (int c = 0; c < kMaxChannels; ++c)
        if (c < channels) out_colors[r * channels + c] = (float)(s[kQ + c] / m);
}

__global__ void __launch_bounds__(kThreads)
simplify_emit_faces(const int32_t* __restrict__ face_index, const uint8_t* __restrict__ keep, const int32_t* __restrict__ keep_rank,
                    int n_faces, int n_kept, int32_t* __restrict__ out_faces) {
    const int64_t f = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (f >= n_faces || !keep[f]) return;
    const int64_t at = (int64_t)keep_rank[f] - 1;
    if (at < 0 || at >= n_kept) return;                // keep_rank is the inclusive prefix sum of keep: never taken
#pragma unroll
    for (int k = 0; k < 3; ++k) out_faces[3 * at + k] = face_index[3 * f + k];
}

}  // namespace

extern "C" int64_t ls2fm_mesh_simplify_workspace_bytes(int64_t n_verts, int64_t n_faces) {
    if (!counts_ok(n_verts, n_faces)) return (int64_t)LS2FM_ERR_INVALID_ARGUMENT;
    return (int64_t)simplify_layout(n_verts, nullptr, nullptr);
}

extern "C" int ls2fm_mesh_simplify_keys(const float* verts, int64_t n_verts, const int32_t* faces, int64_t n_faces, float cell,
                                        int64_t* vert_key, uint8_t* face_class, int64_t* counts, void* stream) {
    LS2FM_CHECK_ARG(counts_ok(n_verts, n_faces) && cell_ok(cell) && counts);
    LS2FM_CHECK_ARG((verts && vert_key) || n_verts == 0);
    LS2FM_CHECK_ARG((faces && n_verts > 0) || n_faces == 0);
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(counts, 0, 2 * sizeof(int64_t), st) != hipSuccess) return ls2fm_launch_status();
    if (n_verts) simplify_vertex_keys<<<blocks_of(n_verts), kThreads, 0, st>>>(verts, (int)n_verts, (double)cell, vert_key, counts);
    if (n_faces) simplify_face_classes<<<blocks_of(n_faces), kThreads, 0, st>>>(vert_key, faces, (int)n_faces, face_class, counts);
    return ls2fm_launch_status();
}

extern "C" int ls2fm_mesh_simplify_mark(const int64_t* sorted_key, const int64_t* sorted_vert, int64_t n_verts, const int32_t* faces,
                                        int64_t n_faces, const uint8_t* face_class, int32_t* corner_head, int32_t* head_used,
                                        void* workspace, int64_t workspace_bytes, void* stream) {
    LS2FM_CHECK_ARG(counts_ok(n_verts, n_faces));
    LS2FM_CHECK_ARG((sorted_key && sorted_vert && head_used) || n_verts == 0);
    LS2FM_CHECK_ARG((faces && face_class && corner_head && n_verts > 0) || n_faces == 0);
    if (!workspace || workspace_bytes < (int64_t)simplify_layout(n_verts, nullptr, nullptr)) return LS2FM_ERR_WORKSPACE;
    if (n_verts == 0) return LS2FM_OK;
    hipStream_t st = (hipStream_t)stream;
    SimplifyWs w;
    simplify_layout(n_verts, workspace, &w);
    if (hipMemsetAsync(head_used, 0, (size_t)n_verts * sizeof(int32_t), st) != hipSuccess) return ls2fm_launch_status();
    simplify_vertex_heads<<<blocks_of(n_verts), kThreads, 0, st>>>(sorted_key, sorted_vert, (int)n_verts, w.vert_head);
    if (n_faces) simplify_corners<<<blocks_of(n_faces), kThreads, 0, st>>>(w.vert_head, faces, face_class, (int)n_faces, (int)n_verts, corner_head,
                                                                            head_used);
    return ls2fm_launch_status();
}

extern "C" int ls2fm_mesh_simplify_index(const int32_t* head_used, const int32_t* head_rank, int64_t n_verts, const int32_t* faces,
                                         int64_t n_faces, const uint8_t* face_class, int32_t* vertex_map, int32_t* face_index,
                                         void* workspace, int64_t workspace_bytes, void* stream) {
    LS2FM_CHECK_ARG(counts_ok(n_verts, n_faces));
    LS2FM_CHECK_ARG((head_used && head_rank && vertex_map) || n_verts == 0);
    LS2FM_CHECK_ARG((faces && face_class && face_index && n_verts > 0) || n_faces == 0);
    if (!workspace || workspace_bytes < (int64_t)simplify_layout(n_verts, nullptr, nullptr)) return LS2FM_ERR_WORKSPACE;
    if (n_verts == 0) return LS2FM_OK;
    hipStream_t st = (hipStream_t)stream;
    SimplifyWs w;
    simplify_layout(n_verts, workspace, &w);
    simplify_vertex_index<<<blocks_of(n_verts), kThreads, 0, st>>>(w.vert_head, head_used, head_rank, (int)n_verts, vertex_map, w.out_head);
    if (n_faces) simplify_face_index<<<blocks_of(n_faces), kThreads, 0, st>>>(vertex_map, faces, face_class, (int)n_faces, face_index);
    return ls2fm_launch_status();
}

extern "C" int ls2fm_mesh_simplify_place(const float* verts, const float* colors, int32_t channels, int64_t n_verts, const int32_t* faces,
                                         int64_t n_faces, float cell, int32_t placement, double reg, const int64_t* sorted_key,
                                         const int64_t* sorted_vert, const int32_t* sorted_corner_head, const int64_t* sorted_corner,
                                         int64_t n_out, int32_t stages, double* sums, int32_t* count, float* out_verts, float* out_colors,
                                         void* workspace, int64_t workspace_bytes, void* stream) {
    LS2FM_CHECK_ARG(counts_ok(n_verts, n_faces) && cell_ok(cell) && n_out >= 0 && n_out <= n_verts);
    LS2FM_CHECK_ARG(channels >= 0 && channels <= kMaxChannels && (channels == 0) == (colors == nullptr));
    LS2FM_CHECK_ARG(colors == nullptr || out_colors || !(stages & LS2FM_SIMPLIFY_STAGE_SOLVE));
    LS2FM_CHECK_ARG((placement == LS2FM_SIMPLIFY_QUADRIC || placement == LS2FM_SIMPLIFY_MEAN) && reg >= 0.0 && reg < (double)INFINITY);
    LS2FM_CHECK_ARG(stages >= 1 && stages <= (LS2FM_SIMPLIFY_STAGE_SUMS | LS2FM_SIMPLIFY_STAGE_SOLVE));
    LS2FM_CHECK_ARG((verts && sorted_key && sorted_vert) || n_verts == 0);
    LS2FM_CHECK_ARG((faces && sorted_corner_head && sorted_corner) || n_faces == 0);
    LS2FM_CHECK_ARG((sums && count && (out_verts || !(stages & LS2FM_SIMPLIFY_STAGE_SOLVE))) || n_out == 0);
    if (!workspace || workspace_bytes < (int64_t)simplify_layout(n_verts, nullptr, nullptr)) return LS2FM_ERR_WORKSPACE;
    if (n_out == 0) return LS2FM_OK;
    hipStream_t st = (hipStream_t)stream;
    SimplifyWs w;
    simplify_layout(n_verts, workspace, &w);
    if (stages & LS2FM_SIMPLIFY_STAGE_SUMS)
        simplify_sums<<<(unsigned)((n_out + kWaves - 1) / kWaves), kThreads, 0, st>>>(verts, colors, channels, faces, (double)cell, sorted_key,
                                                                                     sorted_vert, n_verts, sorted_corner_head, sorted_corner,
                                                                                     3 * n_faces, w.out_head, (int)n_out, sums, count);
    if (stages & LS2FM_SIMPLIFY_STAGE_SOLVE)
        simplify_solve<<<blocks_of(n_out), kThreads, 0, st>>>(sums, count, channels, (double)cell, placement == LS2FM_SIMPLIFY_MEAN, reg,
                                                              sorted_key, w.out_head, (int)n_verts, (int)n_out, out_verts, out_colors);
    return ls2fm_launch_status();
}

extern "C" int ls2fm_mesh_simplify_emit(const int32_t* face_index, const uint8_t* keep, const int32_t* keep_rank, int64_t n_faces,
                                        int64_t n_kept, int32_t* out_faces, void* stream) {
    LS2FM_CHECK_ARG(n_faces >= 0 && 3 * n_faces < ((int64_t)1 << 31) && n_kept >= 0 && n_kept <= n_faces);
    LS2FM_CHECK_ARG((face_index && keep && keep_rank) || n_faces == 0);
    LS2FM_CHECK_ARG(out_faces || n_kept == 0);
    if (n_faces == 0 || n_kept == 0) return LS2FM_OK;
    simplify_emit_faces<<<blocks_of(n_faces), kThreads, 0, (hipStream_t)stream>>>(face_index, keep, keep_rank, (int)n_faces, (int)n_kept,
                                                                                  out_faces);
    return ls2fm_launch_status();
}
