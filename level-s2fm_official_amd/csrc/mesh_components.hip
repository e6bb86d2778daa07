// Connected components of a triangle mesh and extraction of the largest one by area (replaces trimesh's
// Trimesh.split(only_watertight=False) + argmax over c.area + submesh, as the reference's get_surface_high_res_mesh calls them,
// utils/plots.py:163-166).
//
// Two faces are in one component when a chain of faces, each consecutive pair sharing a vertex index, links them.  The label of
// a vertex is the smallest vertex index of its component (an unused vertex is its own component), so labels do not depend on
// the order of the unions.  Union-find over vertices, every parent pointer pointing to a SMALLER index (a root is its tree's
// minimum):
//   cc_init     parent[v] = v (+ the area accumulators of the largest-component path)
//   cc_hook     per face: unite(a, b), unite(a, c).  Lock-free: every access to `parent` is an agent-scope atomic (workgroups on
//               other XCDs read and move the same pointers inside the launch); find() halves paths with a compare-exchange to
//               the grandparent; unite() hooks the larger root under the smaller one with a compare-exchange that fails when the
//               root has been hooked meanwhile, and then retries from the new roots.  Nothing waits on another workgroup.
//   cc_flatten  parent[v] = root(v): the labels (next launch, so it reads the finished forest)
// Largest component (each pass reads the previous pass's results across a launch boundary):
//   lc_max_area     per face: area = 0.5 |(b - a) x (c - a)| in double; max over all faces (64-bit max of the bits: areas >= 0)
//   lc_accumulate   per face: q = rint(area 2^s) as uint64 with s = 63 - bitlen(F) - exponent(max area), so the sum of all
//                   faces is < 2^63; integer atomics add q into the face's label and take the min face index.  Integer sums do
//                   not depend on the order of the additions: the area of a component is the same bits on every call
//   lc_select_max   per root: max of the sums (and the areas output)
//   lc_select_face  per root holding the max: min of the first faces -> the winner (largest area, ties to the lowest face)
//   lc_count        per tile of faces / of vertices: how many are kept (label == the winner's label)
//   lc_scan         ONE workgroup: per-tile offsets and the two counts
//   lc_emit_verts   kept vertices in index order; their new ids
//   lc_emit_faces   kept faces in order, renumbered
#include "ls2fm_device.h"
#include "union_find.h"
#include "workspace.h"

namespace {

using namespace union_find;

constexpr int kThreads = 256;
constexpr int kPer = 8;
constexpr uint32_t kTile = kThreads * kPer;
constexpr int kScanThreads = 1024;
constexpr int32_t kNoFace = 0x7fffffff;

struct LcSlots {
    unsigned long long max_area_bits;   // bits of the largest face area (a double >= 0)
    unsigned long long q_max;           // largest component sum
    int32_t win_face;                   // lowest first face among the components holding q_max
    int32_t pad;
};

__global__ void __launch_bounds__(kThreads)
cc_init(int32_t* __restrict__ parent, uint32_t n_verts, unsigned long long* __restrict__ comp_q, int32_t* __restrict__ comp_first,
        LcSlots* __restrict__ slots) {
    const uint32_t v = blockIdx.x * kThreads + threadIdx.x;
    if (v < n_verts) {
        parent[v] = (int32_t)v;
        if (comp_q) {
            comp_q[v] = 0ull;
            comp_first[v] = kNoFace;
        }
    }
    if (slots && v == 0) {
        slots->max_area_bits = 0ull;
        slots->q_max = 0ull;
        slots->win_face = kNoFace;
        slots->pad = 0;
    }
}

__global__ void __launch_bounds__(kThreads)
cc_hook(const int32_t* __restrict__ faces, uint32_t n_faces, int32_t* parent) {
    const uint32_t f = blockIdx.x * kThreads + threadIdx.x;
    if (f >= n_faces) return;
    const int32_t* t = faces + (int64_t)f * 3;
    const int32_t a = t[0], b = t[1], c = t[2];
    unite(parent, a, b);
    unite(parent, a, c);
}

__global__ void __launch_bounds__(kThreads)
cc_flatten(int32_t* parent, uint32_t n_verts) {
    const uint32_t v = blockIdx.x * kThreads + threadIdx.x;
    if (v >= n_verts) return;
    const int32_t r = find_root(parent, (int32_t)v);
    __hip_atomic_store(parent + v, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// 0.5 |(b - a) x (c - a)| in double from the fp32 corners, in numpy's order: cross = (u1 v2 - u2 v1, u2 v0 - u0 v2,
// u0 v1 - u1 v0), sqrt((x^2 + y^2) + z^2) / 2 (the library builds with -ffp-contract=off: each operation rounded)
__device__ __forceinline__ double face_area(const float* __restrict__ verts, const int32_t* __restrict__ faces, uint32_t f) {
    const int32_t* t = faces + (int64_t)f * 3;
    const float* pa = verts + (int64_t)t[0] * 3;
    const float* pb = verts + (int64_t)t[1] * 3;
    const float* pc = verts + (int64_t)t[2] * 3;
    const double ax = pa[0], ay = pa[1], az = pa[2];
    const double u0 = (double)pb[0] - ax, u1 = (double)pb[1] - ay, u2 = (double)pb[2] - az;
    const double v0 = (double)pc[0] - ax, v1 = (double)pc[1] - ay, v2 = (double)pc[2] - az;
    const double cx = u1 * v2 - u2 * v1;
    const double cy = u2 * v0 - u0 * v2;
    const double cz = u0 * v1 - u1 * v0;
    return sqrt(cx * cx + cy * cy + cz * cz) * 0.5;
}

// the fixed-point exponent s: every face's q = rint(area 2^s) <= 2^(63 - bitlen(F)), so the sum of all F faces is < 2^63
__device__ __forceinline__ int fixed_shift(const LcSlots* slots, uint32_t n_faces) {
    const double amax = __longlong_as_double((long long)slots->max_area_bits);
    int e = 0;
    frexp(amax, &e);                                         // amax < 2^e (e = 0 for amax = 0)
    return 63 - (32 - __clz(n_faces)) - e;
}

__global__ void __launch_bounds__(kThreads)
lc_max_area(const float* __restrict__ verts, const int32_t* __restrict__ faces, uint32_t n_faces, LcSlots* slots) {
    const uint32_t first = blockIdx.x * kTile + threadIdx.x * kPer;
    double m = 0.0;
#pragma unroll
    for (int r = 0; r < kPer; ++r) {
        const uint32_t f = first + r;
        if (f < n_faces) {
            const double a = face_area(verts, faces, f);
            m = a > m ? a : m;                               // a NaN area is dropped
        }
    }
    const unsigned long long bits = wave_max((unsigned long long)__double_as_longlong(m));
    if ((threadIdx.x & 63) == 0)
        __hip_atomic_fetch_max(&slots->max_area_bits, bits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// adds each lane's (label, q, first) into the component arrays: the lanes of one label are summed in the wave first, and the
// lowest such lane does the two atomics (integer: the result does not depend on which lanes go together)
__device__ __forceinline__ void flush_runs(unsigned long long* comp_q, int32_t* comp_first, bool live, int32_t label,
                                           unsigned long long q, int32_t first) {
    const int lane = threadIdx.x & 63;
    unsigned long long pending = __ballot(live);
    while (pending) {
        const int leader = __ffsll((long long)pending) - 1;
        const int32_t L = __shfl(label, leader, 64);
        const bool mine = live && label == L;
        pending &= ~__ballot(mine);
        const unsigned long long s = wave_sum(mine ? q : 0ull);
        const int32_t m = wave_min(mine ? first : kNoFace);
        if (lane == leader) {
            __hip_atomic_fetch_add(comp_q + L, s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_fetch_min(comp_first + L, m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

// each thread walks kPer consecutive faces and keeps one run per label; a label change flushes the run on its own (rare on a
// mesh whose consecutive faces share components), the last run goes through the wave
__global__ void __launch_bounds__(kThreads)
lc_accumulate(const float* __restrict__ verts, const int32_t* __restrict__ faces, uint32_t n_faces,
              const int32_t* __restrict__ labels, const LcSlots* __restrict__ slots, unsigned long long* comp_q,
              int32_t* comp_first) {
    const int s = fixed_shift(slots, n_faces);
    const uint32_t first = blockIdx.x * kTile + threadIdx.x * kPer;
    bool live = false;
    int32_t label = -1, run_first = kNoFace;
    unsigned long long q = 0ull;
    for (int r = 0; r < kPer; ++r) {
        const uint32_t f = first + r;
        if (f >= n_faces) break;
        const int32_t L = labels[faces[(int64_t)f * 3]];
        const unsigned long long qf = (unsigned long long)llrint(ldexp(face_area(verts, faces, f), s));
        if (live && L != label) {
            __hip_atomic_fetch_add(comp_q + label, q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_fetch_min(comp_first + label, run_first, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            live = false;
        }
        if (!live) {
            live = true;
            label = L;
            run_first = (int32_t)f;
            q = 0ull;
        }
        q += qf;
    }
    flush_runs(comp_q, comp_first, live, label, q, run_first);
}

__global__ void __launch_bounds__(kThreads)
lc_select_max(const int32_t* __restrict__ labels, uint32_t n_verts, uint32_t n_faces, const unsigned long long* __restrict__ comp_q,
              LcSlots* slots, double* __restrict__ areas) {
    const uint32_t v = blockIdx.x * kThreads + threadIdx.x;
    unsigned long long q = 0ull;
    if (v < n_verts) {
        const bool root = labels[v] == (int32_t)v;
        q = root ? comp_q[v] : 0ull;
        if (areas) areas[v] = ldexp((double)q, -fixed_shift(slots, n_faces));
    }
    q = wave_max(q);
    if ((threadIdx.x & 63) == 0 && q)
        __hip_atomic_fetch_max(&slots->q_max, q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ void __launch_bounds__(kThreads)
lc_select_face(const int32_t* __restrict__ labels, uint32_t n_verts, const unsigned long long* __restrict__ comp_q,
               const int32_t* __restrict__ comp_first, LcSlots* slots) {
    const uint32_t v = blockIdx.x * kThreads + threadIdx.x;
    const unsigned long long q_max = slots->q_max;
    int32_t f = kNoFace;
    if (v < n_verts && labels[v] == (int32_t)v && comp_q[v] == q_max) f = comp_first[v];
    f = wave_min(f);
    if ((threadIdx.x & 63) == 0 && f != kNoFace)
        __hip_atomic_fetch_min(&slots->win_face, f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ int32_t winner_label(const int32_t* __restrict__ faces, const int32_t* __restrict__ labels,
                                                const LcSlots* __restrict__ slots) {
    const int32_t f = slots->win_face;                      // always set when n_faces > 0; -1 (keep nothing) otherwise
    return f == kNoFace ? -1 : labels[faces[(int64_t)f * 3]];
}

// blocks [0, tiles_f): faces; [tiles_f, tiles_f + tiles_v): vertices.  A vertex is kept iff its label is the winner's: a
// vertex joins a component only through a face, and the winner's root is in one of its faces.
__global__ void __launch_bounds__(kThreads)
lc_count(const int32_t* __restrict__ faces, uint32_t n_faces, const int32_t* __restrict__ labels, uint32_t n_verts,
         const LcSlots* __restrict__ slots, uint32_t tiles_f, uint32_t* __restrict__ tile_f, uint32_t* __restrict__ tile_v) {
    const int32_t win = winner_label(faces, labels, slots);
    const bool on_faces = blockIdx.x < tiles_f;
    const uint32_t tile = on_faces ? blockIdx.x : blockIdx.x - tiles_f;
    const uint32_t n = on_faces ? n_faces : n_verts;
    const uint32_t first = tile * kTile + threadIdx.x * kPer;
    uint32_t c = 0;
#pragma unroll
    for (int r = 0; r < kPer; ++r) {
        const uint32_t i = first + r;
        if (i < n) c += (on_faces ? labels[faces[(int64_t)i * 3]] : labels[i]) == win ? 1u : 0u;
    }
    uint32_t total;
    block_exclusive_scan<kThreads>(c, total);
    if (threadIdx.x == 0) (on_faces ? tile_f : tile_v)[tile] = total;
}

// one workgroup: exclusive scans of the per-tile totals, 1024 tiles per round, carried across rounds
__device__ __forceinline__ uint32_t scan_tiles(const uint32_t* __restrict__ tile_n, uint32_t n_tiles, uint32_t* __restrict__ offset) {
    uint32_t carry = 0;
    for (uint32_t base = 0; base < n_tiles; base += kScanThreads) {
        const uint32_t t = base + threadIdx.x;
        const uint32_t v = t < n_tiles ? tile_n[t] : 0u;
        uint32_t sum;
        const uint32_t e = block_exclusive_scan<kScanThreads>(v, sum);
        if (t < n_tiles) offset[t] = carry + e;          // < 2^31: counts of kept faces / vertices
        carry += sum;
    }
    return carry;
}

__global__ void __launch_bounds__(kScanThreads)
lc_scan(const uint32_t* __restrict__ tile_f, uint32_t tiles_f, const uint32_t* __restrict__ tile_v, uint32_t tiles_v,
        uint32_t* __restrict__ off_f, uint32_t* __restrict__ off_v, int64_t* __restrict__ counts) {
    const uint32_t nf = scan_tiles(tile_f, tiles_f, off_f);
    const uint32_t nv = scan_tiles(tile_v, tiles_v, off_v);
    if (threadIdx.x == 0) {
        counts[0] = (int64_t)nv;
        counts[1] = (int64_t)nf;
    }
}

__global__ void __launch_bounds__(kThreads)
lc_emit_verts(const float* __restrict__ verts, uint32_t n_verts, const int32_t* __restrict__ faces, const int32_t* __restrict__ labels,
              const LcSlots* __restrict__ slots, const uint32_t* __restrict__ off_v, int32_t* __restrict__ new_id,
              float* __restrict__ out_verts) {
    const int32_t win = winner_label(faces, labels, slots);
    const uint32_t first = blockIdx.x * kTile + threadIdx.x * kPer;
    uint32_t c = 0;
#pragma unroll
    for (int r = 0; r < kPer; ++r)
        if (first + r < n_verts) c += labels[first + r] == win ? 1u : 0u;
    uint32_t unused;
    uint32_t id = off_v[blockIdx.x] + block_exclusive_scan<kThreads>(c, unused);
    for (int r = 0; r < kPer; ++r) {
        const uint32_t v = first + r;
        if (v >= n_verts) break;
        if (labels[v] != win) continue;
        new_id[v] = (int32_t)id;
        const float* p = verts + (int64_t)v * 3;
        float* o = out_verts + (int64_t)id * 3;
        o[0] = p[0];
        o[1] = p[1];
        o[2] = p[2];
        ++id;
    }
}

__global__ void __launch_bounds__(kThreads)
lc_emit_faces(const int32_t* __restrict__ faces, uint32_t n_faces, const int32_t* __restrict__ labels,
              const LcSlots* __restrict__ slots, const uint32_t* __restrict__ off_f, const int32_t* __restrict__ new_id,
              int32_t* __restrict__ out_faces) {
    const int32_t win = winner_label(faces, labels, slots);
    const uint32_t first = blockIdx.x * kTile + threadIdx.x * kPer;
    uint32_t c = 0;
#pragma unroll
    for (int r = 0; r < kPer; ++r)
        if (first + r < n_faces) c += labels[faces[(int64_t)(first + r) * 3]] == win ? 1u : 0u;
    uint32_t unused;
    uint32_t id = off_f[blockIdx.x] + block_exclusive_scan<kThreads>(c, unused);
    for (int r = 0; r < kPer; ++r) {
        const uint32_t f = first + r;
        if (f >= n_faces) break;
        const int32_t* t = faces + (int64_t)f * 3;
        if (labels[t[0]] != win) continue;
        int32_t* o = out_faces + (int64_t)id * 3;
        o[0] = new_id[t[0]];
        o[1] = new_id[t[1]];
        o[2] = new_id[t[2]];
        ++id;
    }
}

// Sizes: 0 <= n_verts, n_faces < 2^31, and a mesh with faces has vertices.  false when refused.
bool sizes_ok(int64_t n_verts, int64_t n_faces) {
    const int64_t lim = (int64_t)1 << 31;
    return n_verts >= 0 && n_faces >= 0 && n_verts < lim && n_faces < lim && (n_faces == 0 || n_verts > 0);
}

struct LcLayout {
    uint32_t nv, nf, tiles_v, tiles_f;
    int32_t* labels;
    unsigned long long* comp_q;
    int32_t *comp_first, *new_id;
    uint32_t *tile_f, *tile_v, *off_f, *off_v;
    LcSlots* slots;
    int64_t bytes;
};

void lc_layout(int64_t n_verts, int64_t n_faces, void* base, LcLayout& L) {
    L.nv = (uint32_t)n_verts;
    L.nf = (uint32_t)n_faces;
    L.tiles_v = (uint32_t)((n_verts + kTile - 1) / kTile);
    L.tiles_f = (uint32_t)((n_faces + kTile - 1) / kTile);
    Workspace ws(base, 256);
    L.labels = ws.take<int32_t>(n_verts);
    L.comp_q = ws.take<unsigned long long>(n_verts);
    L.comp_first = ws.take<int32_t>(n_verts);
    L.new_id = ws.take<int32_t>(n_verts);
    L.tile_f = ws.take<uint32_t>(L.tiles_f);
    L.tile_v = ws.take<uint32_t>(L.tiles_v);
    L.off_f = ws.take<uint32_t>(L.tiles_f);
    L.off_v = ws.take<uint32_t>(L.tiles_v);
    L.slots = ws.take<LcSlots>(1);
    L.bytes = (int64_t)ws.bytes();
}

uint32_t blocks_of(uint32_t n) { return (n + kThreads - 1) / kThreads; }

}  // namespace

extern "C" int64_t ls2fm_mesh_components_workspace_bytes(int64_t n_verts, int64_t n_faces) {
    if (!sizes_ok(n_verts, n_faces)) return (int64_t)LS2FM_ERR_INVALID_ARGUMENT;
    LcLayout L;
    lc_layout(n_verts, n_faces, nullptr, L);
    return L.bytes;
}

extern "C" int ls2fm_mesh_components(const int32_t* faces, int64_t n_verts, int64_t n_faces, int32_t* labels, void* stream) {
    LS2FM_CHECK_ARG(sizes_ok(n_verts, n_faces) && (faces || n_faces == 0) && (labels || n_verts == 0));
    if (n_verts == 0) return LS2FM_OK;
    hipStream_t s = (hipStream_t)stream;
    const uint32_t nv = (uint32_t)n_verts, nf = (uint32_t)n_faces;
    cc_init<<<blocks_of(nv), kThreads, 0, s>>>(labels, nv, nullptr, nullptr, nullptr);
    if (nf) {
        cc_hook<<<blocks_of(nf), kThreads, 0, s>>>(faces, nf, labels);
        cc_flatten<<<blocks_of(nv), kThreads, 0, s>>>(labels, nv);
    }
    return ls2fm_launch_status();
}

extern "C" int ls2fm_mesh_largest_component_count(const float* verts, int64_t n_verts, const int32_t* faces, int64_t n_faces,
                                                  void* workspace, int64_t workspace_bytes, int64_t* counts, double* areas,
                                                  void* stream) {
    LS2FM_CHECK_ARG(sizes_ok(n_verts, n_faces) && ((verts && faces && counts) || n_faces == 0));
    if (n_faces == 0) return LS2FM_OK;
    LcLayout L;
    lc_layout(n_verts, n_faces, workspace, L);
    if (!workspace || workspace_bytes < L.bytes) return LS2FM_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    cc_init<<<blocks_of(L.nv), kThreads, 0, s>>>(L.labels, L.nv, L.comp_q, L.comp_first, L.slots);
    cc_hook<<<blocks_of(L.nf), kThreads, 0, s>>>(faces, L.nf, L.labels);
    cc_flatten<<<blocks_of(L.nv), kThreads, 0, s>>>(L.labels, L.nv);
    lc_max_area<<<L.tiles_f, kThreads, 0, s>>>(verts, faces, L.nf, L.slots);
    lc_accumulate<<<L.tiles_f, kThreads, 0, s>>>(verts, faces, L.nf, L.labels, L.slots, L.comp_q, L.comp_first);
    lc_select_max<<<blocks_of(L.nv), kThreads, 0, s>>>(L.labels, L.nv, L.nf, L.comp_q, L.slots, areas);
    lc_select_face<<<blocks_of(L.nv), kThreads, 0, s>>>(L.labels, L.nv, L.comp_q, L.comp_first, L.slots);
    lc_count<<<L.tiles_f + L.tiles_v, kThreads, 0, s>>>(faces, L.nf, L.labels, L.nv, L.slots, L.tiles_f, L.tile_f, L.tile_v);
    lc_scan<<<1, kScanThreads, 0, s>>>(L.tile_f, L.tiles_f, L.tile_v, L.tiles_v, L.off_f, L.off_v, counts);
    return ls2fm_launch_status();
}

extern "C" int ls2fm_mesh_largest_component_emit(const float* verts, int64_t n_verts, const int32_t* faces, int64_t n_faces,
                                                 void* workspace, int64_t workspace_bytes, float* out_verts, int32_t* out_faces,
                                                 void* stream) {
    LS2FM_CHECK_ARG(sizes_ok(n_verts, n_faces) && ((verts && faces && out_verts && out_faces) || n_faces == 0));
    if (n_faces == 0) return LS2FM_OK;
    LcLayout L;
    lc_layout(n_verts, n_faces, workspace, L);
    if (!workspace || workspace_bytes < L.bytes) return LS2FM_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    lc_emit_verts<<<L.tiles_v, kThreads, 0, s>>>(verts, L.nv, faces, L.labels, L.slots, L.off_v, L.new_id, out_verts);
    lc_emit_faces<<<L.tiles_f, kThreads, 0, s>>>(faces, L.nf, L.labels, L.slots, L.off_f, L.new_id, out_faces);
    return ls2fm_launch_status();
}
