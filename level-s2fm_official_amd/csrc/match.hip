// Batched SIFT descriptor matching (include/ls2fm.h, "Descriptor matching"): what `colmap exhaustive_matcher` writes into the
// `matches` table (preparation/main.py:98, read back at :30-37), for ALL image pairs in one call.
//
//   match_prep_kernel      descriptors -> signed bytes (a - 128, the operand type of the i8 MFMA) and 128 * sum(a) per descriptor
//   match_sweep_kernel     the hot path: one wave = 64 rows of one directed job (a -> b or b -> a of a pair) against one chunk of
//                          its columns; 32 x 32 products by v_mfma_i32_32x32x32_i8 (4 per tile, K = 128), the exact dot restored
//                          through the accumulator's initial value and one add, the running top-2 per row as the epilogue.  The
//                          product matrix is never written.
//   match_finalize_kernel  chunks merged in column order, raw best / best_j / second, the two fp64 comparisons -> proposals
//   match_cross_kernel     cross check, matched index per row of the first image, matches counted per pair
//
// Exactness of the biased product: sum a b = sum (a - 128)(b - 128) + 128 (sum a + sum b) - 2^21.  The accumulator starts at
// 128 sum a_i - 2^21 (the row's constant, fed as the MFMA's C operand: no vector instruction), 128 sum b_j is added with the
// key's shift.  Every true dot is in [0, 128 * 255^2] < 2^23, so `dot << 9 | (511 - tile)` fits 32 bits: a lane sees one column
// per tile, the tile id recovers it, and the unsigned max keeps the LOWEST column among equal dots.  Three vector instructions
// per product: v_lshl_add_u32 (key), v_med3_u32 (second), v_max_u32 (best).
//
// Both directions are swept (the b -> a job recomputes the transposed products) rather than reducing rows and columns from one
// tile: by the instruction count the vector pipe is the longer of the two, a column reduction from the same tile costs the same three instructions per
// product, and it would add a cross-workgroup merge of column partials; two sweeps share one code path and stay free of atomics.
#include "ls2fm_device.h"
#include "workspace.h"

#include <algorithm>
#include <cmath>
#include <vector>

namespace {

constexpr int kRowBlocks = 2;                  // 32-row MFMA blocks per wave
constexpr int kWaveRows = 32 * kRowBlocks;
constexpr int kTile = 32;                      // columns per MFMA tile
constexpr int kTileBits = 9;                   // tile id inside a chunk
constexpr int kMaxChunk = kTile << kTileBits;  // 16384 columns
constexpr int kMinChunk = 1024;
constexpr int kSweepThreads = 256;             // 4 waves, one work item each
constexpr int kSweepWaves = kSweepThreads / 64;
constexpr int64_t kTargetItems = 8192;         // 256 CUs x 4 SIMDs x 8 waves: chunks shrink until the grid has this many waves
constexpr int kThreads = 256;

typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v16i __attribute__((ext_vector_type(16)));

// one directed job: rows = descriptors of image a, columns = descriptors of image b (as rows of the descriptor array)
struct Job {
    int32_t a_start, n_a, b_start, n_b;
    int32_t item_start;     // first work item (wave) of the job; items = n_rb * n_chunks, chunk-major
    int32_t row_start;      // first entry of the job in the per-directed-row arrays (best / best_j / second / proposals)
    int32_t n_rb, n_chunks;
    int64_t part_start;     // first entry of the job's [n_chunks][n_a] partials
};

struct Plan {
    std::vector<Job> jobs;          // 2 n_pairs + 1 (sentinel)
    std::vector<int32_t> first_start;  // n_pairs + 1: prefix sum of n_a (the layout of match_index)
    int64_t n_desc = 0, n_items = 0, n_rows = 0, n_parts = 0;
    int32_t chunk_cols = kMaxChunk;
};

struct Ws {
    Job* jobs;
    int32_t* first_start;
    int32_t* bias128;
    uint8_t* dbias;
    int32_t* proposal;
    uint4* part;
};

size_t ws_layout(const Plan& p, int32_t n_pairs, char* base, Ws* w) {
    Workspace ws(base, 256);
    Ws t;
    t.jobs = ws.take<Job>(2 * (size_t)n_pairs + 1);
    t.first_start = ws.take<int32_t>((size_t)n_pairs + 1);
    t.bias128 = ws.take<int32_t>((size_t)p.n_desc);
    t.dbias = ws.take<uint8_t>((size_t)128 * (size_t)p.n_desc);
    t.proposal = ws.take<int32_t>((size_t)p.n_rows);
    t.part = ws.take<uint4>((size_t)p.n_parts);
    if (w) *w = t;
    return ws.bytes();
}

// host-side plan of a call; every size comes from image_start and pairs (host arrays)
int make_plan(const int32_t* image_start, int32_t n_images, const int32_t* pairs, int32_t n_pairs, Plan* plan) {
    LS2FM_CHECK_ARG(image_start && n_images >= 1 && n_pairs >= 0 && (pairs || n_pairs == 0) && image_start[0] == 0);
    bool big = false;
    for (int32_t v = 0; v < n_images; ++v) {
        LS2FM_CHECK_ARG(image_start[v + 1] >= image_start[v]);
        big = big || image_start[v + 1] - image_start[v] > LS2FM_MATCH_MAX_DESCRIPTORS;
    }
    for (int32_t p = 0; p < n_pairs; ++p)
        LS2FM_CHECK_ARG(pairs[2 * p] >= 0 && pairs[2 * p] < n_images && pairs[2 * p + 1] >= 0 && pairs[2 * p + 1] < n_images);
    if (big) return LS2FM_ERR_UNSUPPORTED;
    plan->n_desc = image_start[n_images];
    auto count = [&](int v) { return image_start[v + 1] - image_start[v]; };
    auto items_at = [&](int32_t chunk) {
        int64_t items = 0;
        for (int32_t p = 0; p < n_pairs; ++p) {
            const int64_t na = count(pairs[2 * p]), nb = count(pairs[2 * p + 1]);
            items += ((na + kWaveRows - 1) / kWaveRows) * ((nb + chunk - 1) / chunk) + ((nb + kWaveRows - 1) / kWaveRows) * ((na + chunk - 1) / chunk);
        }
        return items;
    };
    int32_t chunk = kMaxChunk;
    while (chunk > kMinChunk && items_at(chunk) < kTargetItems) chunk /= 2;
    plan->chunk_cols = chunk;
    plan->jobs.resize(2 * (size_t)n_pairs + 1);
    plan->first_start.resize((size_t)n_pairs + 1);
    int64_t items = 0, rows = 0, parts = 0, first = 0;
    for (int32_t p = 0; p < n_pairs; ++p) {
        plan->first_start[p] = (int32_t)first;
        for (int dir = 0; dir < 2; ++dir) {
            const int va = pairs[2 * p + dir], vb = pairs[2 * p + 1 - dir];
            Job& j = plan->jobs[2 * (size_t)p + dir];
            j.a_start = image_start[va]; j.n_a = count(va);
            j.b_start = image_start[vb]; j.n_b = count(vb);
            j.n_rb = (j.n_a + kWaveRows - 1) / kWaveRows;
            j.n_chunks = (j.n_b + chunk - 1) / chunk;
            j.item_start = (int32_t)items; j.row_start = (int32_t)rows; j.part_start = parts;
            items += (int64_t)j.n_rb * j.n_chunks;
            rows += j.n_a;
            parts += (int64_t)j.n_a * j.n_chunks;
            if (items >= (1ll << 31) - kSweepWaves || rows >= (1ll << 31) - kThreads) return LS2FM_ERR_UNSUPPORTED;
        }
        first += count(pairs[2 * p]);
    }
    plan->first_start[n_pairs] = (int32_t)first;
    Job& end = plan->jobs[2 * (size_t)n_pairs];
    end = Job{0, 0, 0, 0, (int32_t)items, (int32_t)rows, 0, 0, parts};
    plan->n_items = items; plan->n_rows = rows; plan->n_parts = parts;
    return LS2FM_OK;
}

__device__ __forceinline__ uint32_t byte_sum(uint32_t x) { return (x & 255u) + ((x >> 8) & 255u) + ((x >> 16) & 255u) + (x >> 24); }

// 8 threads per descriptor, 16 bytes each
__global__ void __launch_bounds__(kThreads) match_prep_kernel(const uint4* __restrict__ desc, int64_t n, uint4* __restrict__ dbias,
                                                               int32_t* __restrict__ bias128) {
    const int64_t t = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    const bool live = t < n * 8;
    uint32_t sum = 0;
    if (live) {
        uint4 v = desc[t];
        sum = byte_sum(v.x) + byte_sum(v.y) + byte_sum(v.z) + byte_sum(v.w);
        v.x ^= 0x80808080u; v.y ^= 0x80808080u; v.z ^= 0x80808080u; v.w ^= 0x80808080u;
        dbias[t] = v;
    }
    sum += __shfl_xor(sum, 1, 64);
    sum += __shfl_xor(sum, 2, 64);
    sum += __shfl_xor(sum, 4, 64);
    if (live && (t & 7) == 0) bias128[t >> 3] = (int32_t)(128u * sum);
}

// the last job whose first item / row (field at `field`) is <= x; empty jobs share their successor's start and are passed over
template <int32_t Job::*F>
__device__ __forceinline__ int find_job(const Job* __restrict__ jobs, int n_jobs, int32_t x) {
    int lo = 0, hi = n_jobs;          // jobs[n_jobs] is the sentinel: its start is the total, > x
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (jobs[mid].*F <= x) lo = mid; else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ uint32_t umed3(uint32_t a, uint32_t b, uint32_t c) {
    return max(min(a, b), min(max(a, b), c));
}

// (d, j) of one side merged into the running top-2 (bd, bj, sd): the larger dot wins, the lower column among equals
__device__ __forceinline__ void merge_top2(uint32_t& bd, uint32_t& bj, uint32_t& sd, uint32_t d, uint32_t j, uint32_t s) {
    const bool better = d > bd || (d == bd && j < bj);
    sd = max(max(sd, s), better ? bd : d);
    bd = better ? d : bd;
    bj = better ? j : bj;
}

__global__ void __launch_bounds__(kSweepThreads) match_sweep_kernel(const Job* __restrict__ jobs, int n_jobs, int n_items,
                                                                    const uint4* __restrict__ dbias, const int32_t* __restrict__ bias128,
                                                                    int chunk_cols, uint4* __restrict__ part) {
    __shared__ uint2 lds[kSweepWaves][32][33];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, lc = lane & 31, h = lane >> 5;
    const int item = __builtin_amdgcn_readfirstlane((int)blockIdx.x * kSweepWaves + wave);
    const bool active = item < n_items;
    int a_start = 0, n_a = 0, b_start = 0, row0 = 0, col0 = 0, col1 = 0, chunk = 0;
    int64_t part_start = 0;
    if (active) {
        const Job jb = jobs[find_job<&Job::item_start>(jobs, n_jobs, item)];
        const int local = item - jb.item_start;
        chunk = local / jb.n_rb;
        row0 = (local - chunk * jb.n_rb) * kWaveRows;
        col0 = chunk * chunk_cols;
        col1 = min(jb.n_b, col0 + chunk_cols);
        a_start = jb.a_start; n_a = jb.n_a; b_start = jb.b_start; part_start = jb.part_start;
    }
    const int n_tiles = (col1 - col0 + kTile - 1) / kTile;      // <= 512

    // A fragments (lane: row lc of the block, 16 consecutive k at 32 s + 16 h; B uses the same k map, so the sum over k is the
    // dot whatever order the instruction walks them in) and the accumulators' initial values, one row per register
    v4i afrag[kRowBlocks][4];
    v16i cinit[kRowBlocks];
    const int last_row = max(n_a - 1, 0);
#pragma unroll
    for (int r = 0; r < kRowBlocks; ++r) {
        const int64_t src = a_start + min(row0 + r * 32 + lc, last_row);     // rows past n_a repeat the last one and are not written
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            uint4 v = make_uint4(0, 0, 0, 0);
            if (active) v = dbias[src * 8 + s * 2 + h];
            afrag[r][s] = v4i{(int)v.x, (int)v.y, (int)v.z, (int)v.w};
        }
#pragma unroll
        for (int g = 0; g < 16; ++g) {
            const int rr = min(row0 + r * 32 + (g & 3) + 8 * (g >> 2) + 4 * h, last_row);
            cinit[r][g] = active ? bias128[a_start + rr] - (1 << 21) : 0;
        }
    }

    uint32_t best[kRowBlocks][16], second[kRowBlocks][16];
#pragma unroll
    for (int r = 0; r < kRowBlocks; ++r)
#pragma unroll
        for (int g = 0; g < 16; ++g) { best[r][g] = 0; second[r][g] = 0; }

    // a column past the chunk reads the chunk's last column and is replaced by the zero descriptor (signed bytes -128, column sum
    // 0), whose dot is exactly 0: selects, no branch, so the loads of the next tile stay in flight under this tile's arithmetic
    auto load_tile = [&](int t, uint4* raw, uint32_t& cb) {
        const int64_t src = b_start + min(col0 + t * kTile + lc, col1 - 1);
        cb = (uint32_t)bias128[src];
#pragma unroll
        for (int s = 0; s < 4; ++s) raw[s] = dbias[src * 8 + s * 2 + h];
    };
    auto fold_tile = [&](int t, const uint4* raw, uint32_t cb) {
        const bool ok = col0 + t * kTile + lc < col1;
        const uint32_t colterm = ((ok ? cb : 0u) << kTileBits) | (uint32_t)((1 << kTileBits) - 1 - t);
        v4i bf[4];
#pragma unroll
        for (int s = 0; s < 4; ++s)
            bf[s] = v4i{(int)(ok ? raw[s].x : 0x80808080u), (int)(ok ? raw[s].y : 0x80808080u), (int)(ok ? raw[s].z : 0x80808080u),
                        (int)(ok ? raw[s].w : 0x80808080u)};
#pragma unroll
        for (int r = 0; r < kRowBlocks; ++r) {
            v16i acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(afrag[r][0], bf[0], cinit[r], 0, 0, 0);
#pragma unroll
            for (int s = 1; s < 4; ++s) acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(afrag[r][s], bf[s], acc, 0, 0, 0);
#pragma unroll
            for (int g = 0; g < 16; ++g) {
                const uint32_t key = ((uint32_t)acc[g] << kTileBits) + colterm;
                second[r][g] = umed3(best[r][g], second[r][g], key);
                best[r][g] = max(best[r][g], key);
            }
        }
    };

    // two tiles per trip, each in its own registers: the loads of one are issued before the other is folded
    uint4 b0[4], b1[4];
    uint32_t cb0 = 0, cb1 = 0;
    if (n_tiles > 0) load_tile(0, b0, cb0);
    for (int t = 0; t < n_tiles; t += 2) {
        load_tile(min(t + 1, n_tiles - 1), b1, cb1);      // unconditional (the last tile again at the end): no branch around a load,
        __builtin_amdgcn_sched_barrier(0);                // and the scheduler may not sink the loads to their use
        fold_tile(t, b0, cb0);                            // so the wait before a fold counts exactly the loads issued after its own
        __builtin_amdgcn_sched_barrier(0);
        load_tile(min(t + 2, n_tiles - 1), b0, cb0);
        __builtin_amdgcn_sched_barrier(0);
        fold_tile(t + 1, b1, cb1);                        // tile n_tiles of an odd count (<= 511) is all zero descriptors: dots 0
    }

    // the 32 lanes that share a row, through LDS: lane (row lc, half h) folds 16 of them in column-lane order, then the halves
#pragma unroll
    for (int r = 0; r < kRowBlocks; ++r) {
        __syncthreads();
#pragma unroll
        for (int g = 0; g < 16; ++g) lds[wave][(g & 3) + 8 * (g >> 2) + 4 * h][lc] = make_uint2(best[r][g], second[r][g]);
        __syncthreads();
        uint32_t bd = 0, bj = 0xffffffffu, sd = 0;
        for (int e = h * 16; e < h * 16 + 16; ++e) {
            const uint2 v = lds[wave][lc][e];
            const uint32_t tile = (uint32_t)((1 << kTileBits) - 1) - (v.x & (uint32_t)((1 << kTileBits) - 1));
            merge_top2(bd, bj, sd, v.x >> kTileBits, (uint32_t)col0 + tile * kTile + (uint32_t)e, v.y >> kTileBits);
        }
        const uint32_t od = __shfl_xor(bd, 32, 64), oj = __shfl_xor(bj, 32, 64), os = __shfl_xor(sd, 32, 64);
        merge_top2(bd, bj, sd, od, oj, os);
        const int row = row0 + r * 32 + lc;
        if (h == 0 && row < n_a) part[part_start + (int64_t)chunk * n_a + row] = make_uint4(bd, bj, sd, 0u);
    }
}

// one thread per directed row: chunks in increasing column order (strict >, so the lowest column of equal dots stays), the raw
// integers, and the proposal from the two fp64 comparisons
__global__ void __launch_bounds__(kThreads) match_finalize_kernel(const Job* __restrict__ jobs, int n_jobs, int n_rows,
                                                                  const uint4* __restrict__ part, double max_ratio, double max_distance,
                                                                  int32_t* __restrict__ best, int32_t* __restrict__ best_j,
                                                                  int32_t* __restrict__ second, int32_t* __restrict__ proposal) {
    const int g = (int)blockIdx.x * kThreads + threadIdx.x;
    if (g >= n_rows) return;
    const Job jb = jobs[find_job<&Job::row_start>(jobs, n_jobs, g)];
    const int row = g - jb.row_start;
    uint32_t bd = 0, bj = 0, sd = 0;
    for (int c = 0; c < jb.n_chunks; ++c) {
        const uint4 p = part[jb.part_start + (int64_t)c * jb.n_a + row];
        sd = max(max(sd, p.z), min(bd, p.x));
        if (p.x > bd) { bd = p.x; bj = p.y; }
    }
    const int32_t j = bd > 0 ? (int32_t)bj : -1;
    if (best) best[g] = (int32_t)bd;
    if (best_j) best_j[g] = j;
    if (second) second[g] = (int32_t)sd;
    const double ang_b = acos(fmin((double)bd / 262144.0, 1.0));
    const double ang_s = acos(fmin((double)sd / 262144.0, 1.0));
    const bool ok = bd > 0 && !(ang_b > max_distance) && !(ang_b >= max_ratio * ang_s);
    proposal[g] = ok ? j : -1;
}

// one thread per row of every pair's first image
__global__ void __launch_bounds__(kThreads) match_cross_kernel(const Job* __restrict__ jobs, const int32_t* __restrict__ first_start,
                                                               int n_pairs, int n_first, const int32_t* __restrict__ proposal,
                                                               int cross_check, int32_t* __restrict__ match_index,
                                                               int32_t* __restrict__ num_matches) {
    const int g = (int)blockIdx.x * kThreads + threadIdx.x;
    const bool live = g < n_first;
    int p = 0;
    bool hit = false;
    if (live) {
        int lo = 0, hi = n_pairs;     // first_start[n_pairs] = n_first > g
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (first_start[mid] <= g) lo = mid; else hi = mid;
        }
        p = lo;
        const int i = g - first_start[p];
        int j = proposal[jobs[2 * p].row_start + i];
        if (cross_check && j >= 0 && proposal[jobs[2 * p + 1].row_start + j] != i) j = -1;
        match_index[g] = j;
        hit = j >= 0;
    }
    // integer counts: one add per wave when its rows belong to one pair
    const int p0 = __builtin_amdgcn_readfirstlane(p);
    const bool uniform = __all(!live || p == p0);
    if (uniform) {
        const int n = __popcll(__ballot(hit));
        if (n > 0 && (threadIdx.x & 63) == 0) atomicAdd(&num_matches[p0], n);
    } else if (hit) {
        atomicAdd(&num_matches[p], 1);
    }
}

}  // namespace

extern "C" int64_t ls2fm_match_descriptors_workspace_bytes(const int32_t* image_start, int32_t n_images, const int32_t* pairs,
                                                           int32_t n_pairs) {
    Plan plan;
    const int st = make_plan(image_start, n_images, pairs, n_pairs, &plan);
    if (st != LS2FM_OK) return st;
    return (int64_t)ws_layout(plan, n_pairs, nullptr, nullptr);
}

extern "C" int ls2fm_match_descriptors(const uint8_t* desc, const int32_t* image_start, int32_t n_images, const int32_t* pairs,
                                       int32_t n_pairs, double max_ratio, double max_distance, int32_t cross_check,
                                       int32_t* match_index, int32_t* num_matches, int32_t* best, int32_t* best_j, int32_t* second,
                                       void* workspace, void* stream) {
    Plan plan;
    const int st = make_plan(image_start, n_images, pairs, n_pairs, &plan);
    if (st != LS2FM_OK) return st;
    LS2FM_CHECK_ARG(std::isfinite(max_ratio) && std::isfinite(max_distance) && max_ratio >= 0.0 && max_distance >= 0.0);
    if (n_pairs == 0) return LS2FM_OK;
    const int32_t n_first = plan.first_start[n_pairs];
    LS2FM_CHECK_ARG(num_matches && (desc || plan.n_desc == 0) && (match_index || n_first == 0));
    LS2FM_CHECK_ARG(((uintptr_t)desc & 15) == 0);
    if (!workspace || ((uintptr_t)workspace & 15) != 0) return LS2FM_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    Ws w;
    ws_layout(plan, n_pairs, (char*)workspace, &w);
    const int n_jobs = 2 * n_pairs;
    // the two tables come from pageable host memory: the runtime stages that copy (or waits for it) before this returns, so the
    // vectors may go out of scope; nothing is read back from the device
    if (hipMemcpyAsync(w.jobs, plan.jobs.data(), sizeof(Job) * ((size_t)n_jobs + 1), hipMemcpyHostToDevice, s) != hipSuccess ||
        hipMemcpyAsync(w.first_start, plan.first_start.data(), sizeof(int32_t) * ((size_t)n_pairs + 1), hipMemcpyHostToDevice, s) != hipSuccess ||
        hipMemsetAsync(num_matches, 0, sizeof(int32_t) * (size_t)n_pairs, s) != hipSuccess)
        return ls2fm_launch_status();
    if (plan.n_desc > 0) {
        const int64_t threads = plan.n_desc * 8;
        match_prep_kernel<<<(unsigned)((threads + kThreads - 1) / kThreads), kThreads, 0, s>>>((const uint4*)desc, plan.n_desc, (uint4*)w.dbias,
                                                                                              w.bias128);
    }
    if (plan.n_items > 0)
        match_sweep_kernel<<<(unsigned)((plan.n_items + kSweepWaves - 1) / kSweepWaves), kSweepThreads, 0, s>>>(
            w.jobs, n_jobs, (int)plan.n_items, (const uint4*)w.dbias, w.bias128, plan.chunk_cols, w.part);
    if (plan.n_rows > 0)
        match_finalize_kernel<<<(unsigned)((plan.n_rows + kThreads - 1) / kThreads), kThreads, 0, s>>>(
            w.jobs, n_jobs, (int)plan.n_rows, w.part, max_ratio, max_distance, best, best_j, second, w.proposal);
    if (n_first > 0)
        match_cross_kernel<<<(unsigned)((n_first + kThreads - 1) / kThreads), kThreads, 0, s>>>(w.jobs, w.first_start, n_pairs, n_first,
                                                                                                w.proposal, cross_check, match_index, num_matches);
    return ls2fm_launch_status();
}
