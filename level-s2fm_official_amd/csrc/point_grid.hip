// Exact nearest neighbours between two point clouds over a uniform grid: the primitive under ls2fm.metrics (Chamfer distance of a
// mesh against ground truth) and under any later point-merging or ICP step.  include/ls2fm.h states the rules;
// tests/metrics_restate.py repeats the distance rule in numpy.
//
// The DISTANCE RULE makes the answer a pure function of the two clouds -- no grid, batch or visiting order shows in it:
//   dx = q.x - r.x (dy, dz likewise), d2 = (dx dx + dy dy) + dz dz, every operation one rounded fp32 operation (d2_rule, grid_walk.h);
//   a reference QUALIFIES when d2 <= max_d2 and d2 < +inf; the winner is the smallest d2, among equal d2 the lowest original index.
//
// ls2fm_point_grid_build (five launches after one memset):
//   pg_count      one lane per reference point: cursor[cell]++ (32-bit integer atomic)
//   pg_scan_local per 1024 cells an exclusive prefix sum into cell_start, the block's total into block_sum
//   pg_scan_sums  ONE workgroup: exclusive prefix sum of block_sum, cell_start[n_cells] = N
//   pg_scan_add   cell_start[c] += block_sum[block of c], cursor[c] = 0
//   pg_scatter    one lane per reference point: slot = cell_start[cell] + cursor[cell]++, sorted[slot] = (x, y, z, bits of index).
//                 The order inside a cell is the order the atomics arrived in; it cannot show, ties break on the stored index.
// ls2fm_point_grid_query (one launch): pg_query, one query per lane -- its own cell, then Chebyshev rings 1, 2, ... (ring_bound).
// ls2fm_point_grid_knn (one launch): pg_knn<8 | 16 | 32>, one query per lane, the K-NEIGHBOUR RULE: the same rings with a sorted
// list of the k best in registers (KList, k_nearest), the instantiation the smallest capacity >= k.
// The walk itself -- cells, distance rule, ring bound, ring loops -- is grid_walk.h's, shared with icp.hip.
#include "grid_walk.h"
#include "ls2fm_device.h"
#include "workspace.h"

namespace {

using namespace grid_walk;

constexpr int kThreads = 256;
constexpr int kScanThreads = 1024;

// ------------------------------------------------------------------------------------------------------------------ build
__global__ void __launch_bounds__(kThreads)
pg_count(PgGrid g, const float* __restrict__ ref, int64_t n, int32_t* cursor) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    atomicAdd(cursor + cell_of(g, ref[3 * i], ref[3 * i + 1], ref[3 * i + 2]), 1);
}

__global__ void __launch_bounds__(kScanThreads)
pg_scan_local(const int32_t* __restrict__ count, int64_t n_cells, int32_t* __restrict__ cell_start, int32_t* __restrict__ block_sum) {
    const int tid = threadIdx.x;
    const int64_t c = (int64_t)blockIdx.x * kScanThreads + tid;
    int total;
    const int excl = block_exclusive_scan<kScanThreads>(c < n_cells ? count[c] : 0, total);
    if (c < n_cells) cell_start[c] = excl;
    if (tid == 0) block_sum[blockIdx.x] = total;
}

__global__ void __launch_bounds__(kScanThreads)
pg_scan_sums(int32_t* block_sum, int64_t n_blocks, int32_t* __restrict__ cell_start_end) {
    const int tid = threadIdx.x;
    int carry = 0;
    for (int64_t base = 0; base < n_blocks; base += kScanThreads) {
        const int64_t b = base + tid;
        int total;
        const int excl = block_exclusive_scan<kScanThreads>(b < n_blocks ? block_sum[b] : 0, total);
        if (b < n_blocks) block_sum[b] = carry + excl;
        carry += total;
    }
    if (tid == 0) *cell_start_end = carry;
}

__global__ void __launch_bounds__(kScanThreads)
pg_scan_add(int32_t* __restrict__ cell_start, int64_t n_cells, const int32_t* __restrict__ block_sum, int32_t* __restrict__ cursor) {
    const int64_t c = (int64_t)blockIdx.x * kScanThreads + threadIdx.x;
    if (c >= n_cells) return;
    cell_start[c] += block_sum[blockIdx.x];
    cursor[c] = 0;
}

__global__ void __launch_bounds__(kThreads)
pg_scatter(PgGrid g, const float* __restrict__ ref, int64_t n, const int32_t* __restrict__ cell_start, int32_t* cursor,
           float4* __restrict__ sorted) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const float x = ref[3 * i], y = ref[3 * i + 1], z = ref[3 * i + 2];
    const int64_t c = cell_of(g, x, y, z);
    // cell_start[c] + (arrival number) < cell_start[c + 1] <= n: pg_count counted this very point into cell c
    const int64_t slot = (int64_t)cell_start[c] + atomicAdd(cursor + c, 1);
    if (slot < n) sorted[slot] = make_float4(x, y, z, __int_as_float((int32_t)i));
}

// ------------------------------------------------------------------------------------------------------------------ query
// ring_bound, visit and the ring loop (nearest): grid_walk.h
__global__ void __launch_bounds__(kThreads)
pg_query(PgGrid g, const float4* __restrict__ sorted, const int32_t* __restrict__ cell_start, const float* __restrict__ q, int64_t m,
         float max_d2, int max_rings, int32_t* __restrict__ idx, float* __restrict__ d2_out) {
    const int64_t t = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (t >= m) return;
    const Best b = nearest(g, sorted, cell_start, q[3 * t], q[3 * t + 1], q[3 * t + 2], max_d2, max_rings);
    idx[t] = b.d2 < INFINITY ? b.i : -1;
    d2_out[t] = b.d2;
}

// KList and the ring loop (k_nearest): grid_walk.h.  Row t of idx / d2 is the list's first k slots; only compile-time slots.
template <int CAP>
__global__ void __launch_bounds__(kThreads)
pg_knn(PgGrid g, const float4* __restrict__ sorted, const int32_t* __restrict__ cell_start, const float* __restrict__ q, int64_t m, int k,
       float max_d2, int skip_own, int max_rings, int32_t* __restrict__ idx, float* __restrict__ d2_out, int32_t* __restrict__ count) {
    const int64_t t = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (t >= m) return;
    KList<CAP> l;
    k_nearest<CAP>(g, sorted, cell_start, q[3 * t], q[3 * t + 1], q[3 * t + 2], max_d2, skip_own ? (int32_t)t : -1, k, max_rings, l);
    int n = 0;
#pragma unroll
    for (int j = 0; j < CAP; ++j) {
        if (j < k) {
            const bool has = l.d2[j] < INFINITY;
            idx[t * k + j] = has ? l.i[j] : -1;
            d2_out[t * k + j] = l.d2[j];
            n += has ? 1 : 0;
        }
    }
    count[t] = n;
}

template <int CAP>
void launch_knn(unsigned blocks, hipStream_t s, const PgGrid& g, const float* sorted, const int32_t* cell_start, const float* q, int64_t m,
                int k, float max_d2, int skip_own, int max_rings, int32_t* idx, float* d2, int32_t* count) {
    pg_knn<CAP><<<blocks, kThreads, 0, s>>>(g, (const float4*)sorted, cell_start, q, m, k, max_d2, skip_own, max_rings, idx, d2, count);
}

// ------------------------------------------------------------------------------------------------------------------- host
// grid_ok, make_grid and max_rings: grid_walk.h
int64_t scan_blocks(int64_t n_cells) { return (n_cells + kScanThreads - 1) / kScanThreads; }

struct PgWs {
    int32_t* cursor;           // [n_cells]
    int32_t* block_sum;        // [scan_blocks(n_cells)]
};

size_t pg_layout(int64_t n_cells, void* base, PgWs* w) {
    Workspace ws(base, 256);
    int32_t* cursor = ws.take<int32_t>((size_t)n_cells);
    int32_t* block_sum = ws.take<int32_t>((size_t)scan_blocks(n_cells));
    if (w) *w = {cursor, block_sum};
    return ws.bytes();
}

}  // namespace

extern "C" int64_t ls2fm_point_grid_workspace_bytes(int64_t n_points, int64_t n_cells) {
    if (n_points < 0 || n_points >= ((int64_t)1 << 31) || n_cells < 1 || n_cells >= ((int64_t)1 << 31) - 1)
        return (int64_t)LS2FM_ERR_INVALID_ARGUMENT;
    return (int64_t)pg_layout(n_cells, nullptr, nullptr);
}

extern "C" int ls2fm_point_grid_build(const float* ref, int64_t n_points, const float* origin, float cell_size, float inv_cell_size,
                                      const int32_t* dim, int32_t* cell_start, float* sorted, void* workspace, void* stream) {
    int64_t n_cells = 0;
    LS2FM_CHECK_ARG(n_points >= 0 && n_points < ((int64_t)1 << 31) && grid_ok(origin, cell_size, inv_cell_size, dim, &n_cells));
    LS2FM_CHECK_ARG(cell_start && ((ref && sorted) || n_points == 0) && ((uintptr_t)sorted & 15) == 0);
    if (!workspace) return LS2FM_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    if (n_points == 0) {
        if (hipMemsetAsync(cell_start, 0, (size_t)(n_cells + 1) * sizeof(int32_t), s) != hipSuccess) return ls2fm_launch_status();
        return LS2FM_OK;
    }
    const PgGrid g = make_grid(origin, cell_size, inv_cell_size, dim);
    PgWs w;
    pg_layout(n_cells, workspace, &w);
    const int64_t n_blocks = scan_blocks(n_cells);
    const unsigned point_blocks = (unsigned)((n_points + kThreads - 1) / kThreads);
    if (hipMemsetAsync(w.cursor, 0, (size_t)n_cells * sizeof(int32_t), s) != hipSuccess) return ls2fm_launch_status();
    pg_count<<<point_blocks, kThreads, 0, s>>>(g, ref, n_points, w.cursor);
    pg_scan_local<<<(unsigned)n_blocks, kScanThreads, 0, s>>>(w.cursor, n_cells, cell_start, w.block_sum);
    pg_scan_sums<<<1, kScanThreads, 0, s>>>(w.block_sum, n_blocks, cell_start + n_cells);
    pg_scan_add<<<(unsigned)n_blocks, kScanThreads, 0, s>>>(cell_start, n_cells, w.block_sum, w.cursor);
    pg_scatter<<<point_blocks, kThreads, 0, s>>>(g, ref, n_points, cell_start, w.cursor, (float4*)sorted);
    return ls2fm_launch_status();
}

extern "C" int ls2fm_point_grid_query(const float* queries, int64_t n_queries, const float* sorted, const int32_t* cell_start,
                                      int64_t n_points, const float* origin, float cell_size, float inv_cell_size, const int32_t* dim,
                                      float max_d2, int32_t* idx, float* d2, void* stream) {
    int64_t n_cells = 0;
    LS2FM_CHECK_ARG(n_queries >= 0 && n_points >= 0 && n_points < ((int64_t)1 << 31) && grid_ok(origin, cell_size, inv_cell_size, dim, &n_cells));
    LS2FM_CHECK_ARG(!(max_d2 != max_d2) && max_d2 >= 0.0f);
    if (n_queries == 0) return LS2FM_OK;
    LS2FM_CHECK_ARG(queries && idx && d2);
    hipStream_t s = (hipStream_t)stream;
    if (n_points == 0) {                       // no reference: every query is without a neighbour
        if (hipMemsetD32Async((hipDeviceptr_t)idx, -1, (size_t)n_queries, s) != hipSuccess) return ls2fm_launch_status();
        if (hipMemsetD32Async((hipDeviceptr_t)d2, 0x7f800000, (size_t)n_queries, s) != hipSuccess) return ls2fm_launch_status();
        return LS2FM_OK;
    }
    LS2FM_CHECK_ARG(sorted && cell_start && ((uintptr_t)sorted & 15) == 0);
    const PgGrid g = make_grid(origin, cell_size, inv_cell_size, dim);
    const int64_t blocks = (n_queries + kThreads - 1) / kThreads;
    LS2FM_CHECK_ARG(blocks < ((int64_t)1 << 31));
    pg_query<<<(unsigned)blocks, kThreads, 0, s>>>(g, (const float4*)sorted, cell_start, queries, n_queries, max_d2, max_rings(dim), idx, d2);
    return ls2fm_launch_status();
}

extern "C" int ls2fm_point_grid_knn(const float* queries, int64_t n_queries, const float* sorted, const int32_t* cell_start,
                                    int64_t n_points, const float* origin, float cell_size, float inv_cell_size, const int32_t* dim,
                                    int32_t k, float max_d2, int32_t skip_own, int32_t* idx, float* d2, int32_t* count, void* stream) {
    int64_t n_cells = 0;
    LS2FM_CHECK_ARG(n_queries >= 0 && n_points >= 0 && n_points < ((int64_t)1 << 31) && grid_ok(origin, cell_size, inv_cell_size, dim, &n_cells));
    LS2FM_CHECK_ARG(!(max_d2 != max_d2) && max_d2 >= 0.0f && k >= 1 && k <= 32);
    LS2FM_CHECK_ARG(!skip_own || n_queries == n_points);
    if (n_queries == 0) return LS2FM_OK;
    LS2FM_CHECK_ARG(queries && idx && d2 && count);
    hipStream_t s = (hipStream_t)stream;
    if (n_points == 0) {                       // no reference: every slot is empty
        if (hipMemsetD32Async((hipDeviceptr_t)idx, -1, (size_t)n_queries * k, s) != hipSuccess) return ls2fm_launch_status();
        if (hipMemsetD32Async((hipDeviceptr_t)d2, 0x7f800000, (size_t)n_queries * k, s) != hipSuccess) return ls2fm_launch_status();
        if (hipMemsetD32Async((hipDeviceptr_t)count, 0, (size_t)n_queries, s) != hipSuccess) return ls2fm_launch_status();
        return LS2FM_OK;
    }
    LS2FM_CHECK_ARG(sorted && cell_start && ((uintptr_t)sorted & 15) == 0);
    const PgGrid g = make_grid(origin, cell_size, inv_cell_size, dim);
    const int64_t blocks = (n_queries + kThreads - 1) / kThreads;
    LS2FM_CHECK_ARG(blocks < ((int64_t)1 << 31));
    const int rings = max_rings(dim);
    if (k <= 8) launch_knn<8>((unsigned)blocks, s, g, sorted, cell_start, queries, n_queries, k, max_d2, skip_own, rings, idx, d2, count);
    else if (k <= 16) launch_knn<16>((unsigned)blocks, s, g, sorted, cell_start, queries, n_queries, k, max_d2, skip_own, rings, idx, d2, count);
    else launch_knn<32>((unsigned)blocks, s, g, sorted, cell_start, queries, n_queries, k, max_d2, skip_own, rings, idx, d2, count);
    return ls2fm_launch_status();
}
