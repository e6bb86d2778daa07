// Exact nearest neighbours between two point clouds over a uniform grid: the primitive under ls2fm.metrics (Chamfer distance of a
// mesh against ground truth) and under any later point-merging or ICP step.  include/ls2fm.h states the rules;
// tests/metrics_restate.py repeats the distance rule in numpy.
//
// The DISTANCE RULE makes the answer a pure function of the two clouds -- no grid, batch or visiting order shows in it:
//   dx = q.x - r.x (dy, dz likewise), d2 = (dx dx + dy dy) + dz dz, every operation one rounded fp32 operation (d2_rule below);
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
#include "ls2fm_device.h"
#include "workspace.h"

#include <algorithm>
#include <climits>
#include <cmath>

namespace {

constexpr int kThreads = 256;
constexpr int kScanThreads = 1024;

struct PgGrid {
    float ox, oy, oz;      // origin: the per-axis minimum of the reference cloud
    float h, inv_h;        // cell size and the fp32 reciprocal the cells are assigned with
    float slack;           // cells by which the fp32 cell assignment can misplace a pair of points (ring_bound)
    int nx, ny, nz;
};

// the cell of coordinate p on one axis: clamp(floor((p - o) * inv_h), 0, dim - 1).  Clamped in float first -- fminf / fmaxf return
// the operand that is not NaN, so a NaN or infinite coordinate lands in a border cell -- and again as an integer, since
// (float)(dim - 1) rounds up above 2^24.  Nothing is indexed with an unclamped value.
__device__ __forceinline__ int cell_axis(float p, float o, float inv_h, int dim) {
    const float u = __fmul_rn(__fsub_rn(p, o), inv_h);
    const float c = fmaxf(fminf(floorf(u), (float)(dim - 1)), 0.0f);
    return min(max((int)c, 0), dim - 1);
}

__device__ __forceinline__ int64_t cell_of(const PgGrid& g, float x, float y, float z) {
    const int cx = cell_axis(x, g.ox, g.inv_h, g.nx), cy = cell_axis(y, g.oy, g.inv_h, g.ny), cz = cell_axis(z, g.oz, g.inv_h, g.nz);
    return ((int64_t)cz * g.ny + cy) * g.nx + cx;
}

// the distance rule.  Spelled with the rounded-operation intrinsics and compiled with contraction off for this function, so
// the result does not depend on the build's -ffp-contract flag.
__device__ __forceinline__ float d2_rule(float qx, float qy, float qz, float rx, float ry, float rz) {
#pragma clang fp contract(off)
    const float dx = __fsub_rn(qx, rx), dy = __fsub_rn(qy, ry), dz = __fsub_rn(qz, rz);
    return __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz));
}

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
// What may be skipped.  Once rings 0 .. k are done, an unvisited reference r differs from the query q by more than k cells on
// some axis, so u(r) - u(q) > k there, u(p) = fl(fl(p - o) * inv_h) being what the cell is the floor of (clamping a query that
// lies outside the box only moves its cell TOWARD the references).  u carries two roundings, an error of at most 2^-23 |u|
// <= 2^-23 dim cells per point, and inv_h one more on the difference: the true separation is at least (k - slack) h with
// slack = 2^-21 max(dim), twice the error of the pair.  fp32 d2 is within 2^-22 relative of the true squared distance,
// and the factor 1 - 2^-18 leaves that sixteen-fold: every unvisited reference has d2 > bound.  So the walk may stop when
// best_d2 < bound -- strictly, so that a tied reference of a later ring, which may hold the lower index, is still visited --
// or when max_d2 < bound, since nothing further out can qualify.
__device__ __forceinline__ float ring_bound(const PgGrid& g, int k) {
    const float kk = __fsub_rn((float)k, g.slack);
    if (!(kk > 0.0f)) return 0.0f;
    const float l = __fmul_rn(kk, g.h);
    return __fmul_rn(__fmul_rn(l, l), 1.0f - 0x1p-18f);
}

struct Best { float d2; int32_t i; };

__device__ __forceinline__ void visit(const float4* __restrict__ sorted, int32_t s, int32_t e, float qx, float qy, float qz,
                                      float max_d2, Best& b) {
    for (int32_t p = s; p < e; ++p) {
        const float4 r = sorted[p];
        const float d2 = d2_rule(qx, qy, qz, r.x, r.y, r.z);
        const int32_t i = __float_as_int(r.w);
        if (d2 <= max_d2 && d2 < INFINITY && (d2 < b.d2 || (d2 == b.d2 && i < b.i))) { b.d2 = d2; b.i = i; }
    }
}

__global__ void __launch_bounds__(kThreads)
pg_query(PgGrid g, const float4* __restrict__ sorted, const int32_t* __restrict__ cell_start, const float* __restrict__ q, int64_t m,
         float max_d2, int max_rings, int32_t* __restrict__ idx, float* __restrict__ d2_out) {
    const int64_t t = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (t >= m) return;
    const float qx = q[3 * t], qy = q[3 * t + 1], qz = q[3 * t + 2];
    Best b = {INFINITY, INT_MAX};
    const int cx = cell_axis(qx, g.ox, g.inv_h, g.nx), cy = cell_axis(qy, g.oy, g.inv_h, g.ny), cz = cell_axis(qz, g.oz, g.inv_h, g.nz);
    // a NaN or infinite query has no neighbour: it takes no walk at all (its d2 would never compare below +inf)
    const bool finite = isfinite(qx) && isfinite(qy) && isfinite(qz);
    for (int k = 0; finite && k < max_rings; ++k) {
        const int x0 = max(cx - k, 0), x1 = min(cx + k, g.nx - 1);
        const int y0 = max(cy - k, 0), y1 = min(cy + k, g.ny - 1);
        const int z0 = max(cz - k, 0), z1 = min(cz + k, g.nz - 1);
        for (int z = z0; z <= z1; ++z) {
            const bool z_face = z == cz - k || z == cz + k;
            for (int y = y0; y <= y1; ++y) {
                const int64_t row = ((int64_t)z * g.ny + y) * g.nx;
                if (z_face || y == cy - k || y == cy + k) {
                    // a whole row of the shell: its cells are neighbours in cell_start, one range
                    visit(sorted, cell_start[row + x0], cell_start[row + x1 + 1], qx, qy, qz, max_d2, b);
                } else {
                    if (cx - k >= 0) visit(sorted, cell_start[row + cx - k], cell_start[row + cx - k + 1], qx, qy, qz, max_d2, b);
                    if (cx + k < g.nx) visit(sorted, cell_start[row + cx + k], cell_start[row + cx + k + 1], qx, qy, qz, max_d2, b);
                }
            }
        }
        if (fminf(b.d2, max_d2) < ring_bound(g, k)) break;
        if (cx - k <= 0 && cx + k >= g.nx - 1 && cy - k <= 0 && cy + k >= g.ny - 1 && cz - k <= 0 && cz + k >= g.nz - 1) break;   // the whole grid
    }
    idx[t] = b.d2 < INFINITY ? b.i : -1;
    d2_out[t] = b.d2;
}

// ------------------------------------------------------------------------------------------------------------------- host
bool grid_ok(const float* origin, float h, float inv_h, const int32_t* dim, int64_t* n_cells) {
    if (!origin || !dim || !(h > 0.0f) || !std::isfinite(h) || !(inv_h > 0.0f) || !std::isfinite(inv_h)) return false;
    int64_t cells = 1;
    for (int a = 0; a < 3; ++a) {
        if (!std::isfinite(origin[a]) || dim[a] < 1) return false;
        cells *= dim[a];
        if (cells >= ((int64_t)1 << 31) - 1) return false;
    }
    *n_cells = cells;
    return true;
}

PgGrid make_grid(const float* origin, float h, float inv_h, const int32_t* dim) {
    const int max_dim = std::max(dim[0], std::max(dim[1], dim[2]));
    return {origin[0], origin[1], origin[2], h, inv_h, (float)max_dim * 0x1p-21f, dim[0], dim[1], dim[2]};
}

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
    const int max_rings = std::max(dim[0], std::max(dim[1], dim[2])) + 1;          // the hard trip bound of the ring loop
    const int64_t blocks = (n_queries + kThreads - 1) / kThreads;
    LS2FM_CHECK_ARG(blocks < ((int64_t)1 << 31));
    pg_query<<<(unsigned)blocks, kThreads, 0, s>>>(g, (const float4*)sorted, cell_start, queries, n_queries, max_d2, max_rings, idx, d2);
    return ls2fm_launch_status();
}
