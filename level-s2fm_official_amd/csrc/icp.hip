// ICP registration of a moving cloud to a fixed one over the uniform point grid (ls2fm.metrics.icp): Gauss-Newton on the
// similarity (s, R, t) in fp64, correspondences by the distance rule of grid_walk.h.  include/ls2fm.h states the rules;
// tests/icp_restate.py repeats them in numpy.
//
// One iteration is two launches, and nothing is read back:
//   icp_accumulate  one source point per lane in a grid-stride loop: p' = s R p + t in fp64 (stated association), rounded once
//                   to fp32, the grid walk (the winner's xyz comes back in registers), the pair's terms of the normal equations
//                   added to the lane's 36 fp64 sums in index order; block_sum (wave_ops.h) per workgroup, one partial row and
//                   one pair count per workgroup into the workspace.  No atomic of any kind.
//   icp_solve       ONE workgroup: the partial rows added in row order, the pair counts added, H delta = -g by Cholesky
//                   (lm_math.h), the update, the status.
// Both read the status word of the state first and do nothing once it is not RUNNING, so a fixed launch count is correct and
// the whole call replays from a graph.  The launch shape and the layout of the partials depend on n_src alone.
#include "grid_walk.h"
#include "lm_math.h"
#include "ls2fm_device.h"
#include "workspace.h"

namespace {

using namespace grid_walk;

constexpr int kThreads = 512;             // icp_accumulate
constexpr int kMaxBlocks = 512;           // one pass covers 2^18 source points; the lanes stride over the rest
constexpr int kSolveThreads = 256;
constexpr int kSums = 36;                 // 28 of H's upper triangle, 7 of g, the cost
constexpr int kStage = 64;                // partial rows staged through LDS at a time by icp_solve

enum { S_SCALE = 0, S_R = 1, S_T = 10, S_COST = 13, S_PAIRS = 14, S_ITERS = 15, S_STATUS = 16, S_SIZE = 24 };
enum { RUNNING = 0, CONVERGED = 1, DEGENERATE = 2 };
enum { MODE_STEP = 0, MODE_EVALUATE = 1, MODE_EMPTY = 2 };

int64_t blocks_of(int64_t n_src) { return std::max<int64_t>(1, std::min<int64_t>((n_src + kThreads - 1) / kThreads, kMaxBlocks)); }

struct IcpWs {
    double* rows;              // [blocks_of(n_src)][36]
    int32_t* counts;           // [blocks_of(n_src)]
};

size_t icp_layout(int64_t n_src, void* base, IcpWs* w) {
    Workspace ws(base, 256);
    const size_t blocks = (size_t)blocks_of(n_src);
    double* rows = ws.take<double>(blocks * kSums);
    int32_t* counts = ws.take<int32_t>(blocks);
    if (w) *w = {rows, counts};
    return ws.bytes();
}

// the terms of one pair: H's upper triangle row-major, g, the cost.  J has ROWS rows of 7 and r ROWS entries; with three rows a
// term is (row 0 + row 1) + row 2.  Every operation rounds once.
template <int ROWS>
__device__ __forceinline__ void add_terms(const double (&J)[ROWS][7], const double (&r)[ROWS], double (&acc)[kSums]) {
#pragma clang fp contract(off)
    int q = 0;
#pragma unroll
    for (int a = 0; a < 7; ++a)
#pragma unroll
        for (int b = a; b < 7; ++b) {
            double t = J[0][a] * J[0][b];
            if (ROWS == 3) t = (t + J[1][a] * J[1][b]) + J[2][a] * J[2][b];
            acc[q++] += t;
        }
#pragma unroll
    for (int a = 0; a < 7; ++a) {
        double t = J[0][a] * r[0];
        if (ROWS == 3) t = (t + J[1][a] * r[1]) + J[2][a] * r[2];
        acc[q++] += t;
    }
    double c = r[0] * r[0];
    if (ROWS == 3) c = (c + r[1] * r[1]) + r[2] * r[2];
    acc[q] += c;
}

// four waves per SIMD (128 VGPRs): the 36 fp64 sums take 72 of them, and the walk wants the occupancy
template <bool PLANE>
__global__ void __launch_bounds__(kThreads, 4)
icp_accumulate(PgGrid g, const float4* __restrict__ sorted, const int32_t* __restrict__ cell_start, const float* __restrict__ src,
               int64_t n_src, const float* __restrict__ normals, float max_d2, int max_rings, const double* state,
               double* __restrict__ rows, int32_t* __restrict__ counts, int32_t* __restrict__ pair_idx, float* __restrict__ pair_d2) {
#pragma clang fp contract(off)
    __shared__ double s_red[(kThreads / 64) * kSums];
    __shared__ int s_cnt[kThreads / 64];
    if (state[S_STATUS] != (double)RUNNING) return;
    const double s = state[S_SCALE];
    double R[9], t[3];
#pragma unroll
    for (int i = 0; i < 9; ++i) R[i] = state[S_R + i];
#pragma unroll
    for (int i = 0; i < 3; ++i) t[i] = state[S_T + i];
    double acc[kSums];
#pragma unroll
    for (int q = 0; q < kSums; ++q) acc[q] = 0.0;
    int n_pairs = 0;
    const int64_t stride = (int64_t)gridDim.x * kThreads;
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n_src; i += stride) {
        const double x = (double)src[3 * i], y = (double)src[3 * i + 1], z = (double)src[3 * i + 2];
        float pf[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) pf[a] = (float)(s * ((R[3 * a] * x + R[3 * a + 1] * y) + R[3 * a + 2] * z) + t[a]);
        // a non-finite p' takes no walk (nearest): no pair
        const Best b = nearest(g, sorted, cell_start, pf[0], pf[1], pf[2], max_d2, max_rings);
        const bool has = b.d2 < INFINITY;
        if (pair_idx) pair_idx[i] = has ? b.i : -1;
        if (pair_d2) pair_d2[i] = b.d2;
        if (!has) continue;
        ++n_pairs;
        const double px = (double)pf[0], py = (double)pf[1], pz = (double)pf[2];
        const double dx = px - (double)b.x, dy = py - (double)b.y, dz = pz - (double)b.z;
        if (PLANE) {
            const double nx = (double)normals[3 * (int64_t)b.i], ny = (double)normals[3 * (int64_t)b.i + 1], nz = (double)normals[3 * (int64_t)b.i + 2];
            const double J[1][7] = {{py * nz - pz * ny, pz * nx - px * nz, px * ny - py * nx, nx, ny, nz, (nx * px + ny * py) + nz * pz}};
            const double r[1] = {(nx * dx + ny * dy) + nz * dz};
            add_terms<1>(J, r, acc);
        } else {
            const double J[3][7] = {{0.0, pz, -py, 1.0, 0.0, 0.0, px}, {-pz, 0.0, px, 0.0, 1.0, 0.0, py}, {py, -px, 0.0, 0.0, 0.0, 1.0, pz}};
            const double r[3] = {dx, dy, dz};
            add_terms<3>(J, r, acc);
        }
    }
    block_sum<kSums, kThreads>(acc, s_red);
    const int tid = threadIdx.x;
    const int wave_pairs = wave_sum(n_pairs);
    if ((tid & 63) == 0) s_cnt[tid >> 6] = wave_pairs;
    __syncthreads();
    if (tid == 0) {
        int total = 0;
#pragma unroll
        for (int w = 0; w < kThreads / 64; ++w) total += s_cnt[w];
        counts[blockIdx.x] = total;
#pragma unroll
        for (int q = 0; q < kSums; ++q) rows[(int64_t)blockIdx.x * kSums + q] = acc[q];
    }
}

// -1 / +inf into the pair arrays of a call without a reference cloud, under the same status rule
__global__ void __launch_bounds__(kThreads)
icp_no_pairs(const double* state, int64_t n_src, int32_t* __restrict__ pair_idx, float* __restrict__ pair_d2) {
    if (state[S_STATUS] != (double)RUNNING) return;
    const int64_t stride = (int64_t)gridDim.x * kThreads;
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n_src; i += stride) {
        if (pair_idx) pair_idx[i] = -1;
        if (pair_d2) pair_d2[i] = INFINITY;
    }
}

// thread 0: solve and update.  a: the 36 sums.  -> the new status; the transform is written only where a step is taken
template <int M>
__device__ inline int solve_and_update(const double (&a)[kSums], double* state, double tol_rot, double tol_trans) {
#pragma clang fp contract(off)
    constexpr int T = M * (M + 1) / 2;
    double sys[T + M];
    int q = 0;
    // the leading M x M of the 7 x 7 triangle, then the leading M of g
#pragma unroll
    for (int r = 0; r < M; ++r)
#pragma unroll
        for (int c = r; c < M; ++c) sys[q++] = a[r * 7 - r * (r - 1) / 2 + (c - r)];
#pragma unroll
    for (int i = 0; i < M; ++i) sys[T + i] = a[28 + i];
    double d[M];
    const double zero[M] = {};
    if (!lm_math::chol_solve(sys, 0.0, zero, d)) return DEGENERATE;
    const double lambda = M == 7 ? d[M - 1] : 0.0;
    double E[3][3];
    lm_math::rodrigues(d[0], d[1], d[2], E);
    // k = exp(lambda) as 1 + expm1(lambda): the error of the library function then scales with |lambda|
    const double k = M == 7 ? 1.0 + expm1(lambda) : 1.0;
    double R[9], t[3];
#pragma unroll
    for (int i = 0; i < 9; ++i) R[i] = state[S_R + i];
#pragma unroll
    for (int i = 0; i < 3; ++i) t[i] = state[S_T + i];
    state[S_SCALE] = k * state[S_SCALE];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) state[S_R + 3 * i + j] = (E[i][0] * R[j] + E[i][1] * R[3 + j]) + E[i][2] * R[6 + j];
        state[S_T + i] = k * ((E[i][0] * t[0] + E[i][1] * t[1]) + E[i][2] * t[2]) + d[3 + i];
    }
    const double rot = fmax(fmax(fabs(d[0]), fabs(d[1])), fmax(fabs(d[2]), fabs(lambda)));
    const double trans = fmax(fabs(d[3]), fmax(fabs(d[4]), fabs(d[5])));
    return rot <= tol_rot && trans <= tol_trans ? CONVERGED : RUNNING;
}

__global__ void __launch_bounds__(kSolveThreads)
icp_solve(const double* __restrict__ rows, const int32_t* __restrict__ counts, int n_rows, int mode, int with_scale, double tol_rot,
          double tol_trans, double* state, double* __restrict__ sums_out) {
    __shared__ double s_stage[kStage * kSums];
    __shared__ long long s_cnt[kSolveThreads / 64];
    if (state[S_STATUS] != (double)RUNNING) return;
    const int tid = threadIdx.x;
    double acc = 0.0;                                   // thread q < 36: sum q, the rows in row order
    for (int base = 0; base < n_rows; base += kStage) {
        const int n = min(kStage, n_rows - base);
        for (int e = tid; e < n * kSums; e += kSolveThreads) s_stage[e] = rows[(int64_t)base * kSums + e];
        __syncthreads();
        if (tid < kSums)
            for (int r = 0; r < n; ++r) acc += s_stage[r * kSums + tid];
        __syncthreads();
    }
    long long c = 0;                                    // integers: any order
    for (int r = tid; r < n_rows; r += kSolveThreads) c += counts[r];
    c = wave_sum(c);
    if ((tid & 63) == 0) s_cnt[tid >> 6] = c;
    if (tid < kSums) s_stage[tid] = acc;
    __syncthreads();
    if (tid < kSums && sums_out) sums_out[tid] = acc;
    if (tid != 0) return;
    long long n_pairs = 0;
#pragma unroll
    for (int w = 0; w < kSolveThreads / 64; ++w) n_pairs += s_cnt[w];
    double a[kSums];
#pragma unroll
    for (int q = 0; q < kSums; ++q) a[q] = s_stage[q];
    state[S_COST] = a[kSums - 1];
    state[S_PAIRS] = (double)n_pairs;
#pragma unroll
    for (int i = S_STATUS + 1; i < S_SIZE; ++i) state[i] = 0.0;
    if (mode == MODE_EVALUATE) return;
    int status = DEGENERATE;
    if (mode == MODE_STEP && n_pairs >= (with_scale ? 7 : 6))
        status = with_scale ? solve_and_update<7>(a, state, tol_rot, tol_trans) : solve_and_update<6>(a, state, tol_rot, tol_trans);
    if (status != DEGENERATE) state[S_ITERS] = state[S_ITERS] + 1.0;
    state[S_STATUS] = (double)status;
}

bool tol_ok(double v) { return !(v != v) && v >= 0.0; }

}  // namespace

extern "C" int64_t ls2fm_icp_workspace_bytes(int64_t n_src) {
    if (n_src < 0 || n_src >= ((int64_t)1 << 31)) return (int64_t)LS2FM_ERR_INVALID_ARGUMENT;
    return (int64_t)icp_layout(n_src, nullptr, nullptr);
}

extern "C" int ls2fm_icp_run(const float* src, int64_t n_src, const float* sorted, const int32_t* cell_start, int64_t n_dst,
                             const float* origin, float cell_size, float inv_cell_size, const int32_t* dim, const float* dst_normals,
                             float max_d2, int32_t with_scale, int32_t iters, double tol_rot, double tol_trans, double* state,
                             double* sums, int32_t* pair_idx, float* pair_d2, void* workspace, void* stream) {
    int64_t n_cells = 0;
    LS2FM_CHECK_ARG(n_src >= 0 && n_src < ((int64_t)1 << 31) && n_dst >= 0 && n_dst < ((int64_t)1 << 31));
    LS2FM_CHECK_ARG(grid_ok(origin, cell_size, inv_cell_size, dim, &n_cells));
    LS2FM_CHECK_ARG(!(max_d2 != max_d2) && max_d2 >= 0.0f && tol_ok(tol_rot) && tol_ok(tol_trans));
    LS2FM_CHECK_ARG(iters >= 0 && iters <= LS2FM_ICP_MAX_ITERS && state);
    LS2FM_CHECK_ARG(src || n_src == 0);
    LS2FM_CHECK_ARG((sorted && cell_start && ((uintptr_t)sorted & 15) == 0) || n_dst == 0 || n_src == 0);
    if (!workspace) return LS2FM_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    IcpWs w;
    icp_layout(n_src, workspace, &w);
    const unsigned blocks = (unsigned)blocks_of(n_src);
    if (n_src == 0 || n_dst == 0) {                    // no pairs: no walk, status DEGENERATE at once
        if (n_src && (pair_idx || pair_d2)) icp_no_pairs<<<blocks, kThreads, 0, st>>>(state, n_src, pair_idx, pair_d2);
        icp_solve<<<1, kSolveThreads, 0, st>>>(w.rows, w.counts, 0, MODE_EMPTY, with_scale, tol_rot, tol_trans, state, sums);
        return ls2fm_launch_status();
    }
    const PgGrid g = make_grid(origin, cell_size, inv_cell_size, dim);
    const int rings = max_rings(dim);
    for (int it = 0; it < std::max(iters, 1); ++it) {
        if (dst_normals)
            icp_accumulate<true><<<blocks, kThreads, 0, st>>>(g, (const float4*)sorted, cell_start, src, n_src, dst_normals, max_d2, rings,
                                                             state, w.rows, w.counts, pair_idx, pair_d2);
        else
            icp_accumulate<false><<<blocks, kThreads, 0, st>>>(g, (const float4*)sorted, cell_start, src, n_src, nullptr, max_d2, rings,
                                                              state, w.rows, w.counts, pair_idx, pair_d2);
        icp_solve<<<1, kSolveThreads, 0, st>>>(w.rows, w.counts, (int)blocks, iters ? MODE_STEP : MODE_EVALUATE, with_scale, tol_rot,
                                               tol_trans, state, sums);
    }
    return ls2fm_launch_status();
}
