// What the three two-view models of ransac.h share -- EModel (relative_pose.hip: essential matrices between K-normalised points),
// FModel and HModel (two_view.hip: fundamental matrices and homographies between pixels): the Gauss-Jordan null space of their
// minimal solvers, the kernel of the minimal solvers alone, the sampled solve of ransac.h's hyp_kernel, and final_kernel, one
// workgroup per pair: the inlier count of the rounds' best hypothesis, the local optimisation, the final mask and the outputs.
// pose_math.h holds the pure math.
//
// Besides ransac.h's concept, a two-view model M has a Point of four doubles (x1, y1, x2, y2: what its models relate) and
//     int   solve(p1, p2, column, emit)        the minimal solver on kSample correspondences: emit(slot, M[9]), the number emitted
//     bool  test(M, x1, y1, x2, y2, thr2)      one model against one correspondence (inlier() with the Point unpacked)
//     accumulate(a, x, y, u, v)                the correspondence's row(s) r, as r r^T, onto the 9 x 9 normal matrix's upper triangle
//     kMinInliers, kMaxCand, Lds               the least inlier count worth a re-fit, the re-fit's candidates, its LDS (with cand)
//     int   refit(in, ctx, s0, n, X, cur, lds, s_red)   collective: the inlier set of X (cur of them) -> the number of candidates
//                                              written to lds.cand (the same number in every thread)
//     bool  keeps(have, cur)                   whether the result is written or zeroed (have: the rounds found a hypothesis)
//     Tail                                     the model's own outputs after the local optimisation (E: the pose; F, H: none)
#pragma once

#include "pose_math.h"
#include "ransac.h"

namespace two_view {

using namespace pose_math;
using namespace ransac;

constexpr int kPairThreads = 256;              // final workgroups
constexpr int kLoIters = 10;
constexpr int kNe = 45;                        // upper triangle of the 9 x 9 normal matrix

struct Point { double x1, y1, x2, y2; };

// -------------------------------------------------------------------------------------------------------------- null space
// the (9 - R)-dimensional null space of the R x 9 system at word A of the column: Gauss-Jordan with partial pivoting (a column
// whose largest remaining |entry| is <= 1e-12 of the matrix's largest is free) -> basis vector j (free column f_j, ascending) at
// Bas + 9 j: 1 at f_j, -R[i][f_j] at pivot column i.  Piv: the pivot columns [0, R), then the free ones.  false: rank != R
template <int R, int A, int Piv, int Bas, int S>
HD inline bool gj_nullspace(Col<S> w) {
    double amax = 0.0;
    for (int i = 0; i < 9 * R; ++i) amax = fmax(amax, fabs(w[A + i]));
    if (!(amax > 0.0) || !is_finite(amax)) return false;
    int rank = 0, nfree = 0;
    for (int c = 0; c < 9; ++c) {
        int p = -1;
        double best = 0.0;
        for (int r = rank; r < R; ++r) {
            const double v = fabs(w[A + 9 * r + c]);
            if (p < 0 || v > best) { best = v; p = r; }
        }
        if (rank == R || !(best > 1e-12 * amax)) {
            if (nfree == 9 - R) return false;          // one free column too many: the rank cannot reach R
            w[Piv + R + nfree] = c;
            ++nfree;
            continue;
        }
        for (int k = 0; k < 9; ++k) {
            const double t = w[A + 9 * rank + k];
            w[A + 9 * rank + k] = w[A + 9 * p + k];
            w[A + 9 * p + k] = t;
        }
        const double inv = 1.0 / w[A + 9 * rank + c];
        for (int k = 0; k < 9; ++k) w[A + 9 * rank + k] = w[A + 9 * rank + k] * inv;
        for (int r = 0; r < R; ++r) {
            if (r == rank) continue;
            const double f = w[A + 9 * r + c];
            for (int k = 0; k < 9; ++k) w[A + 9 * r + k] -= f * w[A + 9 * rank + k];
        }
        w[Piv + rank] = c;
        ++rank;
    }
    if (rank != R || nfree != 9 - R) return false;
    for (int j = 0; j < 9 - R; ++j) {
        const int f = (int)w[Piv + R + j];
        for (int k = 0; k < 9; ++k) w[Bas + 9 * j + k] = k == f ? 1.0 : 0.0;
        for (int i = 0; i < R; ++i) w[Bas + 9 * j + (int)w[Piv + i]] = -w[A + 9 * i + f];
    }
    return true;
}

// --------------------------------------------------------------------------------------------------------- minimal solvers
template <class M>
__global__ void __launch_bounds__(M::kHypThreads)
minimal_kernel(const double* __restrict__ x1, const double* __restrict__ x2, int64_t m, double* __restrict__ Mout,
               int32_t* __restrict__ n_sol) {
    constexpr int kK = M::kSample, kS = M::kMaxSol, kT = M::kHypThreads;
    __shared__ double s_buf[M::kHypLdsWords * kT];
    const int64_t i = (int64_t)blockIdx.x * kT + threadIdx.x;
    if (i >= m) return;
    double a[kK][2], b[kK][2];
#pragma unroll
    for (int s = 0; s < kK; ++s) {
        a[s][0] = x1[2 * kK * i + 2 * s]; a[s][1] = x1[2 * kK * i + 2 * s + 1];
        b[s][0] = x2[2 * kK * i + 2 * s]; b[s][1] = x2[2 * kK * i + 2 * s + 1];
    }
    double* __restrict__ out = Mout + 9 * kS * i;
    const int n = M::solve(a, b, Col<kT>{s_buf + threadIdx.x}, [&](int s, const double* e) {
        for (int q = 0; q < 9; ++q) out[9 * s + q] = e[q];
    });
    for (int q = 9 * n; q < 9 * kS; ++q) out[q] = 0.0;
    n_sol[i] = n;
}

// ls2fm_five_point, ls2fm_seven_point, ls2fm_four_point_homography
template <class M>
int minimal_call(const double* x1, const double* x2, int64_t m, double* out, int32_t* n_solutions, void* stream) {
    LS2FM_CHECK_ARG(m >= 0);
    if (m == 0) return LS2FM_OK;
    LS2FM_CHECK_ARG(x1 && x2 && out && n_solutions);
    minimal_kernel<M><<<(unsigned)((m + M::kHypThreads - 1) / M::kHypThreads), M::kHypThreads, 0, (hipStream_t)stream>>>(x1, x2, m, out,
                                                                                                                      n_solutions);
    return ls2fm_launch_status();
}

// M::hypotheses of the three models: the sampled correspondences as M::load gives them, then the minimal solver
template <class M, class Emit>
__device__ __forceinline__ void sampled_solve(const typename M::Input& in, const typename M::Ctx& ctx, int64_t s0,
                                              const int64_t (&id)[M::kSample], double* column, Emit emit) {
    double a[M::kSample][2], b[M::kSample][2];
#pragma unroll
    for (int s = 0; s < M::kSample; ++s) {
        const Point pt = M::load(in, ctx, s0 + id[s]);
        a[s][0] = pt.x1; a[s][1] = pt.y1;
        b[s][0] = pt.x2; b[s][1] = pt.y2;
    }
    M::solve(a, b, Col<M::kHypThreads>{column}, emit);
}

// ------------------------------------------------------------------------------------------------------ local optimisation
// f(j, x1, y1, x2, y2) on the pair's correspondences j = thread, thread + kPairThreads, ... (the order of every per-thread sum)
template <class M, class F>
__device__ __forceinline__ void for_each_corr(const typename M::Input& in, const typename M::Ctx& ctx, int64_t s0, int64_t n, F f) {
    for (int64_t j = threadIdx.x; j < n; j += kPairThreads) {
        const Point pt = M::load(in, ctx, s0 + j);
        f(j, pt.x1, pt.y1, pt.x2, pt.y2);
    }
}

struct Epipolar {                // what E and F share: x2h^T M x1h = 0, scored by the squared Sampson error
    static HD inline bool test(const double* M, double x1, double y1, double x2, double y2, double thr2) {
        return sampson2(M, x1, y1, x2, y2) <= thr2;       // NaN (0 / 0) is not an inlier
    }
    static __device__ __forceinline__ void accumulate(double (&a)[kNe], double x, double y, double u, double v) {
        const double r[9] = {u * x, u * y, u, v * x, v * y, v, x, y, 1.0};
#pragma unroll
        for (int i = 0; i < 9; ++i)
#pragma unroll
            for (int k = i; k < 9; ++k) a[sidx(i, k)] += r[i] * r[k];
    }
};

// collective: the fixed-order sum of the threads' normal matrices a, its eigen-decomposition, and the NV eigenvectors of the
// smallest eigenvalues to dst: the smallest at dst + 9 (NV - 1), the NV-th smallest at dst.  A barrier follows the writes
template <int NV>
__device__ __forceinline__ void smallest_eigenvectors(double (&a)[kNe], double* s_red, double* dst) {
    const int tid = threadIdx.x;
    block_sum<kNe, kPairThreads>(a, s_red);
    double v[9];
    jacobi9(a, tid < 9 ? tid : 0, v);
    if (tid < 9)
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            double x = 0.0;
#pragma unroll
            for (int k = 0; k < 9; ++k) x = eigen_rank9(a, k) == NV - 1 - j ? v[k] : x;
            dst[9 * j + tid] = x;
        }
    __syncthreads();
}

// model: [P][9]; poses: E's [R | t] [P][12], unused by F and H
template <class M>
__global__ void __launch_bounds__(kPairThreads)
final_kernel(typename M::Input in, const int32_t* __restrict__ ps, Ws w, double* __restrict__ model, double* __restrict__ poses,
             uint8_t* __restrict__ inliers, int32_t* __restrict__ num_inliers, int32_t* __restrict__ trials,
             int32_t* __restrict__ best_trial, int32_t* __restrict__ success) {
    __shared__ double s_red[(kPairThreads / 64) * kNe];
    __shared__ typename M::Lds lds;
    __shared__ double X[9];                    // the current model: in LDS, not in registers across the re-fit's 9 x 9 eigenproblem
    __shared__ int s_int;
    const int p = blockIdx.x, tid = threadIdx.x;
    const int64_t s0 = ps[p], n = ps[p + 1] - s0;
    const typename M::Ctx ctx = M::context(in, p);
    const double thr2 = ctx.thr2;
    const unsigned long long bk = w.best_key[p];
    int cur = 0;
    if (tid < 9) X[tid] = bk != 0ull ? w.best[9 * p + tid] : 0.0;
    __syncthreads();
    if (bk != 0ull) {
        for_each_corr<M>(in, ctx, s0, n, [&](int64_t, double x1, double y1, double x2, double y2) {
            cur += M::test(X, x1, y1, x2, y2, thr2) ? 1 : 0;
        });
        cur = block_count(cur, &s_int);
    }
    // every condition below is uniform over the workgroup: it comes from a block-wide sum or from LDS (refit has barriers)
    for (int it = 0; it < kLoIters && cur >= M::kMinInliers; ++it) {
        const int nc = M::refit(in, ctx, s0, n, X, cur, lds, s_red);
        // the first candidate with the largest count.  A lone candidate's changed memberships are counted along with its inliers;
        // among several, the winner's in a pass of its own
        int best_c = -1, best_cnt = -1, chg = 0;
        for (int c = 0; c < M::kMaxCand && c < nc; ++c) {
            int k = 0, d = 0;
            for_each_corr<M>(in, ctx, s0, n, [&](int64_t, double x1, double y1, double x2, double y2) {
                const bool is = M::test(lds.cand[c], x1, y1, x2, y2, thr2);
                k += is ? 1 : 0;
                if constexpr (M::kMaxCand == 1) d += is != M::test(X, x1, y1, x2, y2, thr2) ? 1 : 0;
            });
            k = block_count(k, &s_int);
            if constexpr (M::kMaxCand == 1) chg = block_count(d, &s_int);
            if (k > best_cnt) { best_cnt = k; best_c = c; }
        }
        if (best_c < 0 || best_cnt < cur) break;
        if constexpr (M::kMaxCand > 1) {
            for_each_corr<M>(in, ctx, s0, n, [&](int64_t, double x1, double y1, double x2, double y2) {
                chg += M::test(lds.cand[best_c], x1, y1, x2, y2, thr2) != M::test(X, x1, y1, x2, y2, thr2) ? 1 : 0;
            });
            chg = block_count(chg, &s_int);
        }
        if (tid < 9) X[tid] = lds.cand[best_c][tid];           // after block_count's barrier: nobody reads X any more
        __syncthreads();
        cur = best_cnt;
        if (chg == 0) break;
    }
    const bool keep = M::keeps(bk != 0ull, cur);
    typename M::Tail tail;
    tail.begin(X, keep, lds);
    for_each_corr<M>(in, ctx, s0, n, [&](int64_t j, double x1, double y1, double x2, double y2) {
        const bool is = keep && M::test(X, x1, y1, x2, y2, thr2);
        inliers[s0 + j] = is ? 1 : 0;
        if (is) tail.inlier(lds, x1, y1, x2, y2);
    });
    const bool ok = tail.finish(keep, cur, lds, &s_int, poses, p);
    if (tid < 9) model[9 * p + tid] = keep ? X[tid] : 0.0;
    if (tid == 0) {
        num_inliers[p] = keep ? cur : 0;
        trials[p] = w.trials[p];
        best_trial[p] = bk != 0ull ? best_trial_of<M>(bk) : -1;
        success[p] = ok ? 1 : 0;
    }
}

struct NoTail {                  // F and H: success is a kept result
    template <class Lds> __device__ __forceinline__ void begin(const double*, bool, Lds&) {}
    template <class Lds> __device__ __forceinline__ void inlier(Lds&, double, double, double, double) {}
    template <class Lds> __device__ __forceinline__ bool finish(bool keep, int, Lds&, int*, double*, int) { return keep; }
};

// ------------------------------------------------------------------------------------------------------------------- host
// ls2fm_relative_pose, ls2fm_fundamental_matrix, ls2fm_homography after their own argument checks: the rounds, the final kernel
template <class M>
int estimate(const typename M::Input& in, const int32_t* pair_start, int32_t n_pairs, bool have_corr, const ls2fm_pose_ransac_opts* opts,
             double* model, double* poses, uint8_t* inliers, int32_t* num_inliers, int32_t* trials, int32_t* best_trial, int32_t* success,
             void* workspace, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    Ws w;
    const int st = run_rounds<M>(in, pair_start, n_pairs, have_corr, opts, workspace, s, &w);
    if (st != LS2FM_OK) return st;
    final_kernel<M><<<(unsigned)n_pairs, kPairThreads, 0, s>>>(in, pair_start, w, model, poses, inliers, num_inliers, trials, best_trial,
                                                               success);
    return ls2fm_launch_status();
}

template <class M>
int64_t workspace_bytes(int32_t n_pairs, int64_t n_corr) {
    if (n_pairs < 1 || n_pairs > LS2FM_RELPOSE_MAX_PAIRS || n_corr < 0) return LS2FM_ERR_INVALID_ARGUMENT;
    return (int64_t)ws_layout<M>(n_pairs, nullptr, nullptr);
}

}  // namespace two_view
