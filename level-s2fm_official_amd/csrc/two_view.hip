// Uncalibrated two-view geometry of many view pairs in one call: LO-RANSAC over the seven-point fundamental matrix and over the
// four-point homography, in pixels, all geometry in fp64 -- the F and H of COLMAP's two-view geometry, whose inlier counts (with
// ls2fm_relative_pose's E) give the CALIBRATED / UNCALIBRATED / PLANAR_OR_PANORAMIC / DEGENERATE verdict of ls2fm.pose.
// include/ls2fm.h states the rules; tests/twoview_restate.py repeats them in numpy.  Correspondences are SORTED BY PAIR.
//
// The rounds (hypotheses, scoring, selection, the stopping rule) are csrc/ransac.h's, run on the models FModel (squared Sampson
// error) and HModel (squared forward transfer error): one thread per (pair, trial), the minimal solver on kSample distinct
// correspondences.  Then csrc/two_view.h's final_kernel, which relative_pose.hip's EModel shares: local optimisation (here the
// Hartley-normalised DLT on the inlier set through the 9 x 9 normal matrix's smallest eigenvector) and the final mask, one
// workgroup per pair with fixed-order reductions: every bit is a function of the pair's own data, seed and options.
//
// A minimal solve's run-time-indexed state (the R x 9 system, the pivot columns, the null-space basis: kWords fp64 words) is a
// column of LDS, word k of thread j at s_buf[k * kMsThreads + j], as in relative_pose.hip: no kernel of this file indexes a
// private array at run time.  64 threads per workgroup: kWords x 64 x 8 B = 50 KB.
#include "two_view.h"

#include <cfloat>
#include <cmath>

namespace {

using namespace two_view;

constexpr int kMsThreads = 64;                 // minimal-solver workgroups (hypotheses, ls2fm_seven_point, ls2fm_four_point_homography)
constexpr int kNewtonIters = 5;

// LDS words of one minimal solve
constexpr int kA = 0;            // the R x 9 system, R <= 8
constexpr int kPiv = 72;         // pivot columns [0, R), then the free columns (9 - R)
constexpr int kBas = 81;         // null-space basis, (9 - R) x 9, R >= 7
constexpr int kWords = 99;

// ------------------------------------------------------------------------------------------------------------ conditioning
struct Norm { double cx, cy, s; };             // Hartley: x_n = s (x - c)

// from the sums of a set of n points: centroid = sum / n, s = sqrt(2) / sqrt(d2 / n), d2 = sum |x - c|^2
HD inline bool norm_scale(double d2, double n, Norm& t) {
    const double rms = sqrt(d2 / n);
    if (!(rms > 0.0) || !is_finite(rms)) return false;
    t.s = sqrt(2.0) / rms;
    return true;
}

template <int K>
HD inline bool hartley(const double (&x)[K][2], Norm& t) {
    double sx = 0.0, sy = 0.0;
#pragma unroll
    for (int i = 0; i < K; ++i) { sx += x[i][0]; sy += x[i][1]; }
    t.cx = sx / (double)K;
    t.cy = sy / (double)K;
    double d2 = 0.0;
#pragma unroll
    for (int i = 0; i < K; ++i) {
        const double dx = x[i][0] - t.cx, dy = x[i][1] - t.cy;
        d2 += dx * dx + dy * dy;
    }
    return norm_scale(d2, (double)K, t);
}

// m (row-major 3 x 3, between normalised points) T1, T = [s 0 -s cx; 0 s -s cy; 0 0 1]
HD inline void times_t1(const double (&m)[9], const Norm& t1, double (&g)[9]) {
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        g[3 * i] = m[3 * i] * t1.s;
        g[3 * i + 1] = m[3 * i + 1] * t1.s;
        g[3 * i + 2] = m[3 * i + 2] - t1.s * (m[3 * i] * t1.cx + m[3 * i + 1] * t1.cy);
    }
}

HD inline void denormalise_f(const double (&f)[9], const Norm& t1, const Norm& t2, double (&out)[9]) {      // T2^T F T1
    double g[9];
    times_t1(f, t1, g);
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        out[j] = t2.s * g[j];
        out[3 + j] = t2.s * g[3 + j];
        out[6 + j] = g[6 + j] - t2.s * (t2.cx * g[j] + t2.cy * g[3 + j]);
    }
}

HD inline void denormalise_h(const double (&h)[9], const Norm& t1, const Norm& t2, double (&out)[9]) {      // T2^-1 H T1
    double g[9];
    times_t1(h, t1, g);
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        out[j] = g[j] / t2.s + t2.cx * g[6 + j];
        out[3 + j] = g[3 + j] / t2.s + t2.cy * g[6 + j];
        out[6 + j] = g[6 + j];
    }
}

// ------------------------------------------------------------------------------------------------------------------ cubic
HD inline double det_rows(const double* r0, const double* r1, const double* r2) {
    return (r0[0] * (r1[1] * r2[2] - r1[2] * r2[1]) - r0[1] * (r1[0] * r2[2] - r1[2] * r2[0])) + r0[2] * (r1[0] * r2[1] - r1[1] * r2[0]);
}

// <= kNewtonIters Newton steps on c (ascending coefficients) that stay inside [lo, hi]
HD inline double cubic_polish(const double (&c)[4], double x, double lo, double hi) {
    for (int it = 0; it < kNewtonIters; ++it) {
        const double f = ((c[3] * x + c[2]) * x + c[1]) * x + c[0];
        const double df = (3.0 * c[3] * x + 2.0 * c[2]) * x + c[1];
        if (df == 0.0) break;
        const double xn = x - f / df;
        if (!(xn >= lo && xn <= hi) || xn == x) break;
        x = xn;
    }
    return x;
}

HD inline void sort2(double& a, double& b) {
    const double lo = a <= b ? a : b, hi = a <= b ? b : a;
    a = lo;
    b = hi;
}

// real roots, ascending, of c[0] + c[1] x + c[2] x^2 + c[3] x^3 by the closed form and the bracketed polish; count returned.
// c is divided by its largest |coefficient|; |c[3]| < 1e-14 then: a quadratic (|c[2]| < 1e-14 as well: linear)
HD inline int cubic_roots(double (&c)[4], double (&r)[3]) {
    double m = 0.0;
#pragma unroll
    for (int i = 0; i < 4; ++i) m = fmax(m, fabs(c[i]));
    if (!(m > 0.0) || !is_finite(m)) return 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        if (!is_finite(c[i])) return 0;
        c[i] = c[i] / m;
    }
    const double inf = HUGE_VAL;
    r[0] = r[1] = r[2] = 0.0;
    if (fabs(c[3]) < 1e-14) {
        c[3] = 0.0;
        if (fabs(c[2]) < 1e-14) {
            if (c[1] == 0.0) return 0;
            r[0] = -c[0] / c[1];
            return is_finite(r[0]) ? 1 : 0;
        }
        const double disc = c[1] * c[1] - 4.0 * c[2] * c[0];
        if (!(disc >= 0.0)) return 0;
        const double q = -0.5 * (c[1] + (c[1] >= 0.0 ? 1.0 : -1.0) * sqrt(disc));
        double x0 = q / c[2], x1 = q != 0.0 ? c[0] / q : x0;
        sort2(x0, x1);
        const double vertex = -c[1] / (2.0 * c[2]);
        r[0] = cubic_polish(c, x0, -inf, vertex);
        r[1] = cubic_polish(c, x1, vertex, inf);
        sort2(r[0], r[1]);
        return is_finite(r[0]) && is_finite(r[1]) ? 2 : 0;
    }
    const double a = c[2] / c[3], b = c[1] / c[3], d = c[0] / c[3];
    const double Q = (a * a - 3.0 * b) / 9.0;
    const double R = ((2.0 * a * a - 9.0 * b) * a + 27.0 * d) / 54.0;
    const double R2 = R * R, Q3 = Q * Q * Q, mid = -a / 3.0;
    if (R2 < Q3) {                                   // three real roots, one per monotone stretch of the cubic
        const double sq = sqrt(Q);
        const double th = acos(fmin(1.0, fmax(-1.0, R / sqrt(Q3))));
        const double kTwoPi = 6.283185307179586476925286766559;
        r[0] = cubic_polish(c, -2.0 * sq * cos(th / 3.0) + mid, -inf, mid - sq);
        r[1] = cubic_polish(c, -2.0 * sq * cos((th - kTwoPi) / 3.0) + mid, mid - sq, mid + sq);
        r[2] = cubic_polish(c, -2.0 * sq * cos((th + kTwoPi) / 3.0) + mid, mid + sq, inf);
        sort2(r[0], r[1]);
        sort2(r[1], r[2]);
        sort2(r[0], r[1]);
        return is_finite(r[0]) && is_finite(r[1]) && is_finite(r[2]) ? 3 : 0;
    }
    const double A = -(R >= 0.0 ? 1.0 : -1.0) * cbrt(fabs(R) + sqrt(R2 - Q3));
    const double B = A != 0.0 ? Q / A : 0.0;
    const double x = (A + B) + mid;
    double lo = -inf, hi = inf;
    if (Q > 0.0) {                                   // outside the two turning points, on the estimate's side
        const double sq = sqrt(Q);
        if (x < mid) hi = mid - sq; else lo = mid + sq;
    }
    r[0] = cubic_polish(c, x, lo, hi);
    return is_finite(r[0]) ? 1 : 0;
}

// --------------------------------------------------------------------------------------------------------- minimal solvers
// emit(slot, const double M[9]) per kept solution; returns the number emitted
template <int S, class Emit>
HD inline int seven_point(const double (&p1)[7][2], const double (&p2)[7][2], Col<S> w, Emit emit) {
    Norm t1, t2;
    if (!hartley<7>(p1, t1) || !hartley<7>(p2, t2)) return 0;
#pragma unroll
    for (int r = 0; r < 7; ++r) {
        const double a[3] = {(p1[r][0] - t1.cx) * t1.s, (p1[r][1] - t1.cy) * t1.s, 1.0};
        const double b[3] = {(p2[r][0] - t2.cx) * t2.s, (p2[r][1] - t2.cy) * t2.s, 1.0};
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) w[kA + 9 * r + 3 * i + j] = b[i] * a[j];
    }
    if (!gj_nullspace<7, kA, kPiv, kBas>(w)) return 0;
    double F1[9], F2[9], D[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) { F1[k] = w[kBas + k]; F2[k] = w[kBas + 9 + k]; }
    // modified Gram-Schmidt, F1 then F2 (ls2fm_five_point's): the raw Gauss-Jordan pencil loses digits of the cubic
    double n1 = 0.0, dot = 0.0, n2 = 0.0;
#pragma unroll
    for (int k = 0; k < 9; ++k) n1 += F1[k] * F1[k];
    if (!(n1 > 0.0) || !is_finite(n1)) return 0;
    const double i1 = 1.0 / sqrt(n1);
#pragma unroll
    for (int k = 0; k < 9; ++k) { F1[k] = F1[k] * i1; dot += F1[k] * F2[k]; }
#pragma unroll
    for (int k = 0; k < 9; ++k) { F2[k] -= dot * F1[k]; n2 += F2[k] * F2[k]; }
    if (!(n2 > 0.0) || !is_finite(n2)) return 0;
    const double i2 = 1.0 / sqrt(n2);
#pragma unroll
    for (int k = 0; k < 9; ++k) { F2[k] = F2[k] * i2; D[k] = F1[k] - F2[k]; }
    // det(F2 + l D), multilinear in the rows
    double c[4];
    c[0] = det_rows(F2, F2 + 3, F2 + 6);
    c[1] = (det_rows(D, F2 + 3, F2 + 6) + det_rows(F2, D + 3, F2 + 6)) + det_rows(F2, F2 + 3, D + 6);
    c[2] = (det_rows(D, D + 3, F2 + 6) + det_rows(D, F2 + 3, D + 6)) + det_rows(F2, D + 3, D + 6);
    c[3] = det_rows(D, D + 3, D + 6);
    double roots[3];
    const int nr = cubic_roots(c, roots);
    int n = 0;
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        if (q >= nr) continue;
        const double l = roots[q];
        double f[9], out[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) f[k] = l * F1[k] + (1.0 - l) * F2[k];
        denormalise_f(f, t1, t2, out);
        if (!canonical9(out)) continue;
        emit(n, out);
        ++n;
    }
    return n;
}

template <int S, class Emit>
HD inline int four_point(const double (&p1)[4][2], const double (&p2)[4][2], Col<S> w, Emit emit) {
    Norm t1, t2;
    if (!hartley<4>(p1, t1) || !hartley<4>(p2, t2)) return 0;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const double x = (p1[r][0] - t1.cx) * t1.s, y = (p1[r][1] - t1.cy) * t1.s;
        const double u = (p2[r][0] - t2.cx) * t2.s, v = (p2[r][1] - t2.cy) * t2.s;
        const double ra[9] = {-x, -y, -1.0, 0.0, 0.0, 0.0, u * x, u * y, u};
        const double rb[9] = {0.0, 0.0, 0.0, -x, -y, -1.0, v * x, v * y, v};
#pragma unroll
        for (int k = 0; k < 9; ++k) { w[kA + 18 * r + k] = ra[k]; w[kA + 18 * r + 9 + k] = rb[k]; }
    }
    if (!gj_nullspace<8, kA, kPiv, kBas>(w)) return 0;
    double h[9], out[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) h[k] = w[kBas + k];
    denormalise_h(h, t1, t2, out);
    if (!canonical9(out)) return 0;
    emit(0, out);
    return 1;
}

// ------------------------------------------------------------------------------------------------------ local optimisation
// the fundamental matrix of the normal matrix's smallest eigenvector v (between normalised points): its smallest singular value
// zeroed, de-normalised
__device__ inline void f_from_vector(const double (&v)[9], const Norm& t1, const Norm& t2, double (&out)[9]) {
    double a[3][3], V[3][3];          // a[c]: column c of F V ; V[c]: column c of V
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int r = 0; r < 3; ++r) { a[c][r] = v[3 * r + c]; V[c][r] = c == r ? 1.0 : 0.0; }
    onesided_jacobi3(a, V);
    double nr[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) nr[c] = (a[c][0] * a[c][0] + a[c][1] * a[c][1]) + a[c][2] * a[c][2];
    const int lo = (nr[0] <= nr[1] && nr[0] <= nr[2]) ? 0 : (nr[1] <= nr[2] ? 1 : 2);      // the lower index among equals
    double f[9];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            double s = 0.0;
#pragma unroll
            for (int c = 0; c < 3; ++c) s += c == lo ? 0.0 : a[c][r] * V[c][j];
            f[3 * r + j] = s;
        }
    denormalise_f(f, t1, t2, out);
}

// ----------------------------------------------------------------------------------------------------------------- models
struct TvInput { const double* uv0; const double* uv1; double err_px; };
struct TvCtx { double thr2; };
struct TvLds { double vec[9]; double cand[1][9]; int ok; };

template <class M>
struct TvBase {                  // what the two models share: pixels in, the squared threshold, the re-fit but for its rows
    static constexpr int kHypWords = 9, kHypThreads = kMsThreads, kHypLdsWords = kWords, kMaxCand = 1;
    using Input = TvInput;
    using Ctx = TvCtx;
    using Point = two_view::Point;
    using Lds = TvLds;
    using Tail = NoTail;
    static __device__ __forceinline__ Ctx context(const Input& in, int) { return {in.err_px * in.err_px}; }
    static __device__ __forceinline__ Point load(const Input& in, const Ctx&, int64_t i) {
        return {in.uv0[2 * i], in.uv0[2 * i + 1], in.uv1[2 * i], in.uv1[2 * i + 1]};
    }
    static __device__ __forceinline__ bool inlier(const double* X, const Point& pt, const Ctx& c) {
        return M::test(X, pt.x1, pt.y1, pt.x2, pt.y2, c.thr2);
    }
    template <int K, class Emit>
    static __device__ __forceinline__ void hypotheses(const Input& in, const Ctx& c, int64_t s0, const int64_t (&id)[K], double* column,
                                                      Emit emit) {
        sampled_solve<M>(in, c, s0, id, column, emit);
    }
    static __device__ __forceinline__ bool keeps(bool, int cur) { return cur >= M::kMinInliers; }
    // the Hartley-normalised DLT of X's inliers: the model of the normal matrix's smallest eigenvector, de-normalised, unit norm,
    // sign fixed; no candidate when the inliers coincide or the model is not finite
    static __device__ __forceinline__ int refit(const Input& in, const Ctx& ctx, int64_t s0, int64_t n, const double* X, int cur, Lds& lds,
                                       double* s_red) {
        const double thr2 = ctx.thr2;
        // per image: centroids, then the squared distances
        double sm[4] = {0.0, 0.0, 0.0, 0.0};
        for_each_corr<M>(in, ctx, s0, n, [&](int64_t, double x1, double y1, double x2, double y2) {
            if (!M::test(X, x1, y1, x2, y2, thr2)) return;
            sm[0] += x1; sm[1] += y1; sm[2] += x2; sm[3] += y2;
        });
        block_sum<4, kPairThreads>(sm, s_red);
        Norm t1, t2;
        t1.cx = sm[0] / (double)cur; t1.cy = sm[1] / (double)cur;
        t2.cx = sm[2] / (double)cur; t2.cy = sm[3] / (double)cur;
        double d2[2] = {0.0, 0.0};
        for_each_corr<M>(in, ctx, s0, n, [&](int64_t, double x1, double y1, double x2, double y2) {
            if (!M::test(X, x1, y1, x2, y2, thr2)) return;
            const double ax = x1 - t1.cx, ay = y1 - t1.cy, bx = x2 - t2.cx, by = y2 - t2.cy;
            d2[0] += ax * ax + ay * ay;
            d2[1] += bx * bx + by * by;
        });
        block_sum<2, kPairThreads>(d2, s_red);
        if (!norm_scale(d2[0], (double)cur, t1) || !norm_scale(d2[1], (double)cur, t2)) return 0;
        double a[kNe];
#pragma unroll
        for (int q = 0; q < kNe; ++q) a[q] = 0.0;
        for_each_corr<M>(in, ctx, s0, n, [&](int64_t, double x1, double y1, double x2, double y2) {
            if (!M::test(X, x1, y1, x2, y2, thr2)) return;
            M::accumulate(a, (x1 - t1.cx) * t1.s, (y1 - t1.cy) * t1.s, (x2 - t2.cx) * t2.s, (y2 - t2.cy) * t2.s);
        });
        smallest_eigenvectors<1>(a, s_red, lds.vec);
        if (threadIdx.x == 0) {
            double v[9], out[9];
#pragma unroll
            for (int q = 0; q < 9; ++q) v[q] = lds.vec[q];
            M::from_vector(v, t1, t2, out);
            lds.ok = canonical9(out) ? 1 : 0;
#pragma unroll
            for (int q = 0; q < 9; ++q) lds.cand[0][q] = out[q];
        }
        __syncthreads();
        return lds.ok;
    }
};

struct FModel : TvBase<FModel>, Epipolar {     // fundamental matrices scored by the squared Sampson error in pixels
    static constexpr int kSample = 7, kMaxSol = LS2FM_SEVEN_POINT_MAX_SOLUTIONS, kMinGroup = 7, kMinInliers = 8;
    template <int S, class Emit>
    static HD inline int solve(const double (&p1)[7][2], const double (&p2)[7][2], Col<S> w, Emit emit) {
        return seven_point(p1, p2, w, emit);
    }
    static __device__ inline void from_vector(const double (&v)[9], const Norm& t1, const Norm& t2, double (&out)[9]) {
        f_from_vector(v, t1, t2, out);
    }
};

struct HModel : TvBase<HModel> {     // homographies scored by the squared forward transfer error in pixels
    static constexpr int kSample = 4, kMaxSol = 1, kMinGroup = 4, kMinInliers = 4;
    static HD inline bool test(const double* H, double x1, double y1, double x2, double y2, double thr2) {
        const double w3 = (H[6] * x1 + H[7] * y1) + H[8];
        if (!(fabs(w3) > DBL_EPSILON) || !is_finite(w3)) return false;
        const double dx = ((H[0] * x1 + H[1] * y1) + H[2]) / w3 - x2;
        const double dy = ((H[3] * x1 + H[4] * y1) + H[5]) / w3 - y2;
        return dx * dx + dy * dy <= thr2;
    }
    template <int S, class Emit>
    static HD inline int solve(const double (&p1)[4][2], const double (&p2)[4][2], Col<S> w, Emit emit) {
        return four_point(p1, p2, w, emit);
    }
    static __device__ __forceinline__ void accumulate(double (&a)[kNe], double x, double y, double u, double v) {      // the two DLT rows
        const double ra[9] = {-x, -y, -1.0, 0.0, 0.0, 0.0, u * x, u * y, u};
        const double rb[9] = {0.0, 0.0, 0.0, -x, -y, -1.0, v * x, v * y, v};
#pragma unroll
        for (int i = 0; i < 9; ++i)
#pragma unroll
            for (int k = i; k < 9; ++k) a[sidx(i, k)] += ra[i] * ra[k] + rb[i] * rb[k];
    }
    static __device__ inline void from_vector(const double (&v)[9], const Norm& t1, const Norm& t2, double (&out)[9]) {
        denormalise_h(v, t1, t2, out);
    }
};

// ls2fm_fundamental_matrix, ls2fm_homography
template <class M>
int ransac_call(const double* uv0, const double* uv1, const int32_t* pair_start, int32_t n_pairs, const ls2fm_pose_ransac_opts* opts,
                double* model, uint8_t* inliers, int32_t* num_inliers, int32_t* trials, int32_t* best_trial, int32_t* success,
                void* workspace, void* stream) {
    LS2FM_CHECK_ARG(n_pairs >= 1 && n_pairs <= LS2FM_RELPOSE_MAX_PAIRS && pair_start && opts_ok(opts) && opts->refine == 0);
    LS2FM_CHECK_ARG(model && num_inliers && trials && best_trial && success);
    return estimate<M>({uv0, uv1, opts->max_error_px}, pair_start, n_pairs, uv0 && uv1 && inliers, opts, model, nullptr, inliers,
                       num_inliers, trials, best_trial, success, workspace, stream);
}

}  // namespace

extern "C" int ls2fm_seven_point(const double* uv0, const double* uv1, int64_t m, double* F, int32_t* n_solutions, void* stream) {
    return minimal_call<FModel>(uv0, uv1, m, F, n_solutions, stream);
}

extern "C" int ls2fm_four_point_homography(const double* uv0, const double* uv1, int64_t m, double* H, int32_t* n_solutions,
                                           void* stream) {
    return minimal_call<HModel>(uv0, uv1, m, H, n_solutions, stream);
}

extern "C" int64_t ls2fm_fundamental_matrix_workspace_bytes(int32_t n_pairs, int64_t n_corr) {
    return workspace_bytes<FModel>(n_pairs, n_corr);
}

extern "C" int64_t ls2fm_homography_workspace_bytes(int32_t n_pairs, int64_t n_corr) { return workspace_bytes<HModel>(n_pairs, n_corr); }

extern "C" int ls2fm_fundamental_matrix(const double* uv0, const double* uv1, const int32_t* pair_start, int32_t n_pairs,
                                        const ls2fm_pose_ransac_opts* opts, double* F, uint8_t* inliers, int32_t* num_inliers,
                                        int32_t* trials, int32_t* best_trial, int32_t* success, void* workspace, void* stream) {
    return ransac_call<FModel>(uv0, uv1, pair_start, n_pairs, opts, F, inliers, num_inliers, trials, best_trial, success, workspace,
                               stream);
}

extern "C" int ls2fm_homography(const double* uv0, const double* uv1, const int32_t* pair_start, int32_t n_pairs,
                                const ls2fm_pose_ransac_opts* opts, double* H, uint8_t* inliers, int32_t* num_inliers, int32_t* trials,
                                int32_t* best_trial, int32_t* success, void* workspace, void* stream) {
    return ransac_call<HModel>(uv0, uv1, pair_start, n_pairs, opts, H, inliers, num_inliers, trials, best_trial, success, workspace,
                               stream);
}
