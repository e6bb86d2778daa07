// Uncalibrated two-view geometry of many view pairs in one call: LO-RANSAC over the seven-point fundamental matrix and over the
// four-point homography, in pixels, all geometry in fp64 -- the F and H of COLMAP's two-view geometry, whose inlier counts (with
// ls2fm_relative_pose's E) give the CALIBRATED / UNCALIBRATED / PLANAR_OR_PANORAMIC / DEGENERATE verdict of ls2fm.pose.
// include/ls2fm.h states the rules; tests/twoview_restate.py repeats them in numpy.  Correspondences are SORTED BY PAIR.
//
// The rounds (scoring, selection, the stopping rule) are csrc/ransac.h's, run on the models FModel (squared Sampson error) and
// HModel (squared forward transfer error) with this file's tv_hyp_kernel: one thread per (pair, trial), the minimal solver on
// kSample distinct correspondences.  Then tv_final_kernel: local optimisation (Hartley-normalised DLT on the inlier set through
// the 9 x 9 normal matrix's smallest eigenvector) and the final mask, one workgroup per pair with fixed-order reductions: every
// bit is a function of the pair's own data, seed and options.
//
// A minimal solve's run-time-indexed state (the R x 9 system, the pivot columns, the null-space basis: kWords fp64 words) is a
// column of LDS, word k of thread j at s_buf[k * kMsThreads + j], as in relative_pose.hip: no kernel of this file indexes a
// private array at run time.  64 threads per workgroup: kWords x 64 x 8 B = 50 KB.
#include "pose_math.h"
#include "ransac.h"

#include <cfloat>
#include <cmath>

namespace {

using namespace ransac;
using namespace pose_math;

constexpr int kMsThreads = 64;                 // minimal-solver workgroups (hypotheses, ls2fm_seven_point, ls2fm_four_point_homography)
constexpr int kPairThreads = 256;              // final workgroups
constexpr int kLoIters = 10;
constexpr int kNewtonIters = 5;

// LDS words of one minimal solve
constexpr int kA = 0;            // the R x 9 system, R <= 8
constexpr int kPiv = 72;         // pivot columns [0, R), then the free columns (9 - R)
constexpr int kBas = 81;         // null-space basis, (9 - R) x 9, R >= 7
constexpr int kWords = 99;

static_assert(kRound % kMsThreads == 0, "round shape");

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

// -------------------------------------------------------------------------------------------------------------- null space
// the (9 - R)-dimensional null space of the R x 9 system at kA: Gauss-Jordan with partial pivoting (ls2fm_five_point's rule: a
// column whose largest remaining |entry| is <= 1e-12 of the matrix's largest is free) -> basis vector j (free column f_j,
// ascending) at kBas + 9 j: 1 at f_j, -R[i][f_j] at pivot column i.  false: rank != R
template <int R, int S>
HD inline bool gj_nullspace(Col<S> w) {
    double amax = 0.0;
    for (int i = 0; i < 9 * R; ++i) amax = fmax(amax, fabs(w[kA + i]));
    if (!(amax > 0.0) || !is_finite(amax)) return false;
    int rank = 0, nfree = 0;
    for (int c = 0; c < 9; ++c) {
        int p = -1;
        double best = 0.0;
        for (int r = rank; r < R; ++r) {
            const double v = fabs(w[kA + 9 * r + c]);
            if (p < 0 || v > best) { best = v; p = r; }
        }
        if (rank == R || !(best > 1e-12 * amax)) {
            if (nfree == 9 - R) return false;          // one free column too many: the rank cannot reach R
            w[kPiv + R + nfree] = c;
            ++nfree;
            continue;
        }
        for (int k = 0; k < 9; ++k) {
            const double t = w[kA + 9 * rank + k];
            w[kA + 9 * rank + k] = w[kA + 9 * p + k];
            w[kA + 9 * p + k] = t;
        }
        const double inv = 1.0 / w[kA + 9 * rank + c];
        for (int k = 0; k < 9; ++k) w[kA + 9 * rank + k] = w[kA + 9 * rank + k] * inv;
        for (int r = 0; r < R; ++r) {
            if (r == rank) continue;
            const double f = w[kA + 9 * r + c];
            for (int k = 0; k < 9; ++k) w[kA + 9 * r + k] -= f * w[kA + 9 * rank + k];
        }
        w[kPiv + rank] = c;
        ++rank;
    }
    if (rank != R || nfree != 9 - R) return false;
    for (int j = 0; j < 9 - R; ++j) {
        const int f = (int)w[kPiv + R + j];
        for (int k = 0; k < 9; ++k) w[kBas + 9 * j + k] = k == f ? 1.0 : 0.0;
        for (int i = 0; i < R; ++i) w[kBas + 9 * j + (int)w[kPiv + i]] = -w[kA + 9 * i + f];
    }
    return true;
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
    if (!gj_nullspace<7>(w)) return 0;
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
    if (!gj_nullspace<8>(w)) return 0;
    double h[9], out[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) h[k] = w[kBas + k];
    denormalise_h(h, t1, t2, out);
    if (!canonical9(out)) return 0;
    emit(0, out);
    return 1;
}

// ----------------------------------------------------------------------------------------------------------------- models
struct TvInput { const double* uv0; const double* uv1; double err_px; };
struct TvCtx { double thr2; };
struct TvPoint { double x1, y1, x2, y2; };

struct TvBase {                  // what the two models of ransac.h share: pixels in, the squared threshold
    static constexpr int kHypWords = 9;
    using Input = TvInput;
    using Ctx = TvCtx;
    using Point = TvPoint;
    static __device__ __forceinline__ Ctx context(const Input& in, int) { return {in.err_px * in.err_px}; }
    static __device__ __forceinline__ Point load(const Input& in, const Ctx&, int64_t i) {
        return {in.uv0[2 * i], in.uv0[2 * i + 1], in.uv1[2 * i], in.uv1[2 * i + 1]};
    }
};

struct FModel : TvBase {         // fundamental matrices scored by the squared Sampson error in pixels
    static constexpr int kSample = 7, kMaxSol = LS2FM_SEVEN_POINT_MAX_SOLUTIONS, kMinGroup = 7, kMinInliers = 8;
    static constexpr bool kIsF = true;
    static HD inline bool test(const double* F, double x1, double y1, double x2, double y2, double thr2) {
        return sampson2(F, x1, y1, x2, y2) <= thr2;       // NaN (0 / 0) is not an inlier
    }
    static __device__ __forceinline__ bool inlier(const double* F, const Point& pt, const Ctx& c) {
        return test(F, pt.x1, pt.y1, pt.x2, pt.y2, c.thr2);
    }
    template <int S, class Emit>
    static HD inline int solve(const double (&p1)[7][2], const double (&p2)[7][2], Col<S> w, Emit emit) {
        return seven_point(p1, p2, w, emit);
    }
};

struct HModel : TvBase {         // homographies scored by the squared forward transfer error in pixels
    static constexpr int kSample = 4, kMaxSol = 1, kMinGroup = 4, kMinInliers = 4;
    static constexpr bool kIsF = false;
    static HD inline bool test(const double* H, double x1, double y1, double x2, double y2, double thr2) {
        const double w3 = (H[6] * x1 + H[7] * y1) + H[8];
        if (!(fabs(w3) > DBL_EPSILON) || !is_finite(w3)) return false;
        const double dx = ((H[0] * x1 + H[1] * y1) + H[2]) / w3 - x2;
        const double dy = ((H[3] * x1 + H[4] * y1) + H[5]) / w3 - y2;
        return dx * dx + dy * dy <= thr2;
    }
    static __device__ __forceinline__ bool inlier(const double* H, const Point& pt, const Ctx& c) {
        return test(H, pt.x1, pt.y1, pt.x2, pt.y2, c.thr2);
    }
    template <int S, class Emit>
    static HD inline int solve(const double (&p1)[4][2], const double (&p2)[4][2], Col<S> w, Emit emit) {
        return four_point(p1, p2, w, emit);
    }
};

// ---------------------------------------------------------------------------------------------------------------- kernels
template <class M>
__global__ void __launch_bounds__(kMsThreads)
tv_minimal_kernel(const double* __restrict__ uv0, const double* __restrict__ uv1, int64_t m, double* __restrict__ Mout,
                  int32_t* __restrict__ n_sol) {
    __shared__ double s_buf[kWords * kMsThreads];
    const int64_t i = (int64_t)blockIdx.x * kMsThreads + threadIdx.x;
    if (i >= m) return;
    constexpr int kK = M::kSample, kS = M::kMaxSol;
    double a[kK][2], b[kK][2];
#pragma unroll
    for (int s = 0; s < kK; ++s) {
        a[s][0] = uv0[2 * kK * i + 2 * s]; a[s][1] = uv0[2 * kK * i + 2 * s + 1];
        b[s][0] = uv1[2 * kK * i + 2 * s]; b[s][1] = uv1[2 * kK * i + 2 * s + 1];
    }
    double* __restrict__ out = Mout + 9 * kS * i;
    const int n = M::solve(a, b, Col<kMsThreads>{s_buf + threadIdx.x}, [&](int s, const double* e) {
        for (int q = 0; q < 9; ++q) out[9 * s + q] = e[q];
    });
    for (int q = 9 * n; q < 9 * kS; ++q) out[q] = 0.0;
    n_sol[i] = n;
}

template <class M>
__global__ void __launch_bounds__(kMsThreads)
tv_hyp_kernel(const double* __restrict__ uv0, const double* __restrict__ uv1, const int32_t* __restrict__ ps, uint64_t seed, Ws w) {
    const int p = blockIdx.y;
    if (!w.active[p]) return;
    __shared__ double s_buf[kWords * kMsThreads];
    constexpr int kK = M::kSample, kS = M::kMaxSol;
    const int tl = blockIdx.x * kMsThreads + threadIdx.x;
    const int64_t slot = (int64_t)p * kRound + tl;
    int32_t* __restrict__ cnt = w.counts + kS * slot;
    for (int s = 0; s < kS; ++s) cnt[s] = 0;
    const int64_t s0 = ps[p], n = ps[p + 1] - s0;
    const uint64_t t = (uint64_t)(w.trials[p] + tl);
    int64_t id[kK];
    int mask = 0;
    if (sample_distinct(trial_key(seed, t), n, id)) {
        double a[kK][2], b[kK][2];
#pragma unroll
        for (int s = 0; s < kK; ++s) {
            a[s][0] = uv0[2 * (s0 + id[s])]; a[s][1] = uv0[2 * (s0 + id[s]) + 1];
            b[s][0] = uv1[2 * (s0 + id[s])]; b[s][1] = uv1[2 * (s0 + id[s]) + 1];
        }
        double* __restrict__ out = w.hyp + kS * 9 * slot;
        M::solve(a, b, Col<kMsThreads>{s_buf + threadIdx.x}, [&](int s, const double* e) {
            for (int q = 0; q < 9; ++q) out[9 * s + q] = e[q];
            mask |= 1 << s;
        });
    }
    w.valid[slot] = mask;
}

// ------------------------------------------------------------------------------------------------------ local optimisation
constexpr int kNe = 45;

// the model of the normal matrix's smallest eigenvector v (between normalised points): F with its smallest singular value
// zeroed, H as it is; de-normalised, unit norm, sign fixed.  false when not finite
template <class M>
__device__ inline bool model_from_vector(const double (&v)[9], const Norm& t1, const Norm& t2, double (&out)[9]) {
    if constexpr (M::kIsF) {
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
    } else {
        denormalise_h(v, t1, t2, out);
    }
    return canonical9(out);
}

template <class M>
__global__ void __launch_bounds__(kPairThreads)
tv_final_kernel(const double* __restrict__ uv0, const double* __restrict__ uv1, const int32_t* __restrict__ ps, double err_px, Ws w,
                double* __restrict__ Mout, uint8_t* __restrict__ inliers, int32_t* __restrict__ num_inliers,
                int32_t* __restrict__ trials, int32_t* __restrict__ best_trial, int32_t* __restrict__ success) {
    __shared__ double s_red[(kPairThreads / 64) * kNe];
    __shared__ double s_vec[9];
    __shared__ double s_cand[9];
    __shared__ int s_ok, s_int;
    const int p = blockIdx.x, tid = threadIdx.x;
    const int64_t s0 = ps[p], n = ps[p + 1] - s0;
    const double thr2 = err_px * err_px;
    const unsigned long long bk = w.best_key[p];
    int cur = 0;
    double X[9];
#pragma unroll
    for (int q = 0; q < 9; ++q) X[q] = 0.0;
    if (bk != 0ull) {
#pragma unroll
        for (int q = 0; q < 9; ++q) X[q] = w.best[9 * p + q];
        for (int64_t j = tid; j < n; j += kPairThreads)
            cur += M::test(X, uv0[2 * (s0 + j)], uv0[2 * (s0 + j) + 1], uv1[2 * (s0 + j)], uv1[2 * (s0 + j) + 1], thr2) ? 1 : 0;
        cur = block_count(cur, &s_int);
    }
    // every condition below is uniform over the workgroup: it comes from a block-wide sum or from LDS
    for (int it = 0; it < kLoIters && cur >= M::kMinInliers; ++it) {
        // Hartley normalisation of the inlier set, per image: centroids, then the squared distances
        double sm[4] = {0.0, 0.0, 0.0, 0.0};
        for (int64_t j = tid; j < n; j += kPairThreads) {
            const double x1 = uv0[2 * (s0 + j)], y1 = uv0[2 * (s0 + j) + 1], x2 = uv1[2 * (s0 + j)], y2 = uv1[2 * (s0 + j) + 1];
            if (!M::test(X, x1, y1, x2, y2, thr2)) continue;
            sm[0] += x1; sm[1] += y1; sm[2] += x2; sm[3] += y2;
        }
        block_sum<4, kPairThreads>(sm, s_red);
        Norm t1, t2;
        t1.cx = sm[0] / (double)cur; t1.cy = sm[1] / (double)cur;
        t2.cx = sm[2] / (double)cur; t2.cy = sm[3] / (double)cur;
        double d2[2] = {0.0, 0.0};
        for (int64_t j = tid; j < n; j += kPairThreads) {
            const double x1 = uv0[2 * (s0 + j)], y1 = uv0[2 * (s0 + j) + 1], x2 = uv1[2 * (s0 + j)], y2 = uv1[2 * (s0 + j) + 1];
            if (!M::test(X, x1, y1, x2, y2, thr2)) continue;
            const double ax = x1 - t1.cx, ay = y1 - t1.cy, bx = x2 - t2.cx, by = y2 - t2.cy;
            d2[0] += ax * ax + ay * ay;
            d2[1] += bx * bx + by * by;
        }
        block_sum<2, kPairThreads>(d2, s_red);
        if (!norm_scale(d2[0], (double)cur, t1) || !norm_scale(d2[1], (double)cur, t2)) break;
        // normal matrix of the inliers' normalised rows, upper triangle, fixed-order sum
        double a[kNe];
#pragma unroll
        for (int q = 0; q < kNe; ++q) a[q] = 0.0;
        for (int64_t j = tid; j < n; j += kPairThreads) {
            const double x1 = uv0[2 * (s0 + j)], y1 = uv0[2 * (s0 + j) + 1], x2 = uv1[2 * (s0 + j)], y2 = uv1[2 * (s0 + j) + 1];
            if (!M::test(X, x1, y1, x2, y2, thr2)) continue;
            const double x = (x1 - t1.cx) * t1.s, y = (y1 - t1.cy) * t1.s, u = (x2 - t2.cx) * t2.s, v = (y2 - t2.cy) * t2.s;
            if constexpr (M::kIsF) {
                const double r[9] = {u * x, u * y, u, v * x, v * y, v, x, y, 1.0};
#pragma unroll
                for (int i = 0; i < 9; ++i)
#pragma unroll
                    for (int k = i; k < 9; ++k) a[sidx(i, k)] += r[i] * r[k];
            } else {
                const double ra[9] = {-x, -y, -1.0, 0.0, 0.0, 0.0, u * x, u * y, u};
                const double rb[9] = {0.0, 0.0, 0.0, -x, -y, -1.0, v * x, v * y, v};
#pragma unroll
                for (int i = 0; i < 9; ++i)
#pragma unroll
                    for (int k = i; k < 9; ++k) a[sidx(i, k)] += ra[i] * ra[k] + rb[i] * rb[k];
            }
        }
        block_sum<kNe, kPairThreads>(a, s_red);
        {
            double v[9];
            jacobi9(a, tid < 9 ? tid : 0, v);
            if (tid < 9) {
                double x = 0.0;
#pragma unroll
                for (int k = 0; k < 9; ++k) x = eigen_rank9(a, k) == 0 ? v[k] : x;
                s_vec[tid] = x;
            }
        }
        __syncthreads();
        if (tid == 0) {
            double v[9], out[9];
#pragma unroll
            for (int q = 0; q < 9; ++q) v[q] = s_vec[q];
            const bool ok = model_from_vector<M>(v, t1, t2, out);
#pragma unroll
            for (int q = 0; q < 9; ++q) s_cand[q] = out[q];
            s_ok = ok ? 1 : 0;
        }
        __syncthreads();
        if (!s_ok) break;
        int c = 0, chg = 0;
        for (int64_t j = tid; j < n; j += kPairThreads) {
            const double x1 = uv0[2 * (s0 + j)], y1 = uv0[2 * (s0 + j) + 1], x2 = uv1[2 * (s0 + j)], y2 = uv1[2 * (s0 + j) + 1];
            const bool in = M::test(s_cand, x1, y1, x2, y2, thr2);
            c += in ? 1 : 0;
            chg += in != M::test(X, x1, y1, x2, y2, thr2) ? 1 : 0;
        }
        c = block_count(c, &s_int);
        chg = block_count(chg, &s_int);
        if (c < cur) break;
#pragma unroll
        for (int q = 0; q < 9; ++q) X[q] = s_cand[q];
        cur = c;
        if (chg == 0) break;
    }
    const bool ok = cur >= M::kMinInliers;
    for (int64_t j = tid; j < n; j += kPairThreads)
        inliers[s0 + j] =
            ok && M::test(X, uv0[2 * (s0 + j)], uv0[2 * (s0 + j) + 1], uv1[2 * (s0 + j)], uv1[2 * (s0 + j) + 1], thr2) ? 1 : 0;
    if (tid < 9) Mout[9 * p + tid] = ok ? X[tid] : 0.0;
    if (tid == 0) {
        num_inliers[p] = ok ? cur : 0;
        trials[p] = w.trials[p];
        best_trial[p] = bk != 0ull ? best_trial_of<M>(bk) : -1;
        success[p] = ok ? 1 : 0;
    }
}

// ------------------------------------------------------------------------------------------------------------------- host
template <class M>
int minimal_call(const double* uv0, const double* uv1, int64_t m, double* out, int32_t* n_solutions, void* stream) {
    LS2FM_CHECK_ARG(m >= 0);
    if (m == 0) return LS2FM_OK;
    LS2FM_CHECK_ARG(uv0 && uv1 && out && n_solutions);
    tv_minimal_kernel<M><<<(unsigned)((m + kMsThreads - 1) / kMsThreads), kMsThreads, 0, (hipStream_t)stream>>>(uv0, uv1, m, out,
                                                                                                                n_solutions);
    return ls2fm_launch_status();
}

template <class M>
int ransac_call(const double* uv0, const double* uv1, const int32_t* pair_start, int32_t n_pairs, const ls2fm_pose_ransac_opts* opts,
                double* model, uint8_t* inliers, int32_t* num_inliers, int32_t* trials, int32_t* best_trial, int32_t* success,
                void* workspace, void* stream) {
    LS2FM_CHECK_ARG(n_pairs >= 1 && n_pairs <= LS2FM_RELPOSE_MAX_PAIRS && pair_start && opts_ok(opts) && opts->refine == 0);
    LS2FM_CHECK_ARG(model && num_inliers && trials && best_trial && success);
    if (!workspace) return LS2FM_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    Ws w;
    const int st = run_rounds<M>({uv0, uv1, opts->max_error_px}, pair_start, n_pairs, uv0 && uv1 && inliers, opts, workspace, s, &w,
                                 [&](const Ws& ws) {
        tv_hyp_kernel<M><<<dim3(kRound / kMsThreads, (unsigned)n_pairs), kMsThreads, 0, s>>>(uv0, uv1, pair_start, opts->seed, ws);
    });
    if (st != LS2FM_OK) return st;
    tv_final_kernel<M><<<(unsigned)n_pairs, kPairThreads, 0, s>>>(uv0, uv1, pair_start, opts->max_error_px, w, model, inliers,
                                                                  num_inliers, trials, best_trial, success);
    return ls2fm_launch_status();
}

template <class M>
int64_t workspace_bytes(int32_t n_pairs, int64_t n_corr) {
    if (n_pairs < 1 || n_pairs > LS2FM_RELPOSE_MAX_PAIRS || n_corr < 0) return LS2FM_ERR_INVALID_ARGUMENT;
    return (int64_t)ws_layout<M>(n_pairs, nullptr, nullptr);
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
