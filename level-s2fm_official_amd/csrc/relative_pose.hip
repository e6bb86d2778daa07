// Relative pose of many view pairs in one call: LO-RANSAC over Nister's five-point algorithm, pose recovery by cheirality, and a
// batched two-view DLT -- what Initializer asks of pycolmap (essential_matrix_estimation, pipelines/Initialization.py:86-95) and
// the _Trad drivers of cv2 (triangulatePoints), all geometry in fp64.  include/ls2fm.h states the rules; tests/relpose_restate.py
// repeats them in numpy.  Correspondences are SORTED BY PAIR (pair p owns [pair_start[p], pair_start[p + 1])).
//
// E is the third two-view model beside two_view.hip's F and H (csrc/two_view.h): its correspondences are normalised by K as they
// are loaded, its rows are F's epipolar rows, its re-fit returns up to 10 candidates, and it has a pose-recovery tail.  The rounds
// (hypotheses, scoring, selection, the stopping rule) are csrc/ransac.h's, run on the model EModel below (squared Sampson error):
// one thread per (pair, trial), five-point on five distinct correspondences, <= 10 E.  Then two_view.h's final_kernel: local
// optimisation (five-point on the inlier set's normal matrix), the final mask and the pose recovery, one workgroup per pair with
// fixed-order reductions: every bit is a function of the pair's own data, seed and options.
//
// The five-point solver's per-problem state (null-space basis 36, quadratic terms 70, the 10 x 20 cubic-constraint matrix 200:
// kWords fp64 words) is a column of LDS: word k of thread j sits at s_buf[k * kFpThreads + j], so every run-time index (pivot
// rows, polynomial degrees, the Sturm sequence) addresses LDS, never a private array, and no kernel of this file uses scratch.
// 32 threads per workgroup: kWords x 32 x 8 B = 78 KB, two workgroups per CU.
#include "two_view.h"

#include <cfloat>
#include <cmath>

namespace {

using namespace two_view;

constexpr int kMaxSol = LS2FM_FIVE_POINT_MAX_SOLUTIONS;   // 10
constexpr int kFpThreads = 32;                 // five-point workgroups (hypotheses, ls2fm_five_point)
constexpr int kTriThreads = 256;
constexpr int kBisectIters = 100;
constexpr int kNewtonIters = 5;

// LDS words of one five-point solve
constexpr int kBas = 0;          // basis X, Y, Z, W: 4 x 9 (E = x X + y Y + z Z + W, row-major 3 x 3)
constexpr int kQ = 36;           // E E^T upper triangle, 6 quadratics x 10, trace 10; later minors (3 x 10), then B (3 x 13)
constexpr int kA = 106;          // the 10 x 20 matrix; the 5 x 9 system before it; the Sturm sequence after it
constexpr int kWords = 306;
constexpr int kSeq = kA;         // Sturm sequence: polynomial k (capacity 11 - k) at kSeq + 11 k - k (k - 1) / 2, 66 words
constexpr int kDeg = kA + 66;    // their degrees (11)
constexpr int kRoot = kA + 77;   // real roots (10)
constexpr int kTmp = kA + 100;   // scratch polynomials (minors of B, the long division's dividend), pivot columns

// ------------------------------------------------------------------------------------------------------- monomial indexing
// quadratic monomials: x^2 y^2 z^2 xy xz yz x y z 1 ; variables 0..3 = x, y, z, 1
HD inline int quad_index(int a, int b) {
    if (a > b) { const int t = a; a = b; b = t; }
    if (a == b) return a == 3 ? 9 : a;
    if (b == 3) return 6 + a;
    return a == 0 ? (b == 1 ? 3 : 4) : 5;
}
HD inline void quad_exps(int q, int& ex, int& ey, int& ez) {
    ex = (q == 0) * 2 + (q == 3 || q == 4 || q == 6);
    ey = (q == 1) * 2 + (q == 3 || q == 5 || q == 7);
    ez = (q == 2) * 2 + (q == 4 || q == 5 || q == 8);
}
// cubic monomials in COLMAP's order: x^3 y^3 x^2y xy^2 x^2z x^2 y^2z y^2 xyz xy | xz^2 xz x yz^2 yz y z^3 z^2 z 1
HD inline int cubic_index(int ex, int ey, int ez) {
    switch (ex * 16 + ey * 4 + ez) {
        case 48: return 0;  case 12: return 1;  case 36: return 2;  case 24: return 3;  case 33: return 4;
        case 32: return 5;  case 9: return 6;   case 8: return 7;   case 21: return 8;  case 20: return 9;
        case 18: return 10; case 17: return 11; case 16: return 12; case 6: return 13;  case 5: return 14;
        case 4: return 15;  case 3: return 16;  case 2: return 17;  case 1: return 18;  default: return 19;
    }
}
HD inline int cubic_of(int q, int v) {          // quadratic monomial q times variable v
    int ex, ey, ez;
    quad_exps(q, ex, ey, ez);
    return cubic_index(ex + (v == 0), ey + (v == 1), ez + (v == 2));
}

// ------------------------------------------------------------------------------------------------------------ polynomials
template <int S>
HD inline double horner(Col<S> w, int off, int deg, double x) {
    double r = w[off + deg];
    for (int i = deg - 1; i >= 0; --i) r = r * x + w[off + i];
    return r;
}

template <int S>
HD inline void poly_mul_acc(Col<S> w, int a, int da, int b, int db, int out, double sgn) {   // out += sgn a b
    for (int i = 0; i <= da; ++i)
        for (int j = 0; j <= db; ++j) w[out + i + j] += sgn * (w[a + i] * w[b + j]);
}

HD inline int seq_off(int k) { return kSeq + 11 * k - (k * (k - 1)) / 2; }

template <int S>
HD inline void poly_normalise(Col<S> w, int off, int deg) {       // divide by the largest |coefficient| (a positive factor)
    double m = 0.0;
    for (int i = 0; i <= deg; ++i) m = fmax(m, fabs(w[off + i]));
    if (m > 0.0)
        for (int i = 0; i <= deg; ++i) w[off + i] = w[off + i] / m;
}

template <int S>
HD inline int sign_changes(Col<S> w, int m, double x) {
    int changes = 0;
    double last = 0.0;
    for (int k = 0; k < m; ++k) {
        const double v = horner(w, seq_off(k), (int)w[kDeg + k], x);
        if (v != 0.0) {
            if (last != 0.0 && (v > 0.0) != (last > 0.0)) ++changes;
            last = v;
        }
    }
    return changes;
}

// real roots of the polynomial at seq_off(0) (ascending coefficients, degree <= 10) in ascending order -> kRoot; count returned
template <int S>
HD inline int sturm_roots(Col<S> w) {
    int d = 10;
    while (d >= 0 && w[seq_off(0) + d] == 0.0) --d;
    if (d < 1) return 0;
    for (int i = 0; i <= d; ++i)
        if (!is_finite(w[seq_off(0) + i])) return 0;
    poly_normalise(w, seq_off(0), d);
    for (int i = 0; i < d; ++i) w[seq_off(1) + i] = (double)(i + 1) * w[seq_off(0) + i + 1];
    poly_normalise(w, seq_off(1), d - 1);
    w[kDeg] = d;
    w[kDeg + 1] = d - 1;
    int m = 2;
    while (m < 11 && (int)w[kDeg + m - 1] > 0) {
        const int a = seq_off(m - 2), b = seq_off(m - 1), du = (int)w[kDeg + m - 2], dv = (int)w[kDeg + m - 1];
        for (int i = 0; i <= du; ++i) w[kTmp + i] = w[a + i];
        for (int k = du - dv; k >= 0; --k) {
            const double q = w[kTmp + dv + k] / w[b + dv];
            for (int j = 0; j < dv; ++j) w[kTmp + j + k] -= q * w[b + j];
            w[kTmp + dv + k] = 0.0;
        }
        int dr = dv - 1;
        while (dr >= 0 && !(fabs(w[kTmp + dr]) > LS2FM_STURM_TRIM)) --dr;     // the dividend's largest |coefficient| is 1
        if (dr < 0) break;
        const int c = seq_off(m);
        for (int i = 0; i <= dr; ++i) w[c + i] = -w[kTmp + i];
        poly_normalise(w, c, dr);
        w[kDeg + m] = dr;
        ++m;
    }
    // Cauchy bound of the (normalised) polynomial
    const int p0 = seq_off(0);
    double bound = 0.0;
    for (int i = 0; i < d; ++i) bound = fmax(bound, fabs(w[p0 + i] / w[p0 + d]));
    bound = 1.0 + bound;
    if (!is_finite(bound)) return 0;
    const int v_lo = sign_changes(w, m, -bound);
    const int total = v_lo - sign_changes(w, m, bound);
    int n = 0;
    double lo = -bound;
    for (int k = 1; k <= total && n < kMaxSol; ++k) {
        double hi = bound;
        // roots in (-bound, x] = v_lo - V(x); the k-th root is the smallest x with at least k
        for (int it = 0; it < kBisectIters; ++it) {
            const double mid = 0.5 * (lo + hi);
            if (!(hi - lo > LS2FM_BISECT_TOL * fmax(1.0, fmax(fabs(lo), fabs(hi)))) || mid == lo || mid == hi) break;
            if (v_lo - sign_changes(w, m, mid) >= k) hi = mid; else lo = mid;
        }
        double x = 0.5 * (lo + hi);
        for (int it = 0; it < kNewtonIters; ++it) {            // polish on the polynomial itself, inside the bracket
            double f = w[p0 + d], df = 0.0;
            for (int i = d - 1; i >= 0; --i) { df = df * x + f; f = f * x + w[p0 + i]; }
            if (df == 0.0) break;
            const double xn = x - f / df;
            if (!(xn >= lo && xn <= hi) || xn == x) break;
            x = xn;
        }
        w[kRoot + n] = x;
        ++n;
    }
    return n;
}

// ------------------------------------------------------------------------------------------------------ five-point solver
// the 4-dimensional null space of the 5 x 9 epipolar system (rows kron((x2, 1), (x1, 1))) -> kBas; the pivot columns at kTmp.
// false: rank != 5
template <int S>
HD inline bool nullspace5(const double (&x1)[5][2], const double (&x2)[5][2], Col<S> w) {
#pragma unroll
    for (int r = 0; r < 5; ++r) {
        const double a[3] = {x1[r][0], x1[r][1], 1.0}, b[3] = {x2[r][0], x2[r][1], 1.0};
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) w[kA + 9 * r + 3 * i + j] = b[i] * a[j];
    }
    return gj_nullspace<5, kA, kTmp, kBas>(w);
}

template <int S>
HD inline bool orthonormalise_basis(Col<S> w) {         // modified Gram-Schmidt, in the order X, Y, Z, W
    for (int j = 0; j < 4; ++j) {
        for (int i = 0; i < j; ++i) {
            double d = 0.0;
            for (int k = 0; k < 9; ++k) d += w[kBas + 9 * i + k] * w[kBas + 9 * j + k];
            for (int k = 0; k < 9; ++k) w[kBas + 9 * j + k] -= d * w[kBas + 9 * i + k];
        }
        double n = 0.0;
        for (int k = 0; k < 9; ++k) n += w[kBas + 9 * j + k] * w[kBas + 9 * j + k];
        if (!(n > 0.0) || !is_finite(n)) return false;
        const double inv = 1.0 / sqrt(n);
        for (int k = 0; k < 9; ++k) w[kBas + 9 * j + k] = w[kBas + 9 * j + k] * inv;
    }
    return true;
}

// linear polynomial of E entry e: coefficient of variable v (x, y, z, 1)
template <int S>
HD inline double lin(Col<S> w, int e, int v) { return w[kBas + 9 * v + e]; }

// Nister's constraints from the basis at kBas, elimination, the degree-10 polynomial, its real roots, E per root.
// emit(slot, const double E[9]) in ascending root order; returns the number emitted
template <int S, class Emit>
HD inline int solve_from_basis(Col<S> w, Emit emit) {
    // E E^T (upper triangle, pairs (0,0) (0,1) (0,2) (1,1) (1,2) (2,2)) as quadratics, then its trace
    for (int i = 0; i < 70; ++i) w[kQ + i] = 0.0;
    int k6 = 0;
    for (int i = 0; i < 3; ++i)
        for (int j = i; j < 3; ++j, ++k6)
            for (int k = 0; k < 3; ++k)
                for (int a = 0; a < 4; ++a)
                    for (int b = 0; b < 4; ++b) w[kQ + 10 * k6 + quad_index(a, b)] += lin(w, 3 * i + k, a) * lin(w, 3 * j + k, b);
    for (int q = 0; q < 10; ++q) w[kQ + 60 + q] = (w[kQ + q] + w[kQ + 30 + q]) + w[kQ + 50 + q];
    // rows 0..8: (2 E E^T E - tr(E E^T) E)_ij
    for (int i = 0; i < 200; ++i) w[kA + i] = 0.0;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            const int row = kA + 20 * (3 * i + j);
            for (int k = 0; k < 3; ++k) {
                const int lo = i < k ? i : k, hi = i < k ? k : i;
                const int q6 = lo == 0 ? hi : (lo == 1 ? 2 + hi : 5);
                for (int q = 0; q < 10; ++q)
                    for (int v = 0; v < 4; ++v) w[row + cubic_of(q, v)] += 2.0 * (w[kQ + 10 * q6 + q] * lin(w, 3 * k + j, v));
            }
            for (int q = 0; q < 10; ++q)
                for (int v = 0; v < 4; ++v) w[row + cubic_of(q, v)] -= w[kQ + 60 + q] * lin(w, 3 * i + j, v);
        }
    // row 9: det E by the first row's cofactors (minors as quadratics in kQ)
    for (int i = 0; i < 30; ++i) w[kQ + i] = 0.0;
    const int mi[3][4] = {{4, 8, 5, 7}, {3, 8, 5, 6}, {3, 7, 4, 6}};    // E11 E22 - E12 E21, E10 E22 - E12 E20, E10 E21 - E11 E20
#pragma unroll
    for (int m = 0; m < 3; ++m)
        for (int a = 0; a < 4; ++a)
            for (int b = 0; b < 4; ++b) {
                const int q = quad_index(a, b);
                w[kQ + 10 * m + q] += lin(w, mi[m][0], a) * lin(w, mi[m][1], b) - lin(w, mi[m][2], a) * lin(w, mi[m][3], b);
            }
#pragma unroll
    for (int m = 0; m < 3; ++m) {
        const double sg = m == 1 ? -1.0 : 1.0;
        for (int q = 0; q < 10; ++q)
            for (int v = 0; v < 4; ++v) w[kA + 180 + cubic_of(q, v)] += sg * (lin(w, m, v) * w[kQ + 10 * m + q]);
    }
    // Gauss-Jordan with partial pivoting on the left 10 x 10 block: [I | AA]
    double amax = 0.0;
    for (int i = 0; i < 200; ++i) amax = fmax(amax, fabs(w[kA + i]));
    if (!(amax > 0.0) || !is_finite(amax)) return 0;
    for (int c = 0; c < 10; ++c) {
        int p = c;
        double best = fabs(w[kA + 20 * c + c]);
        for (int r = c + 1; r < 10; ++r) {
            const double v = fabs(w[kA + 20 * r + c]);
            if (v > best) { best = v; p = r; }
        }
        if (!(best > 1e-14 * amax)) return 0;
        if (p != c)
            for (int k = c; k < 20; ++k) {
                const double t = w[kA + 20 * c + k];
                w[kA + 20 * c + k] = w[kA + 20 * p + k];
                w[kA + 20 * p + k] = t;
            }
        const double inv = 1.0 / w[kA + 20 * c + c];
        for (int k = c + 1; k < 20; ++k) w[kA + 20 * c + k] = w[kA + 20 * c + k] * inv;
        w[kA + 20 * c + c] = 1.0;
        for (int r = 0; r < 10; ++r) {
            if (r == c) continue;
            const double f = w[kA + 20 * r + c];
            for (int k = c + 1; k < 20; ++k) w[kA + 20 * r + k] -= f * w[kA + 20 * c + k];
            w[kA + 20 * r + c] = 0.0;
        }
    }
    // B(z) [x y 1]^T = 0 from rows (x^2 z, x^2), (y^2 z, y^2), (xyz, xy): <e> - z <f>; ascending powers of z.
    // B row i at kQ + 13 i: x column (4 coefficients), y column (4), 1 column (5)
#define AA(r, c) w[kA + 20 * (r) + 10 + (c)]
    for (int i = 0; i < 3; ++i) {
        const int e = 2 * i + 4, f = 2 * i + 5, o = kQ + 13 * i;
        for (int col = 0; col < 2; ++col) {
            const int c0 = 3 * col;
            w[o + 4 * col + 3] = -AA(f, c0);
            w[o + 4 * col + 2] = AA(e, c0) - AA(f, c0 + 1);
            w[o + 4 * col + 1] = AA(e, c0 + 1) - AA(f, c0 + 2);
            w[o + 4 * col + 0] = AA(e, c0 + 2);
        }
        w[o + 12] = -AA(f, 6);
        w[o + 11] = AA(e, 6) - AA(f, 7);
        w[o + 10] = AA(e, 7) - AA(f, 8);
        w[o + 9] = AA(e, 8) - AA(f, 9);
        w[o + 8] = AA(e, 9);
    }
#undef AA
    // det B(z): minors of rows 1, 2 (kTmp: 8 + 8 + 7 words), then the first row's cofactor expansion -> seq_off(0)
    auto bo = [](int i, int c) { return kQ + 13 * i + 4 * c; };
    auto bd = [](int c) { return c == 2 ? 4 : 3; };
    for (int i = 0; i < 23; ++i) w[kTmp + i] = 0.0;
    for (int i = 0; i < 11; ++i) w[seq_off(0) + i] = 0.0;
    const int mc[3][2] = {{1, 2}, {0, 2}, {0, 1}};
#pragma unroll
    for (int m = 0; m < 3; ++m) {
        const int a = mc[m][0], b = mc[m][1], out = kTmp + 8 * m;
        poly_mul_acc(w, bo(1, a), bd(a), bo(2, b), bd(b), out, 1.0);
        poly_mul_acc(w, bo(1, b), bd(b), bo(2, a), bd(a), out, -1.0);
    }
#pragma unroll
    for (int m = 0; m < 3; ++m)
        poly_mul_acc(w, bo(0, m), bd(m), kTmp + 8 * m, bd(mc[m][0]) + bd(mc[m][1]), seq_off(0), m == 1 ? -1.0 : 1.0);
    const int nroots = sturm_roots(w);
    int n = 0;
    for (int r = 0; r < nroots; ++r) {
        const double z = w[kRoot + r];
        double Bz[3][3];
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int c = 0; c < 3; ++c) Bz[i][c] = horner(w, bo(i, c), bd(c), z);
        // null vector of Bz: the largest cross product of two rows
        double cr[3][3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const int a = k == 2 ? 1 : 0, b = k == 0 ? 1 : 2;
            cr[k][0] = Bz[a][1] * Bz[b][2] - Bz[a][2] * Bz[b][1];
            cr[k][1] = Bz[a][2] * Bz[b][0] - Bz[a][0] * Bz[b][2];
            cr[k][2] = Bz[a][0] * Bz[b][1] - Bz[a][1] * Bz[b][0];
        }
        const double n0 = (cr[0][0] * cr[0][0] + cr[0][1] * cr[0][1]) + cr[0][2] * cr[0][2];
        const double n1 = (cr[1][0] * cr[1][0] + cr[1][1] * cr[1][1]) + cr[1][2] * cr[1][2];
        const double n2 = (cr[2][0] * cr[2][0] + cr[2][1] * cr[2][1]) + cr[2][2] * cr[2][2];
        const bool u0 = n0 >= n1;
        double X0 = u0 ? cr[0][0] : cr[1][0], X1 = u0 ? cr[0][1] : cr[1][1], X2 = u0 ? cr[0][2] : cr[1][2], nb = u0 ? n0 : n1;
        const bool keep = nb >= n2;
        X0 = keep ? X0 : cr[2][0]; X1 = keep ? X1 : cr[2][1]; X2 = keep ? X2 : cr[2][2]; nb = keep ? nb : n2;
        if (!(nb > 0.0) || !is_finite(nb)) continue;
        if (!(fabs(X2) >= 1e-10 * sqrt(nb))) continue;
        const double x = X0 / X2, y = X1 / X2;
        double e[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) e[k] = ((x * lin(w, k, 0) + y * lin(w, k, 1)) + z * lin(w, k, 2)) + lin(w, k, 3);
        if (!canonical9(e)) continue;
        emit(n, e);
        ++n;
    }
    return n;
}

// ------------------------------------------------------------------------------------------------------ pose from E (COLMAP)
// E = U diag(s, s, 0) V^T by one-sided Jacobi on E's columns; U, V made proper; R1 = U W V^T, R2 = U W^T V^T, t = U col 2.
// cand[k] = [R | t] for (R1, t), (R2, t), (R1, -t), (R2, -t)
HD inline void pose_candidates(const double* E, double (&cand)[4][12]) {
    double a[3][3], V[3][3];          // a[c]: column c of E V ; V[c]: column c of V
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int r = 0; r < 3; ++r) { a[c][r] = E[3 * r + c]; V[c][r] = c == r ? 1.0 : 0.0; }
    onesided_jacobi3(a, V);
    // order the columns by descending norm (three compare-and-swaps)
    double nr[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) nr[c] = (a[c][0] * a[c][0] + a[c][1] * a[c][1]) + a[c][2] * a[c][2];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int p = k == 1 ? 1 : 0, q = p + 1;
        const bool sw = nr[q] > nr[p];
        const double tn = nr[p];
        nr[p] = sw ? nr[q] : nr[p];
        nr[q] = sw ? tn : nr[q];
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const double ta = a[p][r], tv = V[p][r];
            a[p][r] = sw ? a[q][r] : a[p][r];
            a[q][r] = sw ? ta : a[q][r];
            V[p][r] = sw ? V[q][r] : V[p][r];
            V[q][r] = sw ? tv : V[q][r];
        }
    }
    double U[3][3];                   // U[c]: column c
    const double i0 = 1.0 / sqrt(nr[0]), i1 = 1.0 / sqrt(nr[1]);
#pragma unroll
    for (int r = 0; r < 3; ++r) { U[0][r] = a[0][r] * i0; U[1][r] = a[1][r] * i1; }
    U[2][0] = U[0][1] * U[1][2] - U[0][2] * U[1][1];
    U[2][1] = U[0][2] * U[1][0] - U[0][0] * U[1][2];
    U[2][2] = U[0][0] * U[1][1] - U[0][1] * U[1][0];
    const double detV = (V[0][0] * (V[1][1] * V[2][2] - V[1][2] * V[2][1]) - V[1][0] * (V[0][1] * V[2][2] - V[0][2] * V[2][1])) +
                        V[2][0] * (V[0][1] * V[1][2] - V[0][2] * V[1][1]);
    const double sv = detV < 0.0 ? -1.0 : 1.0;
    // U W V^T: W = [[0, 1, 0], [-1, 0, 0], [0, 0, 1]] -> U W = [-u1, u0, u2];  U W^T = [u1, -u0, u2]
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const double v0 = sv * V[0][j], v1 = sv * V[1][j], v2 = sv * V[2][j];
            const double r1 = (-U[1][i] * v0 + U[0][i] * v1) + U[2][i] * v2;
            const double r2 = (U[1][i] * v0 - U[0][i] * v1) + U[2][i] * v2;
            cand[0][4 * i + j] = r1; cand[2][4 * i + j] = r1;
            cand[1][4 * i + j] = r2; cand[3][4 * i + j] = r2;
        }
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        cand[0][4 * i + 3] = U[2][i]; cand[1][4 * i + 3] = U[2][i];
        cand[2][4 * i + 3] = -U[2][i]; cand[3][4 * i + 3] = -U[2][i];
    }
}

// COLMAP's CheckCheirality for one correspondence: depth in (DBL_EPSILON, 1000 |R^T t|) in both cameras
HD inline bool in_front(const double* P, double x1, double y1, double x2, double y2) {
    const double P0[12] = {1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0};
    double X[4];
    triangulate_dlt(P0, P, x1, y1, x2, y2, X);
    if (!(X[3] > 0.0)) return false;
    const double px = X[0] / X[3], py = X[1] / X[3], pz = X[2] / X[3];
    const double ctx = (P[0] * P[3] + P[4] * P[7]) + P[8] * P[11];       // R^T t
    const double cty = (P[1] * P[3] + P[5] * P[7]) + P[9] * P[11];
    const double ctz = (P[2] * P[3] + P[6] * P[7]) + P[10] * P[11];
    const double max_depth = 1000.0 * sqrt((ctx * ctx + cty * cty) + ctz * ctz);
    if (!(pz > DBL_EPSILON && pz < max_depth)) return false;
    const double z2 = ((P[8] * px + P[9] * py) + P[10] * pz) + P[11];
    const double c2 = sqrt((P[2] * P[2] + P[6] * P[6]) + P[10] * P[10]);
    const double d2 = z2 * c2;
    return d2 > DBL_EPSILON && d2 < max_depth;
}

// ------------------------------------------------------------------------------------------------------------------ model
struct EModel : Epipolar {      // essential matrices between K-normalised points, scored by the squared Sampson error
    static constexpr int kSample = 5, kMaxSol = LS2FM_FIVE_POINT_MAX_SOLUTIONS, kHypWords = 9, kMinGroup = 5, kHypThreads = kFpThreads, kHypLdsWords = kWords;
    static constexpr int kMinInliers = 5, kMaxCand = kMaxSol;
    struct Input { const double* uv0; const double* uv1; const double* intr0; const double* intr1; double err_px; };
    struct Ctx { const double* K0; const double* K1; double thr2; };
    using Point = two_view::Point;
    struct Lds { double solve[kWords]; double cand[kMaxCand][9]; double pose[4][12]; int ncand; };
    static __device__ __forceinline__ Ctx context(const Input& in, int p) {
        const double* K0 = in.intr0 + 4 * p;
        const double* K1 = in.intr1 + 4 * p;
        const double f0 = 0.5 * (K0[0] + K0[1]), f1 = 0.5 * (K1[0] + K1[1]);
        const double e = 0.5 * (in.err_px / f0 + in.err_px / f1);
        return {K0, K1, e * e};
    }
    static __device__ __forceinline__ Point load(const Input& in, const Ctx& c, int64_t i) {
        return {(in.uv0[2 * i] - c.K0[2]) / c.K0[0], (in.uv0[2 * i + 1] - c.K0[3]) / c.K0[1],
                (in.uv1[2 * i] - c.K1[2]) / c.K1[0], (in.uv1[2 * i + 1] - c.K1[3]) / c.K1[1]};
    }
    static __device__ __forceinline__ bool inlier(const double* E, const Point& pt, const Ctx& c) {
        return test(E, pt.x1, pt.y1, pt.x2, pt.y2, c.thr2);
    }
    template <int S, class Emit>
    static HD inline int solve(const double (&p1)[5][2], const double (&p2)[5][2], Col<S> w, Emit emit) {
        return nullspace5(p1, p2, w) && orthonormalise_basis(w) ? solve_from_basis(w, emit) : 0;
    }
    template <class Emit>
    static __device__ __forceinline__ void hypotheses(const Input& in, const Ctx& c, int64_t s0, const int64_t (&id)[5], double* column,
                                                      Emit emit) {
        sampled_solve<EModel>(in, c, s0, id, column, emit);
    }
    static __device__ __forceinline__ bool keeps(bool have, int) { return have; }     // E and the count are written below 5 inliers too
    // five-point on the normal matrix of X's inliers: its four smallest eigenvectors are the basis W, Z, Y, X
    static __device__ __forceinline__ int refit(const Input& in, const Ctx& ctx, int64_t s0, int64_t n, const double* X, int, Lds& lds,
                                                double* s_red) {
        double a[kNe];
#pragma unroll
        for (int q = 0; q < kNe; ++q) a[q] = 0.0;
        for_each_corr<EModel>(in, ctx, s0, n, [&](int64_t, double x1, double y1, double x2, double y2) {
            if (test(X, x1, y1, x2, y2, ctx.thr2)) accumulate(a, x1, y1, x2, y2);
        });
        smallest_eigenvectors<4>(a, s_red, lds.solve + kBas);
        if (threadIdx.x == 0)
            lds.ncand = solve_from_basis(Col<1>{lds.solve}, [&](int s, const double* e) {
                for (int q = 0; q < 9; ++q) lds.cand[s][q] = e[q];
            });
        __syncthreads();
        return lds.ncand;
    }
    // the pose: the candidate with the most triangulated inliers in front of both cameras (ties: the later); success: at least 5
    // inliers and one of them in front
    struct Tail {
        int front[4];
        __device__ __forceinline__ void begin(const double* E, bool keep, Lds& lds) {
#pragma unroll
            for (int k = 0; k < 4; ++k) front[k] = 0;
            if (keep && threadIdx.x == 0) {
                double cand[4][12];
                pose_candidates(E, cand);
#pragma unroll
                for (int k = 0; k < 4; ++k)
#pragma unroll
                    for (int q = 0; q < 12; ++q) lds.pose[k][q] = cand[k][q];
            }
            __syncthreads();
        }
        __device__ __forceinline__ void inlier(Lds& lds, double x1, double y1, double x2, double y2) {
#pragma unroll
            for (int k = 0; k < 4; ++k) front[k] += in_front(lds.pose[k], x1, y1, x2, y2) ? 1 : 0;
        }
        __device__ __forceinline__ bool finish(bool keep, int cur, Lds& lds, int* s_int, double* __restrict__ poses, int p) {
            int bestk = 0, bestf = -1;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int f = block_count(front[k], s_int);
                if (f >= bestf) { bestf = f; bestk = k; }
            }
            const bool ok = keep && cur >= kMinInliers && bestf > 0;
            const int tid = threadIdx.x;
            if (tid < 12) {
                double v = (tid == 0 || tid == 5 || tid == 10) ? 1.0 : 0.0;
#pragma unroll
                for (int k = 0; k < 4; ++k) v = (ok && bestk == k) ? lds.pose[k][tid] : v;
                poses[12 * p + tid] = v;
            }
            return ok;
        }
    };
};

// ---------------------------------------------------------------------------------------------------------- triangulation
__global__ void __launch_bounds__(kTriThreads)
triangulate_kernel(const double* __restrict__ P0, const double* __restrict__ P1, const double* __restrict__ uv0,
                   const double* __restrict__ uv1, const int32_t* __restrict__ ps, int32_t n_pairs, int64_t n, double* __restrict__ X) {
    const int64_t i = (int64_t)blockIdx.x * kTriThreads + threadIdx.x;
    if (i >= n) return;
    int lo = 0, hi = n_pairs;                 // the last pair with pair_start <= i
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if ((int64_t)ps[mid] <= i) lo = mid; else hi = mid;
    }
    double A[12], B[12];
#pragma unroll
    for (int q = 0; q < 12; ++q) { A[q] = P0[12 * lo + q]; B[q] = P1[12 * lo + q]; }
    double h[4];
    triangulate_dlt(A, B, uv0[2 * i], uv0[2 * i + 1], uv1[2 * i], uv1[2 * i + 1], h);
#pragma unroll
    for (int r = 0; r < 4; ++r) X[4 * i + r] = h[r];
}

}  // namespace

extern "C" int ls2fm_five_point(const double* x1, const double* x2, int64_t m, double* E, int32_t* n_solutions, void* stream) {
    return minimal_call<EModel>(x1, x2, m, E, n_solutions, stream);
}

extern "C" int64_t ls2fm_relative_pose_workspace_bytes(int32_t n_pairs, int64_t n_corr) { return workspace_bytes<EModel>(n_pairs, n_corr); }

extern "C" int ls2fm_relative_pose(const double* uv0, const double* uv1, const int32_t* pair_start, int32_t n_pairs, const double* intr0,
                                   const double* intr1, const ls2fm_pose_ransac_opts* opts, double* E, double* poses, uint8_t* inliers,
                                   int32_t* num_inliers, int32_t* trials, int32_t* best_trial, int32_t* success, void* workspace,
                                   void* stream) {
    LS2FM_CHECK_ARG(n_pairs >= 1 && n_pairs <= LS2FM_RELPOSE_MAX_PAIRS && pair_start && intr0 && intr1 && opts_ok(opts) &&
                    opts->refine == 0);
    LS2FM_CHECK_ARG(E && poses && num_inliers && trials && best_trial && success);
    return estimate<EModel>({uv0, uv1, intr0, intr1, opts->max_error_px}, pair_start, n_pairs, uv0 && uv1 && inliers, opts, E, poses,
                            inliers, num_inliers, trials, best_trial, success, workspace, stream);
}

extern "C" int ls2fm_triangulate(const double* P0, const double* P1, const double* uv0, const double* uv1, const int32_t* pair_start,
                                 int32_t n_pairs, int64_t n, double* X, void* stream) {
    LS2FM_CHECK_ARG(n_pairs >= 1 && n_pairs <= LS2FM_RELPOSE_MAX_PAIRS && n >= 0 && P0 && P1 && pair_start);
    if (n == 0) return LS2FM_OK;
    LS2FM_CHECK_ARG(uv0 && uv1 && X);
    triangulate_kernel<<<(unsigned)((n + kTriThreads - 1) / kTriThreads), kTriThreads, 0, (hipStream_t)stream>>>(P0, P1, uv0, uv1,
                                                                                                              pair_start, n_pairs, n, X);
    return ls2fm_launch_status();
}
