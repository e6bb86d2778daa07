// Small fp64 routines shared by relative_pose.hip, two_view.hip and tracks.hip: the LDS column view of a solver's run-time-indexed state, the
// unit-norm-and-sign rule of a 3 x 3 model, the squared Sampson error, the cyclic Jacobi of a symmetric 9 x 9 (and 4 x 4), the one-sided
// Jacobi of a 3 x 3 and the two-view DLT (also used by tracks.hip).
// Every routine is a fixed sequence of fp64 operations (the library is built with -ffp-contract=off): the same bits on the host,
// on the device and in whichever file includes it.
#pragma once

#include <cmath>

#ifndef HD
#define HD __host__ __device__
#endif

namespace pose_math {

constexpr int kJacobiSweeps = 30;

HD inline bool is_finite(double x) { return x - x == 0.0; }       // host and device alike (inf - inf and NaN are NaN)

template <int S>
struct Col {                     // one solve's words in LDS, stride S
    double* p;
    HD double& operator[](int k) const { return p[k * S]; }
};

// unit Frobenius norm, the largest |entry| positive (the first of equals, row-major); false when zero or not finite
HD inline bool canonical9(double (&e)[9]) {
    double nrm = 0.0;
#pragma unroll
    for (int i = 0; i < 9; ++i) nrm += e[i] * e[i];
    if (!(nrm > 0.0) || !is_finite(nrm)) return false;
    const double inv = 1.0 / sqrt(nrm);
    double big = 0.0, sgn = 1.0;
#pragma unroll
    for (int i = 0; i < 9; ++i) {
        e[i] = e[i] * inv;
        if (fabs(e[i]) > big) { big = fabs(e[i]); sgn = e[i] < 0.0 ? -1.0 : 1.0; }
    }
#pragma unroll
    for (int i = 0; i < 9; ++i) e[i] = sgn * e[i];
    return true;
}

// --------------------------------------------------------------------------------------------------------- Sampson error
// squared Sampson error of x2h^T E x1h = 0 (E an essential matrix between normalised points or a fundamental matrix between pixels)
HD inline double sampson2(const double* E, double x1, double y1, double x2, double y2) {
    const double a0 = (E[0] * x1 + E[1] * y1) + E[2];
    const double a1 = (E[3] * x1 + E[4] * y1) + E[5];
    const double a2 = (E[6] * x1 + E[7] * y1) + E[8];
    const double b0 = (E[0] * x2 + E[3] * y2) + E[6];
    const double b1 = (E[1] * x2 + E[4] * y2) + E[7];
    const double num = (x2 * a0 + y2 * a1) + a2;
    const double den = ((a0 * a0 + a1 * a1) + b0 * b0) + b1 * b1;
    return num * num / den;
}

// ------------------------------------------------------------------------------------------------------ one-sided Jacobi
// a[c] = column c of a 3 x 3 M, V = identity on entry: rotations of column pairs (while |a_p . a_q| > 1e-15 |a_p| |a_q|, at most
// kJacobiSweeps sweeps) until the columns are orthogonal: a = M V, |a[c]| the singular values (unordered), V[c] = column c of V
HD inline void onesided_jacobi3(double (&a)[3][3], double (&V)[3][3]) {
    for (int sweep = 0; sweep < kJacobiSweeps; ++sweep) {
        bool rotated = false;
#pragma unroll
        for (int p = 0; p < 2; ++p)
#pragma unroll
            for (int q = p + 1; q < 3; ++q) {
                const double al = (a[p][0] * a[p][0] + a[p][1] * a[p][1]) + a[p][2] * a[p][2];
                const double be = (a[q][0] * a[q][0] + a[q][1] * a[q][1]) + a[q][2] * a[q][2];
                const double ga = (a[p][0] * a[q][0] + a[p][1] * a[q][1]) + a[p][2] * a[q][2];
                if (!(fabs(ga) > 1e-15 * sqrt(al * be))) continue;
                rotated = true;
                const double zeta = (be - al) / (2.0 * ga);
                const double t = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
                const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
#pragma unroll
                for (int r = 0; r < 3; ++r) {
                    const double ap = a[p][r], aq = a[q][r];
                    a[p][r] = c * ap - s * aq;
                    a[q][r] = s * ap + c * aq;
                    const double vp = V[p][r], vq = V[q][r];
                    V[p][r] = c * vp - s * vq;
                    V[q][r] = s * vp + c * vq;
                }
            }
        if (!rotated) break;
    }
}

// ------------------------------------------------------------------------------------------------------ symmetric Jacobi
constexpr int sidx(int i, int j) { return i <= j ? i * 9 - (i * (i - 1)) / 2 + (j - i) : j * 9 - (j * (j - 1)) / 2 + (i - j); }

// eigen-decomposition of the symmetric 9 x 9 a (upper triangle, 45 entries): cyclic Jacobi, at most kJacobiSweeps sweeps.
// The caller holds ONE component of the eigenvectors: v[k] = component `row` of the eigenvector of eigenvalue a[sidx(k, k)]
// (every thread of a workgroup runs the same rotations on the same a, thread r < 9 keeps row r)
HD inline void jacobi9(double (&a)[45], int row, double (&v)[9]) {
#pragma unroll
    for (int k = 0; k < 9; ++k) v[k] = k == row ? 1.0 : 0.0;
    for (int sweep = 0; sweep < kJacobiSweeps; ++sweep) {
        double off = 0.0, dia = 0.0;
#pragma unroll
        for (int i = 0; i < 9; ++i) {
            dia += a[sidx(i, i)] * a[sidx(i, i)];
#pragma unroll
            for (int j = i + 1; j < 9; ++j) off += a[sidx(i, j)] * a[sidx(i, j)];
        }
        if (!(off > 1e-30 * dia)) break;
#pragma unroll
        for (int p = 0; p < 8; ++p)
#pragma unroll
            for (int q = p + 1; q < 9; ++q) {
                const double apq = a[sidx(p, q)];
                if (apq == 0.0) continue;
                const double theta = (a[sidx(q, q)] - a[sidx(p, p)]) / (2.0 * apq);
                const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
#pragma unroll
                for (int k = 0; k < 9; ++k) {
                    if (k == p || k == q) continue;
                    const double akp = a[sidx(k, p)], akq = a[sidx(k, q)];
                    a[sidx(k, p)] = c * akp - s * akq;
                    a[sidx(k, q)] = s * akp + c * akq;
                }
                a[sidx(p, p)] = a[sidx(p, p)] - t * apq;
                a[sidx(q, q)] = a[sidx(q, q)] + t * apq;
                a[sidx(p, q)] = 0.0;
                const double vp = v[p], vq = v[q];
                v[p] = c * vp - s * vq;
                v[q] = s * vp + c * vq;
            }
    }
}

// the place of eigenvalue k of jacobi9's diagonal in ascending order (the lower index first among equals)
HD inline int eigen_rank9(const double (&a)[45], int k) {
    int rank = 0;
#pragma unroll
    for (int j = 0; j < 9; ++j) {
        const double ej = a[sidx(j, j)], ek = a[sidx(k, k)];
        rank += (ej < ek || (ej == ek && j < k)) ? 1 : 0;
    }
    return rank;
}

// ----------------------------------------------------------------------------------------------------------- triangulation
// the 4 x 4 DLT of cv2.triangulatePoints (rows x P[2] - P[0], y P[2] - P[1] of both views); right singular vector of the smallest
// singular value by one-sided Jacobi on A; unit norm, w >= 0
HD inline void triangulate_dlt(const double* P0, const double* P1, double u0, double v0, double u1, double v1, double (&X)[4]) {
    double a[4][4], V[4][4];          // a[c][r]: column c of A
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        a[c][0] = u0 * P0[8 + c] - P0[c];
        a[c][1] = v0 * P0[8 + c] - P0[4 + c];
        a[c][2] = u1 * P1[8 + c] - P1[c];
        a[c][3] = v1 * P1[8 + c] - P1[4 + c];
#pragma unroll
        for (int r = 0; r < 4; ++r) V[c][r] = c == r ? 1.0 : 0.0;       // V[c]: column c of V
    }
    for (int sweep = 0; sweep < kJacobiSweeps; ++sweep) {
        bool rotated = false;
#pragma unroll
        for (int p = 0; p < 3; ++p)
#pragma unroll
            for (int q = p + 1; q < 4; ++q) {
                const double al = ((a[p][0] * a[p][0] + a[p][1] * a[p][1]) + a[p][2] * a[p][2]) + a[p][3] * a[p][3];
                const double be = ((a[q][0] * a[q][0] + a[q][1] * a[q][1]) + a[q][2] * a[q][2]) + a[q][3] * a[q][3];
                const double ga = ((a[p][0] * a[q][0] + a[p][1] * a[q][1]) + a[p][2] * a[q][2]) + a[p][3] * a[q][3];
                if (!(fabs(ga) > 1e-15 * sqrt(al * be))) continue;
                rotated = true;
                const double zeta = (be - al) / (2.0 * ga);
                const double t = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
                const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const double ap = a[p][r], aq = a[q][r];
                    a[p][r] = c * ap - s * aq;
                    a[q][r] = s * ap + c * aq;
                    const double vp = V[p][r], vq = V[q][r];
                    V[p][r] = c * vp - s * vq;
                    V[q][r] = s * vp + c * vq;
                }
            }
        if (!rotated) break;
    }
    double best = 0.0;
    int bi = 0;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const double n = ((a[c][0] * a[c][0] + a[c][1] * a[c][1]) + a[c][2] * a[c][2]) + a[c][3] * a[c][3];
        if (c == 0 || n < best) { best = n; bi = c; }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) X[r] = bi == 0 ? V[0][r] : (bi == 1 ? V[1][r] : (bi == 2 ? V[2][r] : V[3][r]));
    const double nrm = sqrt(((X[0] * X[0] + X[1] * X[1]) + X[2] * X[2]) + X[3] * X[3]);
    const double s = (X[3] < 0.0 ? -1.0 : 1.0) / nrm;
#pragma unroll
    for (int r = 0; r < 4; ++r) X[r] = X[r] * s;
}

// ------------------------------------------------------------------------------------------------- symmetric Jacobi, 4 x 4
// jacobi9's rules at size 4, every lane holding the whole problem: a = upper triangle of the symmetric 4 x 4, row-major (00 01 02
// 03 11 12 13 22 23 33); on return its diagonal entries are the eigenvalues and V[k] the eigenvector of eigenvalue k
constexpr int sidx4(int i, int j) { return i <= j ? i * 4 - (i * (i - 1)) / 2 + (j - i) : j * 4 - (j * (j - 1)) / 2 + (i - j); }

HD inline void jacobi4(double (&a)[10], double (&V)[4][4]) {
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int r = 0; r < 4; ++r) V[k][r] = k == r ? 1.0 : 0.0;
    for (int sweep = 0; sweep < kJacobiSweeps; ++sweep) {
        double off = 0.0, dia = 0.0;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            dia += a[sidx4(i, i)] * a[sidx4(i, i)];
#pragma unroll
            for (int j = i + 1; j < 4; ++j) off += a[sidx4(i, j)] * a[sidx4(i, j)];
        }
        if (!(off > 1e-30 * dia)) break;
#pragma unroll
        for (int p = 0; p < 3; ++p)
#pragma unroll
            for (int q = p + 1; q < 4; ++q) {
                const double apq = a[sidx4(p, q)];
                if (apq == 0.0) continue;
                const double theta = (a[sidx4(q, q)] - a[sidx4(p, p)]) / (2.0 * apq);
                const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    if (k == p || k == q) continue;
                    const double akp = a[sidx4(k, p)], akq = a[sidx4(k, q)];
                    a[sidx4(k, p)] = c * akp - s * akq;
                    a[sidx4(k, q)] = s * akp + c * akq;
                }
                a[sidx4(p, p)] = a[sidx4(p, p)] - t * apq;
                a[sidx4(q, q)] = a[sidx4(q, q)] + t * apq;
                a[sidx4(p, q)] = 0.0;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const double vp = V[p][r], vq = V[q][r];
                    V[p][r] = c * vp - s * vq;
                    V[q][r] = s * vp + c * vq;
                }
            }
    }
}

// ------------------------------------------------------------------------------------------------- symmetric Jacobi, 3 x 3
// jacobi4's rules at size 3 (cloud_normals.hip: the covariance of a neighbourhood): a = upper triangle row-major (00 01 02 11 12
// 22); on return its diagonal entries are the eigenvalues and V[k] the eigenvector of eigenvalue k
constexpr int sidx3(int i, int j) { return i <= j ? i * 3 - (i * (i - 1)) / 2 + (j - i) : j * 3 - (j * (j - 1)) / 2 + (i - j); }

HD inline void jacobi3_sym(double (&a)[6], double (&V)[3][3]) {
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int r = 0; r < 3; ++r) V[k][r] = k == r ? 1.0 : 0.0;
    for (int sweep = 0; sweep < kJacobiSweeps; ++sweep) {
        double off = 0.0, dia = 0.0;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            dia += a[sidx3(i, i)] * a[sidx3(i, i)];
#pragma unroll
            for (int j = i + 1; j < 3; ++j) off += a[sidx3(i, j)] * a[sidx3(i, j)];
        }
        if (!(off > 1e-30 * dia)) break;
#pragma unroll
        for (int p = 0; p < 2; ++p)
#pragma unroll
            for (int q = p + 1; q < 3; ++q) {
                const double apq = a[sidx3(p, q)];
                if (apq == 0.0) continue;
                const double theta = (a[sidx3(q, q)] - a[sidx3(p, p)]) / (2.0 * apq);
                const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    if (k == p || k == q) continue;
                    const double akp = a[sidx3(k, p)], akq = a[sidx3(k, q)];
                    a[sidx3(k, p)] = c * akp - s * akq;
                    a[sidx3(k, q)] = s * akp + c * akq;
                }
                a[sidx3(p, p)] = a[sidx3(p, p)] - t * apq;
                a[sidx3(q, q)] = a[sidx3(q, q)] + t * apq;
                a[sidx3(p, q)] = 0.0;
#pragma unroll
                for (int r = 0; r < 3; ++r) {
                    const double vp = V[p][r], vq = V[q][r];
                    V[p][r] = c * vp - s * vq;
                    V[q][r] = s * vp + c * vq;
                }
            }
    }
}

}  // namespace pose_math
