// The fp64 pieces of a Levenberg-Marquardt step that absolute_pose.hip (one pose), two_view.h and bundle_adjust_lm.hip (poses and
// points) share: the damped 6 x 6 Cholesky solve and the pose update; the fixed-order workgroup sum they go with (block_sum) is
// wave_ops.h's, included here.  Every routine is a fixed sequence of fp64 operations (the library is built with
// -ffp-contract=off): the same bits in whichever file includes it.
#pragma once

#include <cmath>

#include "wave_ops.h"

namespace lm_math {

// solve (H + lam diag(dg)) x = -g by Cholesky; a: the 21-entry upper triangle of H (row-major), then g at a[21 .. 26]
template <int N>
__device__ inline bool chol_solve(const double (&a)[N], double lam, const double* dg, double (&x)[6]) {
    static_assert(N >= 27, "21 entries of H and 6 of g");
    double L[6][6];
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int j = 0; j < 6; ++j) L[i][j] = 0.0;
    int q = 0;
#pragma unroll
    for (int r = 0; r < 6; ++r)
#pragma unroll
        for (int c = r; c < 6; ++c) L[c][r] = a[q++] + (r == c ? lam * dg[r] : 0.0);       // lower triangle of the matrix
    bool ok = true;
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        double d = L[j][j];
#pragma unroll
        for (int k = 0; k < j; ++k) d -= L[j][k] * L[j][k];
        ok = ok && d > 0.0;
        const double ljj = sqrt(d > 0.0 ? d : 1.0);
        L[j][j] = ljj;
#pragma unroll
        for (int i = j + 1; i < 6; ++i) {
            double s = L[i][j];
#pragma unroll
            for (int k = 0; k < j; ++k) s -= L[i][k] * L[j][k];
            L[i][j] = s / ljj;
        }
    }
    double z[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        double s = -a[21 + i];
#pragma unroll
        for (int k = 0; k < i; ++k) s -= L[i][k] * z[k];
        z[i] = s / L[i][i];
    }
#pragma unroll
    for (int i = 5; i >= 0; --i) {
        double s = z[i];
#pragma unroll
        for (int k = i + 1; k < 6; ++k) s -= L[k][i] * x[k];
        x[i] = s / L[i][i];
    }
#pragma unroll
    for (int i = 0; i < 6; ++i) ok = ok && isfinite(x[i]);
    return ok;
}

// R <- exp([w]x) R, t <- exp([w]x) t + dt
__device__ inline void pose_update(const double* P, const double (&d)[6], double* C) {
    const double w0 = d[0], w1 = d[1], w2 = d[2];
    const double th2 = (w0 * w0 + w1 * w1) + w2 * w2;
    double A = 1.0, Bc = 0.0;
    if (th2 >= 1e-30) {
        const double th = sqrt(th2);
        A = sin(th) / th;
        Bc = (1.0 - cos(th)) / th2;
    }
    const double K[3][3] = {{0.0, -w2, w1}, {w2, 0.0, -w0}, {-w1, w0, 0.0}};
    double E[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const double kk = (K[i][0] * K[0][j] + K[i][1] * K[1][j]) + K[i][2] * K[2][j];
            E[i][j] = ((i == j ? 1.0 : 0.0) + A * K[i][j]) + Bc * kk;
        }
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) C[4 * i + j] = (E[i][0] * P[j] + E[i][1] * P[4 + j]) + E[i][2] * P[8 + j];
#pragma unroll
    for (int i = 0; i < 3; ++i) C[4 * i + 3] += d[3 + i];
}

}  // namespace lm_math
