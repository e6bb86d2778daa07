// The fp64 pieces of a Levenberg-Marquardt step that absolute_pose.hip (one pose), two_view.h and bundle_adjust_lm.hip (poses and
// points) share, and icp.hip with them: the damped Cholesky solve (6 x 6 for the three; icp.hip takes it at 7 x 7 too), Rodrigues'
// formula and the pose update; the fixed-order workgroup sum they go with (block_sum) is wave_ops.h's, included here.  Every
// routine is a fixed sequence of fp64 operations (the library is built with -ffp-contract=off): the same bits in whichever file
// includes it.
#pragma once

#include <cmath>

#include "wave_ops.h"

namespace lm_math {

// solve (H + lam diag(dg)) x = -g by Cholesky, M unknowns (the size of x): a holds the M (M + 1) / 2 entries of the upper triangle of
// H (row-major), then g.  dg has M entries (read even where lam = 0).  false for a pivot <= 0 or a solution that is not finite.
template <int M, int N>
__device__ inline bool chol_solve(const double (&a)[N], double lam, const double* dg, double (&x)[M]) {
    constexpr int T = M * (M + 1) / 2;
    static_assert(N >= T + M, "M (M + 1) / 2 entries of H and M of g");
    double L[M][M];
#pragma unroll
    for (int i = 0; i < M; ++i)
#pragma unroll
        for (int j = 0; j < M; ++j) L[i][j] = 0.0;
    int q = 0;
#pragma unroll
    for (int r = 0; r < M; ++r)
#pragma unroll
        for (int c = r; c < M; ++c) L[c][r] = a[q++] + (r == c ? lam * dg[r] : 0.0);       // lower triangle of the matrix
    bool ok = true;
#pragma unroll
    for (int j = 0; j < M; ++j) {
        double d = L[j][j];
#pragma unroll
        for (int k = 0; k < j; ++k) d -= L[j][k] * L[j][k];
        ok = ok && d > 0.0;
        const double ljj = sqrt(d > 0.0 ? d : 1.0);
        L[j][j] = ljj;
#pragma unroll
        for (int i = j + 1; i < M; ++i) {
            double s = L[i][j];
#pragma unroll
            for (int k = 0; k < j; ++k) s -= L[i][k] * L[j][k];
            L[i][j] = s / ljj;
        }
    }
    double z[M];
#pragma unroll
    for (int i = 0; i < M; ++i) {
        double s = -a[T + i];
#pragma unroll
        for (int k = 0; k < i; ++k) s -= L[i][k] * z[k];
        z[i] = s / L[i][i];
    }
#pragma unroll
    for (int i = M - 1; i >= 0; --i) {
        double s = z[i];
#pragma unroll
        for (int k = i + 1; k < M; ++k) s -= L[k][i] * x[k];
        x[i] = s / L[i][i];
    }
#pragma unroll
    for (int i = 0; i < M; ++i) ok = ok && isfinite(x[i]);
    return ok;
}

// E = exp([w]x) by Rodrigues' formula: I + (sin th / th) K + ((1 - cos th) / th^2) K K, K = [w]x; below th^2 = 1e-30, I + K
__device__ inline void rodrigues(double w0, double w1, double w2, double (&E)[3][3]) {
    const double th2 = (w0 * w0 + w1 * w1) + w2 * w2;
    double A = 1.0, Bc = 0.0;
    if (th2 >= 1e-30) {
        const double th = sqrt(th2);
        A = sin(th) / th;
        Bc = (1.0 - cos(th)) / th2;
    }
    const double K[3][3] = {{0.0, -w2, w1}, {w2, 0.0, -w0}, {-w1, w0, 0.0}};
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const double kk = (K[i][0] * K[0][j] + K[i][1] * K[1][j]) + K[i][2] * K[2][j];
            E[i][j] = ((i == j ? 1.0 : 0.0) + A * K[i][j]) + Bc * kk;
        }
}

// R <- exp([w]x) R, t <- exp([w]x) t + dt
__device__ inline void pose_update(const double* P, const double (&d)[6], double* C) {
    double E[3][3];
    rodrigues(d[0], d[1], d[2], E);
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) C[4 * i + j] = (E[i][0] * P[j] + E[i][1] * P[4 + j]) + E[i][2] * P[8 + j];
#pragma unroll
    for (int i = 0; i < 3; ++i) C[4 * i + 3] += d[3 + i];
}

}  // namespace lm_math
