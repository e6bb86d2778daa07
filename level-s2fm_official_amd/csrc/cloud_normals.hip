// Normals of a point cloud from a neighbour list: the PCA of each query's neighbourhood, behind ls2fm.cloud.estimate_normals.
// include/ls2fm.h states the NORMAL RULE; tests/cloud_restate.py repeats it in numpy.
//
// ls2fm_cloud_normals (one launch): cn_normals, one query per lane.  The lane reads its row of the list (ls2fm_point_grid_knn's
// idx, or any other) twice -- once for the mean, once for the covariance; the second gather hits the cache -- and solves the 3 x 3
// symmetric eigenproblem by pose_math.h's jacobi3_sym.  Everything is fp64 of the fp32 points, every operation rounded once in the
// stated order, so the covariance is a pure function of the points and the list: its bits are tested.  No atomics, no workspace,
// nothing read back.
#include "ls2fm_device.h"
#include "pose_math.h"

namespace {

constexpr int kThreads = 256;

__global__ void __launch_bounds__(kThreads)
cn_normals(const float* __restrict__ points, int64_t n_points, const int32_t* __restrict__ idx, int64_t m, int k,
           const float* __restrict__ queries, const float* __restrict__ toward, int64_t n_toward, double* __restrict__ normal,
           double* __restrict__ curvature, double* __restrict__ cov) {
#pragma clang fp contract(off)
    const int64_t t = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (t >= m) return;
    const int32_t* row = idx + t * k;
    // the mean, in list order.  An entry outside [0, n_points) is no neighbour: nothing is read outside points.
    int n = 0;
    double sx = 0.0, sy = 0.0, sz = 0.0;
    for (int j = 0; j < k; ++j) {
        const int64_t i = row[j];
        if (i < 0 || i >= n_points) continue;
        const double x = (double)points[3 * i], y = (double)points[3 * i + 1], z = (double)points[3 * i + 2];
        if (n == 0) { sx = x; sy = y; sz = z; } else { sx = sx + x; sy = sy + y; sz = sz + z; }
        ++n;
    }
    const double dn = (double)n;
    const double mx = sx / dn, my = sy / dn, mz = sz / dn;
    double a[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    bool first = true;
    for (int j = 0; j < k; ++j) {
        const int64_t i = row[j];
        if (i < 0 || i >= n_points) continue;
        const double dx = (double)points[3 * i] - mx, dy = (double)points[3 * i + 1] - my, dz = (double)points[3 * i + 2] - mz;
        const double xx = dx * dx, xy = dx * dy, xz = dx * dz, yy = dy * dy, yz = dy * dz, zz = dz * dz;
        if (first) { a[0] = xx; a[1] = xy; a[2] = xz; a[3] = yy; a[4] = yz; a[5] = zz; first = false; }
        else { a[0] = a[0] + xx; a[1] = a[1] + xy; a[2] = a[2] + xz; a[3] = a[3] + yy; a[4] = a[4] + yz; a[5] = a[5] + zz; }
    }
#pragma unroll
    for (int e = 0; e < 6; ++e) a[e] = a[e] / dn;                       // n = 0: 0 / 0, the NaN the rule asks for
    if (cov) {
#pragma unroll
        for (int e = 0; e < 6; ++e) cov[6 * t + e] = n > 0 ? a[e] : NAN;
    }
    const double trace = (a[0] + a[3]) + a[5];
    double nx = NAN, ny = NAN, nz = NAN, curv = NAN;
    if (n >= 3 && trace != 0.0 && trace == trace) {
        double V[3][3];
        pose_math::jacobi3_sym(a, V);
        const double e0 = a[0], e1 = a[3], e2 = a[5];
        int best = 0;
        double lam = e0;
        if (e1 < lam) { best = 1; lam = e1; }
        if (e2 < lam) { best = 2; lam = e2; }
        double vx = best == 0 ? V[0][0] : (best == 1 ? V[1][0] : V[2][0]);
        double vy = best == 0 ? V[0][1] : (best == 1 ? V[1][1] : V[2][1]);
        double vz = best == 0 ? V[0][2] : (best == 1 ? V[1][2] : V[2][2]);
        const double len = sqrt((vx * vx + vy * vy) + vz * vz);
        vx = vx / len; vy = vy / len; vz = vz / len;
        bool flip;
        if (toward) {
            const float* tw = toward + (n_toward == 1 ? 0 : 3 * t);
            const double tx = (double)tw[0] - (double)queries[3 * t], ty = (double)tw[1] - (double)queries[3 * t + 1],
                         tz = (double)tw[2] - (double)queries[3 * t + 2];
            flip = (vx * tx + vy * ty) + vz * tz < 0.0;
        } else {
            double big = vx;
            if (fabs(vy) > fabs(big)) big = vy;
            if (fabs(vz) > fabs(big)) big = vz;
            flip = big < 0.0;
        }
        if (flip) { vx = -vx; vy = -vy; vz = -vz; }
        nx = vx; ny = vy; nz = vz;
        curv = lam / ((e0 + e1) + e2);
    }
    normal[3 * t] = nx;
    normal[3 * t + 1] = ny;
    normal[3 * t + 2] = nz;
    curvature[t] = curv;
}

}  // namespace

extern "C" int ls2fm_cloud_normals(const float* points, int64_t n_points, const int32_t* idx, int64_t n_queries, int32_t k,
                                   const float* queries, const float* toward, int64_t n_toward, double* normal, double* curvature,
                                   double* cov, void* stream) {
    LS2FM_CHECK_ARG(n_points >= 0 && n_points < ((int64_t)1 << 31) && n_queries >= 0 && k >= 1);
    LS2FM_CHECK_ARG(!toward || (queries && (n_toward == 1 || n_toward == n_queries)));
    if (n_queries == 0) return LS2FM_OK;
    LS2FM_CHECK_ARG(idx && normal && curvature && (points || n_points == 0));
    const int64_t blocks = (n_queries + kThreads - 1) / kThreads;
    LS2FM_CHECK_ARG(blocks < ((int64_t)1 << 31));
    cn_normals<<<(unsigned)blocks, kThreads, 0, (hipStream_t)stream>>>(points, n_points, idx, n_queries, k, queries, toward, n_toward, normal,
                                                                       curvature, cov);
    return ls2fm_launch_status();
}
