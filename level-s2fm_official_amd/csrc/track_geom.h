// What tracks.hip (triangulation) and mapper.hip (the mapper's upkeep of observations and points) share: the extent of a track,
// the numbering of the pairs of a track's first LS2FM_TRACK_HYP_OBS observations, the camera centre, the pixel error and depth of
// an observation, and the triangulation angle (wave_ops.h's workgroup scan numbers all tracks' pairs in one flat range).  include/ls2fm.h
// states the rules ("Feature tracks and multi-view triangulation"); all geometry in fp64, every sum in the order written here.
#pragma once
#include "ls2fm_device.h"

#include <cstdint>

namespace track_geom {

constexpr double kPi = 3.14159265358979323846;
constexpr int kHypObs = LS2FM_TRACK_HYP_OBS;
constexpr int kMaxObs = LS2FM_TRACK_MAX_OBS;

// the extent of track t: false (n = 0) when it is not inside [0, n_obs], runs backwards or is too long
__device__ __forceinline__ bool track_extent(const int32_t* __restrict__ track_start, int64_t n_obs, int64_t t, int64_t& s0, int& n) {
    const int64_t a = track_start[t], b = track_start[t + 1];
    const bool ok = a >= 0 && b >= a && b <= n_obs && b - a <= kMaxObs;
    s0 = ok ? a : 0;
    n = ok ? (int)(b - a) : 0;
    return ok;
}

// the last t of [0, T) with start[t] <= x (entries that share an offset: the last of them); T >= 1
template <typename S>
__device__ __forceinline__ int64_t last_not_above(const S* __restrict__ start, int64_t T, long long x) {
    int64_t lo = 0, hi = T;
    while (hi - lo > 1) {
        const int64_t mid = (lo + hi) >> 1;
        if ((long long)start[mid] <= x) lo = mid; else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ int pair_count(int n) {
    const int m = n < kHypObs ? n : kHypObs;
    return m >= 2 ? m * (m - 1) / 2 : 0;
}

// pair q of m observations in lexicographic order: q = i (2 m - i - 1) / 2 + (j - i - 1)
__device__ __forceinline__ void pair_of(int q, int m, int& i, int& j) {
    int row = 0, left = q;
    while (row < m - 2 && left >= m - 1 - row) {
        left -= m - 1 - row;
        ++row;
    }
    i = row;
    j = row + 1 + left;
}

// centre C_k = -((R0k t0 + R1k t1) + R2k t2) of the pose P [12]
__device__ __forceinline__ void centre_of(const double* __restrict__ P, double* __restrict__ C) {
#pragma unroll
    for (int k = 0; k < 3; ++k) C[k] = -((P[k] * P[3] + P[4 + k] * P[7]) + P[8 + k] * P[11]);
}

// the pixel (u, v) of the camera P [12], K [4] against X: the squared pixel error and the depth
__device__ __forceinline__ void pixel_error(const double* __restrict__ P, const double* __restrict__ K, double u, double v,
                                            const double (&X)[3], double& e2, double& depth) {
    const double xc = ((P[0] * X[0] + P[1] * X[1]) + P[2] * X[2]) + P[3];
    const double yc = ((P[4] * X[0] + P[5] * X[1]) + P[6] * X[2]) + P[7];
    const double zc = ((P[8] * X[0] + P[9] * X[1]) + P[10] * X[2]) + P[11];
    const double du = (K[0] * (xc / zc) + K[2]) - u;
    const double dv = (K[1] * (yc / zc) + K[3]) - v;
    e2 = du * du + dv * dv;
    depth = zc;
}

// min(a, pi - a) of the angle at X between the centres of views va and vb
__device__ __forceinline__ double tri_angle_of(const double* __restrict__ centre, int32_t va, int32_t vb, const double (&X)[3]) {
    const double* __restrict__ A = centre + 3 * (int64_t)va;
    const double* __restrict__ B = centre + 3 * (int64_t)vb;
    const double a0 = X[0] - A[0], a1 = X[1] - A[1], a2 = X[2] - A[2];
    const double b0 = X[0] - B[0], b1 = X[1] - B[1], b2 = X[2] - B[2];
    const double na = sqrt((a0 * a0 + a1 * a1) + a2 * a2), nb = sqrt((b0 * b0 + b1 * b1) + b2 * b2);
    double c = ((a0 * b0 + a1 * b1) + a2 * b2) / (na * nb);
    c = c > 1.0 ? 1.0 : (c < -1.0 ? -1.0 : c);                  // a NaN stays a NaN
    const double a = acos(c);
    return a < kPi - a ? a : kPi - a;
}

}  // namespace track_geom
