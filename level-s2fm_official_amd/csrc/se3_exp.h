// The se(3) -> SE(3) exponential of one view and its gradient, as device functions a whole WAVE calls (utils/camera.py:85-147 of the
// reference: the 11-term series A, B, C; R = (I + A W) + B W2; V = (I + B W) + C W2; t = V u).  Behind ls2fm_se3_exp_fwd / _bwd and
// the fused ray construction (camera_rays.hip), and inside the classical bundle adjustment (bundle_adjust.hip): one restatement, so
// the three produce the same bits.  Arithmetic order: see camera_rays.hip.
#pragma once

#include "camera_ray.h"

namespace {

constexpr int kTerms = 11;

// The three 11-term series A, B, C (and their term-by-term derivatives) of one view, by ONE WAVE: lane 11 s + i forms term i of
// series s -- 33 powf calls side by side instead of one after the other in a single lane (15 us per call of the exponential, in
// front of every ray pick of a BA iteration) -- and every lane then sums the terms in the reference's order, left to right.
// Denominators by the reference's running products (utils/camera.py:100-147): A (2i+1)!, B (2i+2)!, C (2i+3)!.  All 64 lanes of
// the wave must be here.
template <bool WANT_D>
__device__ __forceinline__ void se3_series(float theta, float (&abc)[3], float (&dabc)[3]) {
    const int lane = threadIdx.x & 63;
    const int s = lane / kTerms, i = lane % kTerms;                 // lanes >= 33: s = 3.., never read
    double denom = s == 0 ? 1.0 : (s == 1 ? 2.0 : 6.0);
    for (int q = 1; q <= i; ++q)
        denom *= s == 0 ? (double)((2 * q) * (2 * q + 1)) : (s == 1 ? (double)((2 * q + 1) * (2 * q + 2)) : (double)((2 * q + 2) * (2 * q + 3)));
    const float sign = (i & 1) ? -1.0f : 1.0f;
    const float term = (sign * powf(theta, (float)(2 * i))) / (float)denom;
    float dterm = 0.f;
    if (WANT_D && i > 0) dterm = (sign * ((float)(2 * i) * powf(theta, (float)(2 * i - 1)))) / (float)denom;
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        float total = __shfl(term, q * kTerms, 64), dtotal = 0.f;
#pragma unroll
        for (int k = 1; k < kTerms; ++k) {
            total = total + __shfl(term, q * kTerms + k, 64);
            if (WANT_D) dtotal += __shfl(dterm, q * kTerms + k, 64);
        }
        abc[q] = total;
        dabc[q] = dtotal;
    }
}

// pose [3][4] of one view from its se(3) parameters (w, u): a whole wave calls this, every lane ends with the same pose
__device__ void se3_exp(const float* __restrict__ wu, float pose[12]) {
    const float w0 = wu[0], w1 = wu[1], w2 = wu[2];
    const float theta = sqrtf(w0 * w0 + w1 * w1 + w2 * w2);
    float abc[3], unused[3];
    se3_series<false>(theta, abc, unused);
    const float A = abc[0], B = abc[1], C = abc[2];
    const float W[3][3] = {{0.f, -w2, w1}, {w2, 0.f, -w0}, {-w1, w0, 0.f}};
    float W2[3][3], R[3][3], V[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) W2[i][j] = dot3(W[i][0], W[0][j], W[i][1], W[1][j], W[i][2], W[2][j]);
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const float eye = i == j ? 1.0f : 0.0f;
            R[i][j] = (eye + A * W[i][j]) + B * W2[i][j];
            V[i][j] = (eye + B * W[i][j]) + C * W2[i][j];
        }
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        pose[4 * i + 0] = R[i][0]; pose[4 * i + 1] = R[i][1]; pose[4 * i + 2] = R[i][2];
        pose[4 * i + 3] = dot3(V[i][0], wu[3], V[i][1], wu[4], V[i][2], wu[5]);
    }
}

// d L / d (w, u) from d L / d pose [3][4]: the chain rule through  t = V u,  R = I + A W + B W2,  V = I + B W + C W2,  W2 = W W,
// W = skew(w),  theta = |w|  and the series' term-by-term derivatives  X'(theta) = sum_i (-1)^i 2i theta^(2i-1) / d_i  -- what
// autograd forms from the truncated series (the i = 0 terms are constants; |w| at 0 has the zero subgradient, as in torch).
// A whole wave calls this (se3_series); every lane computes the same d_wu, the caller lets one lane store it.
__device__ void se3_exp_bwd(const float* __restrict__ wu, const float* __restrict__ g, float* __restrict__ d_wu) {
    const float w[3] = {wu[0], wu[1], wu[2]}, u[3] = {wu[3], wu[4], wu[5]};
    const float theta = sqrtf(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
    float abc[3], dabc[3];
    se3_series<true>(theta, abc, dabc);
    const float A = abc[0], B = abc[1], C = abc[2];
    const float W[3][3] = {{0.f, -w[2], w[1]}, {w[2], 0.f, -w[0]}, {-w[1], w[0], 0.f}};
    float W2[3][3], V[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) W2[i][j] = dot3(W[i][0], W[0][j], W[i][1], W[1][j], W[i][2], W[2][j]);
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) V[i][j] = ((i == j ? 1.0f : 0.0f) + B * W[i][j]) + C * W2[i][j];
    float gR[3][3], gV[3][3], gT[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        gT[i] = g[4 * i + 3];
#pragma unroll
        for (int j = 0; j < 3; ++j) { gR[i][j] = g[4 * i + j]; gV[i][j] = gT[i] * u[j]; }
    }
    float gA = 0.f, gB = 0.f, gC = 0.f;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            gA = fmaf(gR[i][j], W[i][j], gA);
            gB = fmaf(gR[i][j], W2[i][j], fmaf(gV[i][j], W[i][j], gB));
            gC = fmaf(gV[i][j], W2[i][j], gC);
        }
    float gW[3][3], gW2[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) { gW[i][j] = fmaf(B, gV[i][j], A * gR[i][j]); gW2[i][j] = fmaf(C, gV[i][j], B * gR[i][j]); }
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            // W2 = W W :  G_W += G_W2 W^T + W^T G_W2
            const float a = dot3(gW2[i][0], W[j][0], gW2[i][1], W[j][1], gW2[i][2], W[j][2]);
            const float b = dot3(W[0][i], gW2[0][j], W[1][i], gW2[1][j], W[2][i], gW2[2][j]);
            gW[i][j] += a + b;
        }
    const float g_theta = fmaf(gC, dabc[2], fmaf(gB, dabc[1], gA * dabc[0]));
    const float inv = theta > 0.f ? g_theta / theta : 0.f;
    d_wu[0] = fmaf(inv, w[0], gW[2][1] - gW[1][2]);
    d_wu[1] = fmaf(inv, w[1], gW[0][2] - gW[2][0]);
    d_wu[2] = fmaf(inv, w[2], gW[1][0] - gW[0][1]);
#pragma unroll
    for (int j = 0; j < 3; ++j) d_wu[3 + j] = dot3(V[0][j], gT[0], V[1][j], gT[1], V[2][j], gT[2]);
}

}  // namespace
