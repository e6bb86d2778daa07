// The wave64 and workgroup primitives of the library, stated once: reductions, scans, and the fixed-order fp64 workgroup sums.
// Every routine is a fixed sequence of operations -- the same bits in whichever file includes it.  A floating-point call site
// belongs here only if each lane then performs the very sequence of additions written below.  Sub-wave reductions (8, 16 or
// 32 lanes) stay where they are used: they have other widths and orders.
#pragma once

#include <hip/hip_runtime.h>

// ------------------------------------------------------------------------------------------------------------- wave reductions
// xor butterfly 32 ... 1 across the 64 lanes: every lane receives the result
template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// integers by comparison; float by fmaxf / fminf and double by fmax / fmin (the operand that is not NaN)
template <typename T>
__device__ __forceinline__ T wave_max(T v) {
    static_assert(__is_integral(T), "floating-point types have their own overloads");
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const T t = __shfl_xor(v, o, 64);
        v = v > t ? v : t;
    }
    return v;
}

template <typename T>
__device__ __forceinline__ T wave_min(T v) {
    static_assert(__is_integral(T), "floating-point types have their own overloads");
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const T t = __shfl_xor(v, o, 64);
        v = t < v ? t : v;
    }
    return v;
}

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

__device__ __forceinline__ float wave_min(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o, 64));
    return v;
}

__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
    return v;
}

__device__ __forceinline__ double wave_min(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmin(v, __shfl_xor(v, o, 64));
    return v;
}

// ------------------------------------------------------------------------------------------------------------------ wave scans
// inclusive prefix sum across the 64 lanes
template <typename T>
__device__ __forceinline__ T wave_scan_incl(T v, int lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const T t = __shfl_up(v, o, 64);
        if (lane >= o) v += t;
    }
    return v;
}

// exclusive suffix sum across the 64 lanes: sum of v over the lanes above this one
template <typename T>
__device__ __forceinline__ T wave_suffix_excl(T v, int lane) {
    T s = __shfl_down(v, 1, 64);
    if (lane == 63) s = T(0);
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const T t = __shfl_down(s, o, 64);
        if (lane + o < 64) s += t;
    }
    return s;
}

// ------------------------------------------------------------------------------------------------------------- workgroup scan
// Exclusive scan over the NT threads of the workgroup (wave64 shuffles, then the wave totals through LDS); `total` = the sum.
template <int NT, typename T>
__device__ __forceinline__ T block_exclusive_scan(T v, T& total) {
    __shared__ T s_wave[NT / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const T x = wave_scan_incl(v, lane);
    if (lane == 63) s_wave[wave] = x;
    __syncthreads();
    T before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < NT / 64; ++w) {
        const T s = s_wave[w];
        before += w < wave ? s : T(0);
        all += s;
    }
    __syncthreads();                                   // s_wave may be written again by the next scan
    total = all;
    return before + x - v;
}

// ------------------------------------------------------------------------------------------- workgroup reductions in fp64
// fixed-order sum of a[N] over a workgroup of Threads: xor-shuffles inside each wave, then the waves in index order through
// s_red [Threads / 64][N]; every thread receives the sums.  s_red is read last: a barrier before it is written again (the next
// block_sum has its own)
template <int N, int Threads>
__device__ __forceinline__ void block_sum(double (&a)[N], double* s_red) {
    const int tid = threadIdx.x;
#pragma unroll
    for (int q = 0; q < N; ++q) a[q] = wave_sum(a[q]);
    __syncthreads();
    if ((tid & 63) == 0)
#pragma unroll
        for (int q = 0; q < N; ++q) s_red[(tid >> 6) * N + q] = a[q];
    __syncthreads();
#pragma unroll
    for (int q = 0; q < N; ++q) {
        double t = s_red[q];
#pragma unroll
        for (int wv = 1; wv < Threads / 64; ++wv) t += s_red[wv * N + q];
        a[q] = t;
    }
}

// max over a workgroup of Threads (order-free and exact); every thread receives it.  s_mx [Threads / 64], read last like s_red
template <int Threads>
__device__ __forceinline__ double block_max(double m, double* s_mx) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmax(m, __shfl_xor(m, o, 64));       // wave_max(m), spelled in place: through the call
    __syncthreads();                                                        // balm_linearize is allocated one VGPR more
    if ((threadIdx.x & 63) == 0) s_mx[threadIdx.x >> 6] = m;
    __syncthreads();
    m = s_mx[0];
#pragma unroll
    for (int wv = 1; wv < Threads / 64; ++wv) m = fmax(m, s_mx[wv]);
    return m;
}
