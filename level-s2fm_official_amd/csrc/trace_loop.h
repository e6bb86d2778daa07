// The sphere-tracing root-find of the reference (models/SDF.py:149-200), stated once: the state of one ray END, the loop's steps,
// and the three ways a ray's two ends are laid out on the lanes.  The kernels of sdf_eval.hip and trace_image.hip keep their own
// `for`, their own exits and their own stores, and call the steps in the reference's order:
//
//     begin                      start parameter (near / far), first value
//     for k = 0 ..
//         (1)+(2) trace_mask     converged values are ZEROED (not kept); the unfinished flag only ever falls
//         (3)                    the kernel's business: is the ray's start end done?  (trip count, early exit)
//         (5)                    the kernel's business: the pre-update start point is track point k
//         (4) trace_step         BOTH ends step with '+' (the far end too), clamped to far; finished ends keep stepping on their
//                                stale value
//         (6) trace_refresh      the new point; its value only where the end is unfinished -- or, for the track's values, also where
//                                a finished start end still moved (the reference evaluates those points afterwards, SDF.py:203)
//         (7) trace_cross        ends that crossed drop out
//
// A layout (`Ends`) answers four questions: the field's value at p, the other end's t, the start end's unfinished flag, and
// whether this lane writes the end's outputs.  All three evaluate the field with sdf_point.h's pieces in one summation order,
// so a ray traces to the same bits whichever kernel serves it.
#pragma once

#include "sdf_point.h"

namespace {

struct TraceEnd {
    float t, p[3];
    float sdf;          // the step: the field's value, zeroed once converged (1), stale once the end is finished (6)
    float raw;          // the field's value at p
    bool unf;
};

// ---- one lane per end; the two ends of a ray are neighbouring lanes (side = lane & 1)
struct LaneEnds {
    const LevelSet& lv;
    const FieldC& fc;
    int bg_sdf;
    float bg_rad;
    const float* __restrict__ rec;
    const float* __restrict__ table;
    int side;
    __device__ __forceinline__ float at(const float p[3]) const { return lane_sdf(lv, fc, bg_sdf, bg_rad, rec, table, p); }
    __device__ __forceinline__ float other_t(float t, int) const { return __shfl_xor(t, 1, 64); }
    __device__ __forceinline__ bool start_unfinished(bool unf) const { return __shfl((int)unf, (threadIdx.x & 63) & ~1, 64); }
    __device__ __forceinline__ bool writer() const { return true; }
};

// ---- one 16-lane group per end, four ends = two rays per wave (side = bit 4 of the lane); W0 | b0 and the sdf row in LDS
struct GroupEnds {
    const LevelSet& lv;
    const FieldC& fc;
    int bg_sdf;
    float bg_rad;
    const float* __restrict__ table;
    const float* __restrict__ s_w0;
    const float* __restrict__ s_w1;
    float b1_0;
    int side, jl, gbase;
    __device__ __forceinline__ float at(const float p[3]) const {
        // compiler barrier: without it the 144 weight values a lane reads from LDS per evaluation are hoisted out of the
        // trip loop into registers (256 VGPRs + 44 AGPRs, one wave per SIMD) -- and a kernel running BESIDE this one
        // (ls2fm.stage: the render's gather pass) loses more than half of its waves on every SIMD this kernel sits on
        __asm__ volatile("" ::: "memory");
        return group_sdf(lv, fc, bg_sdf, bg_rad, table, s_w0, s_w1, b1_0, p, jl, gbase);
    }
    __device__ __forceinline__ float other_t(float t, int) const { return __shfl_xor(t, 16, 64); }
    __device__ __forceinline__ bool start_unfinished(bool unf) const { return __shfl((int)unf, (threadIdx.x & 63) & ~16, 64); }
    __device__ __forceinline__ bool writer() const { return jl == 0; }
};

// ---- one wave per end, a 128-thread workgroup per ray (side = wave); lane j holds hidden unit j's weights in registers.  The ends
// exchange t through LDS with ONE barrier per trip: slot k & 1 is rewritten two barriers later
struct WaveEnds {
    const LevelSet& lv;
    const FieldC& fc;
    int bg_sdf;
    float bg_rad;
    const float* __restrict__ table;
    const float (&w)[kInMax + 1];
    float w1_me, b1_0;
    float (*s_t)[2];
    int side, lane;
    __device__ __forceinline__ float at(const float p[3]) const { return wave_sdf(lv, fc, bg_sdf, bg_rad, table, w, w1_me, b1_0, p, lane); }
    __device__ __forceinline__ float other_t(float t, int k) const {
        if (lane == 0) s_t[k & 1][side] = t;
        __syncthreads();
        return s_t[k & 1][side ^ 1];
    }
    __device__ __forceinline__ bool start_unfinished(bool unf) const { return unf; }      // asked of the start end's wave only
    __device__ __forceinline__ bool writer() const { return lane == 0; }
};

template <class Ends>
__device__ __forceinline__ void trace_begin(const Ends& ends, const RayGeom& g, TraceEnd& e) {
    e.t = ends.side ? g.t_far : g.t_near;
#pragma unroll
    for (int a = 0; a < 3; ++a) e.p[a] = g.o[a] + e.t * g.d[a];
    e.sdf = ends.at(e.p);
    e.raw = e.sdf;
    e.unf = false;
}

__device__ __forceinline__ void trace_mask(TraceEnd& e, float thr, int k) {
    if (fabsf(e.sdf) <= thr) e.sdf = 0.f;                                 // (1) converged values are zeroed
    const bool m = fabsf(e.sdf) > thr;
    e.unf = k == 0 ? m : (e.unf && m);                                    // (2)
}

// -> the end moved
__device__ __forceinline__ bool trace_step(TraceEnd& e, float far) {
    const float t_before = e.t;
    e.t = e.t + e.sdf;                                                    // (4) both ends step with '+', clamp to far
    if (e.t > far) e.t = far;
    return e.t != t_before;
}

// also_finished: evaluate a finished end too (the caller: a start end that moved, where the track's values are wanted)
template <class Ends>
__device__ __forceinline__ void trace_refresh(const Ends& ends, const RayGeom& g, TraceEnd& e, bool also_finished) {
#pragma unroll
    for (int a = 0; a < 3; ++a) e.p[a] = g.o[a] + e.t * g.d[a];
    if (e.unf || also_finished) {                                         // (6) uniform over the lanes that evaluate one end
        e.raw = ends.at(e.p);
        if (e.unf) e.sdf = e.raw;
    }
}

template <class Ends>
__device__ __forceinline__ void trace_cross(const Ends& ends, TraceEnd& e, int k) {
    const float t_other = ends.other_t(e.t, k);
    const float t_s = ends.side ? t_other : e.t, t_e = ends.side ? e.t : t_other;
    e.unf = e.unf && (t_s < t_e);                                         // (7) crossed ends drop out
}

// track point k of ray r: the start end's point and, where wanted, the field's value there
__device__ __forceinline__ void store_track_point(const TraceEnd& e, int64_t r, int iters_max, int k, float* __restrict__ track,
                                                  float* __restrict__ track_sdf) {
#pragma unroll
    for (int a = 0; a < 3; ++a) track[(r * (iters_max + 1) + k) * 3 + a] = e.p[a];
    if (track_sdf) track_sdf[r * (iters_max + 1) + k] = e.raw;
}

}  // namespace
