// Batched LO-RANSAC rounds shared by absolute_pose.hip (P3P), relative_pose.hip (five-point) and two_view.hip (seven-point,
// four-point): the sample stream, the stopping rule, the workspace, the hypothesis, scoring and selection kernels, the fixed-order
// reductions and the host loop.  include/ls2fm.h states the rules.  Correspondences are SORTED BY GROUP (a view or a view pair;
// group g owns [group_start[g], group_start[g + 1])).
//
//   per round (host loop, run_rounds; a group stops once its trial count reaches the stopping rule's N):
//     hyp_kernel<M>      one thread per (group, trial): M::kSample distinct indices from the SplitMix64 stream (sample_distinct),
//                        the model's minimal solver, <= M::kMaxSol hypotheses of M::kHypWords fp64 words
//     score_kernel<M>    (1024-correspondence tile of some group, 16-trial block): inlier counts of the block's 16 x kMaxSol
//                        hypotheses over the tile, wave ballots + integer atomics (exact, order-independent).  The tiles of all
//                        groups are numbered in one flat range (per-group tile offsets from the host), so a group of n gets
//                        ceil(n / 1024) x 64 workgroups -- 128 for n = 2000, 65 536 for n = 2^20 -- whatever the other groups' sizes
//     select_kernel<M>   one workgroup per group: the best (count, lowest trial * kMaxSol + slot) as a 64-bit max, the stopping rule
//
// A model M is a struct of compile-time values and static device functions (no virtual calls, no run-time branch on the model):
//     kSample, kMaxSol, kHypWords   sample size, hypotheses per trial, fp64 words per hypothesis
//     kMinGroup                     groups with fewer correspondences are never active
//     Input                         the kernel arguments of the model (device pointers, the threshold), passed by value
//     Ctx   context(in, g)          per-group constants, built once per workgroup
//     Point load(in, ctx, i)        correspondence i, loaded once per thread per tile slot
//     bool  inlier(H, pt, ctx)      one hypothesis against one correspondence
//     kHypThreads, kHypLdsWords     workgroup size of hyp_kernel<M> (it divides kRound) and the fp64 words of LDS per thread that the
//                                   minimal solver indexes at run time (word k of thread j at column[k * kHypThreads], 0: none)
//     hypotheses(in, ctx, s0, id, column, emit)   load the sample s0 + id[0 .. kSample) and run the minimal solver: emit(slot, H)
//                                   per kept hypothesis, slot < kMaxSol
#pragma once

#include "ls2fm_device.h"
#include "lm_math.h"
#include "workspace.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>

namespace ransac {

constexpr int kRound = LS2FM_POSE_ROUND;      // trials per group per round (1024)
constexpr int kScoreThreads = 256;
constexpr int kScorePts = 4;                   // correspondences per thread of a scoring tile
constexpr int kScoreTile = kScoreThreads * kScorePts;
constexpr int kScoreTrials = 16;               // trials per scoring workgroup
constexpr int kGroupThreads = 256;             // initialisation / selection workgroups
constexpr int kMaxDraws = 64;

static_assert(kRound % kScoreTrials == 0, "round shape");

// ----------------------------------------------------------------------------------------------------------- sample stream
__host__ __device__ __forceinline__ uint64_t splitmix64(uint64_t x) {
    uint64_t z = x + 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

__host__ __device__ __forceinline__ uint64_t trial_key(uint64_t seed, uint64_t trial) { return splitmix64(seed ^ splitmix64(trial)); }

__host__ __device__ __forceinline__ int64_t draw_index(uint64_t key, int k, int64_t n) {
    return (int64_t)(((splitmix64(key + (uint64_t)k) >> 32) * (uint64_t)n) >> 32);
}

// the first K distinct draws of the key's stream, in draw order, within kMaxDraws draws; false (unfilled entries -1) otherwise
template <int K>
__device__ __forceinline__ bool sample_distinct(uint64_t key, int64_t n, int64_t (&id)[K]) {
#pragma unroll
    for (int q = 0; q < K; ++q) id[q] = -1;
    int got = 0;
    for (int k = 0; k < kMaxDraws && got < K; ++k) {
        const int64_t d = draw_index(key, k, n);
        bool fresh = true;
#pragma unroll
        for (int q = 0; q < K; ++q) fresh = fresh && id[q] != d;
#pragma unroll
        for (int q = 0; q < K; ++q) id[q] = (fresh && q == got) ? d : id[q];
        got += fresh ? 1 : 0;
    }
    return got == K;
}

// -------------------------------------------------------------------------------------------------------------- stopping
template <int K>
__host__ __device__ inline int64_t num_trials(double eps, double confidence, int64_t min_t, int64_t max_t) {
    if (eps <= 0.0) return max_t;
    if (eps >= 1.0) return min_t;
    double pk = eps;                               // eps^K, multiplied left to right
#pragma unroll
    for (int i = 1; i < K; ++i) pk = pk * eps;
    const double den = log(1.0 - pk);
    if (den >= 0.0) return max_t;
    const double n = ceil(log(1.0 - confidence) / den);
    if (n >= (double)max_t) return min_t > max_t ? min_t : max_t;
    const int64_t ni = (int64_t)n;
    return ni < min_t ? min_t : ni;
}

// ------------------------------------------------------------------------------------------------------------- workspace
struct Ws {                     // workspace layout (ls2fm_*_pose_workspace_bytes); G groups, S = kMaxSol, W = kHypWords
    double* hyp;                // [G][kRound][S][W]
    int32_t* valid;             // [G][kRound]   bit s: slot s holds a hypothesis
    int32_t* counts;            // [G][kRound][S]
    unsigned long long* best_key;   // [G]
    double* best;               // [G][W]
    int32_t* trials;            // [G]
    int32_t* active;            // [G]
    int32_t* n_active;          // [1]
    int32_t* tile_off;          // [G + 1]   first scoring tile of group g (ceil(n_g / kScoreTile) tiles each)
};

template <class M>
inline size_t ws_layout(int32_t G, char* base, Ws* w) {
    Workspace ws(base, 256);
    Ws t;
    t.hyp = ws.take<double>((size_t)G * kRound * M::kMaxSol * M::kHypWords);
    t.valid = ws.take<int32_t>((size_t)G * kRound);
    t.counts = ws.take<int32_t>((size_t)G * kRound * M::kMaxSol);
    t.best_key = ws.take<unsigned long long>((size_t)G);
    t.best = ws.take<double>((size_t)G * M::kHypWords);
    t.trials = ws.take<int32_t>((size_t)G);
    t.active = ws.take<int32_t>((size_t)G);
    t.n_active = ws.take<int32_t>(1);
    t.tile_off = ws.take<int32_t>((size_t)G + 1);
    if (w) *w = t;
    return ws.bytes();
}

// --------------------------------------------------------------------------------------------------------------- kernels
template <class M>
__global__ void __launch_bounds__(kGroupThreads)
init_kernel(const int32_t* __restrict__ gs, int32_t G, Ws w) {
    const int g = blockIdx.x * kGroupThreads + threadIdx.x;
    if (g >= G) return;
    w.best_key[g] = 0ull;
    w.trials[g] = 0;
    w.active[g] = (gs[g + 1] - gs[g]) >= M::kMinGroup ? 1 : 0;
}

template <class M>
__global__ void __launch_bounds__(M::kHypThreads)
hyp_kernel(typename M::Input in, const int32_t* __restrict__ gs, uint64_t seed, Ws w) {
    constexpr int kS = M::kMaxSol, kW = M::kHypWords, kT = M::kHypThreads, kLds = M::kHypLdsWords * kT;
    static_assert(kRound % kT == 0, "round shape");
    const int g = blockIdx.y;
    if (!w.active[g]) return;
    __shared__ double s_buf[kLds > 0 ? kLds : 1];          // unused, and dropped by the compiler, for a model without LDS words
    const int tl = blockIdx.x * kT + threadIdx.x;
    const int64_t slot = (int64_t)g * kRound + tl;
    int32_t* __restrict__ cnt = w.counts + kS * slot;
#pragma unroll
    for (int s = 0; s < kS; ++s) cnt[s] = 0;
    const int64_t s0 = gs[g], n = gs[g + 1] - s0;
    int64_t id[M::kSample];
    int mask = 0;
    if (sample_distinct(trial_key(seed, (uint64_t)(w.trials[g] + tl)), n, id)) {
        double* __restrict__ out = w.hyp + kS * kW * slot;
        M::hypotheses(in, M::context(in, g), s0, id, s_buf + threadIdx.x, [&](int s, const double* h) {
#pragma unroll
            for (int q = 0; q < kW; ++q) out[kW * s + q] = h[q];
            mask |= 1 << s;
        });
    }
    w.valid[slot] = mask;
}

template <class M>
__global__ void __launch_bounds__(kScoreThreads)
score_kernel(typename M::Input in, const int32_t* __restrict__ gs, int32_t G, Ws w) {
    // the group of this tile: the last g with tile_off[g] <= blockIdx.x (groups without a tile share its offset)
    const int32_t bx = (int32_t)blockIdx.x;
    int lo = 0, hi = G;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (w.tile_off[mid] <= bx) lo = mid; else hi = mid;
    }
    const int g = lo;
    if (!w.active[g]) return;
    const int64_t s0 = gs[g], n = gs[g + 1] - s0;
    const int64_t base = (int64_t)(bx - w.tile_off[g]) * kScoreTile;
    if (base >= n) return;
    constexpr int kS = M::kMaxSol, kW = M::kHypWords, kH = kS * kScoreTrials;
    __shared__ double s_h[kH][kW];
    __shared__ int s_valid[kScoreTrials];
    __shared__ int s_cnt[kH];
    const int tid = threadIdx.x, lane = tid & 63;
    const int64_t slot0 = (int64_t)g * kRound + (int64_t)blockIdx.y * kScoreTrials;
    for (int q = tid; q < kH * kW; q += kScoreThreads) s_h[q / kW][q % kW] = w.hyp[kS * kW * slot0 + q];
    if (tid < kScoreTrials) s_valid[tid] = w.valid[slot0 + tid];
    if (tid < kH) s_cnt[tid] = 0;
    const typename M::Ctx ctx = M::context(in, g);
    typename M::Point pt[kScorePts];
    bool live[kScorePts];
#pragma unroll
    for (int k = 0; k < kScorePts; ++k) {
        const int64_t j = base + tid + (int64_t)k * kScoreThreads;
        live[k] = j < n;
        pt[k] = M::load(in, ctx, s0 + (live[k] ? j : 0));
    }
    __syncthreads();
    for (int h = 0; h < kH; ++h) {
        if (!((s_valid[h / kS] >> (h % kS)) & 1)) continue;
        const double* H = s_h[h];
        int c = 0;
#pragma unroll
        for (int k = 0; k < kScorePts; ++k) {
            const bool in = M::inlier(H, pt[k], ctx);          // every lane evaluates it: no branch around the slots past the end
            c += __popcll(__ballot(live[k] && in));
        }
        if (lane == 0 && c) atomicAdd(&s_cnt[h], c);
    }
    __syncthreads();
    if (tid < kH && s_cnt[tid]) atomicAdd(&w.counts[kS * slot0 + tid], s_cnt[tid]);
}

template <class M>
__global__ void __launch_bounds__(kGroupThreads)
select_kernel(const int32_t* __restrict__ gs, double confidence, int64_t min_trials, int64_t max_trials, Ws w) {
    const int g = blockIdx.x;
    if (!w.active[g]) return;
    constexpr int kS = M::kMaxSol, kW = M::kHypWords;
    const int tid = threadIdx.x;
    __shared__ unsigned long long s_k[kGroupThreads / 64];
    const int32_t t0 = w.trials[g];
    unsigned long long best = 0ull;
    for (int c = tid; c < kS * kRound; c += kGroupThreads) {
        const int64_t slot = (int64_t)g * kRound + c / kS;
        const int s = c % kS;
        const int cnt = w.counts[kS * slot + s];
        if (cnt > 0 && ((w.valid[slot] >> s) & 1)) {
            const uint32_t idx = (uint32_t)(t0 + c / kS) * (uint32_t)kS + (uint32_t)s;
            const unsigned long long key = ((unsigned long long)(uint32_t)cnt << 32) | (unsigned long long)(0xFFFFFFFFu - idx);
            best = key > best ? key : best;
        }
    }
    best = wave_max(best);
    if ((tid & 63) == 0) s_k[tid >> 6] = best;
    __syncthreads();
    if (tid != 0) return;
    for (int q = 0; q < kGroupThreads / 64; ++q) best = s_k[q] > best ? s_k[q] : best;
    if (best > w.best_key[g]) {
        w.best_key[g] = best;
        const uint32_t idx = 0xFFFFFFFFu - (uint32_t)(best & 0xFFFFFFFFull);
        const int64_t slot = (int64_t)g * kRound + (int64_t)(idx / (uint32_t)kS - (uint32_t)t0);
        for (int q = 0; q < kW; ++q) w.best[kW * g + q] = w.hyp[kS * kW * slot + kW * (idx % (uint32_t)kS) + q];
    }
    const int32_t done = t0 + kRound;
    w.trials[g] = done;
    const double eps = (double)(w.best_key[g] >> 32) / (double)(gs[g + 1] - gs[g]);
    const bool on = done < num_trials<M::kSample>(eps, confidence, min_trials, max_trials);
    w.active[g] = on ? 1 : 0;
    if (on) atomicAdd(w.n_active, 1);
}

// the trial that a non-zero best_key names
template <class M>
__device__ __forceinline__ int32_t best_trial_of(unsigned long long best_key) {
    return (int32_t)((0xFFFFFFFFu - (uint32_t)(best_key & 0xFFFFFFFFull)) / (uint32_t)M::kMaxSol);
}

// ---------------------------------------------------------------------------------------------------- workgroup reductions
// (the fixed-order fp64 sum over a workgroup is wave_ops.h's block_sum)
__device__ __forceinline__ int block_count(int c, int* s_int) {     // exact integer sum over the workgroup
    __syncthreads();
    if (threadIdx.x == 0) *s_int = 0;
    __syncthreads();
    if (c) atomicAdd(s_int, c);
    __syncthreads();
    return *s_int;
}

// ------------------------------------------------------------------------------------------------------------------ host
inline bool opts_ok(const ls2fm_pose_ransac_opts* o) {       // all but the model's own rule for o->refine
    return o && o->max_error_px > 0.0 && std::isfinite(o->max_error_px) && o->confidence > 0.0 && o->confidence < 1.0 &&
           o->min_inlier_ratio >= 0.0 && o->min_inlier_ratio < 1.0 && o->min_num_trials >= 0 && o->max_num_trials >= 1 &&
           o->max_num_trials <= LS2FM_POSE_MAX_TRIALS && o->min_num_trials <= o->max_num_trials;
}

// The rounds of one call, after the entry's own argument checks: the workspace must be there; group_start [G + 1] (device) is copied
// to the host and checked (have_corr: the correspondence arrays and the mask are there, required once there is a correspondence),
// the tile offsets and the initial state are written, then rounds run until no group is active.  The call synchronises.
// *w: the workspace's arrays, for the entry's own kernels that follow a return of LS2FM_OK.
template <class M>
int run_rounds(const typename M::Input& in, const int32_t* group_start, int32_t G, bool have_corr, const ls2fm_pose_ransac_opts* opts,
               void* workspace, hipStream_t s, Ws* w) {
    if (!workspace) return LS2FM_ERR_WORKSPACE;
    // the groups' extents, on the host: the grid of the scoring pass and the argument checks
    int32_t* h_gs = (int32_t*)malloc(sizeof(int32_t) * ((size_t)G + 1));
    if (!h_gs) return LS2FM_ERR_LAUNCH;
    if (hipMemcpyAsync(h_gs, group_start, sizeof(int32_t) * ((size_t)G + 1), hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipStreamSynchronize(s) != hipSuccess) {
        free(h_gs);
        return ls2fm_launch_status();
    }
    // per-group scoring tile offsets, reusing the host copy (group_start[g] <= ... fits int32, so do the tile counts)
    int64_t max_n = 0;
    bool mono = h_gs[0] >= 0;
    int32_t tiles = 0;
    for (int g = 0; g < G; ++g) {
        mono = mono && h_gs[g + 1] >= h_gs[g];
        const int64_t ng = (int64_t)h_gs[g + 1] - h_gs[g];
        max_n = std::max<int64_t>(max_n, ng);
        h_gs[g] = tiles;
        tiles += mono ? (int32_t)((ng + kScoreTile - 1) / kScoreTile) : 0;
    }
    const int64_t total = h_gs[G];
    h_gs[G] = tiles;
    if (!(mono && (total == 0 || have_corr))) {
        free(h_gs);
        return LS2FM_ERR_INVALID_ARGUMENT;
    }
    ws_layout<M>(G, (char*)workspace, w);
    const bool copied = hipMemcpyAsync(w->tile_off, h_gs, sizeof(int32_t) * ((size_t)G + 1), hipMemcpyHostToDevice, s) == hipSuccess &&
                        hipStreamSynchronize(s) == hipSuccess;
    free(h_gs);
    if (!copied) return ls2fm_launch_status();
    // the trial cap, and min_num_trials above it lowered to it (the cap wins, as in COLMAP's RANSAC)
    const int64_t cap = num_trials<M::kSample>(opts->min_inlier_ratio, opts->confidence, 0, opts->max_num_trials);
    const int64_t min_trials = std::min<int64_t>(opts->min_num_trials, cap);
    init_kernel<M><<<(unsigned)((G + kGroupThreads - 1) / kGroupThreads), kGroupThreads, 0, s>>>(group_start, G, *w);
    int st = ls2fm_launch_status();
    if (st != LS2FM_OK) return st;
    const int64_t max_rounds = (cap + kRound - 1) / kRound;          // N <= cap: every group has stopped after these
    for (int64_t r = 0; max_n >= M::kMinGroup && r < max_rounds; ++r) {
        hyp_kernel<M><<<dim3(kRound / M::kHypThreads, (unsigned)G), M::kHypThreads, 0, s>>>(in, group_start, opts->seed, *w);
        score_kernel<M><<<dim3((unsigned)tiles, kRound / kScoreTrials), kScoreThreads, 0, s>>>(in, group_start, G, *w);
        if (hipMemsetAsync(w->n_active, 0, sizeof(int32_t), s) != hipSuccess) return ls2fm_launch_status();
        select_kernel<M><<<(unsigned)G, kGroupThreads, 0, s>>>(group_start, opts->confidence, min_trials, cap, *w);
        if ((st = ls2fm_launch_status()) != LS2FM_OK) return st;
        int32_t h_active = 0;
        if (hipMemcpyAsync(&h_active, w->n_active, sizeof(int32_t), hipMemcpyDeviceToHost, s) != hipSuccess ||
            hipStreamSynchronize(s) != hipSuccess)
            return ls2fm_launch_status();
        if (h_active == 0) break;
    }
    return LS2FM_OK;
}

}  // namespace ransac
