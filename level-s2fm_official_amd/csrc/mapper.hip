// The incremental mapper's two per-step device calls: the next-view score and the upkeep of the observation and point state.
// include/ls2fm.h states the rules ("The incremental mapper's two per-step device calls"); tests/mapper_restate.py repeats them in
// numpy.  The track table and the geometry are those of tracks.hip (track_geom.h).  No floating-point atomic anywhere: lanes meet
// in 64-bit integer OR / MAX and in stores of one value, so every output is independent of the launch order.
//
// ls2fm_view_scores: a 4096-bit occupancy mask per view (64 rows of 64 bits: row cy, bit cx).
//   vs_seen    one LANE per observation: its track by bisection over track_start (kept for vs_mark), the checks of the table, and
//              seen[t] = 1 when the observation is a kept one of a registered view of a valid track (every writer stores 1).
//   vs_mark    one lane per observation: a counting observation adds 1 to its view's num_visible (integer) and ORs its cell's bit
//              into the view's mask row.
//   vs_reduce  one WAVE per view, lane r holding row r: level 6 is the popcount; each coarser level ORs the mask with itself
//              shifted by half a cell (columns) and exchanged with the lane half a cell away (rows), and counts the bits at the
//              cells' corners on the lanes at the cells' corners.  The wave's sum is an integer butterfly.
//
// ls2fm_update_observations:
//   uo_keep    one lane per observation: kept or not (the pixel error and depth of X[t] in the observation's view); one lane per
//              view: its centre.  The divisions, the only costly part per observation, are spread flat: a track of 4096
//              observations is 4096 lanes of 16 workgroups.
//   uo_rank    EIGHT lanes per track, eight tracks per 64-thread workgroup, as tt_final: ballots count the kept observations and
//              pack the views of the first 64 of them to the front of the track's own extent of kept_view.  A round is one byte
//              load and a ballot; the rounds are wave-uniform (the longest track of the wave).
//   uo_scan    ONE workgroup: the exclusive prefix sum of the tracks' pair counts (pair_start [T + 1], int64) and best = 0.
//   uo_angle   one lane per (track, pair) over the flat range, as tt_hyp: its track by bisection, the pair's angle, joined into
//              the track's best by a 64-bit integer max of the angle's bits.  The 2016 pairs of a long track spread over eight
//              workgroups.
//   uo_final   one lane per track: tri_angle and track_valid.
#include "track_geom.h"
#include "workspace.h"

#include <algorithm>
#include <cfloat>
#include <cmath>

namespace {

using namespace track_geom;

constexpr int kThreads = 256;
constexpr int kScanThreads = 1024;
constexpr int kSub = 8;                        // lanes per track in uo_rank
constexpr int kRankThreads = 64;
constexpr int kRankTracks = kRankThreads / kSub;
constexpr unsigned kMaxPairBlocks = 4096;      // as tt_hyp: beyond it lanes stride
constexpr int kGrid = 64;                      // cells per side of the finest level
constexpr int kLevels = 6;

static_assert(kGrid == 64 && (1 << kLevels) == kGrid, "a view's mask is 64 rows of 64 bits, one row per lane of a wave");

bool below_2_31(int64_t x) { return x >= 0 && x < ((int64_t)1 << 31); }

unsigned blocks_of(int64_t n) { return (unsigned)((n + kThreads - 1) / kThreads); }

// the track of observation o, -1 when no well-formed extent holds it
__device__ __forceinline__ int64_t track_of_obs(const int32_t* __restrict__ track_start, int64_t T, int64_t n_obs, int64_t o) {
    if (T == 0) return -1;
    const int64_t t = last_not_above(track_start, T, (long long)o);
    int64_t s0;
    int n;
    if (!track_extent(track_start, n_obs, t, s0, n)) return -1;
    return o >= s0 && o < s0 + n ? t : -1;
}

// ------------------------------------------------------------------------------------------------------------- view scores
struct VsWs {
    unsigned long long* mask;   // [V][64]
    uint8_t* seen;              // [T]
    int32_t* obs_track;         // [n_obs]
};

size_t vs_layout(int64_t T, int32_t V, int64_t n_obs, char* base, VsWs* w, size_t* zeroed) {
    Workspace ws(base, 256);
    unsigned long long* m = ws.take<unsigned long long>((size_t)V * kGrid);
    uint8_t* s = ws.take<uint8_t>((size_t)(T ? T : 1));
    if (zeroed) *zeroed = ws.bytes();                           // mask and seen start at zero
    int32_t* t = ws.take<int32_t>((size_t)(n_obs ? n_obs : 1));
    if (w) *w = {m, s, t};
    return ws.bytes();
}

__global__ void __launch_bounds__(kThreads)
vs_seen(const int32_t* __restrict__ track_start, int64_t T, const int32_t* __restrict__ obs_view, int64_t n_obs,
        const uint8_t* __restrict__ obs_keep, const uint8_t* __restrict__ track_valid, const uint8_t* __restrict__ registered, int32_t V,
        VsWs w, int32_t* status) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i < T) {
        int64_t s0;
        int n;
        if (!track_extent(track_start, n_obs, i, s0, n) && status) atomicOr(status, LS2FM_MAPPER_BAD_START);
    }
    if (i >= n_obs) return;
    int64_t t = track_of_obs(track_start, T, n_obs, i);
    const int32_t v = obs_view[i];
    if ((uint32_t)v >= (uint32_t)V) {
        if (status) atomicOr(status, LS2FM_MAPPER_BAD_VIEW);
        t = -1;
    }
    w.obs_track[i] = (int32_t)t;
    if (t >= 0 && track_valid[t] && obs_keep[i] && registered[v]) w.seen[t] = 1;
}

__device__ __forceinline__ int cell_of(double x, double size) {
    const double q = (64.0 * x) / size;
    return q >= 63.0 ? 63 : (q > 0.0 ? (int)floor(q) : 0);       // a NaN q: cell 0
}

__global__ void __launch_bounds__(kThreads)
vs_mark(const int32_t* __restrict__ obs_view, const double* __restrict__ obs_uv, int64_t n_obs, const uint8_t* __restrict__ registered,
        const double* __restrict__ image_size, VsWs w, int32_t* __restrict__ num_visible, int32_t* status) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n_obs) return;
    const int32_t t = w.obs_track[i];
    if (t < 0 || !w.seen[t]) return;
    const int32_t v = obs_view[i];                              // in range: obs_track is -1 otherwise
    if (registered[v]) return;
    atomicAdd(num_visible + v, 1);
    const double x = obs_uv[2 * i], y = obs_uv[2 * i + 1];
    if (!(fabs(x) <= DBL_MAX && fabs(y) <= DBL_MAX)) {          // NaN or infinite
        if (status) atomicOr(status, LS2FM_MAPPER_BAD_PIXEL);
        return;
    }
    const int cx = cell_of(x, image_size[2 * (int64_t)v]), cy = cell_of(y, image_size[2 * (int64_t)v + 1]);
    atomicOr(w.mask + (int64_t)v * kGrid + cy, 1ull << cx);
}

__global__ void __launch_bounds__(kThreads)
vs_reduce(VsWs w, const uint8_t* __restrict__ registered, int32_t V, int64_t* __restrict__ score) {
    const int lane = threadIdx.x & 63;
    const int32_t v = (int32_t)(blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6));       // wave-uniform
    if (v >= V) return;
    unsigned long long m = w.mask[(int64_t)v * kGrid + lane];
    // the bits at the corners of the cells of 2^s columns
    constexpr unsigned long long corner[kLevels] = {~0ull, 0x5555555555555555ull, 0x1111111111111111ull, 0x0101010101010101ull,
                                                    0x0001000100010001ull, 0x0000000100000001ull};
    long long sum = 0;
#pragma unroll
    for (int s = 0; s < kLevels; ++s) {                          // level l = 6 - s: cells of 2^s x 2^s finest cells
        if (s > 0) {
            const int half = 1 << (s - 1);
            m |= m >> half;
            m |= __shfl_xor(m, half, 64);
        }
        const int cells = (lane & ((1 << s) - 1)) == 0 ? __popcll(m & corner[s]) : 0;
        sum += (long long)cells << (2 * (kLevels - s));
    }
    sum = wave_sum(sum);
    if (lane == 0) score[v] = registered[v] ? 0ll : sum;
}

// ------------------------------------------------------------------------------------------------------ update observations
struct UoIn {
    const double* poses;        // [V][12]
    const double* intr;         // [V][4]
    const uint8_t* registered;  // [V]
    const int32_t* track_start; // [T + 1]
    const int32_t* obs_view;    // [n_obs]
    const double* obs_uv;       // [n_obs][2]
    const double* X;            // [T][3]
    const uint8_t* valid_in;    // [T]
    int32_t V;
    int64_t T, n_obs;
    double thr2, min_angle;
};

struct UoWs {
    double* centre;                 // [V][3]
    long long* pair_start;          // [T + 1]
    unsigned long long* best;       // [T]: the bits of the largest angle
    int32_t* kept_view;             // [n_obs]: per track, the views of its first 64 kept observations at the front of its extent
};

size_t uo_layout(int64_t T, int32_t V, int64_t n_obs, char* base, UoWs* w) {
    Workspace ws(base, 256);
    double* c = ws.take<double>((size_t)V * 3);
    long long* h = ws.take<long long>((size_t)T + 1);
    unsigned long long* k = ws.take<unsigned long long>((size_t)(T ? T : 1));
    int32_t* kv = ws.take<int32_t>((size_t)(n_obs ? n_obs : 1));
    if (w) *w = {c, h, k, kv};
    return ws.bytes();
}

__global__ void __launch_bounds__(kThreads)
uo_keep(UoIn in, UoWs w, uint8_t* __restrict__ obs_keep, int32_t* status) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i < in.V) centre_of(in.poses + 12 * i, w.centre + 3 * i);       // of a view that is not registered: never used
    if (i >= in.n_obs) return;
    const int64_t t = track_of_obs(in.track_start, in.T, in.n_obs, i);
    const int32_t v = in.obs_view[i];
    const bool view_ok = (uint32_t)v < (uint32_t)in.V;
    if (!view_ok && status) atomicOr(status, LS2FM_MAPPER_BAD_VIEW);
    bool keep = false;
    if (t >= 0 && view_ok && in.valid_in[t] && in.registered[v]) {
        const double X[3] = {in.X[3 * t], in.X[3 * t + 1], in.X[3 * t + 2]};
        double e2, z;
        pixel_error(in.poses + 12 * (int64_t)v, in.intr + 4 * (int64_t)v, in.obs_uv[2 * i], in.obs_uv[2 * i + 1], X, e2, z);
        keep = z > DBL_EPSILON && e2 <= in.thr2;                       // a NaN keeps nothing
    }
    obs_keep[i] = keep ? 1 : 0;
}

__global__ void __launch_bounds__(kRankThreads)
uo_rank(UoIn in, UoWs w, const uint8_t* __restrict__ obs_keep, int32_t* __restrict__ num_kept, int32_t* status) {
    const int tid = threadIdx.x, sub = tid & (kSub - 1), grp = tid / kSub;
    const int64_t t = (int64_t)blockIdx.x * kRankTracks + grp;
    const bool have = t < in.T;
    int64_t s0 = 0;
    int n = 0;
    if (have && !track_extent(in.track_start, in.n_obs, t, s0, n) && status && sub == 0) atomicOr(status, LS2FM_MAPPER_BAD_START);
    const int rounds = wave_max((n + kSub - 1) / kSub);         // as many as the longest track of the wave needs
    int seen = 0;
    for (int r = 0; r < rounds; ++r) {
        const int k = r * kSub + sub;
        const bool kept = k < n && obs_keep[s0 + k] != 0;
        const unsigned bits = (unsigned)((__ballot(kept) >> (grp * kSub)) & 0xFFull);
        const int rank = seen + __popc(bits & ((1u << sub) - 1u));
        // rank <= k: inside the track's own extent, and at or before every observation still to be read (obs_keep, not kept_view)
        if (kept && rank < kHypObs) w.kept_view[s0 + rank] = in.obs_view[s0 + k];
        seen += __popc(bits);
    }
    if (have && sub == 0) num_kept[t] = seen;
}

__global__ void __launch_bounds__(kScanThreads)
uo_scan(int64_t T, const int32_t* __restrict__ num_kept, UoWs w) {
    const int tid = threadIdx.x;
    long long carry = 0;
    for (int64_t base = 0; base < T; base += kScanThreads) {
        const int64_t t = base + tid;
        long long c = 0;
        if (t < T) {
            c = pair_count(num_kept[t]);
            w.best[t] = 0ull;
        }
        long long sum;
        const long long e = block_exclusive_scan<kScanThreads>(c, sum);
        if (t < T) w.pair_start[t] = carry + e;
        carry += sum;
    }
    if (tid == 0) w.pair_start[T] = carry;
}

__global__ void __launch_bounds__(kThreads)
uo_angle(UoIn in, UoWs w, const int32_t* __restrict__ num_kept, unsigned n_blocks) {
    const long long total = w.pair_start[in.T];
    for (long long h = (long long)blockIdx.x * kThreads + threadIdx.x; h < total; h += (long long)n_blocks * kThreads) {
        const int64_t t = last_not_above(w.pair_start, in.T, h);       // tracks without a pair share an offset
        const int kept = num_kept[t];
        const int q = (int)(h - w.pair_start[t]);
        if (q >= pair_count(kept)) continue;
        int i, j;
        pair_of(q, kept < kHypObs ? kept : kHypObs, i, j);
        const int64_t s0 = in.track_start[t];                          // well formed: the track has kept observations
        const double X[3] = {in.X[3 * t], in.X[3 * t + 1], in.X[3 * t + 2]};
        const double a = tri_angle_of(w.centre, w.kept_view[s0 + i], w.kept_view[s0 + j], X);
        if (!(a >= 0.0)) continue;                                     // a NaN angle (X on a centre) does not count
        __hip_atomic_fetch_max(w.best + t, (unsigned long long)__double_as_longlong(a), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

__global__ void __launch_bounds__(kThreads)
uo_final(int64_t T, double min_angle, UoWs w, const int32_t* __restrict__ num_kept, uint8_t* __restrict__ track_valid,
         double* __restrict__ tri_angle) {
    const int64_t t = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (t >= T) return;
    const double a = __longlong_as_double((long long)w.best[t]);
    tri_angle[t] = a;
    track_valid[t] = num_kept[t] >= 2 && a >= min_angle ? 1 : 0;
}

}  // namespace

extern "C" int64_t ls2fm_view_scores_workspace_bytes(int64_t n_tracks, int32_t n_views, int64_t n_obs) {
    if (!below_2_31(n_tracks) || !below_2_31(n_obs) || n_views < 1) return (int64_t)LS2FM_ERR_INVALID_ARGUMENT;
    return (int64_t)vs_layout(n_tracks, n_views, n_obs, nullptr, nullptr, nullptr);
}

extern "C" int ls2fm_view_scores(const int32_t* track_start, int64_t n_tracks, const int32_t* obs_view, const double* obs_uv, int64_t n_obs,
                                 const uint8_t* obs_keep, const uint8_t* track_valid, const uint8_t* registered, const double* image_size,
                                 int32_t n_views, int64_t* score, int32_t* num_visible, int32_t* status, void* workspace, void* stream) {
    LS2FM_CHECK_ARG(track_start && below_2_31(n_tracks) && below_2_31(n_obs) && n_views >= 1);
    LS2FM_CHECK_ARG(registered && image_size && score && num_visible && (track_valid || n_tracks == 0));
    LS2FM_CHECK_ARG((obs_view && obs_uv && obs_keep) || n_obs == 0);
    if (!workspace) return LS2FM_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    VsWs w;
    size_t zeroed;
    vs_layout(n_tracks, n_views, n_obs, (char*)workspace, &w, &zeroed);
    if (hipMemsetAsync(workspace, 0, zeroed, s) != hipSuccess) return ls2fm_launch_status();
    if (hipMemsetAsync(num_visible, 0, (size_t)n_views * sizeof(int32_t), s) != hipSuccess) return ls2fm_launch_status();
    if (status && hipMemsetAsync(status, 0, sizeof(int32_t), s) != hipSuccess) return ls2fm_launch_status();
    const int64_t lanes = std::max(n_obs, n_tracks);
    if (lanes)
        vs_seen<<<blocks_of(lanes), kThreads, 0, s>>>(track_start, n_tracks, obs_view, n_obs, obs_keep, track_valid, registered, n_views, w,
                                                      status);
    if (n_obs) vs_mark<<<blocks_of(n_obs), kThreads, 0, s>>>(obs_view, obs_uv, n_obs, registered, image_size, w, num_visible, status);
    vs_reduce<<<(unsigned)((n_views + kThreads / 64 - 1) / (kThreads / 64)), kThreads, 0, s>>>(w, registered, n_views, score);
    return ls2fm_launch_status();
}

extern "C" int64_t ls2fm_update_observations_workspace_bytes(int64_t n_tracks, int32_t n_views, int64_t n_obs) {
    if (!below_2_31(n_tracks) || !below_2_31(n_obs) || n_views < 1) return (int64_t)LS2FM_ERR_INVALID_ARGUMENT;
    return (int64_t)uo_layout(n_tracks, n_views, n_obs, nullptr, nullptr);
}

extern "C" int ls2fm_update_observations(const double* poses, const double* intrinsics, const uint8_t* registered, int32_t n_views,
                                         const int32_t* track_start, int64_t n_tracks, const int32_t* obs_view, const double* obs_uv,
                                         int64_t n_obs, const double* X, const uint8_t* track_valid_in, double max_error_px,
                                         double min_tri_angle_deg, uint8_t* obs_keep, uint8_t* track_valid, int32_t* num_kept,
                                         double* tri_angle, int32_t* status, void* workspace, void* stream) {
    LS2FM_CHECK_ARG(poses && intrinsics && registered && n_views >= 1 && track_start && below_2_31(n_tracks) && below_2_31(n_obs));
    LS2FM_CHECK_ARG(std::isfinite(max_error_px) && max_error_px > 0.0 && min_tri_angle_deg >= 0.0 && min_tri_angle_deg <= 90.0);
    LS2FM_CHECK_ARG((obs_view && obs_uv && obs_keep) || n_obs == 0);
    LS2FM_CHECK_ARG((X && track_valid_in && track_valid && num_kept && tri_angle) || n_tracks == 0);
    if (!workspace) return LS2FM_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    UoWs w;
    uo_layout(n_tracks, n_views, n_obs, (char*)workspace, &w);
    const UoIn in = {poses, intrinsics, registered, track_start, obs_view, obs_uv, X, track_valid_in, n_views, n_tracks, n_obs,
                     max_error_px * max_error_px, min_tri_angle_deg * (kPi / 180.0)};
    if (status && hipMemsetAsync(status, 0, sizeof(int32_t), s) != hipSuccess) return ls2fm_launch_status();
    uo_keep<<<blocks_of(std::max<int64_t>(n_obs, n_views)), kThreads, 0, s>>>(in, w, obs_keep, status);
    if (n_tracks == 0) return ls2fm_launch_status();
    uo_rank<<<(unsigned)((n_tracks + kRankTracks - 1) / kRankTracks), kRankThreads, 0, s>>>(in, w, obs_keep, num_kept, status);
    uo_scan<<<1, kScanThreads, 0, s>>>(n_tracks, num_kept, w);
    // a track of n kept observations has at most 31.5 n pairs: the grid covers that bound, capped, and strides (as tt_hyp)
    const int64_t bound = (n_obs * (kHypObs - 1) + 1) / 2;
    const unsigned pair_blocks = (unsigned)std::min<int64_t>(std::max<int64_t>((bound + kThreads - 1) / kThreads, 1), kMaxPairBlocks);
    uo_angle<<<pair_blocks, kThreads, 0, s>>>(in, w, num_kept, pair_blocks);
    uo_final<<<blocks_of(n_tracks), kThreads, 0, s>>>(n_tracks, in.min_angle, w, num_kept, track_valid, tri_angle);
    return ls2fm_launch_status();
}
