// Feature tracks and multi-view triangulation: what the reference keeps in Point3DSet / Camera.idx2d_to_3d one point and one view
// pair at a time (pipelines/Registration_Trad.py:183-215, Initialization_Trad.py:97), for all views in one call.  include/ls2fm.h
// states the rules; tests/tracks_restate.py repeats them in numpy.  All geometry in fp64.
//
// ls2fm_track_labels: the union-find of mesh_components.hip (union_find.h) over key points joined by matches.
//   tl_init     labels[i] = i, status = 0
//   tl_hook     per edge: range and same-image checks (a bad edge sets a status bit and joins nothing), unite
//   tl_flatten  labels[i] = root(i)
//
// ls2fm_triangulate_tracks: hypothesise-and-verify over the pairs of a track's first 64 observations, then local optimisation.
//   tt_prepare  ONE workgroup: camera centres, the exclusive prefix sum of the tracks' pair counts (hyp_start [T + 1], int64) and
//               best_key = 0.  A track of n observations has m (m - 1) / 2 hypotheses, m = min(n, 64): 1 for n = 2, 2016 for n >= 64.
//   tt_hyp      one LANE per (track, pair), all tracks' pairs numbered in one flat range from hyp_start (as ransac.h's score_kernel
//               numbers its tiles): most tracks have 2 to 5 observations, and a wave per track would idle almost all of its lanes.
//               A lane finds its track by bisection, triangulates its pair, scores the point over all of the track's observations
//               and joins the track's 64-bit integer max.  The 2016 pairs of a long track spread over eight workgroups.  The grid
//               is sized from n_obs (a track of n has at most 31.5 n pairs) and strides over the range, whose true length is read on
//               the device: nothing comes back to the host.
//   tt_final    EIGHT lanes per track, eight tracks per 64-thread workgroup: the winner's point again, the local optimisation, the
//               mask and the acceptance.  A track's observations are dealt to its eight lanes; counts are wave ballots, sums the
//               fixed butterfly 4, 2, 1.  Every loop runs a wave-uniform number of rounds (the longest track of the wave, the
//               others predicated off), so every shuffle, ballot and barrier is reached by all 64 lanes.
#include "pose_math.h"
#include "track_geom.h"
#include "union_find.h"
#include "workspace.h"

#include <algorithm>
#include <cfloat>
#include <cmath>

namespace {

using namespace pose_math;
using namespace track_geom;
using namespace union_find;

constexpr int kThreads = 256;
constexpr int kScanThreads = 1024;
constexpr int kSub = 8;                        // lanes per track in tt_final
constexpr int kFinalThreads = 64;
constexpr int kFinalTracks = kFinalThreads / kSub;
constexpr int kLoIters = 10;
constexpr unsigned kMaxHypBlocks = 4096;       // ~5 x the 768 workgroups of tt_hyp the device holds at once; beyond it lanes stride

static_assert(kHypObs == 64 && kFinalThreads == 64, "tt_final keeps a track's first 64 inliers and runs as one wave");

// ------------------------------------------------------------------------------------------------------------------ labels
__global__ void __launch_bounds__(kThreads)
tl_init(int32_t* __restrict__ labels, uint32_t n_nodes, int32_t* __restrict__ status) {
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    if (i < n_nodes) labels[i] = (int32_t)i;
    if (status && i == 0) *status = 0;
}

// the image of node x: the last v with image_start[v] <= x
__device__ __forceinline__ int image_of(const int32_t* __restrict__ image_start, int n_images, int32_t x) {
    int lo = 0, hi = n_images;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (image_start[mid] <= x) lo = mid; else hi = mid;
    }
    return lo;
}

__global__ void __launch_bounds__(kThreads)
tl_hook(const int32_t* __restrict__ image_start, int n_images, uint32_t n_nodes, const int32_t* __restrict__ edges, uint32_t n_edges,
        int32_t* labels, int32_t* status) {
    const uint32_t e = blockIdx.x * kThreads + threadIdx.x;
    if (e >= n_edges) return;
    const int32_t a = edges[2 * (int64_t)e], b = edges[2 * (int64_t)e + 1];
    int bad = 0;
    if ((uint32_t)a >= n_nodes || (uint32_t)b >= n_nodes) bad = LS2FM_TRACK_EDGE_RANGE;
    else if (image_of(image_start, n_images, a) == image_of(image_start, n_images, b)) bad = LS2FM_TRACK_EDGE_IMAGE;
    if (bad) {
        if (status) atomicOr(status, bad);
        return;
    }
    unite(labels, a, b);
}

__global__ void __launch_bounds__(kThreads)
tl_flatten(int32_t* labels, uint32_t n_nodes) {
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= n_nodes) return;
    const int32_t r = find_root(labels, (int32_t)i);
    __hip_atomic_store(labels + i, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ----------------------------------------------------------------------------------------------------------- triangulation
struct TtIn {                   // the call's arrays
    const double* poses;        // [V][12]
    const double* intr;         // [V][4]
    const int32_t* track_start; // [T + 1]
    const int32_t* obs_view;    // [n_obs]
    const double* obs_uv;       // [n_obs][2]
    int32_t V;
    int64_t T, n_obs;
    double thr2, min_angle;
};

struct TtWs {
    double* centre;                 // [V][3]
    long long* hyp_start;           // [T + 1]
    unsigned long long* best_key;   // [T]
};

size_t tt_layout(int64_t T, int32_t V, char* base, TtWs* w) {
    Workspace ws(base, 256);
    double* c = ws.take<double>((size_t)V * 3);
    long long* h = ws.take<long long>((size_t)T + 1);
    unsigned long long* k = ws.take<unsigned long long>((size_t)(T ? T : 1));
    if (w) *w = {c, h, k};
    return ws.bytes();
}

// the extent of track t (track_geom.h): false (n = 0) when it is not inside [0, n_obs], runs backwards or is too long
__device__ __forceinline__ bool track_extent(const TtIn& in, int64_t t, int64_t& s0, int& n) {
    return track_geom::track_extent(in.track_start, in.n_obs, t, s0, n);
}

__global__ void __launch_bounds__(kScanThreads)
tt_prepare(TtIn in, TtWs w, int32_t* __restrict__ status) {
    __shared__ int s_status;
    const int tid = threadIdx.x;
    if (tid == 0) s_status = 0;
    __syncthreads();
    for (int v = tid; v < in.V; v += kScanThreads) {
        centre_of(in.poses + 12 * (int64_t)v, w.centre + 3 * (int64_t)v);
    }
    long long carry = 0;
    for (int64_t base = 0; base < in.T; base += kScanThreads) {
        const int64_t t = base + tid;
        long long c = 0;
        if (t < in.T) {
            int64_t s0;
            int n;
            if (!track_extent(in, t, s0, n)) atomicOr(&s_status, LS2FM_TRACK_BAD_START);
            c = pair_count(n);
            w.best_key[t] = 0ull;
        }
        long long sum;
        const long long e = block_exclusive_scan<kScanThreads>(c, sum);
        if (t < in.T) w.hyp_start[t] = carry + e;
        carry += sum;
    }
    if (tid == 0) w.hyp_start[in.T] = carry;
    __syncthreads();
    if (status && tid == 0) *status = s_status;
}

// observation o against X: the squared pixel error and the depth; false for a view outside [0, V)
__device__ __forceinline__ bool observe(const TtIn& in, int64_t o, const double (&X)[3], double& e2, double& depth) {
    const int32_t v = in.obs_view[o];
    if ((uint32_t)v >= (uint32_t)in.V) return false;
    pixel_error(in.poses + 12 * (int64_t)v, in.intr + 4 * (int64_t)v, in.obs_uv[2 * o], in.obs_uv[2 * o + 1], X, e2, depth);
    return true;
}

__device__ __forceinline__ bool is_inlier(const TtIn& in, int64_t o, const double (&X)[3]) {
    double e2, z;
    return observe(in, o, X, e2, z) && z > DBL_EPSILON && e2 <= in.thr2;         // a NaN error is not an inlier
}

// the hypothesis of observations oi, oj of one track: false when dropped
__device__ __forceinline__ bool hypothesis(const TtIn& in, const double* __restrict__ centre, int64_t oi, int64_t oj, double (&X)[3]) {
    const int32_t vi = in.obs_view[oi], vj = in.obs_view[oj];
    if ((uint32_t)vi >= (uint32_t)in.V || (uint32_t)vj >= (uint32_t)in.V) return false;
    const double* __restrict__ Pi = in.poses + 12 * (int64_t)vi;
    const double* __restrict__ Pj = in.poses + 12 * (int64_t)vj;
    const double* __restrict__ Ki = in.intr + 4 * (int64_t)vi;
    const double* __restrict__ Kj = in.intr + 4 * (int64_t)vj;
    const double xi = (in.obs_uv[2 * oi] - Ki[2]) / Ki[0], yi = (in.obs_uv[2 * oi + 1] - Ki[3]) / Ki[1];
    const double xj = (in.obs_uv[2 * oj] - Kj[2]) / Kj[0], yj = (in.obs_uv[2 * oj + 1] - Kj[3]) / Kj[1];
    double h[4];
    triangulate_dlt(Pi, Pj, xi, yi, xj, yj, h);
    X[0] = h[0] / h[3];
    X[1] = h[1] / h[3];
    X[2] = h[2] / h[3];
    if (!(is_finite(X[0]) && is_finite(X[1]) && is_finite(X[2]))) return false;
    const double zi = ((Pi[8] * X[0] + Pi[9] * X[1]) + Pi[10] * X[2]) + Pi[11];
    const double zj = ((Pj[8] * X[0] + Pj[9] * X[1]) + Pj[10] * X[2]) + Pj[11];
    if (!(zi > DBL_EPSILON && zj > DBL_EPSILON)) return false;
    return tri_angle_of(centre, vi, vj, X) >= in.min_angle;
}

__global__ void __launch_bounds__(kThreads)
tt_hyp(TtIn in, TtWs w, unsigned n_blocks) {
    const long long total = w.hyp_start[in.T];
    for (long long h = (long long)blockIdx.x * kThreads + threadIdx.x; h < total; h += (long long)n_blocks * kThreads) {
        const int64_t t = last_not_above(w.hyp_start, in.T, h);      // tracks without a pair share an offset
        int64_t s0;
        int n;
        track_extent(in, t, s0, n);
        const int q = (int)(h - w.hyp_start[t]);
        if (q >= pair_count(n)) continue;
        int i, j;
        pair_of(q, n < kHypObs ? n : kHypObs, i, j);
        double X[3];
        if (!hypothesis(in, w.centre, s0 + i, s0 + j, X)) continue;
        unsigned count = 0;
        for (int k = 0; k < n; ++k) count += is_inlier(in, s0 + k, X) ? 1u : 0u;
        if (count == 0) continue;
        const unsigned long long key = ((unsigned long long)count << 32) | (unsigned long long)(0xFFFFFFFFu - (uint32_t)q);
        __hip_atomic_fetch_max(w.best_key + t, key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// ballot of `flag` over the wave, cut to the eight lanes of this lane's track
__device__ __forceinline__ unsigned group_bits(bool flag, int grp) {
    return (unsigned)((__ballot(flag) >> (grp * kSub)) & 0xFFull);
}

__device__ __forceinline__ double group_sum(double x) {           // the butterfly 4, 2, 1 over the eight lanes of a track
#pragma unroll
    for (int o = kSub / 2; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
    return x;
}

__global__ void __launch_bounds__(kFinalThreads)
tt_final(TtIn in, TtWs w, double* __restrict__ Xout, uint8_t* __restrict__ inliers, int32_t* __restrict__ num_inliers,
         int32_t* __restrict__ success, double* __restrict__ tri_angle, double* __restrict__ mean_error_px,
         int32_t* __restrict__ best_pair, int32_t* status) {
    __shared__ int32_t s_view[kFinalTracks][kHypObs];          // the views of each track's first 64 inliers
    const int tid = threadIdx.x, sub = tid & (kSub - 1), grp = tid / kSub;
    const int64_t t = (int64_t)blockIdx.x * kFinalTracks + grp;
    const bool have = t < in.T;
    int64_t s0 = 0;
    int n = 0;
    if (have) track_extent(in, t, s0, n);
    // rounds of eight observations: as many as the longest track of the wave needs
    const int rounds = wave_max((n + kSub - 1) / kSub);
    const unsigned long long bk = have ? w.best_key[t] : 0ull;
    const int q = bk ? (int)(0xFFFFFFFFu - (uint32_t)(bk & 0xFFFFFFFFull)) : -1;
    double X[3] = {0.0, 0.0, 0.0};
    bool live = false;                                          // the track has a point (the same on its eight lanes)
    if (q >= 0 && q < pair_count(n)) {
        int i, j;
        pair_of(q, n < kHypObs ? n : kHypObs, i, j);
        live = hypothesis(in, w.centre, s0 + i, s0 + j, X);     // the winner's point again: the same operations, the same bits
    }
    int cur = 0;
    for (int r = 0; r < rounds; ++r) {
        const int k = r * kSub + sub;
        cur += __popc(group_bits(live && k < n && is_inlier(in, s0 + k, X), grp));
    }
    bool act = live && cur >= 2;
    for (int it = 0; it < kLoIters; ++it) {
        if (__ballot(act) == 0ull) break;                       // wave-uniform
        double a[10];
#pragma unroll
        for (int e = 0; e < 10; ++e) a[e] = 0.0;
        for (int r = 0; r < rounds; ++r) {
            const int k = r * kSub + sub;
            if (!(act && k < n && is_inlier(in, s0 + k, X))) continue;
            const int64_t o = s0 + k;
            const int32_t v = in.obs_view[o];
            const double* __restrict__ P = in.poses + 12 * (int64_t)v;
            const double* __restrict__ K = in.intr + 4 * (int64_t)v;
            const double xy[2] = {(in.obs_uv[2 * o] - K[2]) / K[0], (in.obs_uv[2 * o + 1] - K[3]) / K[1]};
#pragma unroll
            for (int row = 0; row < 2; ++row) {
                double d[4];
#pragma unroll
                for (int c = 0; c < 4; ++c) d[c] = xy[row] * P[8 + c] - P[4 * row + c];
                const double inv = 1.0 / sqrt(((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]) + d[3] * d[3]);
#pragma unroll
                for (int c = 0; c < 4; ++c) d[c] = d[c] * inv;
#pragma unroll
                for (int c = 0; c < 4; ++c)
#pragma unroll
                    for (int e = c; e < 4; ++e) a[sidx4(c, e)] += d[c] * d[e];
            }
        }
#pragma unroll
        for (int e = 0; e < 10; ++e) a[e] = group_sum(a[e]);
        double Vv[4][4];
        jacobi4(a, Vv);
        int best = 0;
#pragma unroll
        for (int k = 1; k < 4; ++k) best = a[sidx4(k, k)] < a[sidx4(best, best)] ? k : best;
        double Xn[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const double num = best == 0 ? Vv[0][c] : (best == 1 ? Vv[1][c] : (best == 2 ? Vv[2][c] : Vv[3][c]));
            const double den = best == 0 ? Vv[0][3] : (best == 1 ? Vv[1][3] : (best == 2 ? Vv[2][3] : Vv[3][3]));
            Xn[c] = num / den;
        }
        const bool fin = is_finite(Xn[0]) && is_finite(Xn[1]) && is_finite(Xn[2]);
        int cnt = 0, chg = 0;
        for (int r = 0; r < rounds; ++r) {
            const int k = r * kSub + sub;
            const bool on = act && fin && k < n;
            const bool now = on && is_inlier(in, s0 + k, Xn);
            const bool was = on && is_inlier(in, s0 + k, X);
            cnt += __popc(group_bits(now, grp));
            chg += __popc(group_bits(now != was, grp));
        }
        if (act) {
            if (!fin || cnt < cur) {
                act = false;
            } else {
                X[0] = Xn[0];
                X[1] = Xn[1];
                X[2] = Xn[2];
                cur = cnt;
                act = chg != 0;
            }
        }
    }
    // the mask, the mean error and the views of the first 64 inliers in observation order
    double err = 0.0;
    int seen = 0;
    for (int r = 0; r < rounds; ++r) {
        const int k = r * kSub + sub;
        bool inl = false;
        if (k < n) {
            double e2, z;
            // every observation of a well-formed track passes here once: the place to report a view that does not exist
            if (status && (uint32_t)in.obs_view[s0 + k] >= (uint32_t)in.V) atomicOr(status, LS2FM_TRACK_BAD_VIEW);
            inl = live && observe(in, s0 + k, X, e2, z) && z > DBL_EPSILON && e2 <= in.thr2;
            inliers[s0 + k] = inl ? 1 : 0;
            if (inl) err += sqrt(e2);
        }
        const unsigned bits = group_bits(inl, grp);
        const int rank = seen + __popc(bits & ((1u << sub) - 1u));
        if (inl && rank < kHypObs) s_view[grp][rank] = in.obs_view[s0 + k];
        seen += __popc(bits);
    }
    err = group_sum(err);
    __syncthreads();
    const int m = seen < kHypObs ? seen : kHypObs;             // seen = cur: the inliers of the final X
    double ang = 0.0;
    for (int i = 0; i + 1 < m; ++i)
        for (int j = i + 1 + sub; j < m; j += kSub) {
            const double a = tri_angle_of(w.centre, s_view[grp][i], s_view[grp][j], X);
            ang = a > ang ? a : ang;                            // a NaN angle (X on a centre) does not count
        }
#pragma unroll
    for (int o = kSub / 2; o > 0; o >>= 1) {
        const double y = __shfl_xor(ang, o, 64);
        ang = y > ang ? y : ang;
    }
    if (!have || sub != 0) return;
    const bool ok = cur >= 2 && ang >= in.min_angle;
#pragma unroll
    for (int c = 0; c < 3; ++c) Xout[3 * t + c] = ok ? X[c] : 0.0;
    num_inliers[t] = cur;
    success[t] = ok ? 1 : 0;
    tri_angle[t] = ang;
    mean_error_px[t] = cur > 0 ? err / (double)cur : 0.0;
    best_pair[t] = live ? q : -1;
}

bool below_2_31(int64_t x) { return x >= 0 && x < ((int64_t)1 << 31); }

unsigned blocks_of(int64_t n) { return (unsigned)((n + kThreads - 1) / kThreads); }

}  // namespace

extern "C" int ls2fm_track_labels(const int32_t* image_start, int32_t n_images, int64_t n_nodes, const int32_t* edges, int64_t n_edges,
                                  int32_t* labels, int32_t* status, void* stream) {
    LS2FM_CHECK_ARG(image_start && n_images >= 1 && below_2_31(n_nodes) && below_2_31(n_edges));
    LS2FM_CHECK_ARG((edges || n_edges == 0) && (labels || n_nodes == 0));
    hipStream_t s = (hipStream_t)stream;
    const uint32_t nn = (uint32_t)n_nodes, ne = (uint32_t)n_edges;
    tl_init<<<nn ? blocks_of(nn) : 1u, kThreads, 0, s>>>(labels, nn, status);
    if (ne) {
        tl_hook<<<blocks_of(ne), kThreads, 0, s>>>(image_start, n_images, nn, edges, ne, labels, status);
        if (nn) tl_flatten<<<blocks_of(nn), kThreads, 0, s>>>(labels, nn);
    }
    return ls2fm_launch_status();
}

extern "C" int64_t ls2fm_triangulate_tracks_workspace_bytes(int64_t n_tracks, int32_t n_views) {
    if (!below_2_31(n_tracks) || n_views < 1) return (int64_t)LS2FM_ERR_INVALID_ARGUMENT;
    return (int64_t)tt_layout(n_tracks, n_views, nullptr, nullptr);
}

extern "C" int ls2fm_triangulate_tracks(const double* poses, const double* intrinsics, int32_t n_views, const int32_t* track_start,
                                        int64_t n_tracks, const int32_t* obs_view, const double* obs_uv, int64_t n_obs,
                                        double max_error_px, double min_tri_angle_deg, double* X, uint8_t* inliers, int32_t* num_inliers,
                                        int32_t* success, double* tri_angle, double* mean_error_px, int32_t* best_pair, int32_t* status,
                                        void* workspace, void* stream) {
    LS2FM_CHECK_ARG(poses && intrinsics && n_views >= 1 && track_start && below_2_31(n_tracks) && below_2_31(n_obs));
    LS2FM_CHECK_ARG(std::isfinite(max_error_px) && max_error_px > 0.0 && min_tri_angle_deg >= 0.0 && min_tri_angle_deg <= 90.0);
    LS2FM_CHECK_ARG((obs_view && obs_uv && inliers) || n_obs == 0);
    LS2FM_CHECK_ARG((X && num_inliers && success && tri_angle && mean_error_px && best_pair) || n_tracks == 0);
    if (!workspace) return LS2FM_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    TtWs w;
    tt_layout(n_tracks, n_views, (char*)workspace, &w);
    const TtIn in = {poses, intrinsics, track_start, obs_view, obs_uv, n_views, n_tracks, n_obs, max_error_px * max_error_px,
                     min_tri_angle_deg * (kPi / 180.0)};
    if (n_obs && hipMemsetAsync(inliers, 0, (size_t)n_obs, s) != hipSuccess) return ls2fm_launch_status();
    tt_prepare<<<1, kScanThreads, 0, s>>>(in, w, status);
    if (n_tracks == 0) return ls2fm_launch_status();
    // a track of n observations has at most 31.5 n pairs: the grid covers that bound, capped (short tracks have ~1 pair per
    // observation, so the bound is ~30 x their need: an uncapped grid would be mostly workgroups that read the total and leave)
    const int64_t bound = (n_obs * (kHypObs - 1) + 1) / 2;
    const unsigned hyp_blocks = (unsigned)std::min<int64_t>(std::max<int64_t>((bound + kThreads - 1) / kThreads, 1), kMaxHypBlocks);
    tt_hyp<<<hyp_blocks, kThreads, 0, s>>>(in, w, hyp_blocks);
    tt_final<<<(unsigned)((n_tracks + kFinalTracks - 1) / kFinalTracks), kFinalThreads, 0, s>>>(in, w, X, inliers, num_inliers, success,
                                                                                                tri_angle, mean_error_px, best_pair, status);
    return ls2fm_launch_status();
}
