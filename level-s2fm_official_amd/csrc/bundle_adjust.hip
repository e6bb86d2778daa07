// The CLASSICAL bundle adjustment of the reference's ablation path (pipelines/BA_Trad.py:86-130, `BA.run_ba` behind
// Ablate_config.ba_trad): explicit 3-D points and se(3) poses as the parameters, no field.  Per iteration
//      pose_v = se3_to_SE3(r_v, t_v) ;  x_c = R x + t ;  u = K x_c ;  uv = u_xy / (u_z + 1e-6) ;  err = || uv - key point ||
//      reproj = 0.5 mean(2 log(1 + err^2 / 4)) + 0.5 mean(err)   over ALL observations (no SDF mask, no finite mask)
//      w = reproj > thresh ? w_hi : w_lo                          (the reference's `.item()` decision: a device-side select here)
//      backward of w reproj ;  Adam over {rotations, translations, points} with their own rates ;  ExponentialLR on all three
// As torch ops that is a few dozen tiny kernels, their autograd mirror, three Adam groups and a host read per iteration -- launch-
// and sync-bound.  Here an iteration is TWO plain launches and a whole loop is one C call with no host read inside:
//   ba_residual_kernel  one workgroup per view: exponential (wave 0), per observation the projection (reproject_point.h: the
//                       arithmetic of the BA re-projection term), its gradient w.r.t. the point -> g_obs[i] and w.r.t. the pose,
//                       summed over the view in a fixed order; fp64 partial sums {robust, err} of the view; then the gradient
//                       w.r.t. the view's se(3) parameters through se3_exp_bwd (se3_exp.h).  All for weight 1.
//   ba_update_kernel    every workgroup finishes the loss from the per-view partials (fp64, view order) and selects the weight --
//                       the gradient is linear in it, so it is applied here --; one thread per point sums the gradients of the
//                       point's observations in LIST order through a point -> observations CSR (built once per loop by
//                       ls2fm_bundle_adjust_prepare) and takes the Adam step (adam_element.h); 6 V more threads step the poses.
// No floating-point atomics anywhere: two runs on the same inputs give the same bits.  A point no picked view observes has no
// gradient: it is not touched and its moments stay zero (torch's Adam with a zero gradient leaves both as they are).
// The learning-rate dependent scalars of every iteration are formed on the host as torch forms them (adam.hip's header) from the
// caller's step count: the rates by ExponentialLR's chained multiplication from step 0, so a loop split over several calls steps
// exactly as one call does.
#include "adam_element.h"
#include "ba_index.h"
#include "reproject_point.h"
#include "se3_exp.h"
#include "workspace.h"

namespace {

using ba_index::sizes_ok;

constexpr int kBaThreads = 256;
constexpr int32_t kBaMagic = 0x42415431;           // "BAT1": the workspace was filled by ls2fm_bundle_adjust_prepare for these sizes

struct BaWs {                  // the index arrays: ba_index.h
    int32_t* header;           // [8]: magic, n_views, n_points, n_obs
    double* partial;           // [V][2]: sum robust, sum err of the view
    float* d_se3;              // [V][6]: gradient w.r.t. the se(3) parameters for weight 1
    float* g_obs;              // [n][3]: gradient of observation i w.r.t. its point for weight 1
    int32_t* view_start;       // [V + 1]
    int32_t* obs_point;        // [n]
    int32_t* point_start;      // [P + 1]
    int32_t* point_obs;        // [n]: observations of point p in list order
    int64_t bytes;
};

BaWs ba_layout(void* base, int64_t V, int64_t P, int64_t n) {
    Workspace ws(base, 16);
    BaWs w;
    w.header = ws.take<int32_t>(8);
    w.partial = ws.take<double>(2 * V);
    w.d_se3 = ws.take<float>(6 * V);
    w.g_obs = ws.take<float>(3 * n);
    w.view_start = ws.take<int32_t>(V + 1);
    w.obs_point = ws.take<int32_t>(n);
    w.point_start = ws.take<int32_t>(P + 1);
    w.point_obs = ws.take<int32_t>(n);
    w.bytes = (int64_t)ws.bytes();
    return w;
}

__device__ __forceinline__ bool header_ok(const BaWs& w, int V, int P, int n) {
    return w.header[0] == kBaMagic && w.header[1] == V && w.header[2] == P && w.header[3] == n;
}

// grid: V workgroups.  `last`: this is the call's last iteration -- the state that enters it is copied out (what BA_Trad writes
// back after its loop: BA_Trad.py:124-127)
__global__ void __launch_bounds__(kBaThreads)
ba_residual_kernel(const float* __restrict__ se3, const float* __restrict__ pts, const float* __restrict__ obs_uv, Camera3 K, BaWs w,
                   int V, int P, int n, int last, float* __restrict__ se3_enter, float* __restrict__ pts_enter) {
    const int v = blockIdx.x, tid = threadIdx.x;
    __shared__ float s_pose[12], s_dpose[12];
    __shared__ double s_redd[kBaThreads][2];
    __shared__ float s_red[kBaThreads][12];
    if (!header_ok(w, V, P, n)) return;
    if (tid < 64) {                                  // the first wave: the exponential is a wave-wide job (se3_series)
        float pose[12];
        se3_exp(se3 + 6 * v, pose);
        if (tid == 0)
            for (int q = 0; q < 12; ++q) s_pose[q] = pose[q];
    }
    if (last) {
        if (tid < 6) se3_enter[6 * v + tid] = se3[6 * v + tid];
        for (int64_t q = (int64_t)v * kBaThreads + tid; q < 3 * (int64_t)P; q += (int64_t)V * kBaThreads) pts_enter[q] = pts[q];
    }
    __syncthreads();
    const float g = 0.5f / (float)n;                 // d reproj / d (sum robust) = d reproj / d (sum err)
    double sums[2] = {0.0, 0.0};
    float acc[12];
#pragma unroll
    for (int q = 0; q < 12; ++q) acc[q] = 0.f;
    for (int i = w.view_start[v] + tid; i < w.view_start[v + 1]; i += kBaThreads) {
        const float* __restrict__ x = pts + 3 * (int64_t)w.obs_point[i];
        const Obs o = project(x, s_pose, K, obs_uv + 2 * (int64_t)i, nullptr, 0.f);
        sums[0] += (double)(2.0f * logf(1.0f + o.err * o.err / 4.0f));
        sums[1] += (double)o.err;
        float dx[3] = {0.f, 0.f, 0.f};
        if (o.err > 0.f) {                           // norm backward at 0: zero (torch)
            // d err: 1 from the plain mean, err / (1 + err^2 / 4) from the robust one
            const float d_err = g * (1.0f + o.err / (1.0f + o.err * o.err / 4.0f));
            const float de0 = d_err * o.e[0] / o.err, de1 = d_err * o.e[1] / o.err;
            const float du[3] = {de0 * o.inv, de1 * o.inv, -(de0 * o.u[0] + de1 * o.u[1]) * o.inv * o.inv};
            float dxc[3];
#pragma unroll
            for (int b = 0; b < 3; ++b) dxc[b] = fmaf(K.k[6 + b], du[2], fmaf(K.k[3 + b], du[1], K.k[b] * du[0]));      // K^T du
#pragma unroll
            for (int b = 0; b < 3; ++b) dx[b] = fmaf(s_pose[8 + b], dxc[2], fmaf(s_pose[4 + b], dxc[1], s_pose[b] * dxc[0]));   // R^T
#pragma unroll
            for (int a = 0; a < 3; ++a) {
#pragma unroll
                for (int b = 0; b < 3; ++b) acc[4 * a + b] = fmaf(dxc[a], x[b], acc[4 * a + b]);
                acc[4 * a + 3] += dxc[a];
            }
        }
#pragma unroll
        for (int b = 0; b < 3; ++b) w.g_obs[3 * (int64_t)i + b] = dx[b];
    }
    s_redd[tid][0] = sums[0]; s_redd[tid][1] = sums[1];
#pragma unroll
    for (int q = 0; q < 12; ++q) s_red[tid][q] = acc[q];
    __syncthreads();
    if (tid < 12) {
        float t = 0.f;
        for (int k = 0; k < kBaThreads; ++k) t += s_red[k][tid];
        s_dpose[tid] = t;
    } else if (tid >= 64 && tid < 66) {              // (another wave: the two fp64 sums run beside the twelve fp32 ones)
        double t = 0.0;
        for (int k = 0; k < kBaThreads; ++k) t += s_redd[k][tid - 64];
        w.partial[2 * v + tid - 64] = t;
    }
    __syncthreads();
    if (tid < 64) {
        float d[6];
        se3_exp_bwd(se3 + 6 * v, s_dpose, d);
        if (tid == 0)
            for (int q = 0; q < 6; ++q) w.d_se3[6 * v + q] = d[q];
    }
}

struct BaStep { AdamHyper rot, trans, xyz; float thresh, w_lo, w_hi; };

// grid: ceil((P + 6 V) / 256) workgroups: thread = point, then pose element
__global__ void __launch_bounds__(kBaThreads)
ba_update_kernel(float* __restrict__ se3, float* __restrict__ pts, float* __restrict__ m_se3, float* __restrict__ v_se3,
                 float* __restrict__ m_pts, float* __restrict__ v_pts, BaWs w, int V, int P, int n, BaStep st, float* __restrict__ log_row) {
    const int tid = threadIdx.x;
    __shared__ float s_w;
    if (!header_ok(w, V, P, n)) {                    // an unprepared workspace: nothing moves, the log says so
        if (blockIdx.x == 0 && tid < 3) log_row[tid] = __builtin_nanf("");
        return;
    }
    if (tid == 0) {
        double t0 = 0.0, t1 = 0.0;
        for (int v = 0; v < V; ++v) { t0 += w.partial[2 * v]; t1 += w.partial[2 * v + 1]; }
        const float cnt = (float)n;
        const float reproj = 0.5f * (float)t0 / cnt + 0.5f * (float)t1 / cnt;
        const float wt = reproj > st.thresh ? st.w_hi : st.w_lo;
        s_w = wt;
        if (blockIdx.x == 0) { log_row[0] = reproj; log_row[1] = wt; log_row[2] = (float)t1 / cnt; }
    }
    __syncthreads();
    const float wt = s_w;
    const int64_t idx = (int64_t)blockIdx.x * kBaThreads + tid;
    if (idx < P) {
        const int a = w.point_start[idx], b = w.point_start[idx + 1];
        if (a == b) return;                          // no picked view observes it: no gradient, no step
        float g[3] = {0.f, 0.f, 0.f};
        for (int k = a; k < b; ++k) {
            const int64_t i = w.point_obs[k];
#pragma unroll
            for (int c = 0; c < 3; ++c) g[c] += w.g_obs[3 * i + c];
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const int64_t q = 3 * idx + c;
            float p = pts[q], m = m_pts[q], vv = v_pts[q];
            adam_one(p, wt * g[c], m, vv, st.xyz);
            pts[q] = p; m_pts[q] = m; v_pts[q] = vv;
        }
    } else if (idx < (int64_t)P + 6 * (int64_t)V) {
        const int q = (int)(idx - P);
        float p = se3[q], m = m_se3[q], vv = v_se3[q];
        adam_one(p, wt * w.d_se3[q], m, vv, (q % 6) < 3 ? st.rot : st.trans);
        se3[q] = p; m_se3[q] = m; v_se3[q] = vv;
    }
}

}  // namespace

extern "C" int64_t ls2fm_bundle_adjust_workspace_bytes(int32_t n_views, int64_t n_points, int64_t n_obs) {
    if (!sizes_ok(n_views, n_points, n_obs)) return LS2FM_ERR_INVALID_ARGUMENT;
    return ba_layout(nullptr, n_views, n_points, n_obs).bytes;
}

extern "C" int ls2fm_bundle_adjust_prepare(const int32_t* view_start, int32_t n_views, const int32_t* obs_point, int64_t n_obs,
                                           int64_t n_points, void* workspace, void* stream_) {
    LS2FM_CHECK_ARG(sizes_ok(n_views, n_points, n_obs) && view_start && obs_point);
    if (!workspace) return LS2FM_ERR_WORKSPACE;
    hipStream_t stream = (hipStream_t)stream_;
    const int64_t V = n_views, P = n_points, n = n_obs;
    const BaWs w = ba_layout(workspace, V, P, n);
    ba_index::Index ix;
    if (!ba_index::clear_header(w.header, stream)) { (void)hipGetLastError(); return LS2FM_ERR_LAUNCH; }
    const int st = ba_index::build(view_start, obs_point, V, P, n, stream, &ix);
    if (st != LS2FM_OK) return st;
    const int32_t header[8] = {kBaMagic, (int32_t)V, (int32_t)P, (int32_t)n, 0, 0, 0, 0};
    if (!ba_index::upload(w.view_start, ix.view_start, stream) || !ba_index::upload(w.obs_point, ix.obs_point, stream) ||
        !ba_index::upload(w.point_start, ix.point_start, stream) || !ba_index::upload(w.point_obs, ix.point_obs, stream) ||
        hipMemcpyAsync(w.header, header, sizeof(header), hipMemcpyHostToDevice, stream) != hipSuccess ||
        hipStreamSynchronize(stream) != hipSuccess)                                  // (the host vectors die with this frame)
        { (void)hipGetLastError(); return LS2FM_ERR_LAUNCH; }
    return LS2FM_OK;
}

extern "C" int ls2fm_bundle_adjust_run(float* se3, float* points, const float* obs_uv, int32_t n_views, int64_t n_points, int64_t n_obs,
                                       const float* intrinsic_host, double lr_rot, double lr_trans, double lr_points, double gamma,
                                       float w_lo, float w_hi, float thresh, float* m_se3, float* v_se3, float* m_points, float* v_points,
                                       int64_t steps_done, int32_t n_iters, float* log, float* se3_entering_last,
                                       float* points_entering_last, void* workspace, void* stream_) {
    LS2FM_CHECK_ARG(sizes_ok(n_views, n_points, n_obs) && n_iters >= 1 && steps_done >= 0 && steps_done <= (1 << 24));
    LS2FM_CHECK_ARG(se3 && points && obs_uv && m_se3 && v_se3 && m_points && v_points && log && se3_entering_last && points_entering_last);
    LS2FM_CHECK_ARG(lr_rot >= 0.0 && lr_trans >= 0.0 && lr_points >= 0.0 && gamma > 0.0);
    Camera3 K;
    LS2FM_CHECK_ARG(load_intrinsic(intrinsic_host, &K));
    if (!workspace) return LS2FM_ERR_WORKSPACE;
    hipStream_t stream = (hipStream_t)stream_;
    // the scalars of an iteration come from the HOST's step count: a captured graph would replay one iteration's scalars for ever
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(stream, &cap) != hipSuccess) { (void)hipGetLastError(); return LS2FM_ERR_LAUNCH; }
    if (cap != hipStreamCaptureStatusNone) return LS2FM_ERR_UNSUPPORTED;
    const int V = n_views, P = (int)n_points, n = (int)n_obs;
    const BaWs w = ba_layout(workspace, V, P, n);
    const double beta1 = 0.9, beta2 = 0.999;                                         // torch.optim.Adam's defaults (BA_Trad.py:60)
    AdamHyper h;
    h.step_size = 0.f; h.bc2_sqrt = 1.f;
    h.w1 = (float)(1.0 - beta1); h.beta2 = (float)beta2; h.one_minus_beta2 = (float)(1.0 - beta2);
    h.eps = 1e-8f; h.weight_decay = 0.f;
    double lr[3] = {lr_rot, lr_trans, lr_points};
    for (int64_t s = 0; s < steps_done; ++s)                                         // ExponentialLR: one multiplication per step
        for (int q = 0; q < 3; ++q) lr[q] *= gamma;
    const unsigned blocks = (unsigned)(((int64_t)P + 6 * (int64_t)V + kBaThreads - 1) / kBaThreads);
    for (int32_t it = 0; it < n_iters; ++it) {
        const double step = (double)(steps_done + it + 1);
        const double bc1 = 1.0 - pow(beta1, step), bc2 = 1.0 - pow(beta2, step);
        BaStep st;
        st.rot = st.trans = st.xyz = h;
        st.rot.step_size = (float)(lr[0] / bc1); st.trans.step_size = (float)(lr[1] / bc1); st.xyz.step_size = (float)(lr[2] / bc1);
        st.rot.bc2_sqrt = st.trans.bc2_sqrt = st.xyz.bc2_sqrt = (float)sqrt(bc2);
        st.thresh = thresh; st.w_lo = w_lo; st.w_hi = w_hi;
        ba_residual_kernel<<<(unsigned)V, kBaThreads, 0, stream>>>(se3, points, obs_uv, K, w, V, P, n, it == n_iters - 1 ? 1 : 0,
                                                                  se3_entering_last, points_entering_last);
        ba_update_kernel<<<blocks, kBaThreads, 0, stream>>>(se3, points, m_se3, v_se3, m_points, v_points, w, V, P, n, st, log + 3 * (int64_t)it);
        for (int q = 0; q < 3; ++q) lr[q] *= gamma;
    }
    return ls2fm_launch_status();
}
