// Levenberg-Marquardt bundle adjustment with a Schur complement: explicit 3-D points and [R | t] poses of up to
// LS2FM_BA_LM_MAX_VIEWS picked views, one shared pinhole camera, all arithmetic fp64, no floating-point atomics, every sum in a
// fixed order (two runs give the same bits).  include/ls2fm.h states the rules; tests/ba_lm_restate.py repeats them in numpy.
//
// One iteration is six plain launches on the caller's stream; the host reads nothing inside a call:
//   balm_linearize  one workgroup per view.  First the DECISION on the previous iteration's candidate (every workgroup forms it from
//                   the same words -- the caller's state, the candidate's cost partials in view order, the maxima --, workgroup 0
//                   writes the log row and the iteration's record `it`); then r, w, J_c, J_p of every observation of the view at the
//                   selected state (the candidate when it was accepted, else the current one) into the workspace, and U_v, g_v and
//                   the view's cost by wave_ops.h's fixed-order block sum.
//   balm_points     one thread per point (+ V for the poses): commits the record to the caller's state, copies an accepted candidate
//                   into the caller's poses / points, then V_p, g_p over the point's observations in CSR order, the damped 3 x 3
//                   inverse by Cholesky and V_p*^-1 g_p.
//   balm_schur      one workgroup per view pair i <= j: threads stride over view i's observations, find the same point in view j
//                   by binary search in the point's CSR list (sorted by view position: the list is view-major and prepare refuses a
//                   point seen twice by a view), accumulate W_ip V_p*^-1 W_jp^T as J_ci^T (w_i w_j J_pi V_p*^-1 J_pj^T) J_cj -- the
//                   same 36 sums through a 2 x 2 core, 12 registers of operands instead of two 6 x 3 blocks -- and write S's (i, j)
//                   and (j, i) blocks; i = j adds U_i* and forms b_i.
//   balm_solve      ONE workgroup: the linearization's summary (max |g|, max |parameter|, the cost in view order), then a right-
//                   looking Cholesky of S by 6-column panels in the workspace (the panel in LDS, the trailing matrix in L2), the
//                   right-hand side carried along as one more row (forward substitution), back substitution.
//   balm_backsub    one thread per point and per view: delta_p, the candidate points and poses (lm_math.h's pose_update).
//   balm_cost       one workgroup per view: the candidate's cost partials.
// After the last iteration of a call the decision runs once more on its own (balm_linearize on one workgroup + balm_points, both
// told to stop after the decision), so the caller's poses, points and state are final when the call's launches end.
//
// THE CAMERA BLOCK (ls2fm_bundle_adjust_lm_run_camera): the kernels are instantiated over `bool CAMERA`; false is the pinhole loop above,
// word for word.  true reads the 12-word camera from the device, puts THE DISTORTION RULE (camera_model.h, fp64) between the
// division and the focal lengths, and borders the reduced system with the camera's 12 rows, two more panels of the same Cholesky:
//   balm_linearize  also J_k (2 x 12, masked and tied) of every observation into the workspace
//   balm_points     also Y_p = sum w J_k^T J_p over the point's list, and the accepted candidate camera into the caller's
//   balm_border     one more launch, one workgroup per (view, pair of camera words): the view's part of G, g_k, H_i and of the three
//                   sums that eliminate the points from the border, all as sums over the view's observations (F_o = w J_p V_p*^-1
//                   Y_p^T is shared by them) -- 76 sums per thread instead of the 500 a single pass would hold
//   balm_solve      adds the views' parts in view order into rows 6 V .. 6 V + 11, damps C as one block, V + 2 panels
//   balm_backsub    adds Y_p^T delta_k, forms the candidate camera;  balm_cost evaluates the candidate under it
#include "ba_index.h"
#include "camera_model.h"
#include "lm_math.h"
#include "render_common.h"
#include "workspace.h"

namespace {

using ba_index::sizes_ok;
using lm_math::pose_update;

constexpr int kT = 256;                              // threads of every workgroup here
constexpr int kMaxN = 6 * LS2FM_BA_LM_MAX_VIEWS;     // rows of the reduced system
constexpr int kK = LS2FM_CAMERA_PARAMS;              // the camera's words = its rows of the bordered system
constexpr int kMaxCamViews = LS2FM_BA_LM_MAX_VIEWS - 2;
constexpr int kBorderCols = 2, kBorderSums = 38 * kBorderCols;       // balm_border: camera words per workgroup, sums per thread
using Cam = camera_model::Camera<double>;
constexpr int32_t kMagic = 0x424c4d31;               // "BLM1": filled by ls2fm_bundle_adjust_lm_prepare for these sizes

// the record of an iteration = the caller's state [8]
enum { kLambda = 0, kDone = 1, kIters = 2, kCost = 3, kReason = 4, kGmax = 5, kDmax = 6, kAccepted = 7 };
// the summary words
enum { sGmax = 0, sPmax = 1, sCost = 2, sDmaxC = 3, sFailed = 4 };

struct Ws {                    // the index arrays: ba_index.h
    int32_t* header;           // [8]: magic, V, P, n
    double* it;                // [8]: the record of the running iteration (balm_linearize, workgroup 0)
    double* sum;               // [8]: balm_solve's summary
    double* cost_part;         // [V]: cost of the linearized state, per view
    double* gview;             // [V]: max |g_v|
    double* pview;             // [V]: max |t_v|, |X| of the view's points
    double* cand_part;         // [V]: cost of the candidate, per view
    double* gblk;              // [nb]: max |g_p| per workgroup of balm_points
    double* fblk;              // [nb]: a point's Cholesky met a non-positive pivot
    double* dblk;              // [nb]: max |delta_p| per workgroup of balm_backsub
    double* U;                 // [V][21]: upper triangle, row-major
    double* g;                 // [V][6]
    double* Jc;                // [n][2][6]
    double* Jp;                // [n][2][3]
    double* rw;                // [n][3]: r_u, r_v, w
    double* Vinv;              // [P][6]: upper triangle of V_p*^-1
    double* Vg;                // [P][3]: V_p*^-1 g_p
    double* gp;                // [P][3]
    double* S;                 // [6V][6V]
    double* b;                 // [6V]: right-hand side, then delta_c
    double* cand_poses;        // [V][12]
    double* cand_points;       // [P][3]
    int32_t* view_start;       // [V + 1]
    int32_t* obs_point;        // [n]
    int32_t* obs_view;         // [n]
    int32_t* point_start;      // [P + 1]
    int32_t* point_obs;        // [n]: observations of point p in list order (= rising view position)
    uint8_t* view_const;       // [V]
    uint8_t* point_const;      // [P]: fewer than min_point_views observations
    // THE CAMERA BLOCK's part (ls2fm_bundle_adjust_lm_camera_workspace_bytes), behind the layout above; S and b then point here
    double* cam_ok;            // [1]: the caller's fx, fy are finite and not 0 (balm_linearize, workgroup 0)
    double* cand_cam;          // [12]
    double* Jk;                // [n][2][12]
    double* Yp;                // [P][12][3]
    double* Gv;                // [V][12][12]: the view's sum of w J_k^T J_k
    double* Zv;                // [V][12][12]:                  J_k^T F_o
    double* Hv;                // [V][6][12]:                   w J_c^T J_k
    double* Zh;                // [V][6][12]:                   J_c^T F_o
    double* gkv;               // [V][12]:                      w J_k^T r
    double* ekv;               // [V][12]:                      J_k^T (w J_p V_p*^-1 g_p)
    int64_t bytes;
};

struct Prob {
    int V, P, n, nb, loss;
    double fx, fy, cx, cy, c2, lambda0, grad_tol, step_tol;
    uint32_t mask; int tie; double aspect;           // THE CAMERA BLOCK: the refined words, fy = aspect * fx
};

int64_t n_blocks(int64_t V, int64_t P) { return (P + V + kT - 1) / kT; }

Ws layout(void* base, int64_t V, int64_t P, int64_t n, bool camera = false) {
    Workspace ws(base, 16);
    Ws w = {};
    const int64_t nb = n_blocks(V, P), N = 6 * V;
    w.header = ws.take<int32_t>(8);
    w.it = ws.take<double>(8);
    w.sum = ws.take<double>(8);
    w.cost_part = ws.take<double>(V);
    w.gview = ws.take<double>(V);
    w.pview = ws.take<double>(V);
    w.cand_part = ws.take<double>(V);
    w.gblk = ws.take<double>(nb);
    w.fblk = ws.take<double>(nb);
    w.dblk = ws.take<double>(nb);
    w.U = ws.take<double>(21 * V);
    w.g = ws.take<double>(6 * V);
    w.Jc = ws.take<double>(12 * n);
    w.Jp = ws.take<double>(6 * n);
    w.rw = ws.take<double>(3 * n);
    w.Vinv = ws.take<double>(6 * P);
    w.Vg = ws.take<double>(3 * P);
    w.gp = ws.take<double>(3 * P);
    w.S = ws.take<double>(N * N);
    w.b = ws.take<double>(N);
    w.cand_poses = ws.take<double>(12 * V);
    w.cand_points = ws.take<double>(3 * P);
    w.view_start = ws.take<int32_t>(V + 1);
    w.obs_point = ws.take<int32_t>(n);
    w.obs_view = ws.take<int32_t>(n);
    w.point_start = ws.take<int32_t>(P + 1);
    w.point_obs = ws.take<int32_t>(n);
    w.view_const = ws.take<uint8_t>(V);
    w.point_const = ws.take<uint8_t>(P);
    if (camera) {
        const int64_t Nc = N + kK;
        w.cam_ok = ws.take<double>(1);
        w.cand_cam = ws.take<double>(kK);
        w.Jk = ws.take<double>(2 * kK * n);
        w.Yp = ws.take<double>(3 * kK * P);
        w.Gv = ws.take<double>(kK * kK * V);
        w.Zv = ws.take<double>(kK * kK * V);
        w.Hv = ws.take<double>(6 * kK * V);
        w.Zh = ws.take<double>(6 * kK * V);
        w.gkv = ws.take<double>(kK * V);
        w.ekv = ws.take<double>(kK * V);
        w.S = ws.take<double>(Nc * Nc);
        w.b = ws.take<double>(Nc);
    }
    w.bytes = (int64_t)ws.bytes();
    return w;
}

__device__ __forceinline__ bool header_ok(const Ws& w, const Prob& pb) {
    return w.header[0] == kMagic && w.header[1] == pb.V && w.header[2] == pb.P && w.header[3] == pb.n;
}

__device__ __forceinline__ bool focal_ok(double f) { return f != 0.0 && fabs(f) <= 1.7976931348623157e308; }     // finite, not 0

// what every launch but balm_linearize asks before it touches anything
template <bool CAMERA>
__device__ __forceinline__ bool ready(const Ws& w, const Prob& pb) {
    if constexpr (CAMERA) return header_ok(w, pb) && w.cam_ok[0] != 0.0;
    else return header_ok(w, pb);
}

// one observation: camera point, residual, s = |r|^2 -> rho and the IRLS weight rho'(s)
struct ObsEval { double X, Y, Z, iz, r0, r1, rho, wgt; };
// THE CAMERA BLOCK's part of it: the normalised point before and after THE DISTORTION RULE, and what the rule's Jacobians share
struct Lens { double x, y, xd, yd; camera_model::Radial<double> o; };

template <bool CAMERA>
__device__ __forceinline__ ObsEval eval_obs(const double* __restrict__ P, const double* __restrict__ x, const double* __restrict__ uv,
                                            const Prob& pb, const Cam& cam, Lens& L) {
    ObsEval e;
    e.X = ((P[0] * x[0] + P[1] * x[1]) + P[2] * x[2]) + P[3];
    e.Y = ((P[4] * x[0] + P[5] * x[1]) + P[6] * x[2]) + P[7];
    e.Z = ((P[8] * x[0] + P[9] * x[1]) + P[10] * x[2]) + P[11];
    e.iz = 1.0 / e.Z;
    if constexpr (CAMERA) {
        L.x = e.X / e.Z;
        L.y = e.Y / e.Z;
        L.o = camera_model::distort<double>(cam, L.x, L.y, L.xd, L.yd);
        e.r0 = (cam.fx * L.xd + cam.cx) - uv[0];
        e.r1 = (cam.fy * L.yd + cam.cy) - uv[1];
    } else {
        e.r0 = (pb.fx * (e.X * e.iz) + pb.cx) - uv[0];
        e.r1 = (pb.fy * (e.Y * e.iz) + pb.cy) - uv[1];
    }
    const double s = e.r0 * e.r0 + e.r1 * e.r1;
    if (pb.loss == 0) {
        e.rho = s;
        e.wgt = 1.0;
    } else if (pb.loss == 1) {                       // soft_l1
        const double q = sqrt(1.0 + s / pb.c2);
        e.rho = 2.0 * pb.c2 * (q - 1.0);
        e.wgt = 1.0 / q;
    } else {                                         // cauchy
        e.rho = pb.c2 * log1p(s / pb.c2);
        e.wgt = 1.0 / (1.0 + s / pb.c2);
    }
    return e;
}

// The decision on the pending iteration (one thread).  rec: the caller's state on entry, the new record on return.
__device__ inline void decide(const Ws& w, const Prob& pb, const double* __restrict__ state, bool pending, double (&rec)[8],
                              double* __restrict__ log_row) {
#pragma unroll
    for (int q = 0; q < 8; ++q) rec[q] = state[q];
    if (!(rec[kLambda] > 0.0)) rec[kLambda] = pb.lambda0;          // a zeroed state: the first call
    rec[kAccepted] = 0.0;
    if (!pending) return;
    if (rec[kDone] != 0.0) {                                        // a row after the stop
        if (log_row) {
            log_row[0] = rec[kCost]; log_row[1] = rec[kCost]; log_row[2] = rec[kLambda];
            log_row[3] = -1.0; log_row[4] = 0.0; log_row[5] = 0.0;
        }
        return;
    }
    const double cost = w.sum[sCost], gmax = w.sum[sGmax], lam = rec[kLambda];
    double cand = __builtin_nan(""), dmax = 0.0, acc = 0.0;
    if (gmax <= pb.grad_tol) {
        rec[kDone] = 1.0; rec[kReason] = 1.0;
        cand = cost;
    } else if (w.sum[sFailed] != 0.0) {
        rec[kLambda] = lam * 10.0;
    } else {
        cand = 0.0;
        for (int v = 0; v < pb.V; ++v) cand += w.cand_part[v];
        dmax = w.sum[sDmaxC];
        for (int k = 0; k < pb.nb; ++k) dmax = fmax(dmax, w.dblk[k]);
        if (cand < cost) {
            acc = 1.0;
            rec[kLambda] = fmax(lam * 0.1, 1e-16);
            if (dmax <= pb.step_tol * (1.0 + w.sum[sPmax])) { rec[kDone] = 1.0; rec[kReason] = 2.0; }
        } else {
            rec[kLambda] = lam * 10.0;
        }
    }
    if (rec[kDone] == 0.0 && rec[kLambda] > 1e32) { rec[kDone] = 1.0; rec[kReason] = 3.0; }
    rec[kIters] += 1.0;
    rec[kCost] = acc != 0.0 ? cand : cost;
    rec[kGmax] = gmax; rec[kDmax] = dmax; rec[kAccepted] = acc;
    if (log_row) {
        log_row[0] = cost; log_row[1] = cand; log_row[2] = lam; log_row[3] = acc; log_row[4] = gmax; log_row[5] = dmax;
    }
}

// grid: V workgroups (finish: 1)
template <bool CAMERA>
__global__ void __launch_bounds__(kT)
balm_linearize(const double* __restrict__ poses, const double* __restrict__ points, const double* __restrict__ camera,
               const double* __restrict__ obs_uv, Ws w, Prob pb, const double* __restrict__ state, int pending, int finish,
               double* __restrict__ log_row) {
    const int v = blockIdx.x, tid = threadIdx.x;
    __shared__ double s_rec[8], s_red[(kT / 64) * 28], s_mx[kT / 64];
    bool ok = header_ok(w, pb);
    if constexpr (CAMERA) {                          // nobody writes the caller's camera during this launch
        ok = ok && focal_ok(camera[0]) && focal_ok(camera[1]);
        if (v == 0 && tid == 0 && header_ok(w, pb)) w.cam_ok[0] = ok ? 1.0 : 0.0;
    }
    if (!ok) {                                       // an unprepared workspace: nothing moves, the log says so
        if (v == 0 && tid < 6 && log_row) log_row[tid] = __builtin_nan("");
        return;
    }
    if (tid == 0) {
        double rec[8];
        decide(w, pb, state, pending != 0, rec, v == 0 ? log_row : nullptr);
#pragma unroll
        for (int q = 0; q < 8; ++q) s_rec[q] = rec[q];
        if (v == 0)
#pragma unroll
            for (int q = 0; q < 8; ++q) w.it[q] = rec[q];
    }
    __syncthreads();
    if (finish || s_rec[kDone] != 0.0) return;
    const bool acc = s_rec[kAccepted] != 0.0;
    const double* __restrict__ X = acc ? w.cand_points : points;
    double P[12];
#pragma unroll
    for (int q = 0; q < 12; ++q) P[q] = acc ? w.cand_poses[12 * v + q] : poses[12 * v + q];
    Cam cam = {};
    if constexpr (CAMERA) cam = camera_model::load_camera<double>(acc ? w.cand_cam : camera, 0);
    const bool vconst = w.view_const[v] != 0;
    double a[28];
#pragma unroll
    for (int q = 0; q < 28; ++q) a[q] = 0.0;
    double pm = fmax(fmax(fabs(P[3]), fabs(P[7])), fabs(P[11]));
    for (int i = w.view_start[v] + tid; i < w.view_start[v + 1]; i += kT) {
        const int p = w.obs_point[i];
        const double* __restrict__ x = X + 3 * (int64_t)p;
        Lens L;
        const ObsEval e = eval_obs<CAMERA>(P, x, obs_uv + 2 * (int64_t)i, pb, cam, L);
        pm = fmax(pm, fmax(fmax(fabs(x[0]), fabs(x[1])), fabs(x[2])));
        // d x_c = -[x_c]x omega + dt ; J_p = J_proj R
        double Ju[6], Jv[6], Pu[3], Pv[3];
        if constexpr (CAMERA) {
            // J_proj = diag(fx, fy) J_dist [[1/z, 0, -x/z], [0, 1/z, -y/z]], its rows ju and jv
            double da, db, dc, dd;
            camera_model::jacobian<double>(cam, L.o, L.x, L.y, da, db, dc, dd);
            const double ju[3] = {cam.fx * (da * e.iz), cam.fx * (db * e.iz), -(cam.fx * ((da * L.x + db * L.y) * e.iz))};
            const double jv[3] = {cam.fy * (dc * e.iz), cam.fy * (dd * e.iz), -(cam.fy * ((dc * L.x + dd * L.y) * e.iz))};
            Ju[0] = ju[2] * e.Y - ju[1] * e.Z; Ju[1] = ju[0] * e.Z - ju[2] * e.X; Ju[2] = ju[1] * e.X - ju[0] * e.Y;
            Jv[0] = jv[2] * e.Y - jv[1] * e.Z; Jv[1] = jv[0] * e.Z - jv[2] * e.X; Jv[2] = jv[1] * e.X - jv[0] * e.Y;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                Ju[3 + c] = ju[c]; Jv[3 + c] = jv[c];
                Pu[c] = (ju[0] * P[c] + ju[1] * P[4 + c]) + ju[2] * P[8 + c];
                Pv[c] = (jv[0] * P[c] + jv[1] * P[4 + c]) + jv[2] * P[8 + c];
            }
            // J_k, the unrefined words' columns 0, the tied focal length's column col_fx + aspect col_fy
            double ku[kK], kv[kK];
            camera_model::jacobian_k<double>(cam, L.o, L.x, L.y, L.xd, L.yd, ku, kv);
            if (pb.tie) { ku[0] = ku[0] + pb.aspect * ku[1]; kv[0] = kv[0] + pb.aspect * kv[1]; }
            double* __restrict__ jk = w.Jk + 2 * kK * (int64_t)i;
#pragma unroll
            for (int k = 0; k < kK; ++k) {
                const bool on = (pb.mask >> k) & 1u;
                jk[k] = on ? ku[k] : 0.0;
                jk[kK + k] = on ? kv[k] : 0.0;
            }
        } else {
            const double ju0 = pb.fx * e.iz, ju2 = -pb.fx * e.X * e.iz * e.iz;
            const double jv1 = pb.fy * e.iz, jv2 = -pb.fy * e.Y * e.iz * e.iz;
            Ju[0] = e.Y * ju2; Ju[1] = e.Z * ju0 - e.X * ju2; Ju[2] = -e.Y * ju0; Ju[3] = ju0; Ju[4] = 0.0; Ju[5] = ju2;
            Jv[0] = e.Y * jv2 - e.Z * jv1; Jv[1] = -e.X * jv2; Jv[2] = e.X * jv1; Jv[3] = 0.0; Jv[4] = jv1; Jv[5] = jv2;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                Pu[c] = ju0 * P[c] + ju2 * P[8 + c];
                Pv[c] = jv1 * P[4 + c] + jv2 * P[8 + c];
            }
        }
        if (vconst)
#pragma unroll
            for (int q = 0; q < 6; ++q) { Ju[q] = 0.0; Jv[q] = 0.0; }
        const bool pconst = w.point_const[p] != 0;
        double* __restrict__ jc = w.Jc + 12 * (int64_t)i;
        double* __restrict__ jp = w.Jp + 6 * (int64_t)i;
#pragma unroll
        for (int q = 0; q < 6; ++q) { jc[q] = Ju[q]; jc[6 + q] = Jv[q]; }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            jp[c] = pconst ? 0.0 : Pu[c];
            jp[3 + c] = pconst ? 0.0 : Pv[c];
        }
        w.rw[3 * (int64_t)i] = e.r0; w.rw[3 * (int64_t)i + 1] = e.r1; w.rw[3 * (int64_t)i + 2] = e.wgt;
        int q = 0;
#pragma unroll
        for (int r = 0; r < 6; ++r)
#pragma unroll
            for (int c = r; c < 6; ++c) a[q++] += e.wgt * (Ju[r] * Ju[c]) + e.wgt * (Jv[r] * Jv[c]);
#pragma unroll
        for (int r = 0; r < 6; ++r) a[21 + r] += e.wgt * (Ju[r] * e.r0) + e.wgt * (Jv[r] * e.r1);
        a[27] += 0.5 * e.rho;
    }
    block_sum<28, kT>(a, s_red);
    pm = block_max<kT>(pm, s_mx);
    if (tid == 0) {
#pragma unroll
        for (int q = 0; q < 21; ++q) w.U[21 * v + q] = a[q];
        double gm = 0.0;
#pragma unroll
        for (int q = 0; q < 6; ++q) { w.g[6 * v + q] = a[21 + q]; gm = fmax(gm, fabs(a[21 + q])); }
        w.cost_part[v] = a[27];
        w.gview[v] = gm;
        w.pview[v] = pm;
    }
}

// grid: nb workgroups: thread = point, then view
template <bool CAMERA>
__global__ void __launch_bounds__(kT)
balm_points(double* __restrict__ poses, double* __restrict__ points, double* __restrict__ camera, Ws w, Prob pb,
            double* __restrict__ state, int finish) {
    __shared__ double s_mx[kT / 64];
    if (!ready<CAMERA>(w, pb)) return;
    const int64_t idx = (int64_t)blockIdx.x * kT + threadIdx.x;
    const bool done = w.it[kDone] != 0.0, acc = w.it[kAccepted] != 0.0;
    if (idx == 0)
#pragma unroll
        for (int q = 0; q < 8; ++q) state[q] = w.it[q];
    if (acc) {                                       // the accepted candidate becomes the caller's state
        if (idx < pb.P) {
#pragma unroll
            for (int c = 0; c < 3; ++c) points[3 * idx + c] = w.cand_points[3 * idx + c];
        } else if (idx < (int64_t)pb.P + pb.V) {
            const int v = (int)(idx - pb.P);
#pragma unroll
            for (int q = 0; q < 12; ++q) poses[12 * v + q] = w.cand_poses[12 * v + q];
            if constexpr (CAMERA)
                if (v == 0)
#pragma unroll
                    for (int k = 0; k < kK; ++k) camera[k] = w.cand_cam[k];
        }
    }
    if (finish || done) return;
    const double lam = w.it[kLambda];
    double gm = 0.0, fail = 0.0;
    if (idx < pb.P) {
        double Vi[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, vg[3] = {0.0, 0.0, 0.0}, g[3] = {0.0, 0.0, 0.0};
        if (w.point_const[idx] == 0) {
            double A[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};          // 00 01 02 11 12 22
            for (int k = w.point_start[idx]; k < w.point_start[idx + 1]; ++k) {
                const int64_t o = w.point_obs[k];
                const double* __restrict__ jp = w.Jp + 6 * o;
                const double r0 = w.rw[3 * o], r1 = w.rw[3 * o + 1], wt = w.rw[3 * o + 2];
                int q = 0;
#pragma unroll
                for (int r = 0; r < 3; ++r)
#pragma unroll
                    for (int c = r; c < 3; ++c) A[q++] += wt * (jp[r] * jp[c]) + wt * (jp[3 + r] * jp[3 + c]);
#pragma unroll
                for (int r = 0; r < 3; ++r) g[r] += wt * (jp[r] * r0) + wt * (jp[3 + r] * r1);
            }
            gm = fmax(fmax(fabs(g[0]), fabs(g[1])), fabs(g[2]));
            const double dmx = fmax(fmax(A[0], A[3]), A[5]);
            const double a00 = A[0] + lam * fmax(A[0], 1e-12 * dmx), a11 = A[3] + lam * fmax(A[3], 1e-12 * dmx),
                         a22 = A[5] + lam * fmax(A[5], 1e-12 * dmx);
            // Cholesky of the damped 3 x 3, its inverse as L^-T L^-1
            const double l00 = sqrt(a00 > 0.0 ? a00 : 1.0);
            const double l10 = A[1] / l00, l20 = A[2] / l00;
            const double d1 = a11 - l10 * l10;
            const double l11 = sqrt(d1 > 0.0 ? d1 : 1.0);
            const double l21 = (A[4] - l20 * l10) / l11;
            const double d2 = (a22 - l20 * l20) - l21 * l21;
            const double l22 = sqrt(d2 > 0.0 ? d2 : 1.0);
            const bool ok = a00 > 0.0 && d1 > 0.0 && d2 > 0.0;
            const double m00 = 1.0 / l00, m11 = 1.0 / l11, m22 = 1.0 / l22;
            const double m10 = -(l10 * m00) / l11;
            const double m20 = -(l20 * m00 + l21 * m10) / l22;
            const double m21 = -(l21 * m11) / l22;
            if (ok) {
                Vi[0] = (m00 * m00 + m10 * m10) + m20 * m20;
                Vi[1] = m10 * m11 + m20 * m21;
                Vi[2] = m20 * m22;
                Vi[3] = m11 * m11 + m21 * m21;
                Vi[4] = m21 * m22;
                Vi[5] = m22 * m22;
            } else {
                fail = 1.0;
            }
            vg[0] = (Vi[0] * g[0] + Vi[1] * g[1]) + Vi[2] * g[2];
            vg[1] = (Vi[1] * g[0] + Vi[3] * g[1]) + Vi[4] * g[2];
            vg[2] = (Vi[2] * g[0] + Vi[4] * g[1]) + Vi[5] * g[2];
        }
#pragma unroll
        for (int q = 0; q < 6; ++q) w.Vinv[6 * idx + q] = Vi[q];
#pragma unroll
        for (int c = 0; c < 3; ++c) { w.Vg[3 * idx + c] = vg[c]; w.gp[3 * idx + c] = g[c]; }
        if constexpr (CAMERA) {                      // Y_p = sum w J_k^T J_p in the point's list order (J_p = 0: a constant point)
            double Y[3 * kK];
#pragma unroll
            for (int q = 0; q < 3 * kK; ++q) Y[q] = 0.0;
            for (int k = w.point_start[idx]; k < w.point_start[idx + 1]; ++k) {
                const int64_t o = w.point_obs[k];
                const double* __restrict__ jp = w.Jp + 6 * o;
                const double* __restrict__ jk = w.Jk + 2 * kK * o;
                const double wt = w.rw[3 * o + 2];
#pragma unroll
                for (int r = 0; r < kK; ++r)
#pragma unroll
                    for (int c = 0; c < 3; ++c) Y[3 * r + c] += wt * (jk[r] * jp[c]) + wt * (jk[kK + r] * jp[3 + c]);
            }
#pragma unroll
            for (int q = 0; q < 3 * kK; ++q) w.Yp[3 * kK * idx + q] = Y[q];
        }
    }
    gm = block_max<kT>(gm, s_mx);
    fail = block_max<kT>(fail, s_mx);
    if (threadIdx.x == 0) { w.gblk[blockIdx.x] = gm; w.fblk[blockIdx.x] = fail; }
}

// grid: V (V + 1) / 2 workgroups: pair (i, j), i <= j, row by row
template <bool CAMERA>
__global__ void __launch_bounds__(kT)
balm_schur(Ws w, Prob pb) {
    __shared__ double s_red[(kT / 64) * 42];
    if (!ready<CAMERA>(w, pb) || w.it[kDone] != 0.0) return;
    int i = 0, rem = blockIdx.x;
    while (rem >= pb.V - i) { rem -= pb.V - i; ++i; }
    const int j = i + rem, tid = threadIdx.x;
    const bool ci = w.view_const[i] != 0, cj = w.view_const[j] != 0;
    double a[42];
#pragma unroll
    for (int q = 0; q < 42; ++q) a[q] = 0.0;
    if (!ci && !cj) {
        for (int o = w.view_start[i] + tid; o < w.view_start[i + 1]; o += kT) {
            const int p = w.obs_point[o];
            if (w.point_const[p] != 0) continue;
            int o2 = o;
            if (i != j) {                            // the observation of p by view j: the list rises in view position
                int lo = w.point_start[p], hi = w.point_start[p + 1];
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    if (w.obs_view[w.point_obs[mid]] < j) lo = mid + 1; else hi = mid;
                }
                if (lo >= w.point_start[p + 1]) continue;
                o2 = w.point_obs[lo];
                if (w.obs_view[o2] != j) continue;
            }
            const double* __restrict__ ji = w.Jc + 12 * (int64_t)o;
            const double* __restrict__ jj = w.Jc + 12 * (int64_t)o2;
            const double* __restrict__ pi = w.Jp + 6 * (int64_t)o;
            const double* __restrict__ pj = w.Jp + 6 * (int64_t)o2;
            const double* __restrict__ vi = w.Vinv + 6 * (int64_t)p;
            const double wi = w.rw[3 * (int64_t)o + 2], wj = w.rw[3 * (int64_t)o2 + 2];
            // T = J_pi V^-1 (2 x 3), M = w_i w_j T J_pj^T (2 x 2), N = M J_cj (2 x 6), block += J_ci^T N
            double T[2][3], M[2][2];
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                T[k][0] = (pi[3 * k] * vi[0] + pi[3 * k + 1] * vi[1]) + pi[3 * k + 2] * vi[2];
                T[k][1] = (pi[3 * k] * vi[1] + pi[3 * k + 1] * vi[3]) + pi[3 * k + 2] * vi[4];
                T[k][2] = (pi[3 * k] * vi[2] + pi[3 * k + 1] * vi[4]) + pi[3 * k + 2] * vi[5];
            }
#pragma unroll
            for (int k = 0; k < 2; ++k)
#pragma unroll
                for (int l = 0; l < 2; ++l)
                    M[k][l] = (wi * wj) * ((T[k][0] * pj[3 * l] + T[k][1] * pj[3 * l + 1]) + T[k][2] * pj[3 * l + 2]);
#pragma unroll
            for (int c = 0; c < 6; ++c) {
                const double n0 = M[0][0] * jj[c] + M[0][1] * jj[6 + c];
                const double n1 = M[1][0] * jj[c] + M[1][1] * jj[6 + c];
#pragma unroll
                for (int r = 0; r < 6; ++r) a[6 * r + c] += ji[r] * n0 + ji[6 + r] * n1;
            }
            if (i == j) {                            // W_ip V_p*^-1 g_p
                const double* __restrict__ vg = w.Vg + 3 * (int64_t)p;
                const double e0 = wi * ((pi[0] * vg[0] + pi[1] * vg[1]) + pi[2] * vg[2]);
                const double e1 = wi * ((pi[3] * vg[0] + pi[4] * vg[1]) + pi[5] * vg[2]);
#pragma unroll
                for (int r = 0; r < 6; ++r) a[36 + r] += ji[r] * e0 + ji[6 + r] * e1;
            }
        }
    }
    block_sum<42, kT>(a, s_red);
    if (tid != 0) return;
    const int N = 6 * pb.V + (CAMERA ? kK : 0);      // S's row length
    double* __restrict__ S = w.S;
    if (i != j) {
#pragma unroll
        for (int r = 0; r < 6; ++r)
#pragma unroll
            for (int c = 0; c < 6; ++c) {
                const double s = 0.0 - a[6 * r + c];
                S[(int64_t)(6 * i + r) * N + 6 * j + c] = s;
                S[(int64_t)(6 * j + c) * N + 6 * i + r] = s;
            }
        return;
    }
    if (ci) {                                        // a constant view: identity block, right-hand side 0
#pragma unroll
        for (int r = 0; r < 6; ++r) {
#pragma unroll
            for (int c = 0; c < 6; ++c) S[(int64_t)(6 * i + r) * N + 6 * i + c] = r == c ? 1.0 : 0.0;
            w.b[6 * i + r] = 0.0;
        }
        return;
    }
    const double lam = w.it[kLambda];
    const double* __restrict__ U = w.U + 21 * i;
    const int di[6] = {0, 6, 11, 15, 18, 20};        // diagonal entries of the upper triangle
    double dmx = 0.0;
#pragma unroll
    for (int r = 0; r < 6; ++r) dmx = fmax(dmx, U[di[r]]);
    int q = 0;
#pragma unroll
    for (int r = 0; r < 6; ++r)
#pragma unroll
        for (int c = r; c < 6; ++c) {
            const double u = U[q++] + (r == c ? lam * fmax(U[di[r]], 1e-12 * dmx) : 0.0);
            // the sums of (r, c) and (c, r) are equal up to rounding: the upper one is used for both
            const double s = u - a[6 * r + c];
            S[(int64_t)(6 * i + r) * N + 6 * i + c] = s;
            S[(int64_t)(6 * i + c) * N + 6 * i + r] = s;
        }
#pragma unroll
    for (int r = 0; r < 6; ++r) w.b[6 * i + r] = -(w.g[6 * i + r] - a[36 + r]);
}

// THE CAMERA BLOCK.  grid: (V, kK / kBorderCols) workgroups: view v and the camera words k0, k0 + 1.  Per observation o of the view,
// with E = w J_p V_p*^-1 (2 x 3), F = E Y_p^T (2 x 12, its columns k0..) and e = E g_p:
//   Gv[r][k] += w J_k[:, r] . J_k[:, k]     Zv[r][k] += J_k[:, r] . F[:, k]      (r: the 12 words)
//   Hv[r][k] += w J_c[:, r] . J_k[:, k]     Zh[r][k] += J_c[:, r] . F[:, k]      (r: the view's 6 pose parameters)
//   gkv[k]   += w J_k[:, k] . r             ekv[k]   += J_k[:, k] . e
// so that C = sum_v Gv, sum_p Y_p V_p*^-1 Y_p^T = sum_v Zv, sum_p Y_p V_p*^-1 g_p = sum_v ekv (a point's sum over its observations,
// regrouped by view) and S_ik = Hv - Zh.  balm_solve adds the views in view order.
__global__ void __launch_bounds__(kT)
balm_border(Ws w, Prob pb) {
    __shared__ double s_red[(kT / 64) * kBorderSums];
    if (!ready<true>(w, pb) || w.it[kDone] != 0.0) return;
    constexpr int C = kBorderCols;
    const int v = blockIdx.x, k0 = C * blockIdx.y, tid = threadIdx.x;
    double a[kBorderSums];
#pragma unroll
    for (int q = 0; q < kBorderSums; ++q) a[q] = 0.0;
    for (int o = w.view_start[v] + tid; o < w.view_start[v + 1]; o += kT) {
        const int p = w.obs_point[o];
        const double* __restrict__ jk = w.Jk + 2 * kK * (int64_t)o;
        const double* __restrict__ jc = w.Jc + 12 * (int64_t)o;
        const double* __restrict__ jp = w.Jp + 6 * (int64_t)o;
        const double* __restrict__ vi = w.Vinv + 6 * (int64_t)p;
        const double* __restrict__ vg = w.Vg + 3 * (int64_t)p;
        const double* __restrict__ yp = w.Yp + 3 * kK * (int64_t)p + 3 * k0;
        const double r0 = w.rw[3 * (int64_t)o], r1 = w.rw[3 * (int64_t)o + 1], wt = w.rw[3 * (int64_t)o + 2];
        double E[2][3], F[2][C], e[2], ku[C], kv[C];
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            E[k][0] = wt * ((jp[3 * k] * vi[0] + jp[3 * k + 1] * vi[1]) + jp[3 * k + 2] * vi[2]);
            E[k][1] = wt * ((jp[3 * k] * vi[1] + jp[3 * k + 1] * vi[3]) + jp[3 * k + 2] * vi[4]);
            E[k][2] = wt * ((jp[3 * k] * vi[2] + jp[3 * k + 1] * vi[4]) + jp[3 * k + 2] * vi[5]);
            e[k] = wt * ((jp[3 * k] * vg[0] + jp[3 * k + 1] * vg[1]) + jp[3 * k + 2] * vg[2]);
#pragma unroll
            for (int m = 0; m < C; ++m) F[k][m] = (E[k][0] * yp[3 * m] + E[k][1] * yp[3 * m + 1]) + E[k][2] * yp[3 * m + 2];
        }
#pragma unroll
        for (int m = 0; m < C; ++m) { ku[m] = jk[k0 + m]; kv[m] = jk[kK + k0 + m]; }
#pragma unroll
        for (int r = 0; r < kK; ++r)
#pragma unroll
            for (int m = 0; m < C; ++m) {
                a[C * r + m] += wt * (jk[r] * ku[m]) + wt * (jk[kK + r] * kv[m]);
                a[C * (kK + r) + m] += jk[r] * F[0][m] + jk[kK + r] * F[1][m];
            }
#pragma unroll
        for (int r = 0; r < 6; ++r)
#pragma unroll
            for (int m = 0; m < C; ++m) {
                a[C * (2 * kK + r) + m] += wt * (jc[r] * ku[m]) + wt * (jc[6 + r] * kv[m]);
                a[C * (2 * kK + 6 + r) + m] += jc[r] * F[0][m] + jc[6 + r] * F[1][m];
            }
#pragma unroll
        for (int m = 0; m < C; ++m) {
            a[C * 36 + m] += wt * (ku[m] * r0) + wt * (kv[m] * r1);
            a[C * 37 + m] += ku[m] * e[0] + kv[m] * e[1];
        }
    }
    block_sum<kBorderSums, kT>(a, s_red);
    if (tid != 0) return;
#pragma unroll
    for (int m = 0; m < C; ++m) {
#pragma unroll
        for (int r = 0; r < kK; ++r) {
            w.Gv[kK * (kK * v + r) + k0 + m] = a[C * r + m];
            w.Zv[kK * (kK * v + r) + k0 + m] = a[C * (kK + r) + m];
        }
#pragma unroll
        for (int r = 0; r < 6; ++r) {
            w.Hv[kK * (6 * v + r) + k0 + m] = a[C * (2 * kK + r) + m];
            w.Zh[kK * (6 * v + r) + k0 + m] = a[C * (2 * kK + 6 + r) + m];
        }
        w.gkv[kK * v + k0 + m] = a[C * 36 + m];
        w.ekv[kK * v + k0 + m] = a[C * 37 + m];
    }
}

// grid: ONE workgroup
template <bool CAMERA>
__global__ void __launch_bounds__(kT)
balm_solve(Ws w, Prob pb) {
    __shared__ double s_panel[kMaxN * 6];            // the panel's columns of L, row-major [row][6]
    __shared__ double s_z[kMaxN];                    // the right-hand side: one more row of the matrix
    __shared__ double s_d[36], s_mx[kT / 64];
    __shared__ double s_c[CAMERA ? 2 * kK * kK : 1]; // C and the sum it loses to the points
    __shared__ int s_fail;
    if (!ready<CAMERA>(w, pb) || w.it[kDone] != 0.0) return;
    const int tid = threadIdx.x, V = pb.V, N = 6 * V + (CAMERA ? kK : 0), NP = V + (CAMERA ? kK / 6 : 0);
    double gm = 0.0, pm = 0.0, fl = 0.0;
    for (int v = tid; v < V; v += kT) { gm = fmax(gm, w.gview[v]); pm = fmax(pm, w.pview[v]); }
    for (int k = tid; k < pb.nb; k += kT) { gm = fmax(gm, w.gblk[k]); fl = fmax(fl, w.fblk[k]); }
    if constexpr (CAMERA)
        if (tid < kK) {                              // g_k and what the points take from it, the views' parts in view order
            double gk = 0.0, ek = 0.0;
            for (int v = 0; v < V; ++v) { gk += w.gkv[kK * v + tid]; ek += w.ekv[kK * v + tid]; }
            const bool on = (pb.mask >> tid) & 1u;
            s_z[6 * V + tid] = on ? -(gk - ek) : 0.0;
            if (on) gm = fmax(gm, fabs(gk));
        }
    gm = block_max<kT>(gm, s_mx);
    pm = block_max<kT>(pm, s_mx);
    fl = block_max<kT>(fl, s_mx);
    if (tid == 0) {
        double c = 0.0;
        for (int v = 0; v < V; ++v) c += w.cost_part[v];
        w.sum[sGmax] = gm; w.sum[sPmax] = pm; w.sum[sCost] = c;
        s_fail = fl != 0.0 ? 1 : 0;
    }
    for (int q = tid; q < 6 * V; q += kT) s_z[q] = w.b[q];
    double* __restrict__ S = w.S;
    if constexpr (CAMERA) {                          // the camera's rows 6 V .. of S (and their mirror)
        const double lam = w.it[kLambda];
        const int c6 = 6 * V;
        if (tid < kK * kK) {
            double c = 0.0, z = 0.0;
            for (int v = 0; v < V; ++v) { c += w.Gv[kK * kK * v + tid]; z += w.Zv[kK * kK * v + tid]; }
            s_c[tid] = c; s_c[kK * kK + tid] = z;
        }
        __syncthreads();
        if (tid < kK * kK && tid % kK <= tid / kK) { // C* as ONE block; an unrefined word: the identity's row and column
            const int k = tid / kK, l = tid % kK;
            double dmx = 0.0;
#pragma unroll
            for (int q = 0; q < kK; ++q) dmx = fmax(dmx, s_c[(kK + 1) * q]);
            double val = k == l ? 1.0 : 0.0;
            if (((pb.mask >> k) & 1u) && ((pb.mask >> l) & 1u))
                val = (s_c[tid] + (k == l ? lam * fmax(s_c[tid], 1e-12 * dmx) : 0.0)) - s_c[kK * kK + tid];
            S[(int64_t)(c6 + k) * N + c6 + l] = val;
            S[(int64_t)(c6 + l) * N + c6 + k] = val;
        }
        for (int q = tid; q < kK * c6; q += kT) {    // S_ki = (H_i - its eliminated part)^T
            const int k = q / c6, col = q % c6;
            const double val = w.Hv[kK * col + k] - w.Zh[kK * col + k];
            S[(int64_t)(c6 + k) * N + col] = val;
            S[(int64_t)col * N + c6 + k] = val;
        }
    }
    for (int k = 0; k < NP; ++k) {
        const int c0 = 6 * k;
        __syncthreads();
        if (tid < 36) s_d[tid] = S[(int64_t)(c0 + tid / 6) * N + c0 + tid % 6];
        __syncthreads();
        if (tid == 0) {                              // the 6 x 6 diagonal block, in place (lower triangle)
            for (int jj = 0; jj < 6; ++jj) {
                double d = s_d[7 * jj];
                for (int q = 0; q < jj; ++q) d -= s_d[6 * jj + q] * s_d[6 * jj + q];
                if (!(d > 0.0)) { s_fail = 1; d = 1.0; }
                const double l = sqrt(d);
                s_d[7 * jj] = l;
                for (int ii = jj + 1; ii < 6; ++ii) {
                    double s = s_d[6 * ii + jj];
                    for (int q = 0; q < jj; ++q) s -= s_d[6 * ii + q] * s_d[6 * jj + q];
                    s_d[6 * ii + jj] = s / l;
                }
            }
        }
        __syncthreads();
        // the panel's rows: x L_kk^T = s; row N is the right-hand side
        for (int r = c0 + tid; r <= N; r += kT) {
            double x[6];
            if (r < c0 + 6) {
#pragma unroll
                for (int m = 0; m < 6; ++m) x[m] = m <= r - c0 ? s_d[6 * (r - c0) + m] : 0.0;
            } else {
#pragma unroll
                for (int m = 0; m < 6; ++m) {
                    double s = r < N ? S[(int64_t)r * N + c0 + m] : s_z[c0 + m];
#pragma unroll
                    for (int q = 0; q < m; ++q) s -= x[q] * s_d[6 * m + q];
                    x[m] = s / s_d[7 * m];
                }
            }
            if (r < N) {
#pragma unroll
                for (int m = 0; m < 6; ++m) { S[(int64_t)r * N + c0 + m] = x[m]; s_panel[6 * r + m] = x[m]; }
            } else {                                 // z of this panel (only this thread reads or writes these six words here)
#pragma unroll
                for (int m = 0; m < 6; ++m) s_z[c0 + m] = x[m];
            }
        }
        __syncthreads();
        // trailing update, lower triangle: a wave per row, lanes over the columns
        const int t0 = c0 + 6;
        for (int r = t0 + (tid >> 6); r < N; r += kT / 64) {
            double lr[6];
#pragma unroll
            for (int m = 0; m < 6; ++m) lr[m] = s_panel[6 * r + m];
            for (int c = t0 + (tid & 63); c <= r; c += 64) {
                double t = S[(int64_t)r * N + c];
#pragma unroll
                for (int m = 0; m < 6; ++m) t -= lr[m] * s_panel[6 * c + m];
                S[(int64_t)r * N + c] = t;
            }
        }
        for (int c = t0 + tid; c < N; c += kT) {                    // row N
            double t = s_z[c];
#pragma unroll
            for (int m = 0; m < 6; ++m) t -= s_z[c0 + m] * s_panel[6 * c + m];
            s_z[c] = t;
        }
    }
    // back substitution L^T x = z, by panels from the last
    for (int k = NP - 1; k >= 0; --k) {
        const int c0 = 6 * k;
        __syncthreads();
        if (tid < 36) s_d[tid] = S[(int64_t)(c0 + tid / 6) * N + c0 + tid % 6];
        __syncthreads();
        if (tid == 0) {
            for (int ii = 5; ii >= 0; --ii) {
                double s = s_z[c0 + ii];
                for (int q = ii + 1; q < 6; ++q) s -= s_d[6 * q + ii] * s_z[c0 + q];
                s_z[c0 + ii] = s / s_d[7 * ii];
            }
        }
        __syncthreads();
        for (int r = tid; r < c0; r += kT) {
            double t = s_z[r];
#pragma unroll
            for (int m = 0; m < 6; ++m) t -= S[(int64_t)(c0 + m) * N + r] * s_z[c0 + m];
            s_z[r] = t;
        }
    }
    __syncthreads();
    double dm = 0.0;
    for (int q = tid; q < N; q += kT) {              // (delta_k enters max |delta| scaled, in balm_backsub)
        w.b[q] = s_z[q];
        if (q < 6 * V) dm = fmax(dm, fabs(s_z[q]));
    }
    dm = block_max<kT>(dm, s_mx);
    if (tid == 0) { w.sum[sDmaxC] = dm; w.sum[sFailed] = s_fail ? 1.0 : 0.0; }
}

// grid: nb workgroups: thread = point, then view
template <bool CAMERA>
__global__ void __launch_bounds__(kT)
balm_backsub(const double* __restrict__ poses, const double* __restrict__ points, const double* __restrict__ camera, Ws w, Prob pb) {
    __shared__ double s_mx[kT / 64];
    if (!ready<CAMERA>(w, pb) || w.it[kDone] != 0.0 || w.sum[sFailed] != 0.0) return;
    const int64_t idx = (int64_t)blockIdx.x * kT + threadIdx.x;
    double dm = 0.0;
    if (idx < pb.P) {
        double x[3] = {points[3 * idx], points[3 * idx + 1], points[3 * idx + 2]};
        if (w.point_const[idx] == 0) {
            double s[3] = {w.gp[3 * idx], w.gp[3 * idx + 1], w.gp[3 * idx + 2]};
            for (int k = w.point_start[idx]; k < w.point_start[idx + 1]; ++k) {         // + W_o^T delta_c[view(o)]
                const int64_t o = w.point_obs[k];
                const double* __restrict__ dc = w.b + 6 * w.obs_view[o];
                const double* __restrict__ jc = w.Jc + 12 * o;
                const double* __restrict__ jp = w.Jp + 6 * o;
                double e0 = 0.0, e1 = 0.0;
#pragma unroll
                for (int q = 0; q < 6; ++q) { e0 += jc[q] * dc[q]; e1 += jc[6 + q] * dc[q]; }
                const double wt = w.rw[3 * o + 2];
#pragma unroll
                for (int c = 0; c < 3; ++c) s[c] += wt * (jp[c] * e0 + jp[3 + c] * e1);
            }
            if constexpr (CAMERA) {                  // + Y_p^T delta_k
                const double* __restrict__ dk = w.b + 6 * pb.V;
                const double* __restrict__ yp = w.Yp + 3 * kK * idx;
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    double t = 0.0;
#pragma unroll
                    for (int k = 0; k < kK; ++k) t += yp[3 * k + c] * dk[k];
                    s[c] += t;
                }
            }
            const double* __restrict__ vi = w.Vinv + 6 * idx;
            const double d[3] = {-((vi[0] * s[0] + vi[1] * s[1]) + vi[2] * s[2]), -((vi[1] * s[0] + vi[3] * s[1]) + vi[4] * s[2]),
                                 -((vi[2] * s[0] + vi[4] * s[1]) + vi[5] * s[2])};
#pragma unroll
            for (int c = 0; c < 3; ++c) { x[c] += d[c]; dm = fmax(dm, fabs(d[c])); }
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) w.cand_points[3 * idx + c] = x[c];
    } else if (idx < (int64_t)pb.P + pb.V) {
        const int v = (int)(idx - pb.P);
        double C[12];
        if (w.view_const[v] != 0) {
#pragma unroll
            for (int q = 0; q < 12; ++q) C[q] = poses[12 * v + q];
        } else {
            double d[6];
#pragma unroll
            for (int q = 0; q < 6; ++q) d[q] = w.b[6 * v + q];
            pose_update(poses + 12 * v, d, C);
        }
#pragma unroll
        for (int q = 0; q < 12; ++q) w.cand_poses[12 * v + q] = C[q];
        if constexpr (CAMERA)
            if (v == 0) {                            // the candidate camera; its step enters max |delta| relative to the word
                double cc[kK];
#pragma unroll
                for (int k = 0; k < kK; ++k) {
                    const double ck = camera[k], dk = w.b[6 * pb.V + k];
                    const bool on = (pb.mask >> k) & 1u;
                    cc[k] = on ? ck + dk : ck;
                    if (on) dm = fmax(dm, fabs(dk) / (1.0 + fabs(ck)));
                }
                if (pb.tie) cc[1] = pb.aspect * cc[0];
#pragma unroll
                for (int k = 0; k < kK; ++k) w.cand_cam[k] = cc[k];
            }
    }
    dm = block_max<kT>(dm, s_mx);
    if (threadIdx.x == 0) w.dblk[blockIdx.x] = dm;
}

// grid: V workgroups
template <bool CAMERA>
__global__ void __launch_bounds__(kT)
balm_cost(const double* __restrict__ obs_uv, Ws w, Prob pb) {
    __shared__ double s_red[kT / 64];
    if (!ready<CAMERA>(w, pb) || w.it[kDone] != 0.0 || w.sum[sFailed] != 0.0) return;
    const int v = blockIdx.x, tid = threadIdx.x;
    double P[12];
#pragma unroll
    for (int q = 0; q < 12; ++q) P[q] = w.cand_poses[12 * v + q];
    Cam cam = {};
    if constexpr (CAMERA) cam = camera_model::load_camera<double>(w.cand_cam, 0);
    double a[1] = {0.0};
    for (int i = w.view_start[v] + tid; i < w.view_start[v + 1]; i += kT) {
        Lens L;
        const ObsEval e = eval_obs<CAMERA>(P, w.cand_points + 3 * (int64_t)w.obs_point[i], obs_uv + 2 * (int64_t)i, pb, cam, L);
        a[0] += 0.5 * e.rho;
    }
    block_sum<1, kT>(a, s_red);
    if (tid == 0) w.cand_part[v] = a[0];
}

bool opts_ok(const ls2fm_ba_lm_opts* o) {
    return o && o->loss >= 0 && o->loss <= 2 && o->loss_scale > 0.0 && std::isfinite(o->loss_scale) && o->initial_lambda > 0.0 &&
           std::isfinite(o->initial_lambda) && o->grad_tol >= 0.0 && o->step_tol >= 0.0 && o->min_point_views >= 1;
}

// the launches of a call, shared by the two entry points: pb is filled but for the sizes and the options
template <bool CAMERA>
int run(double* poses, double* points, double* camera, const double* obs_uv, int32_t n_views, int64_t n_points, int64_t n_obs, Prob pb,
        const ls2fm_ba_lm_opts* opts, int32_t n_iters, double* state, double* log, void* workspace, hipStream_t stream) {
    const Ws w = layout(workspace, n_views, n_points, n_obs, CAMERA);
    pb.V = n_views; pb.P = (int)n_points; pb.n = (int)n_obs; pb.nb = (int)n_blocks(n_views, n_points); pb.loss = opts->loss;
    pb.c2 = opts->loss_scale * opts->loss_scale;
    pb.lambda0 = opts->initial_lambda; pb.grad_tol = opts->grad_tol; pb.step_tol = opts->step_tol;
    const unsigned V = (unsigned)n_views, nb = (unsigned)pb.nb, pairs = V * (V + 1) / 2;
    // (the opt-in event pairs of profile.hip bracket every launch: tools/time_ba_lm.py reads the kernels' shares from them)
    auto span = [&](int id, auto&& launch) { ls2fm_prof_begin(id, stream); launch(); ls2fm_prof_end(id, stream); };
    for (int32_t it = 0; it < n_iters; ++it) {
        double* log_prev = it > 0 ? log + 6 * (int64_t)(it - 1) : nullptr;
        span(LS2FM_PROF_BALM_LINEARIZE, [&] { balm_linearize<CAMERA><<<V, kT, 0, stream>>>(poses, points, camera, obs_uv, w, pb, state, it > 0 ? 1 : 0, 0, log_prev); });
        span(LS2FM_PROF_BALM_POINTS, [&] { balm_points<CAMERA><<<nb, kT, 0, stream>>>(poses, points, camera, w, pb, state, 0); });
        span(LS2FM_PROF_BALM_SCHUR, [&] { balm_schur<CAMERA><<<pairs, kT, 0, stream>>>(w, pb); });
        if constexpr (CAMERA)
            span(LS2FM_PROF_BALM_BORDER, [&] { balm_border<<<dim3(V, kK / kBorderCols), kT, 0, stream>>>(w, pb); });
        span(LS2FM_PROF_BALM_SOLVE, [&] { balm_solve<CAMERA><<<1, kT, 0, stream>>>(w, pb); });
        span(LS2FM_PROF_BALM_BACKSUB, [&] { balm_backsub<CAMERA><<<nb, kT, 0, stream>>>(poses, points, camera, w, pb); });
        span(LS2FM_PROF_BALM_COST, [&] { balm_cost<CAMERA><<<V, kT, 0, stream>>>(obs_uv, w, pb); });
    }
    // the decision on the last iteration: the caller's poses, points (and camera) and state are final when these two end
    balm_linearize<CAMERA><<<1, kT, 0, stream>>>(poses, points, camera, obs_uv, w, pb, state, 1, 1, log + 6 * (int64_t)(n_iters - 1));
    balm_points<CAMERA><<<nb, kT, 0, stream>>>(poses, points, camera, w, pb, state, 1);
    return ls2fm_launch_status();
}

}  // namespace

extern "C" int64_t ls2fm_bundle_adjust_lm_workspace_bytes(int32_t n_views, int64_t n_points, int64_t n_obs) {
    if (!sizes_ok(n_views, n_points, n_obs)) return LS2FM_ERR_INVALID_ARGUMENT;
    if (n_views > LS2FM_BA_LM_MAX_VIEWS) return LS2FM_ERR_UNSUPPORTED;
    return layout(nullptr, n_views, n_points, n_obs).bytes;
}

extern "C" int ls2fm_bundle_adjust_lm_prepare(const int32_t* view_start, int32_t n_views, const int32_t* obs_point, int64_t n_obs,
                                              int64_t n_points, const uint8_t* view_constant, int32_t min_point_views, void* workspace,
                                              void* stream_) {
    LS2FM_CHECK_ARG(sizes_ok(n_views, n_points, n_obs) && view_start && obs_point && view_constant && min_point_views >= 1);
    if (n_views > LS2FM_BA_LM_MAX_VIEWS) return LS2FM_ERR_UNSUPPORTED;
    if (!workspace) return LS2FM_ERR_WORKSPACE;
    hipStream_t stream = (hipStream_t)stream_;
    const int64_t V = n_views, P = n_points, n = n_obs;
    const Ws w = layout(workspace, V, P, n);
    // view_constant comes back with the index arrays, under ba_index::build's one synchronisation
    ba_index::Index ix;
    std::vector<uint8_t> vc(V), pc(P);
    if (!ba_index::clear_header(w.header, stream) ||
        hipMemcpyAsync(vc.data(), view_constant, V, hipMemcpyDeviceToHost, stream) != hipSuccess)
        { (void)hipGetLastError(); return LS2FM_ERR_LAUNCH; }
    const int st = ba_index::build(view_start, obs_point, V, P, n, stream, &ix);
    if (st != LS2FM_OK) return st;
    for (int64_t v = 0; v < V; ++v) vc[v] = vc[v] ? 1 : 0;
    const std::vector<int32_t>&ov = ix.obs_view, &ps = ix.point_start, &po = ix.point_obs;
    for (int64_t p = 0; p < P; ++p) {
        for (int64_t k = ps[p] + 1; k < ps[p + 1]; ++k) LS2FM_CHECK_ARG(ov[po[k]] != ov[po[k - 1]]);       // seen twice by one view
        pc[p] = ps[p + 1] - ps[p] < min_point_views ? 1 : 0;
    }
    const int32_t header[8] = {kMagic, (int32_t)V, (int32_t)P, (int32_t)n, 0, 0, 0, 0};
    if (!ba_index::upload(w.view_start, ix.view_start, stream) || !ba_index::upload(w.obs_point, ix.obs_point, stream) ||
        !ba_index::upload(w.obs_view, ix.obs_view, stream) || !ba_index::upload(w.point_start, ix.point_start, stream) ||
        !ba_index::upload(w.point_obs, ix.point_obs, stream) || !ba_index::upload(w.view_const, vc, stream) ||
        !ba_index::upload(w.point_const, pc, stream) ||
        hipMemcpyAsync(w.header, header, sizeof(header), hipMemcpyHostToDevice, stream) != hipSuccess ||
        hipStreamSynchronize(stream) != hipSuccess)                                  // (the host vectors die with this frame)
        { (void)hipGetLastError(); return LS2FM_ERR_LAUNCH; }
    return LS2FM_OK;
}

extern "C" int ls2fm_bundle_adjust_lm_run(double* poses, double* points, const double* obs_uv, int32_t n_views, int64_t n_points,
                                          int64_t n_obs, const double* intrinsic4_host, const ls2fm_ba_lm_opts* opts, int32_t n_iters,
                                          double* state, double* log, void* workspace, void* stream_) {
    LS2FM_CHECK_ARG(sizes_ok(n_views, n_points, n_obs) && n_iters >= 1 && n_iters <= (1 << 20));
    if (n_views > LS2FM_BA_LM_MAX_VIEWS) return LS2FM_ERR_UNSUPPORTED;
    LS2FM_CHECK_ARG(poses && points && obs_uv && intrinsic4_host && state && log && opts_ok(opts));
    for (int q = 0; q < 4; ++q) LS2FM_CHECK_ARG(std::isfinite(intrinsic4_host[q]));
    LS2FM_CHECK_ARG(intrinsic4_host[0] != 0.0 && intrinsic4_host[1] != 0.0);
    if (!workspace) return LS2FM_ERR_WORKSPACE;
    Prob pb = {};
    pb.fx = intrinsic4_host[0]; pb.fy = intrinsic4_host[1]; pb.cx = intrinsic4_host[2]; pb.cy = intrinsic4_host[3];
    return run<false>(poses, points, nullptr, obs_uv, n_views, n_points, n_obs, pb, opts, n_iters, state, log, workspace,
                      (hipStream_t)stream_);
}

extern "C" int64_t ls2fm_bundle_adjust_lm_camera_workspace_bytes(int32_t n_views, int64_t n_points, int64_t n_obs) {
    if (!sizes_ok(n_views, n_points, n_obs)) return LS2FM_ERR_INVALID_ARGUMENT;
    if (n_views > kMaxCamViews) return LS2FM_ERR_UNSUPPORTED;
    return layout(nullptr, n_views, n_points, n_obs, true).bytes;
}

extern "C" int ls2fm_bundle_adjust_lm_run_camera(double* poses, double* points, double* camera, const double* obs_uv, int32_t n_views,
                                                 int64_t n_points, int64_t n_obs, uint32_t refine_mask, int32_t tie_focal, double aspect,
                                                 const ls2fm_ba_lm_opts* opts, int32_t n_iters, double* state, double* log,
                                                 void* workspace, void* stream_) {
    LS2FM_CHECK_ARG(sizes_ok(n_views, n_points, n_obs) && n_iters >= 1 && n_iters <= (1 << 20));
    if (n_views > kMaxCamViews) return LS2FM_ERR_UNSUPPORTED;             // the camera's rows are two of the Cholesky's panels
    LS2FM_CHECK_ARG(poses && points && camera && obs_uv && state && log && opts_ok(opts));
    LS2FM_CHECK_ARG(refine_mask < (1u << kK) && std::isfinite(aspect));
    LS2FM_CHECK_ARG(!tie_focal || ((refine_mask & 1u) && !(refine_mask & 2u)));
    if (!workspace) return LS2FM_ERR_WORKSPACE;
    Prob pb = {};
    pb.mask = refine_mask; pb.tie = tie_focal ? 1 : 0; pb.aspect = aspect;
    return run<true>(poses, points, camera, obs_uv, n_views, n_points, n_obs, pb, opts, n_iters, state, log, workspace,
                     (hipStream_t)stream_);
}
