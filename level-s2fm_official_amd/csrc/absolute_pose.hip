// Absolute pose of many views in one call: LO-RANSAC over Lambda Twist P3P, Gauss-Newton local optimisation and a Cauchy-loss
// Levenberg-Marquardt refinement -- what Registration.PnP asks of pycolmap (pipelines/Registration.py:94-109:
// absolute_pose_estimation + pose_refinement), all geometry in fp64.  include/ls2fm.h states the rules; tests/pose_restate.py
// repeats them step by step in numpy.  Correspondences are SORTED BY VIEW (view v owns [view_start[v], view_start[v + 1])).
//
// The rounds (hypotheses, scoring, selection, the stopping rule) are csrc/ransac.h's, run on the model AbsModel below: one thread
// per (view, trial), P3P on three distinct correspondences, <= 4 poses.  Then pose_lo_kernel (local optimisation, the final mask)
// and pose_lm_kernel (refinement), one workgroup per view with fixed-order reductions: every bit of the result is a function of the
// view's own data, seed and options.
#include "ransac.h"

#include <cmath>

namespace {

using namespace ransac;

constexpr int kP3pThreads = 256;               // P3P workgroups (hypotheses, ls2fm_p3p)
constexpr int kViewThreads = 256;              // LO / LM workgroups
constexpr int kLoIters = 10;
constexpr double kGradTol = 1e-10;
constexpr double kStepTol = 1e-12;

// ------------------------------------------------------------------------------------------------------------------- P3P
struct V3 { double x, y, z; };
__device__ __forceinline__ V3 sub(V3 a, V3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ double dot(V3 a, V3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
__device__ __forceinline__ V3 cross(V3 a, V3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
__device__ __forceinline__ V3 scale(V3 a, double s) { return {a.x * s, a.y * s, a.z * s}; }

struct S3 { double m00, m01, m02, m11, m12, m22; };        // symmetric 3 x 3

__device__ __forceinline__ double det_cols(V3 c0, V3 c1, V3 c2) {
    return (c0.x * (c1.y * c2.z - c1.z * c2.y) - c1.x * (c0.y * c2.z - c0.z * c2.y)) + c2.x * (c0.y * c1.z - c0.z * c1.y);
}
__device__ __forceinline__ V3 col(const S3& s, int c) {
    return c == 0 ? V3{s.m00, s.m01, s.m02} : (c == 1 ? V3{s.m01, s.m11, s.m12} : V3{s.m02, s.m12, s.m22});
}
__device__ __forceinline__ S3 axpy(const S3& a, double g, const S3& b) {            // a + g b
    return {a.m00 + g * b.m00, a.m01 + g * b.m01, a.m02 + g * b.m02, a.m11 + g * b.m11, a.m12 + g * b.m12, a.m22 + g * b.m22};
}
__device__ __forceinline__ S3 sxpy(double g, const S3& a, const S3& b) {            // g a + b
    return {g * a.m00 + b.m00, g * a.m01 + b.m01, g * a.m02 + b.m02, g * a.m11 + b.m11, g * a.m12 + b.m12, g * a.m22 + b.m22};
}
__device__ __forceinline__ double quad(const S3& o, V3 u, V3 v) {                    // u^T O v
    const V3 uo = {(u.x * o.m00 + u.y * o.m01) + u.z * o.m02, (u.x * o.m01 + u.y * o.m11) + u.z * o.m12,
                   (u.x * o.m02 + u.y * o.m12) + u.z * o.m22};
    return dot(uo, v);
}

__device__ __forceinline__ double cubic_root(double b, double c, double d) {       // a real root of x^3 + b x^2 + c x + d (largest of three)
    const double p = c - b * b / 3.0;
    const double q = (2.0 * b * b * b / 27.0 - b * c / 3.0) + d;
    const double disc = q * q / 4.0 + p * p * p / 27.0;
    double x;
    if (disc > 0.0) {
        const double s = sqrt(disc);
        const double u = -q / 2.0 + (q <= 0.0 ? s : -s);
        const double cu = cbrt(u);
        x = (cu != 0.0 ? cu - p / (3.0 * cu) : 0.0) - b / 3.0;
    } else {
        const double m = sqrt(fmax(-p / 3.0, 0.0));
        double arg = p < 0.0 ? 3.0 * q / (2.0 * p) * sqrt(-3.0 / p) : 0.0;
        arg = fmin(fmax(arg, -1.0), 1.0);
        x = 2.0 * m * cos(acos(arg) / 3.0) - b / 3.0;
    }
#pragma unroll
    for (int it = 0; it < 2; ++it) {
        const double f = ((x + b) * x + c) * x + d;
        const double df = (3.0 * x + 2.0 * b) * x + c;
        if (df != 0.0) x = x - f / df;
    }
    return x;
}

__device__ __forceinline__ bool null_vec(const S3& d, double s, V3& out) {         // unit null vector of d - s I
    const V3 r0 = {d.m00 - s, d.m01, d.m02}, r1 = {d.m01, d.m11 - s, d.m12}, r2 = {d.m02, d.m12, d.m22 - s};
    const V3 c01 = cross(r0, r1), c02 = cross(r0, r2), c12 = cross(r1, r2);
    const double n01 = dot(c01, c01), n02 = dot(c02, c02), n12 = dot(c12, c12);
    // component-wise selects: a select of whole structs becomes a select of their addresses in scratch
    const bool u01 = n01 >= n02;
    double bx = u01 ? c01.x : c02.x, by = u01 ? c01.y : c02.y, bz = u01 ? c01.z : c02.z, nb = u01 ? n01 : n02;
    const bool keep = nb >= n12;
    bx = keep ? bx : c12.x; by = keep ? by : c12.y; bz = keep ? bz : c12.z; nb = keep ? nb : n12;
    if (!(nb > 0.0)) return false;
    out = scale(V3{bx, by, bz}, 1.0 / sqrt(nb));
    return true;
}

struct Lam { double a01, a02, a12, b01, b02, b12; };     // the three distance equations

__device__ __forceinline__ double lam_res(double l0, double l1, double l2, const Lam& q, double& r0, double& r1, double& r2) {
    r0 = ((l0 * l0 + l1 * l1) - 2.0 * q.b01 * l0 * l1) - q.a01;
    r1 = ((l0 * l0 + l2 * l2) - 2.0 * q.b02 * l0 * l2) - q.a02;
    r2 = ((l1 * l1 + l2 * l2) - 2.0 * q.b12 * l1 * l2) - q.a12;
    return (r0 * r0 + r1 * r1) + r2 * r2;
}

__device__ __forceinline__ void refine_lambda(double& l0, double& l1, double& l2, const Lam& q) {
    double r0, r1, r2;
    double e = lam_res(l0, l1, l2, q, r0, r1, r2);
#pragma unroll
    for (int it = 0; it < 5; ++it) {
        const V3 j0 = {2.0 * (l0 - q.b01 * l1), 2.0 * (l0 - q.b02 * l2), 0.0};            // columns of the Jacobian
        const V3 j1 = {2.0 * (l1 - q.b01 * l0), 0.0, 2.0 * (l1 - q.b12 * l2)};
        const V3 j2 = {0.0, 2.0 * (l2 - q.b02 * l0), 2.0 * (l2 - q.b12 * l1)};
        const double det = det_cols(j0, j1, j2);
        if (det == 0.0 || !isfinite(det)) break;
        const V3 rv = {r0, r1, r2};
        const double n0 = l0 - det_cols(rv, j1, j2) / det;
        const double n1 = l1 - det_cols(j0, rv, j2) / det;
        const double n2 = l2 - det_cols(j0, j1, rv) / det;
        double s0, s1, s2;
        const double en = lam_res(n0, n1, n2, q, s0, s1, s2);
        if (!(en < e)) break;
        l0 = n0; l1 = n1; l2 = n2; e = en;
        r0 = s0; r1 = s1; r2 = s2;
    }
}

// orthonormal frame (columns e1, e2, e3) of the triangle edges a, b
__device__ __forceinline__ bool frame(V3 a, V3 b, V3& e1, V3& e2, V3& e3) {
    const double na = dot(a, a);
    if (!(na > 0.0)) return false;
    e1 = scale(a, 1.0 / sqrt(na));
    const V3 b2 = sub(b, scale(e1, dot(e1, b)));
    const double nb = dot(b2, b2);
    if (!(nb > 0.0)) return false;
    e2 = scale(b2, 1.0 / sqrt(nb));
    e3 = cross(e1, e2);
    return true;
}

// Lambda Twist (Persson & Nordberg, ECCV 2018).  y: unit bearings, x: world points.  emit(slot, P[12]) for every kept solution,
// slot = 2 line + root; every array is indexed at compile time (the loops are unrolled).
template <class Emit>
__device__ __forceinline__ void p3p_solve(const V3 y[3], const V3 x[3], Emit emit) {
    const V3 d01 = sub(x[0], x[1]), d02 = sub(x[0], x[2]), d12 = sub(x[1], x[2]);
    const double a01 = dot(d01, d01), a02 = dot(d02, d02), a12 = dot(d12, d12);
    const V3 cr = cross(d01, d02);
    if (!(dot(cr, cr) > 1e-20 * a01 * a02) || !(a01 > 0.0 && a02 > 0.0 && a12 > 0.0)) return;
    const double b01 = dot(y[0], y[1]), b02 = dot(y[0], y[2]), b12 = dot(y[1], y[2]);
    // D1 = a12 M01 - a01 M12, D2 = a12 M02 - a02 M12 (M_ij: lambda^T M_ij lambda = |lambda_i y_i - lambda_j y_j|^2)
    const S3 D1 = {a12, -a12 * b01, 0.0, a12 - a01, a01 * b12, -a01};
    const S3 D2 = {a12, 0.0, -a12 * b02, -a02, a02 * b12, a12 - a02};
    const double c0 = det_cols(col(D1, 0), col(D1, 1), col(D1, 2));
    const double c3 = det_cols(col(D2, 0), col(D2, 1), col(D2, 2));
    const double c1 = (det_cols(col(D2, 0), col(D1, 1), col(D1, 2)) + det_cols(col(D1, 0), col(D2, 1), col(D1, 2)))
                      + det_cols(col(D1, 0), col(D1, 1), col(D2, 2));
    const double c2 = (det_cols(col(D1, 0), col(D2, 1), col(D2, 2)) + det_cols(col(D2, 0), col(D1, 1), col(D2, 2)))
                      + det_cols(col(D2, 0), col(D2, 1), col(D1, 2));
    S3 D0, O;
    if (fabs(c3) >= fabs(c0)) {
        if (c3 == 0.0) return;
        const double g = cubic_root(c2 / c3, c1 / c3, c0 / c3);
        D0 = axpy(D1, g, D2);
        O = D2;
    } else {
        const double g = cubic_root(c1 / c0, c2 / c0, c3 / c0);
        D0 = sxpy(g, D1, D2);
        O = D1;
    }
    const double tr = (D0.m00 + D0.m11) + D0.m22;
    const double m2 = ((D0.m00 * D0.m11 - D0.m01 * D0.m01) + (D0.m00 * D0.m22 - D0.m02 * D0.m02)) + (D0.m11 * D0.m22 - D0.m12 * D0.m12);
    if (!(m2 < 0.0)) return;
    const double sq = sqrt(fmax(tr * tr - 4.0 * m2, 0.0));
    double s1, s2;
    if (tr >= 0.0) { s1 = 0.5 * (tr + sq); s2 = m2 / s1; }
    else { s2 = 0.5 * (tr - sq); s1 = m2 / s2; }
    V3 e1, e2;
    if (!null_vec(D0, s1, e1) || !null_vec(D0, s2, e2)) return;
    const double r = sqrt(-s2 / s1);
    const Lam lq = {a01, a02, a12, b01, b02, b12};
    const int ks = (a01 >= a02 && a01 >= a12) ? 0 : (a02 >= a12 ? 1 : 2);
    const double Aks = ks == 0 ? a01 : (ks == 1 ? a02 : a12), Bks = ks == 0 ? b01 : (ks == 1 ? b02 : b12);
#pragma unroll
    for (int li = 0; li < 2; ++li) {
        const double sgn = li == 0 ? 1.0 : -1.0;
        const V3 w = sub(e1, scale(e2, sgn * r));
        const double aw0 = fabs(w.x), aw1 = fabs(w.y), aw2 = fabs(w.z);
        const int k = (aw0 >= aw1 && aw0 >= aw2) ? 0 : (aw1 >= aw2 ? 1 : 2);
        const double wk = k == 0 ? w.x : (k == 1 ? w.y : w.z);
        const double wi = k == 0 ? w.y : (k == 1 ? w.z : w.x);           // i = k + 1, j = k + 2 (mod 3)
        const double wj = k == 0 ? w.z : (k == 1 ? w.x : w.y);
        const double pk = -wi / wk, qk = -wj / wk;
        const V3 p = {k == 0 ? pk : (k == 2 ? 1.0 : 0.0), k == 1 ? pk : (k == 0 ? 1.0 : 0.0), k == 2 ? pk : (k == 1 ? 1.0 : 0.0)};
        const V3 q = {k == 0 ? qk : (k == 1 ? 1.0 : 0.0), k == 1 ? qk : (k == 2 ? 1.0 : 0.0), k == 2 ? qk : (k == 0 ? 1.0 : 0.0)};
        const double qa = quad(O, p, p), qb = quad(O, p, q), qc = quad(O, q, q);
        const double disc = qb * qb - qa * qc;
        if (!(disc >= 0.0)) continue;
        const double qq = -(qb + copysign(sqrt(disc), qb));
#pragma unroll
        for (int ri = 0; ri < 2; ++ri) {
            const double tau = ri == 0 ? (qc != 0.0 ? qq / qc : NAN) : (qq != 0.0 ? qa / qq : NAN);
            if (!isfinite(tau)) continue;
            const V3 dv = {p.x + tau * q.x, p.y + tau * q.y, p.z + tau * q.z};
            const double da = ks == 2 ? dv.y : dv.x, db = ks == 0 ? dv.y : dv.z;
            const double qs = (da * da + db * db) - 2.0 * Bks * da * db;
            if (!(qs > 0.0)) continue;
            double sc = sqrt(Aks / qs);
            if ((dv.x + dv.y) + dv.z < 0.0) sc = -sc;
            double l0 = sc * dv.x, l1 = sc * dv.y, l2 = sc * dv.z;
            refine_lambda(l0, l1, l2, lq);
            if (!(l0 > 0.0 && l1 > 0.0 && l2 > 0.0)) continue;
            const V3 c0v = scale(y[0], l0), c1v = scale(y[1], l1), c2v = scale(y[2], l2);
            V3 f1, f2, f3, g1, g2, g3;
            if (!frame(sub(c0v, c1v), sub(c0v, c2v), f1, f2, f3) || !frame(d01, d02, g1, g2, g3)) continue;
            // R = Fc Fw^T ;  t = mean(c) - R mean(x)
            double P[12];
            const double fc[3][3] = {{f1.x, f2.x, f3.x}, {f1.y, f2.y, f3.y}, {f1.z, f2.z, f3.z}};
            const double fw[3][3] = {{g1.x, g2.x, g3.x}, {g1.y, g2.y, g3.y}, {g1.z, g2.z, g3.z}};
#pragma unroll
            for (int a = 0; a < 3; ++a)
#pragma unroll
                for (int b = 0; b < 3; ++b) P[4 * a + b] = (fc[a][0] * fw[b][0] + fc[a][1] * fw[b][1]) + fc[a][2] * fw[b][2];
            const V3 cm = scale({(c0v.x + c1v.x) + c2v.x, (c0v.y + c1v.y) + c2v.y, (c0v.z + c1v.z) + c2v.z}, 1.0 / 3.0);
            const V3 xm = scale({(x[0].x + x[1].x) + x[2].x, (x[0].y + x[1].y) + x[2].y, (x[0].z + x[1].z) + x[2].z}, 1.0 / 3.0);
            bool ok = true;
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                const double cma = a == 0 ? cm.x : (a == 1 ? cm.y : cm.z);
                P[4 * a + 3] = cma - ((P[4 * a] * xm.x + P[4 * a + 1] * xm.y) + P[4 * a + 2] * xm.z);
            }
#pragma unroll
            for (int q2 = 0; q2 < 12; ++q2) ok = ok && isfinite(P[q2]);
#pragma unroll
            for (int s = 0; s < 3; ++s) ok = ok && ((P[8] * x[s].x + P[9] * x[s].y) + P[10] * x[s].z) + P[11] > 0.0;
            if (ok) emit(2 * li + ri, P);
        }
    }
}

// camera z and squared pixel error of one correspondence (the operation order of tests/pose_restate.py: project_err2)
__device__ __forceinline__ double project_err2(const double* P, double x, double y, double z, double u, double v, double fx, double fy,
                                               double cx, double cy, double& Z) {
    const double X = ((P[0] * x + P[1] * y) + P[2] * z) + P[3];
    const double Y = ((P[4] * x + P[5] * y) + P[6] * z) + P[7];
    Z = ((P[8] * x + P[9] * y) + P[10] * z) + P[11];
    const double iz = 1.0 / Z;
    const double du = (fx * (X * iz) + cx) - u;
    const double dv = (fy * (Y * iz) + cy) - v;
    return du * du + dv * dv;
}

__global__ void __launch_bounds__(kP3pThreads)
p3p_kernel(const double* __restrict__ bear, const double* __restrict__ pts, int64_t m, double* __restrict__ poses,
           int32_t* __restrict__ n_sol) {
    const int64_t i = (int64_t)blockIdx.x * kP3pThreads + threadIdx.x;
    if (i >= m) return;
    V3 y[3], x[3];
#pragma unroll
    for (int s = 0; s < 3; ++s) {
        y[s] = {bear[9 * i + 3 * s], bear[9 * i + 3 * s + 1], bear[9 * i + 3 * s + 2]};
        x[s] = {pts[9 * i + 3 * s], pts[9 * i + 3 * s + 1], pts[9 * i + 3 * s + 2]};
    }
    double* __restrict__ out = poses + 48 * i;
    int n = 0;
    p3p_solve(y, x, [&](int, const double* P) {
#pragma unroll
        for (int q = 0; q < 12; ++q) out[12 * n + q] = P[q];
        ++n;
    });
    for (int q = 12 * n; q < 48; ++q) out[q] = 0.0;
    n_sol[i] = n;
}

// ---------------------------------------------------------------------------------------------------------------- RANSAC
struct AbsModel {               // ransac.h's model of this file: P3P poses [R | t] scored by the squared pixel error
    static constexpr int kSample = 3, kMaxSol = 4, kHypWords = 12, kMinGroup = 3, kHypThreads = kP3pThreads, kHypLdsWords = 0;
    struct Input { const double* uv; const double* xyz; const double* intr; double thr2; };
    struct Ctx { double fx, fy, cx, cy, thr2; };
    struct Point { double x, y, z, u, v; };
    static __device__ __forceinline__ Ctx context(const Input& in, int v) {
        return {in.intr[4 * v], in.intr[4 * v + 1], in.intr[4 * v + 2], in.intr[4 * v + 3], in.thr2};
    }
    static __device__ __forceinline__ Point load(const Input& in, const Ctx&, int64_t i) {
        return {in.xyz[3 * i], in.xyz[3 * i + 1], in.xyz[3 * i + 2], in.uv[2 * i], in.uv[2 * i + 1]};
    }
    static __device__ __forceinline__ bool inlier(const double* P, const Point& p, const Ctx& c) {
        double Z;
        return project_err2(P, p.x, p.y, p.z, p.u, p.v, c.fx, c.fy, c.cx, c.cy, Z) < c.thr2 && Z > 0.0;
    }
    template <class Emit>
    static __device__ __forceinline__ void hypotheses(const Input& in, const Ctx& c, int64_t s0, const int64_t (&id)[3], double*, Emit emit) {
        V3 y[3], x[3];
#pragma unroll
        for (int s = 0; s < 3; ++s) {
            const Point p = load(in, c, s0 + id[s]);
            const V3 b = {(p.u - c.cx) / c.fx, (p.v - c.cy) / c.fy, 1.0};           // the unit bearing of the pixel
            y[s] = scale(b, 1.0 / sqrt(dot(b, b)));
            x[s] = {p.x, p.y, p.z};
        }
        p3p_solve(y, x, emit);
    }
};

// -------------------------------------------------------------------------------------------------------- least squares
constexpr int kNe = 21 + 6 + 3;          // upper triangle of H, g, then {F or count, changed, unused}

// one correspondence's contribution: weight w, residual (du, dv), Jacobian rows through d p / d(w, dt) = [-[p]x | I]
__device__ __forceinline__ void accumulate(double (&a)[kNe], const double* P, double x, double y, double z, double u, double v,
                                           double fx, double fy, double cx, double cy, double c2, bool robust) {
    const double X = ((P[0] * x + P[1] * y) + P[2] * z) + P[3];
    const double Y = ((P[4] * x + P[5] * y) + P[6] * z) + P[7];
    const double Z = ((P[8] * x + P[9] * y) + P[10] * z) + P[11];
    const double iz = 1.0 / Z;
    const double du = (fx * (X * iz) + cx) - u;
    const double dv = (fy * (Y * iz) + cy) - v;
    const double s = du * du + dv * dv;
    const double w = robust ? 1.0 / (1.0 + s / c2) : 1.0;
    a[27] += robust ? 0.5 * (c2 * log1p(s / c2)) : 0.5 * s;
    const double ju0 = fx * iz, ju2 = -fx * X * iz * iz;
    const double jv1 = fy * iz, jv2 = -fy * Y * iz * iz;
    // p x ju, p x jv  (ju = (ju0, 0, ju2), jv = (0, jv1, jv2))
    const double Ju[6] = {Y * ju2, Z * ju0 - X * ju2, -Y * ju0, ju0, 0.0, ju2};
    const double Jv[6] = {Y * jv2 - Z * jv1, -X * jv2, X * jv1, 0.0, jv1, jv2};
    int q = 0;
#pragma unroll
    for (int r = 0; r < 6; ++r)
#pragma unroll
        for (int c = r; c < 6; ++c) a[q++] += w * (Ju[r] * Ju[c]) + w * (Jv[r] * Jv[c]);
#pragma unroll
    for (int r = 0; r < 6; ++r) a[21 + r] += w * (Ju[r] * du) + w * (Jv[r] * dv);
}

// chol_solve (the damped 6 x 6 solve) and pose_update (R <- exp([w]x) R, t <- exp([w]x) t + dt): lm_math.h
using lm_math::chol_solve;
using lm_math::pose_update;

// one pass of the LO loop: counts, changed and the normal equations (w = 1) over the inliers of C; changed against P
__device__ inline void lo_pass(const double* __restrict__ uv, const double* __restrict__ xyz, int64_t s0, int64_t n, const double* C,
                               const double* P, bool cmp, double fx, double fy, double cx, double cy, double thr2, double (&a)[kNe],
                               double* s_red) {
#pragma unroll
    for (int q = 0; q < kNe; ++q) a[q] = 0.0;
    double cnt = 0.0, chg = 0.0;
    for (int64_t j = threadIdx.x; j < n; j += kViewThreads) {
        const int64_t i = s0 + j;
        const double x = xyz[3 * i], y = xyz[3 * i + 1], z = xyz[3 * i + 2], u = uv[2 * i], v = uv[2 * i + 1];
        double Z;
        const bool in = project_err2(C, x, y, z, u, v, fx, fy, cx, cy, Z) < thr2 && Z > 0.0;
        if (cmp) {
            double Zp;
            const bool inp = project_err2(P, x, y, z, u, v, fx, fy, cx, cy, Zp) < thr2 && Zp > 0.0;
            chg += in != inp ? 1.0 : 0.0;
        }
        if (in) {
            accumulate(a, C, x, y, z, u, v, fx, fy, cx, cy, 1.0, false);
            cnt += 1.0;
        }
    }
    a[27] = cnt;
    a[28] = chg;
    block_sum<kNe, kViewThreads>(a, s_red);
}

__global__ void __launch_bounds__(kViewThreads)
pose_lo_kernel(const double* __restrict__ uv, const double* __restrict__ xyz, const int32_t* __restrict__ vs,
               const double* __restrict__ intr, double thr2, Ws w, double* __restrict__ poses, uint8_t* __restrict__ inliers,
               int32_t* __restrict__ num_inliers, int32_t* __restrict__ trials, int32_t* __restrict__ best_trial,
               int32_t* __restrict__ success) {
    __shared__ double s_red[(kViewThreads / 64) * kNe];
    const int v = blockIdx.x, tid = threadIdx.x;
    const int64_t s0 = vs[v], n = vs[v + 1] - s0;
    const double fx = intr[4 * v], fy = intr[4 * v + 1], cx = intr[4 * v + 2], cy = intr[4 * v + 3];
    const unsigned long long bk = w.best_key[v];
    double P[12];
    if (bk == 0ull) {
        for (int64_t j = tid; j < n; j += kViewThreads) inliers[s0 + j] = 0;
        if (tid < 12) poses[12 * v + tid] = (tid == 0 || tid == 5 || tid == 10) ? 1.0 : 0.0;
        if (tid == 0) { num_inliers[v] = 0; trials[v] = w.trials[v]; best_trial[v] = -1; success[v] = 0; }
        return;
    }
#pragma unroll
    for (int q = 0; q < 12; ++q) P[q] = w.best[12 * v + q];
    double a[kNe], b[kNe];
    lo_pass(uv, xyz, s0, n, P, P, false, fx, fy, cx, cy, thr2, a, s_red);
    for (int it = 0; it < kLoIters; ++it) {
        if (a[27] < 3.0) break;
        double d[6];
        const double zero[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        if (!chol_solve(a, 0.0, zero, d)) break;
        double C[12];
        pose_update(P, d, C);
        lo_pass(uv, xyz, s0, n, C, P, true, fx, fy, cx, cy, thr2, b, s_red);
        if (b[27] < a[27]) break;
#pragma unroll
        for (int q = 0; q < 12; ++q) P[q] = C[q];
#pragma unroll
        for (int q = 0; q < kNe; ++q) a[q] = b[q];
        if (b[28] == 0.0) break;
    }
    for (int64_t j = tid; j < n; j += kViewThreads) {
        const int64_t i = s0 + j;
        double Z;
        const bool in = project_err2(P, xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], uv[2 * i], uv[2 * i + 1], fx, fy, cx, cy, Z) < thr2
                        && Z > 0.0;
        inliers[i] = in ? 1 : 0;
    }
    if (tid < 12) poses[12 * v + tid] = P[tid];
    if (tid == 0) {
        const int32_t cnt = (int32_t)a[27];
        num_inliers[v] = cnt;
        trials[v] = w.trials[v];
        best_trial[v] = best_trial_of<AbsModel>(bk);
        success[v] = cnt >= 4 ? 1 : 0;
    }
}

// ------------------------------------------------------------------------------------------------------------ refinement
__device__ inline void lm_pass(const double* __restrict__ uv, const double* __restrict__ xyz, const uint8_t* __restrict__ mask, int64_t s0,
                               int64_t n, const double* P, double fx, double fy, double cx, double cy, double c2, double (&a)[kNe],
                               double* s_red) {
#pragma unroll
    for (int q = 0; q < kNe; ++q) a[q] = 0.0;
    for (int64_t j = threadIdx.x; j < n; j += kViewThreads) {
        const int64_t i = s0 + j;
        if (mask[i]) accumulate(a, P, xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], uv[2 * i], uv[2 * i + 1], fx, fy, cx, cy, c2, true);
    }
    block_sum<kNe, kViewThreads>(a, s_red);
}

// mask: per correspondence; ok (NULL = every view): refine view v only when ok[v] != 0 (else copy)
__global__ void __launch_bounds__(kViewThreads)
pose_lm_kernel(const double* __restrict__ uv, const double* __restrict__ xyz, const int32_t* __restrict__ vs,
               const double* __restrict__ intr, const uint8_t* __restrict__ mask, const double* poses_in, const int32_t* __restrict__ ok,
               double c2, int max_iters, double* poses_out) {
    __shared__ double s_red[(kViewThreads / 64) * kNe];
    const int v = blockIdx.x, tid = threadIdx.x;
    const int64_t s0 = vs[v], n = vs[v + 1] - s0;
    const double fx = intr[4 * v], fy = intr[4 * v + 1], cx = intr[4 * v + 2], cy = intr[4 * v + 3];
    double P[12];
#pragma unroll
    for (int q = 0; q < 12; ++q) P[q] = poses_in[12 * v + q];
    int cnt = 0;
    for (int64_t j = tid; j < n; j += kViewThreads) cnt += mask[s0 + j] ? 1 : 0;
    __shared__ int s_cnt;
    const bool run = block_count(cnt, &s_cnt) >= 3 && (ok == nullptr || ok[v] != 0);
    double lam = 1e-4;
    for (int it = 0; run && it < max_iters; ++it) {
        double a[kNe], b[kNe];
        lm_pass(uv, xyz, mask, s0, n, P, fx, fy, cx, cy, c2, a, s_red);
        double gmax = 0.0;
#pragma unroll
        for (int r = 0; r < 6; ++r) gmax = fmax(gmax, fabs(a[21 + r]));
        if (gmax <= kGradTol) break;
        const int di[6] = {0, 6, 11, 15, 18, 20};           // diagonal entries of the upper triangle
        double dmax = 0.0, dg[6];
#pragma unroll
        for (int r = 0; r < 6; ++r) dmax = fmax(dmax, a[di[r]]);
#pragma unroll
        for (int r = 0; r < 6; ++r) dg[r] = fmax(a[di[r]], 1e-12 * dmax);
        double d[6];
        if (!chol_solve(a, lam, dg, d)) {
            lam *= 10.0;
            if (lam > 1e32) break;
            continue;
        }
        double C[12];
        pose_update(P, d, C);
        lm_pass(uv, xyz, mask, s0, n, C, fx, fy, cx, cy, c2, b, s_red);
        if (b[27] < a[27]) {
#pragma unroll
            for (int q = 0; q < 12; ++q) P[q] = C[q];
            lam = fmax(lam * 0.1, 1e-16);
            double dm = 0.0;
#pragma unroll
            for (int r = 0; r < 6; ++r) dm = fmax(dm, fabs(d[r]));
            const double tm = fmax(fmax(fabs(P[3]), fabs(P[7])), fabs(P[11]));
            if (dm <= kStepTol * (1.0 + tm)) break;
        } else {
            lam *= 10.0;
            if (lam > 1e32) break;
        }
    }
    if (tid < 12) poses_out[12 * v + tid] = P[tid];
}

}  // namespace

extern "C" int ls2fm_p3p(const double* bearings, const double* points, int64_t m, double* poses, int32_t* n_solutions, void* stream) {
    LS2FM_CHECK_ARG(m >= 0);
    if (m == 0) return LS2FM_OK;
    LS2FM_CHECK_ARG(bearings && points && poses && n_solutions);
    p3p_kernel<<<(unsigned)((m + kP3pThreads - 1) / kP3pThreads), kP3pThreads, 0, (hipStream_t)stream>>>(bearings, points, m, poses,
                                                                                                      n_solutions);
    return ls2fm_launch_status();
}

extern "C" int64_t ls2fm_absolute_pose_workspace_bytes(int32_t n_views, int64_t n_corr) {
    if (n_views < 1 || n_views > LS2FM_POSE_MAX_VIEWS || n_corr < 0) return LS2FM_ERR_INVALID_ARGUMENT;
    return (int64_t)ws_layout<AbsModel>(n_views, nullptr, nullptr);
}

extern "C" int ls2fm_absolute_pose(const double* uv, const double* xyz, const int32_t* view_start, int32_t n_views, const double* intr,
                                   const ls2fm_pose_ransac_opts* opts, double* poses, uint8_t* inliers, int32_t* num_inliers,
                                   int32_t* trials, int32_t* best_trial, int32_t* success, void* workspace, void* stream) {
    LS2FM_CHECK_ARG(n_views >= 1 && n_views <= LS2FM_POSE_MAX_VIEWS && view_start && intr && opts_ok(opts) &&
                    (opts->refine == 0 || opts->refine == 1));
    LS2FM_CHECK_ARG(poses && num_inliers && trials && best_trial && success);
    hipStream_t s = (hipStream_t)stream;
    const double thr2 = opts->max_error_px * opts->max_error_px;
    Ws w;
    const int st = run_rounds<AbsModel>({uv, xyz, intr, thr2}, view_start, n_views, uv && xyz && inliers, opts, workspace, s, &w);
    if (st != LS2FM_OK) return st;
    pose_lo_kernel<<<(unsigned)n_views, kViewThreads, 0, s>>>(uv, xyz, view_start, intr, thr2, w, poses, inliers, num_inliers, trials,
                                                              best_trial, success);
    if (opts->refine)
        pose_lm_kernel<<<(unsigned)n_views, kViewThreads, 0, s>>>(uv, xyz, view_start, intr, inliers, poses, success, 1.0,
                                                                  LS2FM_POSE_REFINE_ITERS, poses);
    return ls2fm_launch_status();
}

extern "C" int ls2fm_pose_refine(const double* uv, const double* xyz, const int32_t* view_start, int32_t n_views, const double* intr,
                                 const uint8_t* mask, const double* poses_in, float loss_scale_px, int32_t max_iters, double* poses_out,
                                 void* stream) {
    LS2FM_CHECK_ARG(n_views >= 1 && n_views <= LS2FM_POSE_MAX_VIEWS && view_start && intr && poses_in && poses_out);
    LS2FM_CHECK_ARG(loss_scale_px > 0.f && std::isfinite(loss_scale_px) && max_iters >= 0);
    LS2FM_CHECK_ARG(uv && xyz && mask);
    const double c = (double)loss_scale_px;
    pose_lm_kernel<<<(unsigned)n_views, kViewThreads, 0, (hipStream_t)stream>>>(uv, xyz, view_start, intr, mask, poses_in, nullptr, c * c,
                                                                                max_iters, poses_out);
    return ls2fm_launch_status();
}
