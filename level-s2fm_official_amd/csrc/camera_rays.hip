// Pixels -> camera centers and ray directions through V pinhole cameras, optionally with the se(3) -> SE(3) exponential in
// front: the no-gradient "pose algebra" preamble of a stage-loop iteration (pipelines/Camera.py:129-133, 457-463 with
// utils/camera.py:63-147, 230-252 of the reference) as ONE launch.
//
// As torch ops that preamble is ~95 launch-bound kernels per BA iteration (the Taylor series of the exponential, skew / W @ W /
// V @ u as 3 x 3 hipBLASLt products, K^-1 and [R^T | -R^T t] products, concatenations, index selects): about a millisecond of
// the iteration's 3 (profiles/r04_ba_loop_timeline.txt), a quarter of it before the first kernel of the path proper.
//
// Arithmetic, in the reference's order (every product sum is an fma chain over k = 0, 1, .. with the first product rounded on
// its own -- what a single f32 MFMA block computes for these 3- and 4-term sums; elementwise expressions are separate
// multiplications and additions: -ffp-contract=off):
//     theta = sqrt(w0^2 + w1^2 + w2^2) ;  A, B, C = 11-term series  sum_i (-1)^i theta^(2i) / d_i  (left to right)
//     W = skew(w) ; W2 = W W ;  R = (I + A W) + B W2 ;  V = (I + B W) + C W2 ;  t = V u                 (se3_to_SE3)
//     in_cam = [x, y, 1] K^-T ;  c2w = [R^T | -(R^T t)] ;  center = c2w[:, 3] ;  ray = ([in_cam, 1] c2w^T) - center
#include "se3_exp.h"

namespace {

constexpr int kCrThreads = 256;
// one wave (= one 64-thread workgroup) per view
__global__ void __launch_bounds__(64) se3_exp_fwd_kernel(const float* __restrict__ se3, int n, float* __restrict__ poses) {
    const int v = blockIdx.x;
    float pose[12];
    se3_exp(se3 + 6 * v, pose);
    if (threadIdx.x == 0)
        for (int q = 0; q < 12; ++q) poses[12 * v + q] = pose[q];
}

__global__ void __launch_bounds__(64)
se3_exp_bwd_kernel(const float* __restrict__ se3, const float* __restrict__ d_poses, int n, float* __restrict__ d_se3) {
    const int v = blockIdx.x;
    float d[6];
    se3_exp_bwd(se3 + 6 * v, d_poses + 12 * v, d);
    if (threadIdx.x == 0)
        for (int q = 0; q < 6; ++q) d_se3[6 * v + q] = d[q];
}

// grid: (blocks over the pixels, views).  view_sel != null: ONE view, chosen on the device (blockIdx.y == 0 only), whose
// pixels are xy[view] when xy_per_view
__global__ void __launch_bounds__(kCrThreads)
camera_rays_kernel(const float* __restrict__ poses, const float* __restrict__ se3, Kinv K, const float* __restrict__ xy,
                   const int64_t* __restrict__ pix, int width, int xy_per_view, const int64_t* __restrict__ view_sel, int64_t n,
                   float* __restrict__ centers, float* __restrict__ rays, float* __restrict__ poses_out) {
    __shared__ float s_pose[12];
    const int out_v = (int)blockIdx.y;
    const int v = view_sel ? (int)view_sel[0] : out_v;
    if (threadIdx.x < 64) {                       // the first wave: the exponential is a wave-wide job (se3_series)
        float pose[12];
        if (se3) se3_exp(se3 + 6 * v, pose);
        else
            for (int q = 0; q < 12; ++q) pose[q] = poses[12 * v + q];
        if (threadIdx.x == 0) {
            for (int q = 0; q < 12; ++q) s_pose[q] = pose[q];
            if (poses_out && blockIdx.x == 0)
                for (int q = 0; q < 12; ++q) poses_out[12 * out_v + q] = pose[q];
        }
    }
    __syncthreads();
    // camera-to-world [R^T | -(R^T t)]  (invert_pose: the product first, then the negation)
    float c2w[3][4];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        c2w[a][0] = s_pose[0 + a]; c2w[a][1] = s_pose[4 + a]; c2w[a][2] = s_pose[8 + a];
        c2w[a][3] = -dot3(s_pose[0 + a], s_pose[3], s_pose[4 + a], s_pose[7], s_pose[8 + a], s_pose[11]);
    }
    const int64_t i = (int64_t)blockIdx.x * kCrThreads + threadIdx.x;
    if (i >= n) return;
    float x, y;
    if (pix) {                                   // pixel centres of the image grid (mesh_grid: x + 0.5, y + 0.5)
        const int64_t p = pix[i];
        x = (float)(p % width) + 0.5f;
        y = (float)(p / width) + 0.5f;
    } else {
        const float* q = xy + 2 * ((xy_per_view ? (int64_t)v * n : 0) + i);
        x = q[0]; y = q[1];
    }
    float cam[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) cam[a] = dot3(x, K.k[3 * a], y, K.k[3 * a + 1], 1.0f, K.k[3 * a + 2]);
    float* c = centers + 3 * ((int64_t)out_v * n + i);
    float* r = rays + 3 * ((int64_t)out_v * n + i);
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        // to_hom(0) @ c2w^T = 0 + 0 + 0 + 1 c2w[a][3] ; to_hom(in_cam) @ c2w^T is the four-term chain ending in + 1 c2w[a][3]
        const float ctr = fmaf(1.0f, c2w[a][3], fmaf(0.0f, c2w[a][2], fmaf(0.0f, c2w[a][1], 0.0f * c2w[a][0])));
        const float world = fmaf(1.0f, c2w[a][3], fmaf(cam[2], c2w[a][2], fmaf(cam[1], c2w[a][1], cam[0] * c2w[a][0])));
        c[a] = ctr;
        r[a] = world - ctr;
    }
}

}  // namespace

extern "C" int ls2fm_se3_exp_fwd(const float* se3, int32_t n, float* poses, void* stream) {
    LS2FM_CHECK_ARG(n >= 0 && (n == 0 || (se3 && poses)));
    if (n == 0) return LS2FM_OK;
    se3_exp_fwd_kernel<<<n, 64, 0, (hipStream_t)stream>>>(se3, n, poses);
    return ls2fm_launch_status();
}

extern "C" int ls2fm_se3_exp_bwd(const float* se3, const float* d_poses, int32_t n, float* d_se3, void* stream) {
    LS2FM_CHECK_ARG(n >= 0 && (n == 0 || (se3 && d_poses && d_se3)));
    if (n == 0) return LS2FM_OK;
    se3_exp_bwd_kernel<<<n, 64, 0, (hipStream_t)stream>>>(se3, d_poses, n, d_se3);
    return ls2fm_launch_status();
}

extern "C" int ls2fm_camera_rays(const float* poses, const float* se3, const float* kinv_host, const float* xy, const int64_t* pix,
                                 int32_t width, int32_t xy_per_view, const int64_t* view_sel, int32_t n_views, int64_t n,
                                 float* centers, float* rays, float* poses_out, void* stream) {
    LS2FM_CHECK_ARG((poses != nullptr) != (se3 != nullptr));
    LS2FM_CHECK_ARG(kinv_host && ((xy != nullptr) != (pix != nullptr)) && centers && rays && n_views >= 1 && n >= 0);
    LS2FM_CHECK_ARG(!pix || width >= 1);
    if (n == 0) return LS2FM_OK;
    Kinv K;
    for (int q = 0; q < 9; ++q) K.k[q] = kinv_host[q];
    const dim3 grid((unsigned)((n + kCrThreads - 1) / kCrThreads), view_sel ? 1u : (unsigned)n_views);
    camera_rays_kernel<<<grid, kCrThreads, 0, (hipStream_t)stream>>>(poses, se3, K, xy, pix, width, xy_per_view, view_sel, n, centers, rays,
                                                                    poses_out);
    return ls2fm_launch_status();
}
