// The camera-ray arithmetic of get_center_and_ray (utils/camera.py:230-252 of the reference).  camera_rays.hip uses Kinv and dot3;
// camera_to_world and pixel_ray restate its camera_rays_kernel operation for operation for the image render (render_image.hip),
// so that an image's rays are bit for bit those ls2fm_camera_rays forms for its pixels (tests/test_hip_render_image.py holds the
// two equal).  Every product sum is an fma chain over k = 0, 1, .. with the first product rounded on its own (-ffp-contract=off).
#pragma once

#include "ls2fm_device.h"

namespace {

struct Kinv { float k[9]; };

__device__ __forceinline__ float dot3(float a0, float b0, float a1, float b1, float a2, float b2) {
    return fmaf(a2, b2, fmaf(a1, b1, a0 * b0));
}

// camera-to-world [R^T | -(R^T t)] of a world-to-camera pose [3][4]  (invert_pose: the product first, then the negation)
__device__ __forceinline__ void camera_to_world(const float* pose, float (&c2w)[3][4]) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        c2w[a][0] = pose[0 + a]; c2w[a][1] = pose[4 + a]; c2w[a][2] = pose[8 + a];
        c2w[a][3] = -dot3(pose[0 + a], pose[3], pose[4 + a], pose[7], pose[8 + a], pose[11]);
    }
}

// centre c[3] and direction r[3] of image point (x, y):  in_cam = [x, y, 1] K^-T ;  center = c2w[:, 3] ;
// ray = ([in_cam, 1] c2w^T) - center
__device__ __forceinline__ void pixel_ray(const float (&c2w)[3][4], Kinv K, float x, float y, float* c, float* r) {
    float cam[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) cam[a] = dot3(x, K.k[3 * a], y, K.k[3 * a + 1], 1.0f, K.k[3 * a + 2]);
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
