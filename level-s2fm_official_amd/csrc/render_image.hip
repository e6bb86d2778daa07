// Forward-only rendering of whole images (replaces Camera.render_img_by_slices, pipelines/Camera.py:274-311: get_center_and_ray
// for every pixel, then Renderer.forward over rand_rays slices).
//
// The rays of all views ([n_views][H*W], row-major, pixel centres x + 0.5, y + 0.5) are walked in chunks of a fixed number of
// sample points; per chunk, three launches on the caller's stream:
//   image_rays   : centre and direction of each ray of the chunk from its pixel index (camera_ray.h: ls2fm_camera_rays' arithmetic)
//   ray_encode   : the training forward's gather pass (render_fwd.hip), E / J rows of the chunk into the workspace
//   shade_image  : shade_fwd's body (shade_fwd_body.inc) without the per-sample outputs and save streams: rgb, depth, normal, opacity
// Same kernels' arithmetic, same operands: every pixel's outputs are bit for bit what ls2fm_render_fwd returns for its ray.
// The workspace holds one chunk's rows; it depends on the field and the grids only, never on the image size or the number of views.
// Chunk size by measurement: rows that stay in the 256 MiB Infinity Cache between the two passes (80 or
// 160 MiB) made the gather pass ~7 % faster per sample but the short shading launches of small chunks lost more; 640 MiB
// (8192 rays of 128 samples at L16, dual field) was the fastest of 80 / 160 / 320 / 640 on a DTU and an ETH3D image.
#include "camera_ray.h"
#include "shade_fwd.h"

// MiB of E / J rows per chunk
#ifndef LS2FM_IMAGE_CHUNK_MB
#define LS2FM_IMAGE_CHUNK_MB 640
#endif

namespace {

constexpr int kRayThreads = 256;

// rays g0 .. g0 + n - 1 of the [n_views][hw] image rays
__global__ void __launch_bounds__(kRayThreads)
image_rays_kernel(const float* __restrict__ poses, Kinv K, int64_t hw, int width, int64_t g0, int64_t n, float* __restrict__ centers,
                  float* __restrict__ rays) {
    const int64_t i = (int64_t)blockIdx.x * kRayThreads + threadIdx.x;
    if (i >= n) return;
    const int64_t g = g0 + i;
    const int64_t v = g / hw, p = g - v * hw;
    float pose[12];
#pragma unroll
    for (int q = 0; q < 12; ++q) pose[q] = poses[12 * v + q];
    float c2w[3][4];
    camera_to_world(pose, c2w);
    const float x = (float)(p % width) + 0.5f;
    const float y = (float)(p / width) + 0.5f;
    pixel_ray(c2w, K, x, y, centers + 3 * i, rays + 3 * i);
}

// shade_fwd's kernel without the per-sample outputs (shade_fwd_body.inc with SAVE = false): the parameter names the body reads.
// The partial-tile dual form is given the register budget of 3 waves per SIMD: at 4 it keeps 12 bytes per lane in scratch (as
// its training twin does).  Registers only: same operations, same results.
template <bool DUAL, int MAXS, int CT, bool FULL>
__global__ void __launch_bounds__(MAXS * 4 / CT, CT == 2 ? (DUAL && !FULL ? 3 : 4) : 2)
shade_image_kernel(FieldC fc, int ch1_arg, int ch2_arg, const Packed* __restrict__ pk, const float* __restrict__ center,
                   const float* __restrict__ ray, int64_t p_pad, const float* __restrict__ E1, const float* __restrict__ J1,
                   const float* __restrict__ E2, float* __restrict__ rgb_out, float* __restrict__ depth_out,
                   float* __restrict__ nm_out, float* __restrict__ op_out) {
    constexpr bool SAVE = false;
    float* const sdfs_out = nullptr;            // not read with SAVE = false
    float* const normals_out = nullptr;
    float* const SDFV = nullptr;
    float* const NRM = nullptr;
    float* const RGBS = nullptr;
    float* const FE = nullptr;
    float* const FE2 = nullptr;
    float* const ROUT = nullptr;
    float* const LPART = nullptr;
    const int64_t r_pad = 0;
    const ls2fm_loss_spec loss{};
#include "shade_fwd_body.inc"
}

// workspace carve-up (floats): packed weights, the chunk's rays, its E / J rows ([channel][p_pad], J [channel][p_pad][3])
struct ImageLayout {
    int64_t chunk_rays, p_pad;
    int64_t packed, center, ray, e1, j1, e2, total;
};

ImageLayout make_image_layout(const ls2fm_field_desc* field, int l1, int l2) {
    ImageLayout m;
    const int N = field->n_samples;
    const int64_t floats_per_point = 8 * (int64_t)l1 + 2 * (int64_t)l2;          // E1 (2 L1) + J1 (6 L1) + E2 (2 L2)
    int64_t points = ((int64_t)LS2FM_IMAGE_CHUNK_MB << 20) / (4 * floats_per_point);
    if (points > LS2FM_MAX_RENDER_POINTS) points = LS2FM_MAX_RENDER_POINTS;   // 32-bit offsets inside the kernels
    m.chunk_rays = points / N > 0 ? points / N : 1;
    m.p_pad = (m.chunk_rays * N + 63) / 64 * 64;
    int64_t o = 0;
    auto take = [&](int64_t n) { const int64_t at = o; o += (n + 63) / 64 * 64; return at; };
    m.packed = take((sizeof(Packed) + 3) / 4);
    m.center = take(3 * m.chunk_rays);
    m.ray = take(3 * m.chunk_rays);
    m.e1 = take(2 * l1 * m.p_pad);
    m.j1 = take(6 * l1 * m.p_pad);
    m.e2 = take(2 * l2 * m.p_pad);
    m.total = o;
    return m;
}

// what the kernels serve (the refusals of ls2fm_render_fwd; shade_fwd's widest form is 512 samples per ray)
int image_config(const ls2fm_field_desc* field, const ls2fm_grid_desc* g1, const ls2fm_grid_desc* g2) {
    if (!field || !grid_desc_ok(g1) || (field->dual_field && !grid_desc_ok(g2))) return LS2FM_ERR_INVALID_ARGUMENT;
    if (field->n_samples < 1) return LS2FM_ERR_INVALID_ARGUMENT;
    if (field->bg_sdf) return LS2FM_ERR_UNSUPPORTED;
    if (field->dual_field && !same_grid_geometry(g1, g2)) return LS2FM_ERR_UNSUPPORTED;
    if (field->n_samples > 512) return LS2FM_ERR_UNSUPPORTED;
    return LS2FM_OK;
}

}  // namespace

int ls2fm_launch_image_encode(const ls2fm_field_desc* field, const ls2fm_grid_desc* sdf_grid, const ls2fm_grid_desc* rad_grid,
                              const ls2fm_params* params, const float* center, const float* ray, int64_t n_points, int64_t p_pad,
                              float* e1, float* e2, float* j1, Packed* packed, hipStream_t s);

extern "C" int64_t ls2fm_render_image_workspace_bytes(const ls2fm_field_desc* field, const ls2fm_grid_desc* sdf_grid,
                                                      const ls2fm_grid_desc* rad_grid) {
    const int st = image_config(field, sdf_grid, rad_grid);
    if (st != LS2FM_OK) return st;
    const ImageLayout m = make_image_layout(field, sdf_grid->n_levels, field->dual_field ? rad_grid->n_levels : 0);
    return m.total * (int64_t)sizeof(float);
}

extern "C" int ls2fm_render_image(const ls2fm_field_desc* field, const ls2fm_grid_desc* sdf_grid, const ls2fm_grid_desc* rad_grid,
                                  const ls2fm_params* params, const float* poses, int32_t n_views, const float* kinv_host,
                                  int32_t height, int32_t width, float* rgb, float* depth, float* normal, float* opacity,
                                  void* workspace, void* stream) {
    const int st = image_config(field, sdf_grid, rad_grid);
    if (st != LS2FM_OK) return st;
    LS2FM_CHECK_ARG(params && poses && kinv_host && rgb && depth && normal && n_views >= 1 && height >= 1 && width >= 1);
    if (!workspace) return LS2FM_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    const int dual = field->dual_field ? 1 : 0;
    const int L1 = sdf_grid->n_levels, L2 = dual ? rad_grid->n_levels : 0;
    const ImageLayout m = make_image_layout(field, L1, L2);
    float* ws = (float*)workspace;
    Packed* pk = (Packed*)(ws + m.packed);
    const FieldC fc = make_field_c(field);
    Kinv K;
    for (int q = 0; q < 9; ++q) K.k[q] = kinv_host[q];
    const int N = field->n_samples;
    const int64_t hw = (int64_t)height * width, total = hw * n_views;
    // shade_fwd's launch shapes (ls2fm_launch_shade_fwd)
    const bool small = N <= 256;
    const int threads = (N + (small ? 32 : 64) - 1) / (small ? 32 : 64) * 64;
    const int ch1 = 2 * L1, ch2 = 2 * L2;
    const bool full = small && ch1 == 32 && (!dual || ch2 == 32) && N % 32 == 0;
    for (int64_t g0 = 0; g0 < total; g0 += m.chunk_rays) {
        const int64_t n = total - g0 < m.chunk_rays ? total - g0 : m.chunk_rays;
        const int64_t p_pad = (n * N + 63) / 64 * 64;
        float* ctr = ws + m.center;
        float* dir = ws + m.ray;
        image_rays_kernel<<<(unsigned)((n + kRayThreads - 1) / kRayThreads), kRayThreads, 0, s>>>(poses, K, hw, width, g0, n, ctr, dir);
        int r = ls2fm_launch_image_encode(field, sdf_grid, rad_grid, params, ctr, dir, n * N, p_pad, ws + m.e1, dual ? ws + m.e2 : nullptr,
                                          ws + m.j1, g0 == 0 ? pk : nullptr, s);
        if (r != LS2FM_OK) return r;
        float* op = opacity ? opacity + g0 : nullptr;
        ls2fm_prof_begin(LS2FM_PROF_SHADE_FWD, s);
#define LS2FM_SHADE_IMAGE(DUAL, MAXS, CT, FULL)                                                                                   \
        shade_image_kernel<DUAL, MAXS, CT, FULL><<<(unsigned)n, threads, 0, s>>>(fc, ch1, ch2, pk, ctr, dir, p_pad, ws + m.e1, ws + m.j1, \
                                                                                 DUAL ? ws + m.e2 : nullptr, rgb + 3 * g0, depth + g0,  \
                                                                                 normal + 3 * g0, op)
        if (dual) { if (full) LS2FM_SHADE_IMAGE(true, 256, 2, true); else if (small) LS2FM_SHADE_IMAGE(true, 256, 2, false); else LS2FM_SHADE_IMAGE(true, 512, 4, false); }
        else      { if (full) LS2FM_SHADE_IMAGE(false, 256, 2, true); else if (small) LS2FM_SHADE_IMAGE(false, 256, 2, false); else LS2FM_SHADE_IMAGE(false, 512, 4, false); }
#undef LS2FM_SHADE_IMAGE
        ls2fm_prof_end(LS2FM_PROF_SHADE_FWD, s);
        r = ls2fm_launch_status();
        if (r != LS2FM_OK) return r;
    }
    return LS2FM_OK;
}
