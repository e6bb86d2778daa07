// Sphere-traced depth and normal maps of whole images (replaces Camera.get_depth, pipelines/Camera.py:216-253: get_center_and_ray
// for every pixel, SDF.sphere_tracing (models/SDF.py:149-224) and SDF.gradient (SDF.py:102-114) at the surface points).
//
// The reference's root-find stops when no ray of the call is unfinished and then sums the field over the first K track points of
// EVERY ray (K: the trip at which the last start end finished, SDF.py:149-206), so one pixel's depth depends on the whole view.
// Each view gets the K a call over that view alone gets, in two passes over the rays of all views ([n_views][H*W], row-major,
// pixel centres x + 0.5, y + 0.5, each ray formed from its pixel index with ls2fm_camera_rays' arithmetic, camera_ray.h):
//   trips   : the loop of trace_loop.h (steps 1-7), one lane per ray end, until the ray's start end is finished; max over a view's
//             rays -> trips[view] (one atomic per wave).  Nothing else is written.
//   trace   : the same loop for exactly max(K, 1) trips, summing the field's raw value at the start end's track points in
//             ascending k -- finished start ends that still move on a stale step included (step 6) -- as trace_depth_fwd_kernel
//             sums the values ls2fm_sphere_trace leaves in track_sdf: depth, sdf_last, finish, the surface point, t_end after K.
//   normals : ls2fm_sdf_eval's normal query (sdf_eval.hip) over the surface points, in chunks.
// Every output is bit for bit what SDF.sphere_tracing(static_trips=True) and SDF.gradient return for the view's rays.  The
// workspace holds the packed weights and the normal query's (unread) sdf column for one chunk: it depends on nothing else.
#include "camera_ray.h"
#include "trace_loop.h"

namespace {

constexpr int kThreads = 256;                   // two lanes per ray: side 0 = start end (from near), side 1 = far end
constexpr int64_t kNormalChunk = 1 << 20;       // surface points per launch of the normal query (4 MiB of unread sdf column)

struct ImageRays {
    const float* poses;
    Kinv K;
    int64_t hw, total;
    int width;
};

// ray g of the [n_views][hw] image rays: image_rays_kernel's arithmetic (render_image.hip), then load_ray's box clip
__device__ __forceinline__ RayGeom image_ray(const FieldC& fc, const ImageRays& im, int64_t g, int64_t v) {
    const int64_t p = g - v * im.hw;
    float pose[12];
#pragma unroll
    for (int q = 0; q < 12; ++q) pose[q] = im.poses[12 * v + q];
    float c2w[3][4];
    camera_to_world(pose, c2w);
    const float x = (float)(p % im.width) + 0.5f;
    const float y = (float)(p / im.width) + 0.5f;
    RayGeom rg;
    pixel_ray(c2w, im.K, x, y, rg.o, rg.d);
    bool hit;
    ray_box(rg.o, rg.d, fc.box_c, fc.box_h, rg.t_near, rg.t_far, hit);
    return rg;
}

// pass 1: each ray's finishing trip, max over the view's rays into trips[view] (zeroed before the launch).  The loop with the
// exits "the start end is done" and k == iters_max, and no stores
__global__ void __launch_bounds__(kThreads)
trace_image_trips_kernel(LevelSet lv, FieldC fc, const Packed* __restrict__ pk, const float* __restrict__ table, ImageRays im,
                         float thr, int iters_max, int* __restrict__ trips) {
    const int64_t tidg = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    const int64_t r = tidg >> 1;
    const int lane = threadIdx.x & 63;
    const bool live = r < im.total;
    const int64_t g = live ? r : im.total - 1;
    const int64_t v = g / im.hw;
    const RayGeom rg = image_ray(fc, im, g, v);
    const LaneEnds ends{lv, fc, 0, 0.f, pk->sdf, table, (int)(tidg & 1)};         // no background sphere (trace_config)
    TraceEnd e;
    trace_begin(ends, rg, e);
    int kfin = iters_max;
    // both lanes of a ray leave the loop at the same trip: the shuffles always read a lane that is still in it
    for (int k = 0;; ++k) {
        trace_mask(e, thr, k);
        if (!ends.start_unfinished(e.unf)) { kfin = k; break; }           // (3) the start end is done: K does not need more
        if (k == iters_max) break;
        trace_step(e, rg.t_far);
        trace_refresh(ends, rg, e, false);                                // only the unfinished ends' values are read here
        trace_cross(ends, e, k);
    }
    // one atomic per wave for the view of lane 0's ray; rays of another view in the same wave (view boundaries) add their own
    const int kme = (live && ends.side == 0) ? kfin : 0;
    const int64_t v0 = __shfl((int)v, 0, 64);
    const int kmax = wave_max(v == v0 ? kme : 0);
    if (lane == 0 && kmax > 0) atomicMax(trips + v0, kmax);
    if (v != v0 && kme > 0) atomicMax(trips + v, kme);
}

// pass 2: the loop for max(K, 1) trips per ray with the view's K (exits k == K and k + 1 == k_eff), the depth sum and the
// per-pixel outputs
__global__ void __launch_bounds__(kThreads)
trace_image_kernel(LevelSet lv, FieldC fc, const Packed* __restrict__ pk, const float* __restrict__ table, ImageRays im,
                   float thr, float finish_thr, const int* __restrict__ trips, float* __restrict__ depth,
                   float* __restrict__ sdf_last, uint8_t* __restrict__ finish, float* __restrict__ points,
                   float* __restrict__ t_end_k) {
    const int64_t tidg = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    const int64_t r = tidg >> 1;
    const bool live = r < im.total;
    const int64_t g = live ? r : im.total - 1;
    const int64_t v = g / im.hw;
    const int K = trips[v];
    const int k_eff = K < 1 ? 1 : K;
    const RayGeom rg = image_ray(fc, im, g, v);
    const float far = rg.t_far;
    const LaneEnds ends{lv, fc, 0, 0.f, pk->sdf, table, (int)(tidg & 1)};
    TraceEnd e;
    trace_begin(ends, rg, e);
    float acc = 0.f, last = 0.f;
    for (int k = 0;; ++k) {
        trace_mask(e, thr, k);
        last = e.raw;                                                     // track point k (start end): summed in ascending k
        acc += last;
        if (k == K) break;                                                // K = 0: the far end has not moved
        const bool moved = trace_step(e, far);
        if (k + 1 == k_eff) break;                                        // e.t of the far end: t_end after K trips
        trace_refresh(ends, rg, e, ends.side == 0 && moved);              // the start end's value also where it moved stale
        trace_cross(ends, e, k);
    }
    if (!live) return;
    if (ends.side == 1) {
        if (t_end_k) t_end_k[r] = e.t;
        return;
    }
    const float d_sum = acc + rg.t_near;                                  // trace_depth_fwd_kernel: near + sum, clamped to far
    const float d = d_sum > far ? far : d_sum;
    depth[r] = d;
    sdf_last[r] = last;
    finish[r] = fabsf(last) < finish_thr ? 1 : 0;
#pragma unroll
    for (int a = 0; a < 3; ++a) points[3 * r + a] = __fadd_rn(rg.o[a], __fmul_rn(d, rg.d[a]));      // center + depth * ray
}

struct TraceLayout {
    int64_t packed, sdf, total;            // bytes
};

TraceLayout make_trace_layout() {
    TraceLayout m;
    m.packed = 0;
    m.sdf = ((int64_t)sizeof(Packed) + 255) / 256 * 256;
    m.total = m.sdf + (int64_t)kNormalChunk * 4;
    return m;
}

int trace_config(const ls2fm_field_desc* field, const ls2fm_grid_desc* grid) {
    if (!field || !grid_desc_ok(grid)) return LS2FM_ERR_INVALID_ARGUMENT;
    if (field->bg_sdf) return LS2FM_ERR_UNSUPPORTED;                      // the normal query has no background-sphere min
    return LS2FM_OK;
}

}  // namespace

extern "C" int64_t ls2fm_trace_image_workspace_bytes(const ls2fm_field_desc* field, const ls2fm_grid_desc* grid) {
    const int st = trace_config(field, grid);
    if (st != LS2FM_OK) return st;
    return make_trace_layout().total;
}

extern "C" int ls2fm_trace_image(const ls2fm_field_desc* field, const ls2fm_grid_desc* grid, const ls2fm_params* params,
                                 const float* poses, int32_t n_views, const float* kinv_host, int32_t height, int32_t width,
                                 float sdf_threshold, int32_t iters_max, float finish_threshold, float* depth, float* sdf_last,
                                 uint8_t* finish, float* points, float* gradient, float* t_end_k, int32_t* trips, void* workspace,
                                 void* stream) {
    const int st = trace_config(field, grid);
    if (st != LS2FM_OK) return st;
    LS2FM_CHECK_ARG(params && params->sdf_table && params->sdf_mlp[0].weight_v && params->sdf_mlp[1].weight_v);
    LS2FM_CHECK_ARG(poses && kinv_host && depth && sdf_last && finish && points && trips);
    LS2FM_CHECK_ARG(n_views >= 1 && height >= 1 && width >= 1 && iters_max >= 0);
    const int64_t hw = (int64_t)height * width, total = hw * n_views;
    LS2FM_CHECK_ARG(total < ((int64_t)1 << 30));                          // two lanes per ray: the grid stays below 2^31 threads
    if (!workspace) return LS2FM_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    const TraceLayout m = make_trace_layout();
    Packed* pk = (Packed*)((char*)workspace + m.packed);
    float* sdf_scratch = (float*)((char*)workspace + m.sdf);
    int r = ls2fm_launch_prep_sdf(params, grid->n_levels, pk, s);
    if (r != LS2FM_OK) return r;
    if (hipMemsetAsync(trips, 0, sizeof(int32_t) * (size_t)n_views, s) != hipSuccess) return LS2FM_ERR_LAUNCH;
    ImageRays im;
    im.poses = poses;
    for (int q = 0; q < 9; ++q) im.K.k[q] = kinv_host[q];
    im.hw = hw;
    im.total = total;
    im.width = width;
    const FieldC fc = make_field_c(field);
    const LevelSet lv = make_level_set(grid);
    const unsigned blocks = (unsigned)((2 * total + kThreads - 1) / kThreads);
    ls2fm_prof_begin(LS2FM_PROF_SPHERE_TRACE, s);
    trace_image_trips_kernel<<<blocks, kThreads, 0, s>>>(lv, fc, pk, params->sdf_table, im, sdf_threshold, iters_max, trips);
    trace_image_kernel<<<blocks, kThreads, 0, s>>>(lv, fc, pk, params->sdf_table, im, sdf_threshold, finish_threshold, trips, depth,
                                                   sdf_last, finish, points, t_end_k);
    ls2fm_prof_end(LS2FM_PROF_SPHERE_TRACE, s);
    r = ls2fm_launch_status();
    if (r != LS2FM_OK || !gradient) return r;
    for (int64_t at = 0; at < total; at += kNormalChunk) {
        const int64_t n = total - at < kNormalChunk ? total - at : kNormalChunk;
        r = ls2fm_launch_sdf_normals(field, grid, pk, params->sdf_table, points + 3 * at, n, total, sdf_scratch, gradient + 3 * at, s);
        if (r != LS2FM_OK) return r;
    }
    return LS2FM_OK;
}
