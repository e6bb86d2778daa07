// A triangle rasteriser with a z-buffer: which faces of a mesh each camera sees, mesh depth maps, per-pixel face ids and
// barycentrics (ls2fm_rasterize), and per-vertex mask votes (ls2fm_mesh_mask_votes): the primitives under ls2fm.raster.
// include/ls2fm.h states the RASTERISATION RULE; tests/raster_restate.py repeats it in numpy.
//
// The rule makes the images a pure function of the inputs: fp32 camera points and projections of one rounding per operation, a
// snap to 8 sub-pixel bits, coverage in exact integers with one owner per shared edge, one fp64 depth expression per pixel, and
// the minimum of key = bits(z) << 32 | face over the faces that cover the pixel.  No visiting order or path shows in it.
//
// ls2fm_rasterize (three launches):
//   raster_clear    the z-buffer to all-ones.  A launch, not hipMemsetAsync: captured into a graph, the memset node was seen not to
//                   be ordered with the kernels that follow it (on a second replay the raster kernel met keys the memset had not
//                   yet overwritten, and the z-buffer held none of its bytes afterwards); launches are ordered among themselves.
//   raster_faces    one lane per (view, face); the view is the block's, so the pose and intrinsics are scalar loads.  Set the
//                   face up, clip its box of pixel centres to the image, reject an empty box; a box of at most
//                   LS2FM_RASTER_LANE_PIXELS pixels is walked by the lane.  Then the wave ballots the lanes that hold a larger
//                   box, takes them one at a time, broadcasts the set-up and strides the box with all 64 lanes.  Both paths call
//                   shade(): the same integer and fp64 expressions per pixel.
//   raster_resolve  one lane per pixel: unpack face_id and depth, recompute the winner's barycentrics, count the face's pixels.
// ls2fm_mesh_mask_votes (one launch): mask_votes, one lane per vertex, the views in a loop.
#include "ls2fm_device.h"
#include "raster_project.h"

#include <algorithm>
#include <cmath>

namespace {

constexpr int kThreads = 256;
constexpr int kMaxViewBlocks = 65535;          // gridDim.y; further views are taken by the kernels' view loops
constexpr int64_t kClearBlocks = 1 << 16;       // raster_clear strides the z-buffer with at most this many workgroups
constexpr unsigned long long kEmptyKey = ~0ull;

__device__ __forceinline__ int snap(float u) { return (int)rintf(__fmul_rn(u, 256.0f)); }

// a face set up in one view.  area = |A|, 0 for a face that is not drawn; s = sign(A).
struct Face {
    int ua, va, ub, vb, uc, vc;
    int s;
    int64_t area;
    double ra, rb, rc;
};

__device__ __forceinline__ int64_t mul64(int a, int b) { return (int64_t)a * (int64_t)b; }

__device__ __forceinline__ Face setup_face(const View& w, const float* __restrict__ verts, int64_t n_verts,
                                           const int32_t* __restrict__ faces, int64_t f, float near) {
#pragma clang fp contract(off)
    Face t = {};
    const int32_t ia = faces[3 * f], ib = faces[3 * f + 1], ic = faces[3 * f + 2];
    if (ia < 0 || ib < 0 || ic < 0 || ia >= n_verts || ib >= n_verts || ic >= n_verts) return t;
    const Projected a = project(w, verts[3 * (int64_t)ia], verts[3 * (int64_t)ia + 1], verts[3 * (int64_t)ia + 2], near);
    const Projected b = project(w, verts[3 * (int64_t)ib], verts[3 * (int64_t)ib + 1], verts[3 * (int64_t)ib + 2], near);
    const Projected c = project(w, verts[3 * (int64_t)ic], verts[3 * (int64_t)ic + 1], verts[3 * (int64_t)ic + 2], near);
    if (!(a.usable && b.usable && c.usable)) return t;
    t.ua = snap(a.u); t.va = snap(a.v);
    t.ub = snap(b.u); t.vb = snap(b.v);
    t.uc = snap(c.u); t.vc = snap(c.v);
    const int64_t A = mul64(t.ub - t.ua, t.vc - t.va) - mul64(t.vb - t.va, t.uc - t.ua);
    t.s = A > 0 ? 1 : -1;
    t.area = A > 0 ? A : -A;
    t.ra = 1.0 / (double)a.z;
    t.rb = 1.0 / (double)b.z;
    t.rc = 1.0 / (double)c.z;
    return t;
}

// s E_pq(P) and whether the edge p -> q owns its boundary; P in snapped units
__device__ __forceinline__ bool edge(int s, int up, int vp, int uq, int vq, int X, int Y, int64_t& w) {
    const int dx = s * (uq - up), dy = s * (vq - vp);
    w = mul64(dx, Y - vp) - mul64(dy, X - up);
    return w > 0 || (w == 0 && (dy > 0 || (dy == 0 && dx > 0)));
}

// coverage of pixel (px, py) and the three weights
__device__ __forceinline__ bool cover(const Face& t, int px, int py, int64_t& wa, int64_t& wb, int64_t& wc) {
    const int X = 256 * px + 128, Y = 256 * py + 128;
    const bool a = edge(t.s, t.ub, t.vb, t.uc, t.vc, X, Y, wa);
    const bool b = edge(t.s, t.uc, t.vc, t.ua, t.va, X, Y, wb);
    const bool c = edge(t.s, t.ua, t.va, t.ub, t.vb, X, Y, wc);
    return a && b && c;
}

__device__ __forceinline__ double depth_denominator(const Face& t, int64_t wa, int64_t wb, int64_t wc) {
#pragma clang fp contract(off)
    return ((double)wa * t.ra + (double)wb * t.rb) + (double)wc * t.rc;
}

// one pixel of one face: coverage, depth, z-test.  zbuf is the view's [H][W] plane; (px, py) lies inside the image.
__device__ __forceinline__ void shade(const Face& t, uint32_t f, int px, int py, int width, unsigned long long* zbuf) {
#pragma clang fp contract(off)
    int64_t wa, wb, wc;
    if (!cover(t, px, py, wa, wb, wc)) return;
    const float z = (float)((double)t.area / depth_denominator(t, wa, wb, wc));
    const unsigned long long key = ((unsigned long long)__float_as_uint(z) << 32) | f;
    unsigned long long* p = zbuf + (int64_t)py * width + px;
    if (key < *p) atomicMin(p, key);          // keys only fall: a stale read can only cost an atomic that changes nothing
}

// the pixels whose centres lie inside the face's bounds, clipped to the image: 256 px + 128 >= U_min and <= U_max
struct Box { int x0, x1, y0, y1; };

__device__ __forceinline__ Box clip_box(const Face& t, int height, int width) {
    const int umin = min(t.ua, min(t.ub, t.uc)), umax = max(t.ua, max(t.ub, t.uc));
    const int vmin = min(t.va, min(t.vb, t.vc)), vmax = max(t.va, max(t.vb, t.vc));
    Box b;
    b.x0 = max((umin + 127) >> 8, 0);          // ceil((U_min - 128) / 256); >> is the floor for negatives too
    b.x1 = min((umax - 128) >> 8, width - 1);
    b.y0 = max((vmin + 127) >> 8, 0);
    b.y1 = min((vmax - 128) >> 8, height - 1);
    return b;
}

__device__ __forceinline__ int bcast(int v, int lane) { return __builtin_amdgcn_readlane(v, lane); }

__device__ __forceinline__ double bcast(double v, int lane) {
    const int lo = bcast(__double2loint(v), lane), hi = bcast(__double2hiint(v), lane);
    return __hiloint2double(hi, lo);
}

__global__ void __launch_bounds__(kThreads)
raster_clear(unsigned long long* __restrict__ zbuf, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kThreads) zbuf[i] = kEmptyKey;
}

__global__ void __launch_bounds__(kThreads)
raster_faces(const float* __restrict__ verts, int64_t n_verts, const int32_t* __restrict__ faces, int64_t n_faces,
             const float* __restrict__ poses, const float* __restrict__ intr, int n_views, int height, int width, float near,
             unsigned long long* zbuf) {
    const int64_t f = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    const int lane = threadIdx.x & 63;
    // no lane leaves before the ballots below: a lane past the last face holds a face that is not drawn
    for (int view = blockIdx.y; view < n_views; view += gridDim.y) {
        const View w = load_view(poses, intr, view);
        unsigned long long* plane = zbuf + (int64_t)view * height * width;
        Face t = {};
        if (f < n_faces) t = setup_face(w, verts, n_verts, faces, f, near);
        Box b = {0, -1, 0, -1};
        if (t.area != 0) b = clip_box(t, height, width);
        const bool live = b.x0 <= b.x1 && b.y0 <= b.y1;
        const int n_pix = live ? (b.x1 - b.x0 + 1) * (b.y1 - b.y0 + 1) : 0;          // <= 2^30
        if (live && n_pix <= LS2FM_RASTER_LANE_PIXELS)
            for (int py = b.y0; py <= b.y1; ++py)
                for (int px = b.x0; px <= b.x1; ++px) shade(t, (uint32_t)f, px, py, width, plane);
        unsigned long long large = __ballot(n_pix > LS2FM_RASTER_LANE_PIXELS);
        while (large) {
            const int src = __builtin_amdgcn_readfirstlane(__ffsll(large) - 1);
            large &= large - 1;
            Face g;
            g.ua = bcast(t.ua, src); g.va = bcast(t.va, src);
            g.ub = bcast(t.ub, src); g.vb = bcast(t.vb, src);
            g.uc = bcast(t.uc, src); g.vc = bcast(t.vc, src);
            g.s = bcast(t.s, src);
            g.ra = bcast(t.ra, src); g.rb = bcast(t.rb, src); g.rc = bcast(t.rc, src);
            const int64_t A = mul64(g.ub - g.ua, g.vc - g.va) - mul64(g.vb - g.va, g.uc - g.ua);
            g.area = A > 0 ? A : -A;
            const int x0 = bcast(b.x0, src), x1 = bcast(b.x1, src), y0 = bcast(b.y0, src), n = bcast(n_pix, src);
            const uint32_t gf = (uint32_t)(blockIdx.x * (unsigned)kThreads + (threadIdx.x & ~63u) + (unsigned)src);
            const int bw = x1 - x0 + 1;
            for (int i = lane; i < n; i += 64) {
                const int row = i / bw;
                shade(g, gf, x0 + (i - row * bw), y0 + row, width, plane);
            }
        }
    }
}

__global__ void __launch_bounds__(kThreads)
raster_resolve(const float* __restrict__ verts, int64_t n_verts, const int32_t* __restrict__ faces, int64_t n_faces,
               const float* __restrict__ poses, const float* __restrict__ intr, int n_views, int height, int width, float near,
               const unsigned long long* __restrict__ zbuf, int32_t* __restrict__ face_id, float* __restrict__ depth,
               float* __restrict__ bary, int32_t* face_hits) {
#pragma clang fp contract(off)
    const int64_t hw = (int64_t)height * width;
    const int64_t pix = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (pix >= hw) return;
    for (int view = blockIdx.y; view < n_views; view += gridDim.y) {
        const int64_t at = (int64_t)view * hw + pix;
        const unsigned long long key = zbuf[at];
        // every key raster_faces wrote carries a face below n_faces; the comparison keeps face_hits in bounds whatever zbuf holds
        const bool hit = key != kEmptyKey && (int64_t)(uint32_t)key < n_faces;
        const int32_t f = hit ? (int32_t)(uint32_t)key : -1;
        face_id[at] = f;
        depth[at] = hit ? __uint_as_float((uint32_t)(key >> 32)) : INFINITY;
        if (hit && face_hits) atomicAdd(face_hits + f, 1);
        if (!bary) continue;
        float b0 = 0.0f, b1 = 0.0f, b2 = 0.0f;
        if (hit) {
            const View w = load_view(poses, intr, view);
            const Face t = setup_face(w, verts, n_verts, faces, f, near);
            int64_t wa, wb, wc;
            if (t.area != 0 && cover(t, (int)(pix % width), (int)(pix / width), wa, wb, wc)) {
                const double num = depth_denominator(t, wa, wb, wc);
                b0 = (float)(((double)wa * t.ra) / num);
                b1 = (float)(((double)wb * t.rb) / num);
                b2 = (float)(((double)wc * t.rc) / num);
            }
        }
        bary[3 * at] = b0; bary[3 * at + 1] = b1; bary[3 * at + 2] = b2;
    }
}

__global__ void __launch_bounds__(kThreads)
mask_votes(const float* __restrict__ verts, int64_t n_verts, const float* __restrict__ poses, const float* __restrict__ intr,
           int n_views, int height, int width, float near, const uint8_t* __restrict__ masks, int32_t* __restrict__ seen,
           int32_t* __restrict__ inside) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n_verts) return;
    const float x = verts[3 * i], y = verts[3 * i + 1], z = verts[3 * i + 2];
    int n_seen = 0, n_inside = 0;
    for (int view = 0; view < n_views; ++view) {
        const View w = load_view(poses, intr, view);
        const Projected p = project(w, x, y, z, near);
        int px, py;
        if (pixel_of(p, height, width, px, py)) {
            ++n_seen;
            n_inside += masks[((int64_t)view * height + py) * width + px] != 0;
        }
    }
    seen[i] = n_seen;
    inside[i] = n_inside;
}

bool image_ok(int32_t n_views, int32_t height, int32_t width) { return raster_image_ok(n_views, height, width); }

bool near_ok(float near) { return raster_near_ok(near); }

}  // namespace

extern "C" int64_t ls2fm_rasterize_workspace_bytes(int32_t n_views, int32_t height, int32_t width) {
    if (!image_ok(n_views, height, width)) return (int64_t)LS2FM_ERR_INVALID_ARGUMENT;
    return (int64_t)n_views * height * width * (int64_t)sizeof(unsigned long long);
}

extern "C" int ls2fm_rasterize(const float* verts, int64_t n_verts, const int32_t* faces, int64_t n_faces, const float* poses,
                               const float* intr, int32_t n_views, int32_t height, int32_t width, float near, int32_t* face_id,
                               float* depth, float* bary, int32_t* face_hits, void* workspace, void* stream) {
    LS2FM_CHECK_ARG(n_verts >= 0 && n_faces >= 0 && n_faces < ((int64_t)1 << 31) && image_ok(n_views, height, width) && near_ok(near));
    if (n_views == 0) return LS2FM_OK;
    LS2FM_CHECK_ARG(poses && intr && face_id && depth && ((verts && faces) || n_faces == 0));
    if (!workspace) return LS2FM_ERR_WORKSPACE;
    LS2FM_CHECK_ARG(((uintptr_t)workspace & 7) == 0);
    hipStream_t s = (hipStream_t)stream;
    unsigned long long* zbuf = (unsigned long long*)workspace;
    const int64_t hw = (int64_t)height * width;
    const unsigned view_blocks = (unsigned)std::min<int32_t>(n_views, kMaxViewBlocks);
    const int64_t n_keys = n_views * hw;
    raster_clear<<<(unsigned)std::min<int64_t>((n_keys + kThreads - 1) / kThreads, kClearBlocks), kThreads, 0, s>>>(zbuf, n_keys);
    if (n_faces > 0)
        raster_faces<<<dim3((unsigned)((n_faces + kThreads - 1) / kThreads), view_blocks), kThreads, 0, s>>>(
            verts, n_verts, faces, n_faces, poses, intr, n_views, height, width, near, zbuf);
    raster_resolve<<<dim3((unsigned)((hw + kThreads - 1) / kThreads), view_blocks), kThreads, 0, s>>>(
        verts, n_verts, faces, n_faces, poses, intr, n_views, height, width, near, zbuf, face_id, depth, bary, face_hits);
    return ls2fm_launch_status();
}

extern "C" int ls2fm_mesh_mask_votes(const float* verts, int64_t n_verts, const float* poses, const float* intr, int32_t n_views,
                                     int32_t height, int32_t width, float near, const uint8_t* masks, int32_t* seen, int32_t* inside,
                                     void* stream) {
    LS2FM_CHECK_ARG(n_verts >= 0 && n_verts < ((int64_t)1 << 31) * kThreads && image_ok(n_views, height, width) && near_ok(near));
    if (n_verts == 0) return LS2FM_OK;
    LS2FM_CHECK_ARG(verts && seen && inside && ((poses && intr && masks) || n_views == 0));
    mask_votes<<<(unsigned)((n_verts + kThreads - 1) / kThreads), kThreads, 0, (hipStream_t)stream>>>(
        verts, n_verts, poses, intr, n_views, height, width, near, masks, seen, inside);
    return ls2fm_launch_status();
}
