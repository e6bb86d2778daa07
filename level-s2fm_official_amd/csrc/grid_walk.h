// The walk of the uniform point grid, stated once for point_grid.hip (pg_query, pg_knn) and icp.hip (icp_accumulate): the grid's
// description, the cell assignment, the distance rule, the ring bound and the ring loops -- nearest for the one nearest
// reference, k_nearest for the k nearest in a register-resident sorted list.  include/ls2fm.h states the rules;
// tests/metrics_restate.py repeats the distance rule in numpy.  Every routine is a fixed sequence of fp32 operations, so the
// winner, its d2 and its coordinates are the same bits in whichever file includes it.
#pragma once

#include <algorithm>
#include <climits>
#include <cmath>

#include "ls2fm_device.h"

namespace grid_walk {

struct PgGrid {
    float ox, oy, oz;      // origin: the per-axis minimum of the reference cloud
    float h, inv_h;        // cell size and the fp32 reciprocal the cells are assigned with
    float slack;           // cells by which the fp32 cell assignment can misplace a pair of points (ring_bound)
    int nx, ny, nz;
};

// the cell of coordinate p on one axis: clamp(floor((p - o) * inv_h), 0, dim - 1).  Clamped in float first -- fminf / fmaxf return
// the operand that is not NaN, so a NaN or infinite coordinate lands in a border cell -- and again as an integer, since
// (float)(dim - 1) rounds up above 2^24.  Nothing is indexed with an unclamped value.
__device__ __forceinline__ int cell_axis(float p, float o, float inv_h, int dim) {
    const float u = __fmul_rn(__fsub_rn(p, o), inv_h);
    const float c = fmaxf(fminf(floorf(u), (float)(dim - 1)), 0.0f);
    return min(max((int)c, 0), dim - 1);
}

__device__ __forceinline__ int64_t cell_of(const PgGrid& g, float x, float y, float z) {
    const int cx = cell_axis(x, g.ox, g.inv_h, g.nx), cy = cell_axis(y, g.oy, g.inv_h, g.ny), cz = cell_axis(z, g.oz, g.inv_h, g.nz);
    return ((int64_t)cz * g.ny + cy) * g.nx + cx;
}

// the distance rule.  Spelled with the rounded-operation intrinsics and compiled with contraction off for this function, so
// the result does not depend on the build's -ffp-contract flag.
__device__ __forceinline__ float d2_rule(float qx, float qy, float qz, float rx, float ry, float rz) {
#pragma clang fp contract(off)
    const float dx = __fsub_rn(qx, rx), dy = __fsub_rn(qy, ry), dz = __fsub_rn(qz, rz);
    return __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz));
}

// What may be skipped.  Once rings 0 .. k are done, an unvisited reference r differs from the query q by more than k cells on
// some axis, so u(r) - u(q) > k there, u(p) = fl(fl(p - o) * inv_h) being what the cell is the floor of (clamping a query that
// lies outside the box only moves its cell TOWARD the references).  u carries two roundings, an error of at most 2^-23 |u|
// <= 2^-23 dim cells per point, and inv_h one more on the difference: the true separation is at least (k - slack) h with
// slack = 2^-21 max(dim), twice the error of the pair.  fp32 d2 is within 2^-22 relative of the true squared distance,
// and the factor 1 - 2^-18 leaves that sixteen-fold: every unvisited reference has d2 > bound.  So the walk may stop when
// best_d2 < bound -- strictly, so that a tied reference of a later ring, which may hold the lower index, is still visited --
// or when max_d2 < bound, since nothing further out can qualify.
__device__ __forceinline__ float ring_bound(const PgGrid& g, int k) {
    const float kk = __fsub_rn((float)k, g.slack);
    if (!(kk > 0.0f)) return 0.0f;
    const float l = __fmul_rn(kk, g.h);
    return __fmul_rn(__fmul_rn(l, l), 1.0f - 0x1p-18f);
}

// the winner so far: its d2, its original index and its stored coordinates (i = INT_MAX, d2 = +inf: none yet)
struct Best { float d2; int32_t i; float x, y, z; };

__device__ __forceinline__ void visit(const float4* __restrict__ sorted, int32_t s, int32_t e, float qx, float qy, float qz,
                                      float max_d2, Best& b) {
    for (int32_t p = s; p < e; ++p) {
        const float4 r = sorted[p];
        const float d2 = d2_rule(qx, qy, qz, r.x, r.y, r.z);
        const int32_t i = __float_as_int(r.w);
        if (d2 <= max_d2 && d2 < INFINITY && (d2 < b.d2 || (d2 == b.d2 && i < b.i))) { b.d2 = d2; b.i = i; b.x = r.x; b.y = r.y; b.z = r.z; }
    }
}

// The ring loop: the query's own cell, then Chebyshev rings 1, 2, ... until ring_bound lets it stop or the whole grid is done
// (max_rings is the hard trip bound).  A NaN or infinite query has no neighbour: it takes no walk at all (its d2 would never
// compare below +inf).  -> the winner; b.i stays INT_MAX and b.d2 +inf without one.
__device__ __forceinline__ Best nearest(const PgGrid& g, const float4* __restrict__ sorted, const int32_t* __restrict__ cell_start,
                                        float qx, float qy, float qz, float max_d2, int max_rings) {
    Best b = {INFINITY, INT_MAX, 0.0f, 0.0f, 0.0f};
    const int cx = cell_axis(qx, g.ox, g.inv_h, g.nx), cy = cell_axis(qy, g.oy, g.inv_h, g.ny), cz = cell_axis(qz, g.oz, g.inv_h, g.nz);
    const bool finite = isfinite(qx) && isfinite(qy) && isfinite(qz);
    for (int k = 0; finite && k < max_rings; ++k) {
        const int x0 = max(cx - k, 0), x1 = min(cx + k, g.nx - 1);
        const int y0 = max(cy - k, 0), y1 = min(cy + k, g.ny - 1);
        const int z0 = max(cz - k, 0), z1 = min(cz + k, g.nz - 1);
        for (int z = z0; z <= z1; ++z) {
            const bool z_face = z == cz - k || z == cz + k;
            for (int y = y0; y <= y1; ++y) {
                const int64_t row = ((int64_t)z * g.ny + y) * g.nx;
                if (z_face || y == cy - k || y == cy + k) {
                    // a whole row of the shell: its cells are neighbours in cell_start, one range
                    visit(sorted, cell_start[row + x0], cell_start[row + x1 + 1], qx, qy, qz, max_d2, b);
                } else {
                    if (cx - k >= 0) visit(sorted, cell_start[row + cx - k], cell_start[row + cx - k + 1], qx, qy, qz, max_d2, b);
                    if (cx + k < g.nx) visit(sorted, cell_start[row + cx + k], cell_start[row + cx + k + 1], qx, qy, qz, max_d2, b);
                }
            }
        }
        if (fminf(b.d2, max_d2) < ring_bound(g, k)) break;
        if (cx - k <= 0 && cx + k >= g.nx - 1 && cy - k <= 0 && cy + k >= g.ny - 1 && cz - k <= 0 && cz + k >= g.nz - 1) break;   // the whole grid
    }
    return b;
}

// ------------------------------------------------------------------------------------------------------------- k nearest
// The K-NEIGHBOUR RULE (include/ls2fm.h): the qualifying references ordered by (d2, index) ascending, the first k of them.
// KList is that list in registers: CAP slots kept sorted, an empty slot being (+inf, INT_MAX), which every qualifying candidate
// precedes.  Every index into it is a compile-time one (full unrolling): a runtime index would send it to scratch or to LDS.
// The runtime k is the WORST SLOT: (wd2, wi) is a copy of slot k - 1, a candidate enters only when it precedes that, and the
// walk stops on wd2 -- +inf while fewer than k are held.  Slots k .. CAP - 1 would only ever receive what slot k - 1 sheds; they
// are never read and the insertion skips them, so the capacity shows neither in the result nor in the insertion's length.
template <int CAP>
struct KList {
    float d2[CAP];
    int32_t i[CAP];
    float wd2;
    int32_t wi;
};

template <int CAP>
__device__ __forceinline__ void klist_init(KList<CAP>& l) {
#pragma unroll
    for (int j = 0; j < CAP; ++j) { l.d2[j] = INFINITY; l.i[j] = INT_MAX; }
    l.wd2 = INFINITY;
    l.wi = INT_MAX;
}

__device__ __forceinline__ bool precedes(float d2, int32_t i, float e_d2, int32_t e_i) { return d2 < e_d2 || (d2 == e_d2 && i < e_i); }

// compare-and-shift: slot j takes its left neighbour when the candidate precedes that one, the candidate when it precedes only
// slot j itself, and keeps its entry otherwise (slots are updated from the right, so slot j - 1 is still the old one)
template <int CAP>
__device__ __forceinline__ void klist_insert(KList<CAP>& l, int k, float d2, int32_t i) {
#pragma unroll
    for (int j = CAP - 1; j >= 1; --j) {
        if (j >= k) continue;                                   // never read; k is uniform, so this is a scalar branch
        const bool left = precedes(d2, i, l.d2[j - 1], l.i[j - 1]);
        const bool here = precedes(d2, i, l.d2[j], l.i[j]);
        l.d2[j] = left ? l.d2[j - 1] : (here ? d2 : l.d2[j]);
        l.i[j] = left ? l.i[j - 1] : (here ? i : l.i[j]);
    }
    if (precedes(d2, i, l.d2[0], l.i[0])) { l.d2[0] = d2; l.i[0] = i; }
#pragma unroll
    for (int j = 0; j < CAP; ++j)
        if (j == k - 1) { l.wd2 = l.d2[j]; l.wi = l.i[j]; }
}

// skip: the original index that is not a neighbour (skip_own), -1 for none
template <int CAP>
__device__ __forceinline__ void visit_k(const float4* __restrict__ sorted, int32_t s, int32_t e, float qx, float qy, float qz,
                                        float max_d2, int32_t skip, int k, KList<CAP>& l) {
    for (int32_t p = s; p < e; ++p) {
        const float4 r = sorted[p];
        const float d2 = d2_rule(qx, qy, qz, r.x, r.y, r.z);
        const int32_t i = __float_as_int(r.w);
        if (d2 <= max_d2 && d2 < INFINITY && i != skip && precedes(d2, i, l.wd2, l.wi)) klist_insert(l, k, d2, i);
    }
}

// nearest's ring loop with the list in Best's place.  A row of the shell is one range of cell_start, a row through its inside
// two single cells; both go through the one visit_k below, so that the unrolled insertion is instantiated once.
template <int CAP>
__device__ __forceinline__ void k_nearest(const PgGrid& g, const float4* __restrict__ sorted, const int32_t* __restrict__ cell_start,
                                          float qx, float qy, float qz, float max_d2, int32_t skip, int k, int max_rings, KList<CAP>& l) {
    klist_init(l);
    const int cx = cell_axis(qx, g.ox, g.inv_h, g.nx), cy = cell_axis(qy, g.oy, g.inv_h, g.ny), cz = cell_axis(qz, g.oz, g.inv_h, g.nz);
    const bool finite = isfinite(qx) && isfinite(qy) && isfinite(qz);
    for (int r = 0; finite && r < max_rings; ++r) {
        const int x0 = max(cx - r, 0), x1 = min(cx + r, g.nx - 1);
        const int y0 = max(cy - r, 0), y1 = min(cy + r, g.ny - 1);
        const int z0 = max(cz - r, 0), z1 = min(cz + r, g.nz - 1);
        for (int z = z0; z <= z1; ++z) {
            const bool z_face = z == cz - r || z == cz + r;
            for (int y = y0; y <= y1; ++y) {
                const int64_t row = ((int64_t)z * g.ny + y) * g.nx;
                const bool whole = z_face || y == cy - r || y == cy + r;
                for (int part = 0; part < (whole ? 1 : 2); ++part) {
                    const int xa = whole ? x0 : (part == 0 ? cx - r : cx + r);
                    const int xb = whole ? x1 : xa;
                    if (xa < 0 || xb >= g.nx) continue;                      // that side of the shell lies outside the grid
                    visit_k(sorted, cell_start[row + xa], cell_start[row + xb + 1], qx, qy, qz, max_d2, skip, k, l);
                }
            }
        }
        if (fminf(l.wd2, max_d2) < ring_bound(g, r)) break;
        if (cx - r <= 0 && cx + r >= g.nx - 1 && cy - r <= 0 && cy + r >= g.ny - 1 && cz - r <= 0 && cz + r >= g.nz - 1) break;   // the whole grid
    }
}

// ------------------------------------------------------------------------------------------------------------------- host
inline bool grid_ok(const float* origin, float h, float inv_h, const int32_t* dim, int64_t* n_cells) {
    if (!origin || !dim || !(h > 0.0f) || !std::isfinite(h) || !(inv_h > 0.0f) || !std::isfinite(inv_h)) return false;
    int64_t cells = 1;
    for (int a = 0; a < 3; ++a) {
        if (!std::isfinite(origin[a]) || dim[a] < 1) return false;
        cells *= dim[a];
        if (cells >= ((int64_t)1 << 31) - 1) return false;
    }
    *n_cells = cells;
    return true;
}

inline PgGrid make_grid(const float* origin, float h, float inv_h, const int32_t* dim) {
    const int max_dim = std::max(dim[0], std::max(dim[1], dim[2]));
    return {origin[0], origin[1], origin[2], h, inv_h, (float)max_dim * 0x1p-21f, dim[0], dim[1], dim[2]};
}

// the hard trip bound of the ring loop
inline int max_rings(const int32_t* dim) { return std::max(dim[0], std::max(dim[1], dim[2])) + 1; }

}  // namespace grid_walk
