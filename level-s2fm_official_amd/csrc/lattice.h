// The dense lattice of ls2fm_tsdf_integrate and ls2fm_cloud_implicit, stated once (ls2fm/lattice.py is the Python side): lattice
// point i of an axis sits at fl32(fl32((float) i * voxel) + origin), marching cubes' vertex expression with spacing = (voxel,) * 3.
#pragma once

#include "ls2fm_device.h"

struct LatticeFrame { float origin[3]; float voxel; };

// coordinate `axis` of lattice index i.  Every side is at most 2^24 (lattice_ok), so the index converts exactly
template <typename Index>
__device__ __forceinline__ float lattice_coord(Index i, const LatticeFrame& f, int axis) { return __fadd_rn(__fmul_rn((float)i, f.voxel), f.origin[axis]); }

// host: three sides in [least, 2^24] and a positive finite voxel
static inline bool lattice_ok(int64_t nx, int64_t ny, int64_t nz, int64_t least, float voxel) {
    return nx >= least && ny >= least && nz >= least && nx <= (1 << 24) && ny <= (1 << 24) && nz <= (1 << 24) && voxel > 0.0f && voxel < INFINITY;
}

// host: the frame of a finite origin, three floats read before the call returns.  false for NULL, a NaN or an infinity
static inline bool lattice_frame(const float* origin, float voxel, LatticeFrame* frame) {
    if (!(origin && fabsf(origin[0]) < INFINITY && fabsf(origin[1]) < INFINITY && fabsf(origin[2]) < INFINITY)) return false;
    *frame = LatticeFrame{{origin[0], origin[1], origin[2]}, voxel};
    return true;
}
