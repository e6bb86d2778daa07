// The implicit surface of an oriented point cloud on a dense lattice (ls2fm_cloud_implicit): the primitive under
// ls2fm.cloud_mesh.implicit_from_cloud.  include/ls2fm.h states THE IMPLICIT RULE; tests/cloud_mesh_restate.py repeats it in numpy.
//
// One launch, one lane per lattice point.  The lane forms its own position X (the lattice expression of lattice.h and
// marching_cubes.hip), runs grid_walk.h's k_nearest with the list in registers (capacities 8 / 16 / 32, the smallest that holds
// k), then walks the finished list with compile-time indices, gathers points[i] and normals[i] and forms the two fp64 sums in list
// order.  No atomics, no workspace, nothing read back: the value is a pure function of the cloud, the normals, the lattice, k,
// max_d2 and min_neighbors -- neither the grid's cell size, the brick nor the order of the visits shows in it.
//
// Two launch plans, both instantiated (ls2fm_cloud_implicit_plan chooses, ls2fm_cloud_implicit takes the measured default):
//   brick   0: 2 x 2 x 64, a wave along axis 2 (tsdf_integrate's brick: stores of one 256-byte row, 64 different walks)
//           1: 8 x 8 x 4, a wave a cube of 4 x 4 x 4 lattice points (stores of 16-byte pieces, the lanes walk the same cells)
//   empty   the workgroup first asks whether the grid cells that its brick, grown by the radius, overlaps hold any point: its
//           lanes take the rows of that cell range, one cell_start difference each.  If none does, the brick is written NaN / 0
//           without a walk.  The range is a superset of every cell a qualifying reference of any of the brick's lattice points can
//           lie in (empty_reach), so the test only ever skips walks that would have found nothing: the bits are the same.
#include "grid_walk.h"
#include "lattice.h"
#include "ls2fm_device.h"

#include <cmath>

namespace {

using namespace grid_walk;

constexpr int kThreads = 256;
constexpr int kEmptyTrips = 8;           // rows of the cell range one lane tests at most; a larger range is taken as occupied

template <int BRICK> struct Brick;
template <> struct Brick<0> {
    static constexpr int X = 2, Y = 2, Z = 64;
    static __device__ __forceinline__ void lane(int t, int& x, int& y, int& z) { z = t % 64; y = (t / 64) % 2; x = t / 128; }
};
template <> struct Brick<1> {
    static constexpr int X = 8, Y = 8, Z = 4;
    static __device__ __forceinline__ void lane(int t, int& x, int& y, int& z) {
        const int w = t / 64, l = t % 64;
        z = l & 3;
        y = ((l >> 2) & 3) + 4 * (w >> 1);
        x = (l >> 4) + 4 * (w & 1);
    }
};
static_assert(Brick<0>::X * Brick<0>::Y * Brick<0>::Z == kThreads && Brick<1>::X * Brick<1>::Y * Brick<1>::Z == kThreads, "one lane per point");
static_assert(Brick<0>::X == LS2FM_CLOUD_IMPLICIT_BRICK0_X && Brick<0>::Y == LS2FM_CLOUD_IMPLICIT_BRICK0_Y &&
              Brick<0>::Z == LS2FM_CLOUD_IMPLICIT_BRICK0_Z && Brick<1>::X == LS2FM_CLOUD_IMPLICIT_BRICK1_X &&
              Brick<1>::Y == LS2FM_CLOUD_IMPLICIT_BRICK1_Y && Brick<1>::Z == LS2FM_CLOUD_IMPLICIT_BRICK1_Z, "the header states the bricks");

struct Lattice { int nx, ny, nz; LatticeFrame frame; };

// Whether the cells [cell of (lo - reach), cell of (hi + reach)] per axis hold any point, lo / hi being the brick's lowest and
// highest lattice coordinates.  A reference that qualifies for a lattice point X has fp32 d2 <= max_d2, so |X.a - p.a| <=
// sqrt(max_d2) (1 + 2^-20) on every axis; reach = sqrt(max_d2) * 1.001 + 1e-22 covers that and the rounding of the square root,
// the step to the next float below / above covers the rounding of lo - reach and hi + reach, and cell_axis is monotone in its
// coordinate (a difference, a product with a positive number, a floor and two clamps), so p's cell lies in the range.
template <int BRICK>
__device__ __forceinline__ bool brick_occupied(const PgGrid& g, const int32_t* __restrict__ cell_start, const Lattice& lat, int bx, int by, int bz,
                                               float reach, int t) {
    using B = Brick<BRICK>;
    const float lx = lattice_coord(bx * B::X, lat.frame, 0), hx = lattice_coord(min(bx * B::X + B::X - 1, lat.nx - 1), lat.frame, 0);
    const float ly = lattice_coord(by * B::Y, lat.frame, 1), hy = lattice_coord(min(by * B::Y + B::Y - 1, lat.ny - 1), lat.frame, 1);
    const float lz = lattice_coord(bz * B::Z, lat.frame, 2), hz = lattice_coord(min(bz * B::Z + B::Z - 1, lat.nz - 1), lat.frame, 2);
    const int x0 = cell_axis(nextafterf(__fsub_rn(lx, reach), -INFINITY), g.ox, g.inv_h, g.nx);
    const int x1 = cell_axis(nextafterf(__fadd_rn(hx, reach), INFINITY), g.ox, g.inv_h, g.nx);
    const int y0 = cell_axis(nextafterf(__fsub_rn(ly, reach), -INFINITY), g.oy, g.inv_h, g.ny);
    const int y1 = cell_axis(nextafterf(__fadd_rn(hy, reach), INFINITY), g.oy, g.inv_h, g.ny);
    const int z0 = cell_axis(nextafterf(__fsub_rn(lz, reach), -INFINITY), g.oz, g.inv_h, g.nz);
    const int z1 = cell_axis(nextafterf(__fadd_rn(hz, reach), INFINITY), g.oz, g.inv_h, g.nz);
    // cell_axis is monotone, so the range cannot turn round; were it to, the brick is taken as occupied and walks
    if (x1 < x0 || y1 < y0 || z1 < z0) return true;
    const int span_y = y1 - y0 + 1;
    const int64_t rows = (int64_t)span_y * (z1 - z0 + 1);
    if (rows > (int64_t)kEmptyTrips * kThreads) return true;
    bool found = false;
    for (int r = t; r < (int)rows; r += kThreads) {
        const int64_t row = ((int64_t)(z0 + r / span_y) * g.ny + (y0 + r % span_y)) * g.nx;      // x0 .. x1 + 1 <= nx: inside cell_start
        found = found || cell_start[row + x1 + 1] != cell_start[row + x0];
    }
    return found;
}

template <int CAP, int BRICK>
__global__ void __launch_bounds__(kThreads)
ci_implicit(PgGrid g, const float4* __restrict__ sorted, const int32_t* __restrict__ cell_start, const float* __restrict__ points,
            const float* __restrict__ normals, Lattice lat, int bricks_y, int bricks_z, int k, float max_d2, int min_neighbors, int max_rings,
            int empty_test, float reach, float* __restrict__ value, float* __restrict__ support) {
#pragma clang fp contract(off)
    using B = Brick<BRICK>;
    const int brick = blockIdx.x;
    const int bz = brick % bricks_z, by = (brick / bricks_z) % bricks_y, bx = brick / (bricks_z * bricks_y);
    const int t = threadIdx.x;
    bool occupied = true;
    if (empty_test) occupied = __syncthreads_or(brick_occupied<BRICK>(g, cell_start, lat, bx, by, bz, reach, t)) != 0;   // before any lane leaves
    int lx, ly, lz;
    B::lane(t, lx, ly, lz);
    const int ix = bx * B::X + lx, iy = by * B::Y + ly, iz = bz * B::Z + lz;
    if (ix >= lat.nx || iy >= lat.ny || iz >= lat.nz) return;
    const int64_t at = ((int64_t)ix * lat.ny + iy) * lat.nz + iz;
    if (!occupied) {
        value[at] = NAN;
        if (support) support[at] = 0.0f;
        return;
    }
    const float x = lattice_coord(ix, lat.frame, 0), y = lattice_coord(iy, lat.frame, 1), z = lattice_coord(iz, lat.frame, 2);
    KList<CAP> l;
    k_nearest<CAP>(g, sorted, cell_start, x, y, z, max_d2, -1, k, max_rings, l);
    // the list in its order: filled slots come first, so slot 0 starts both sums
    const double X = (double)x, Y = (double)y, Z = (double)z, lim = (double)max_d2;
    double den = 0.0, num = 0.0;
    int n = 0;
#pragma unroll
    for (int j = 0; j < CAP; ++j) {
        if (j < k && l.d2[j] < INFINITY) {
            const int64_t i = l.i[j];                                    // an index the grid stored: inside points and normals
            const double u = 1.0 - (double)l.d2[j] / lim;
            const double w = (u * u) * u;
            const double px = (double)points[3 * i], py = (double)points[3 * i + 1], pz = (double)points[3 * i + 2];
            const double nx = (double)normals[3 * i], ny = (double)normals[3 * i + 1], nz = (double)normals[3 * i + 2];
            const double s = (nx * (X - px) + ny * (Y - py)) + nz * (Z - pz);
            const double ws = w * s;
            if (j == 0) { den = w; num = ws; } else { den = den + w; num = num + ws; }
            ++n;
        }
    }
    value[at] = (n >= min_neighbors && den > 0.0) ? (float)(num / den) : NAN;
    if (support) support[at] = (float)den;
}

template <int CAP>
void launch(int brick, unsigned blocks, hipStream_t s, const PgGrid& g, const float* sorted, const int32_t* cell_start, const float* points,
            const float* normals, const Lattice& lat, int bricks_y, int bricks_z, int k, float max_d2, int min_neighbors, int rings,
            int empty_test, float reach, float* value, float* support) {
    if (brick == 0)
        ci_implicit<CAP, 0><<<blocks, kThreads, 0, s>>>(g, (const float4*)sorted, cell_start, points, normals, lat, bricks_y, bricks_z, k, max_d2,
                                                        min_neighbors, rings, empty_test, reach, value, support);
    else
        ci_implicit<CAP, 1><<<blocks, kThreads, 0, s>>>(g, (const float4*)sorted, cell_start, points, normals, lat, bricks_y, bricks_z, k, max_d2,
                                                        min_neighbors, rings, empty_test, reach, value, support);
}

}  // namespace

extern "C" int ls2fm_cloud_implicit_plan(const float* points, const float* normals, int64_t n_points, const float* sorted,
                                         const int32_t* cell_start, const float* origin, float cell_size, float inv_cell_size,
                                         const int32_t* dim, int64_t nx, int64_t ny, int64_t nz, const float* lattice_origin, float voxel,
                                         int32_t k, float max_d2, int32_t min_neighbors, int32_t brick, int32_t empty_test, float* value,
                                         float* support, void* stream) {
    int64_t n_cells = 0;
    LS2FM_CHECK_ARG(n_points >= 0 && n_points < ((int64_t)1 << 31) && grid_ok(origin, cell_size, inv_cell_size, dim, &n_cells));
    LS2FM_CHECK_ARG(lattice_ok(nx, ny, nz, 1, voxel) && nx * ny < ((int64_t)1 << 31) && nx * ny * nz < ((int64_t)1 << 31));
    LS2FM_CHECK_ARG(k >= 1 && k <= 32 && max_d2 > 0.0f && max_d2 < INFINITY && min_neighbors >= 1);
    LS2FM_CHECK_ARG((brick == 0 || brick == 1) && (empty_test == 0 || empty_test == 1));
    Lattice lat;
    LS2FM_CHECK_ARG(value && lattice_frame(lattice_origin, voxel, &lat.frame));
    lat.nx = (int)nx; lat.ny = (int)ny; lat.nz = (int)nz;
    hipStream_t s = (hipStream_t)stream;
    const size_t total = (size_t)(nx * ny * nz);
    if (n_points == 0) {                       // no cloud: every lattice point is undefined, without a walk
        if (hipMemsetD32Async((hipDeviceptr_t)value, 0x7fc00000, total, s) != hipSuccess) return ls2fm_launch_status();
        if (support && hipMemsetD32Async((hipDeviceptr_t)support, 0, total, s) != hipSuccess) return ls2fm_launch_status();
        return LS2FM_OK;
    }
    LS2FM_CHECK_ARG(points && normals && sorted && cell_start && ((uintptr_t)sorted & 15) == 0);
    const int bX = brick == 0 ? 2 : 8, bY = brick == 0 ? 2 : 8, bZ = brick == 0 ? 64 : 4;
    const int64_t bricks_x = (nx + bX - 1) / bX, bricks_y = (ny + bY - 1) / bY, bricks_z = (nz + bZ - 1) / bZ;
    const int64_t blocks = bricks_x * bricks_y * bricks_z;             // three factors of at most 2^24: inside int64
    LS2FM_CHECK_ARG(blocks < ((int64_t)1 << 31));
    const PgGrid g = make_grid(origin, cell_size, inv_cell_size, dim);
    const int rings = max_rings(dim);
    const float reach = sqrtf(max_d2) * 1.001f + 1e-22f;
    if (k <= 8) launch<8>(brick, (unsigned)blocks, s, g, sorted, cell_start, points, normals, lat, (int)bricks_y, (int)bricks_z, k, max_d2, min_neighbors, rings, empty_test, reach, value, support);
    else if (k <= 16) launch<16>(brick, (unsigned)blocks, s, g, sorted, cell_start, points, normals, lat, (int)bricks_y, (int)bricks_z, k, max_d2, min_neighbors, rings, empty_test, reach, value, support);
    else launch<32>(brick, (unsigned)blocks, s, g, sorted, cell_start, points, normals, lat, (int)bricks_y, (int)bricks_z, k, max_d2, min_neighbors, rings, empty_test, reach, value, support);
    return ls2fm_launch_status();
}

extern "C" int ls2fm_cloud_implicit(const float* points, const float* normals, int64_t n_points, const float* sorted, const int32_t* cell_start,
                                    const float* origin, float cell_size, float inv_cell_size, const int32_t* dim, int64_t nx, int64_t ny,
                                    int64_t nz, const float* lattice_origin, float voxel, int32_t k, float max_d2, int32_t min_neighbors,
                                    float* value, float* support, void* stream) {
    return ls2fm_cloud_implicit_plan(points, normals, n_points, sorted, cell_start, origin, cell_size, inv_cell_size, dim, nx, ny, nz,
                                     lattice_origin, voxel, k, max_d2, min_neighbors, LS2FM_CLOUD_IMPLICIT_BRICK, LS2FM_CLOUD_IMPLICIT_EMPTY_TEST,
                                     value, support, stream);
}
