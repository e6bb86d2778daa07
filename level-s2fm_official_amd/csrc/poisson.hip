// Screened Poisson reconstruction of an oriented point cloud on the dense lattice (ls2fm_poisson_solve): the solver under
// ls2fm.cloud_mesh.poisson_from_cloud.  include/ls2fm.h states THE POISSON RULE; tests/poisson_restate.py repeats it in numpy.
//
// Every lattice operation is one rounded fp32 operation in the rule's order (__fadd_rn, __fmul_rn, __fdiv_rn: nothing contracts), and
// the splat sums integers, so the result is a pure function of the cloud, the lattice, screen, cycles and gamma: neither the order of
// the atomics, the brick, the launch plan nor a rerun shows in a bit of it.
//
// The stencil expressions are written once, as device functions over anything that indexes like a float array (relaxed, residual_at,
// restrict_at, prolong_at); the global kernels instantiate them over global memory and the tail kernel over LDS:
//   ps_clear/_zero  the accumulators and chi zeroed by launches (a captured memset node is not ordered with the kernels after it)
//   ps_splat        one lane per point: 32 integer atomics, four accumulators per lattice point side by side (32 bytes)
//   ps_finish_rhs   one lane per lattice point: its own sums and those of its six neighbours -> V (optional), W and b
//   ps_sweep        one colour of one sweep: a brick of 2 x 2 x 128 lattice points per workgroup, a wave along axis 2, a lane at
//                   every second point (those of the colour): six neighbours, b and W read, chi written; deg from the indices
//   ps_restrict     one lane per coarse point: the 27 fine residuals formed on the fly (or, without b, the field itself: R W)
//   ps_prolong      one lane per fine point: chi += P e
//   ps_tail         from the first level of at most LS2FM_POISSON_TAIL_POINTS points downward the whole sub-cycle in ONE workgroup
//                   and one launch: sweeps, residuals, transfers and the coarsest sweeps with chi, b and W of all those levels in LDS
#include "lattice.h"
#include "ls2fm_device.h"
#include "workspace.h"

#include <algorithm>
#include <cmath>

namespace {

constexpr int kThreads = 256;
constexpr int kBrickX = LS2FM_POISSON_BRICK_X, kBrickY = LS2FM_POISSON_BRICK_Y, kBrickZ = LS2FM_POISSON_BRICK_Z;
static_assert(kBrickX * kBrickY * (kBrickZ / 2) == kThreads && kBrickZ == 128, "a wave along axis 2, a lane at every second point");
constexpr int kMaxLevels = 26;                      // a side of at most 2^24 halves 24 times
constexpr int kTailThreads = 1024;
constexpr int kTailLevels = 8;                      // at most 4096 points with every side >= 4: a side of at most 256
// the points of all the tail's levels together: a side n >= 4 becomes (n + 1) / 2 <= 0.6 n, a level at most 0.216 of the one above,
// so at most 4096 / (1 - 0.216) = 5225 points.  Three arrays of them are 62 976 bytes of LDS
constexpr int kTailFloats = 5248;
static_assert(LS2FM_POISSON_TAIL_POINTS == 4096 && 3 * kTailFloats * sizeof(float) <= 65536, "the tail's levels fit the LDS");
constexpr int kCoarsestSweeps = 32, kEdgeSweeps = 2;
constexpr double kToFloat = 1.0 / 4294967296.0;     // the accumulators count 2^-32

struct Dim { int n0, n1, n2; };
static inline int total_of(const Dim& d) { return d.n0 * d.n1 * d.n2; }

// ----------------------------------------------------------------------------------------------------- the stencil, stated once
// N_i, the existing neighbours in the order -0, +0, -1, +1, -2, +2 from the first that exists, and deg_i, their count
template <typename F>
__device__ __forceinline__ float neighbour_sum(F chi, const Dim& d, int i0, int i1, int i2, int at, int& deg) {
    const int s0 = d.n1 * d.n2, s1 = d.n2;
    float N = 0.0f;
    int n = 0;
    auto take = [&](bool exists, int j) {
        if (exists) {
            const float v = chi[j];
            N = n ? __fadd_rn(N, v) : v;
            ++n;
        }
    };
    take(i0 > 0, at - s0);
    take(i0 + 1 < d.n0, at + s0);
    take(i1 > 0, at - s1);
    take(i1 + 1 < d.n1, at + s1);
    take(i2 > 0, at - 1);
    take(i2 + 1 < d.n2, at + 1);
    deg = n;
    return N;
}

// the smoother's value of point `at`: fl(fl(b + fl(s N)) / fl(fl(s deg) + fl(a W)))
template <typename F, typename G>
__device__ __forceinline__ float relaxed(F chi, G b, G W, const Dim& d, int i0, int i1, int i2, int at, float s, float a) {
    int deg;
    const float N = neighbour_sum(chi, d, i0, i1, i2, at, deg);
    const float D = __fadd_rn(__fmul_rn(s, (float)deg), __fmul_rn(a, W[at]));
    return __fdiv_rn(__fadd_rn(b[at], __fmul_rn(s, N)), D);
}

// r = fl(b - fl(fl(s fl(fl(deg chi) - N)) + fl(fl(a W) chi)))
template <typename F, typename G>
__device__ __forceinline__ float residual_at(F chi, G b, G W, const Dim& d, int i0, int i1, int i2, float s, float a) {
    const int at = (i0 * d.n1 + i1) * d.n2 + i2;
    int deg;
    const float N = neighbour_sum(chi, d, i0, i1, i2, at, deg);
    const float x = chi[at];
    return __fsub_rn(b[at], __fadd_rn(__fmul_rn(s, __fsub_rn(__fmul_rn((float)deg, x), N)), __fmul_rn(__fmul_rn(a, W[at]), x)));
}

// restriction along one axis of n fine points at coarse index I: 0.5 r[2I] + 0.25 r[2I - 1] + c r[2I + 1], c = 0.5 at the last
// point of an even side, the terms that exist in this order
template <typename G>
__device__ __forceinline__ float restrict3(int n, int I, G get) {
    const int j = 2 * I;
    float acc = __fmul_rn(0.5f, get(j));
    if (j > 0) acc = __fadd_rn(acc, __fmul_rn(0.25f, get(j - 1)));
    if (j + 1 < n) acc = __fadd_rn(acc, __fmul_rn(j + 2 == n ? 0.5f : 0.25f, get(j + 1)));
    return acc;
}

// axes 0, 1, 2 in turn: the innermost lambda is axis 0.  value(j0, j1, j2) is the fine field
template <typename V>
__device__ __forceinline__ float restrict_at(V value, const Dim& fine, int I0, int I1, int I2) {
    return restrict3(fine.n2, I2, [&](int j2) {
        return restrict3(fine.n1, I1, [&](int j1) { return restrict3(fine.n0, I0, [&](int j0) { return value(j0, j1, j2); }); });
    });
}

// prolongation along one axis to fine index i: a copy at even i, the halved sum of the two coarse neighbours at odd i (the upper
// one clamped: the last point of an even side copies its only neighbour)
template <typename G>
__device__ __forceinline__ float prolong2(int nc, int i, G get) {
    const int k = i >> 1;
    if ((i & 1) == 0) return get(k);
    return __fmul_rn(0.5f, __fadd_rn(get(k), get(min(k + 1, nc - 1))));
}

template <typename F>
__device__ __forceinline__ float prolong_at(F e, const Dim& c, int i0, int i1, int i2) {
    return prolong2(c.n2, i2, [&](int c2) {
        return prolong2(c.n1, i1, [&](int c1) { return prolong2(c.n0, i0, [&](int c0) { return e[(c0 * c.n1 + c1) * c.n2 + c2]; }); });
    });
}

// ------------------------------------------------------------------------------------------------------------ splat and finish
// rint(v 2^32) through the double's mantissa: bin_scatter.hip's add_fixed, exact while |v| 2^32 < 2^51
__device__ __forceinline__ void add_fixed(unsigned long long* slot, double v) {
    const double d = fma(v, 4294967296.0, 6755399441055744.0);
    atomicAdd(slot, (unsigned long long)__double_as_longlong(d) - 0x4338000000000000ull);
}

// zeroes n 16-byte pieces.  A launch, not hipMemsetAsync: a captured memset node is not ordered with the kernel nodes after it
// (DESIGN 3.16), kernel nodes are ordered among themselves
__global__ void __launch_bounds__(kThreads)
ps_clear(uint4* __restrict__ out, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i < n) out[i] = uint4{0u, 0u, 0u, 0u};
}

__global__ void __launch_bounds__(kThreads)
ps_zero(float* __restrict__ out, float* __restrict__ also, int total) {
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= total) return;
    out[i] = 0.0f;
    if (also) also[i] = 0.0f;
}

__global__ void __launch_bounds__(kThreads)
ps_splat(const float* __restrict__ points, const float* __restrict__ normals, int n_points, Dim d, LatticeFrame frame,
         unsigned long long* __restrict__ acc) {
    const int p = blockIdx.x * kThreads + threadIdx.x;
    if (p >= n_points) return;
    const float P[3] = {points[3 * (int64_t)p], points[3 * (int64_t)p + 1], points[3 * (int64_t)p + 2]};
    const float N[3] = {normals[3 * (int64_t)p], normals[3 * (int64_t)p + 1], normals[3 * (int64_t)p + 2]};
    const int side[3] = {d.n0, d.n1, d.n2};
    float u[3];
    bool ok = true;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        u[a] = __fdiv_rn(__fsub_rn(P[a], frame.origin[a]), frame.voxel);
        ok = ok && fabsf(P[a]) < INFINITY && fabsf(N[a]) < INFINITY && u[a] >= 0.0f && u[a] < (float)(side[a] - 1);
    }
    if (!ok) return;
    int cell[3];                                      // 0 <= cell[a] <= side[a] - 2 here: the conversion is in range and all eight
    float f[3];                                       // corners are lattice points
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float low = floorf(u[a]);
        cell[a] = (int)low;
        f[a] = __fsub_rn(u[a], low);
    }
    const double N0 = (double)N[0], N1 = (double)N[1], N2 = (double)N[2];
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        const int dx = c >> 2, dy = (c >> 1) & 1, dz = c & 1;
        const float wx = dx ? f[0] : __fsub_rn(1.0f, f[0]), wy = dy ? f[1] : __fsub_rn(1.0f, f[1]), wz = dz ? f[2] : __fsub_rn(1.0f, f[2]);
        const double w = (double)__fmul_rn(__fmul_rn(wx, wy), wz);
        const int64_t at = ((int64_t)(cell[0] + dx) * d.n1 + (cell[1] + dy)) * d.n2 + (cell[2] + dz);
        unsigned long long* slot = acc + 4 * at;
        add_fixed(slot, w * N0);                      // exact in fp64: two 24-bit significands
        add_fixed(slot + 1, w * N1);
        add_fixed(slot + 2, w * N2);
        add_fixed(slot + 3, w);
    }
}

__global__ void __launch_bounds__(kThreads)
ps_finish_rhs(const long long* __restrict__ acc, Dim d, int total, float* __restrict__ V, float* __restrict__ b, float* __restrict__ W) {
    const int at = blockIdx.x * kThreads + threadIdx.x;
    if (at >= total) return;
    const int i2 = at % d.n2, i1 = (at / d.n2) % d.n1, i0 = at / (d.n2 * d.n1);
    const int idx[3] = {i0, i1, i2}, side[3] = {d.n0, d.n1, d.n2}, stride[3] = {d.n1 * d.n2, d.n2, 1};
    auto sum = [&](int j, int a) { return (float)((double)acc[4 * (int64_t)j + a] * kToFloat); };
    float t[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float v = sum(at, a);
        if (V) V[(int64_t)a * total + at] = v;
        float below = 0.0f, above = 0.0f;             // a missing edge counts as 0
        if (idx[a] > 0) below = __fmul_rn(0.5f, __fadd_rn(sum(at - stride[a], a), v));
        if (idx[a] + 1 < side[a]) above = __fmul_rn(0.5f, __fadd_rn(v, sum(at + stride[a], a)));
        t[a] = __fsub_rn(below, above);
    }
    b[at] = __fadd_rn(__fadd_rn(t[0], t[1]), t[2]);
    W[at] = sum(at, 3);
}

// ------------------------------------------------------------------------------------------------------------ the global levels
__global__ void __launch_bounds__(kThreads)
ps_sweep(float* chi, const float* __restrict__ b, const float* __restrict__ W, Dim d, int bricks1, int bricks2, float s, float a, int colour) {
    const int brick = blockIdx.x;
    const int bz = brick % bricks2, by = (brick / bricks2) % bricks1, bx = brick / (bricks2 * bricks1);
    const int t = threadIdx.x;
    const int i0 = bx * kBrickX + (t >> 7), i1 = by * kBrickY + ((t >> 6) & 1);
    const int i2 = bz * kBrickZ + 2 * (t & 63) + ((i0 + i1 + colour) & 1);
    if (i0 >= d.n0 || i1 >= d.n1 || i2 >= d.n2) return;
    const int at = (i0 * d.n1 + i1) * d.n2 + i2;
    chi[at] = relaxed((const float*)chi, b, W, d, i0, i1, i2, at, s, a);        // the six neighbours are of the other colour
}

// coarse[I] = R (residual of chi, b, W), and coarse_chi[I] = 0 when given; with b == NULL, coarse[I] = R chi (the field itself)
__global__ void __launch_bounds__(kThreads)
ps_restrict(const float* __restrict__ chi, const float* __restrict__ b, const float* __restrict__ W, Dim fine, float s, float a, Dim c,
            int coarse_total, float* __restrict__ coarse, float* __restrict__ coarse_chi) {
    const int at = blockIdx.x * kThreads + threadIdx.x;
    if (at >= coarse_total) return;
    const int I2 = at % c.n2, I1 = (at / c.n2) % c.n1, I0 = at / (c.n2 * c.n1);
    if (b)
        coarse[at] = restrict_at([&](int j0, int j1, int j2) { return residual_at(chi, b, W, fine, j0, j1, j2, s, a); }, fine, I0, I1, I2);
    else
        coarse[at] = restrict_at([&](int j0, int j1, int j2) { return chi[(j0 * fine.n1 + j1) * fine.n2 + j2]; }, fine, I0, I1, I2);
    if (coarse_chi) coarse_chi[at] = 0.0f;
}

__global__ void __launch_bounds__(kThreads)
ps_prolong(float* __restrict__ chi, Dim fine, int total, const float* __restrict__ e, Dim c) {
    const int at = blockIdx.x * kThreads + threadIdx.x;
    if (at >= total) return;
    const int i2 = at % fine.n2, i1 = (at / fine.n2) % fine.n1, i0 = at / (fine.n2 * fine.n1);
    chi[at] = __fadd_rn(chi[at], prolong_at(e, c, i0, i1, i2));
}

// ------------------------------------------------------------------------------------------------------------------- the tail
struct TailPlan {
    int levels;                                      // 1 .. kTailLevels
    Dim d[kTailLevels];
    int total[kTailLevels], first[kTailLevels];      // the points of a level and where its arrays start within chi / b / W
    float s[kTailLevels];
};

// every point of a level, the threads striding; the body gets (i0, i1, i2, at)
template <typename Body>
__device__ __forceinline__ void each_point(const Dim& d, int total, Body body) {
    for (int at = threadIdx.x; at < total; at += kTailThreads) body(at / (d.n2 * d.n1), (at / d.n2) % d.n1, at % d.n2, at);
}

// cycle(top) of the rule on the levels of the plan, chi of the top level from and to global memory.  One workgroup; the walk
// through the levels is the same for every thread (`visits` counts the descents from each level, two bits a level)
__global__ void __launch_bounds__(kTailThreads)
ps_tail(TailPlan plan, float* __restrict__ chi_top, const float* __restrict__ b_top, const float* __restrict__ W_top, float a, int gamma) {
    __shared__ float s_chi[kTailFloats], s_b[kTailFloats], s_W[kTailFloats];
    for (int at = threadIdx.x; at < plan.total[0]; at += kTailThreads) {
        s_chi[at] = chi_top[at];
        s_b[at] = b_top[at];
        s_W[at] = W_top[at];
    }
    __syncthreads();
    for (int l = 0; l + 1 < plan.levels; ++l) {      // W_{l + 1} = R W_l
        const Dim fine = plan.d[l], c = plan.d[l + 1];
        const float* Wf = s_W + plan.first[l];
        float* Wc = s_W + plan.first[l + 1];
        each_point(c, plan.total[l + 1], [&](int I0, int I1, int I2, int at) {
            Wc[at] = restrict_at([&](int j0, int j1, int j2) { return Wf[(j0 * fine.n1 + j1) * fine.n2 + j2]; }, fine, I0, I1, I2);
        });
        __syncthreads();
    }
    auto sweeps = [&](int l, int count) {
        const Dim d = plan.d[l];
        float* chi = s_chi + plan.first[l];
        const float *b = s_b + plan.first[l], *W = s_W + plan.first[l];
        const float s = plan.s[l];
        for (int k = 0; k < 2 * count; ++k) {
            each_point(d, plan.total[l], [&](int i0, int i1, int i2, int at) {
                if (((i0 + i1 + i2 + k) & 1) == 0) chi[at] = relaxed((const float*)chi, b, W, d, i0, i1, i2, at, s, a);
            });
            __syncthreads();
        }
    };
    const int last = plan.levels - 1;
    unsigned visits = 0;
    int l = 0;
    bool entering = true;
    while (true) {
        if (entering) {
            if (l == last) {
                sweeps(l, kCoarsestSweeps);
                if (l == 0) break;
                --l;
                entering = false;
                continue;
            }
            sweeps(l, kEdgeSweeps);
            visits &= ~(3u << (2 * l));
        } else {                                     // back from level l + 1: chi_l += P chi_{l + 1}
            const Dim d = plan.d[l], c = plan.d[l + 1];
            float* chi = s_chi + plan.first[l];
            const float* e = s_chi + plan.first[l + 1];
            each_point(d, plan.total[l], [&](int i0, int i1, int i2, int at) { chi[at] = __fadd_rn(chi[at], prolong_at(e, c, i0, i1, i2)); });
            __syncthreads();
        }
        if ((int)((visits >> (2 * l)) & 3u) < gamma) {
            const Dim d = plan.d[l], c = plan.d[l + 1];
            const float *chi = s_chi + plan.first[l], *b = s_b + plan.first[l], *W = s_W + plan.first[l];
            float *cb = s_b + plan.first[l + 1], *cchi = s_chi + plan.first[l + 1];
            const float s = plan.s[l];
            each_point(c, plan.total[l + 1], [&](int I0, int I1, int I2, int at) {
                cb[at] = restrict_at([&](int j0, int j1, int j2) { return residual_at(chi, b, W, d, j0, j1, j2, s, a); }, d, I0, I1, I2);
                cchi[at] = 0.0f;
            });
            __syncthreads();
            visits += 1u << (2 * l);
            ++l;
            entering = true;
        } else {
            sweeps(l, kEdgeSweeps);
            if (l == 0) break;
            --l;
            entering = false;
        }
    }
    for (int at = threadIdx.x; at < plan.total[0]; at += kTailThreads) chi_top[at] = s_chi[at];
}

// ------------------------------------------------------------------------------------------------------------------ the host
static inline unsigned blocks_for(int64_t n) { return (unsigned)((n + kThreads - 1) / kThreads); }

bool dims_ok(int64_t nx, int64_t ny, int64_t nz) {
    return nx >= 2 && ny >= 2 && nz >= 2 && nx <= (1 << 24) && ny <= (1 << 24) && nz <= (1 << 24) && nx * ny < ((int64_t)1 << 31) &&
           nx * ny * nz < ((int64_t)1 << 31);
}

void launch_sweep_colour(float* chi, const float* b, const float* W, const Dim& d, float s, float a, int colour, hipStream_t st) {
    const int b0 = (d.n0 + kBrickX - 1) / kBrickX, b1 = (d.n1 + kBrickY - 1) / kBrickY, b2 = (d.n2 + kBrickZ - 1) / kBrickZ;
    ps_sweep<<<(unsigned)((int64_t)b0 * b1 * b2), kThreads, 0, st>>>(chi, b, W, d, b1, b2, s, a, colour);    // fewer bricks than lattice points
}

void launch_restrict(const float* chi, const float* b, const float* W, const Dim& fine, float s, float a, float* coarse, float* coarse_chi,
                     hipStream_t st) {
    const Dim c{(fine.n0 + 1) / 2, (fine.n1 + 1) / 2, (fine.n2 + 1) / 2};
    ps_restrict<<<blocks_for(total_of(c)), kThreads, 0, st>>>(chi, b, W, fine, s, a, c, total_of(c), coarse, coarse_chi);
}

void launch_prolong(float* chi, const Dim& fine, const float* e, hipStream_t st) {
    const Dim c{(fine.n0 + 1) / 2, (fine.n1 + 1) / 2, (fine.n2 + 1) / 2};
    ps_prolong<<<blocks_for(total_of(fine)), kThreads, 0, st>>>(chi, fine, total_of(fine), e, c);
}

struct Level { Dim d; float s; float *chi, *b, *W; };

struct Solver {
    int levels = 0, tail = -1;                       // tail: the first level the tail kernel runs, -1 without one
    Level level[kMaxLevels];
    TailPlan plan;
    float a;
    int gamma;
    hipStream_t st;

    void sweeps(const Level& L, int count) const {
        for (int k = 0; k < 2 * count; ++k) launch_sweep_colour(L.chi, L.b, L.W, L.d, L.s, a, k & 1, st);
    }

    void cycle(int l) const {
        const Level& L = level[l];
        if (l == tail) {
            ps_tail<<<1, kTailThreads, 0, st>>>(plan, L.chi, L.b, L.W, a, gamma);
            return;
        }
        if (l == levels - 1) {
            sweeps(L, kCoarsestSweeps);
            return;
        }
        sweeps(L, kEdgeSweeps);
        for (int g = 0; g < gamma; ++g) {
            launch_restrict(L.chi, L.b, L.W, L.d, L.s, a, level[l + 1].b, level[l + 1].chi, st);
            cycle(l + 1);
            launch_prolong(L.chi, L.d, level[l + 1].chi, st);
        }
        sweeps(L, kEdgeSweeps);
    }
};

// the shapes of the levels: level l + 1 exists while level l has its smallest side >= 4 and its largest >= 5
int level_dims(Dim d, Dim* out) {
    int n = 0;
    out[n++] = d;
    while (n < kMaxLevels && std::min({d.n0, d.n1, d.n2}) >= 4 && std::max({d.n0, d.n1, d.n2}) >= 5) {
        d = Dim{(d.n0 + 1) / 2, (d.n1 + 1) / 2, (d.n2 + 1) / 2};
        out[n++] = d;
    }
    return n;
}

// The workspace: the accumulators (32 bytes a lattice point), whose bytes the coarse levels' chi, b and W take over once the
// finish has read them, then b of level 0.  Run over a NULL base it only sizes
struct Layout { unsigned long long* acc; float* b0; float* coarse[kMaxLevels][3]; };

size_t layout(void* base, const Dim* dims, int levels, Layout* out) {
    const size_t total = (size_t)total_of(dims[0]);
    Workspace coarse(base, 256);
    for (int l = 1; l < levels; ++l)
        for (int q = 0; q < 3; ++q) {
            float* p = coarse.take<float>((size_t)total_of(dims[l]));
            if (out) out->coarse[l][q] = p;
        }
    Workspace ws(base, 256);
    unsigned long long* acc = ws.take<unsigned long long>(4 * total);
    if (coarse.bytes() > ws.bytes()) ws.take<char>(coarse.bytes() - ws.bytes());
    float* b0 = ws.take<float>(total);
    if (out) { out->acc = acc; out->b0 = b0; }
    return ws.bytes();
}

int splat_finish(const float* points, const float* normals, int64_t n, const Dim& d, const LatticeFrame& frame, unsigned long long* acc,
                 float* V, float* b, float* W, hipStream_t st) {
    const int total = total_of(d);
    ps_clear<<<blocks_for(2 * (int64_t)total), kThreads, 0, st>>>((uint4*)acc, 2 * (int64_t)total);       // 32 bytes a lattice point
    if (n) ps_splat<<<blocks_for(n), kThreads, 0, st>>>(points, normals, (int)n, d, frame, acc);
    ps_finish_rhs<<<blocks_for(total), kThreads, 0, st>>>((const long long*)acc, d, total, V, b, W);
    return ls2fm_launch_status();
}

}  // namespace

extern "C" int64_t ls2fm_poisson_workspace_bytes(int64_t nx, int64_t ny, int64_t nz) {
    if (!dims_ok(nx, ny, nz)) return -1;
    Dim dims[kMaxLevels];
    const int levels = level_dims(Dim{(int)nx, (int)ny, (int)nz}, dims);
    return (int64_t)layout(nullptr, dims, levels, nullptr);
}

extern "C" int ls2fm_poisson_solve_plan(const float* points, const float* normals, int64_t n_points, int64_t nx, int64_t ny, int64_t nz,
                                        const float* origin, float voxel, float screen, int32_t cycles, int32_t gamma, int32_t tail_points,
                                        float* value, float* density, void* workspace, int64_t workspace_bytes, void* stream) {
    LS2FM_CHECK_ARG(n_points >= 0 && n_points < ((int64_t)1 << 31) && dims_ok(nx, ny, nz) && lattice_ok(nx, ny, nz, 2, voxel));
    LS2FM_CHECK_ARG(cycles >= 0 && (gamma == 1 || gamma == 2) && screen > 0.0f && screen < INFINITY);
    LS2FM_CHECK_ARG(tail_points == 0 || tail_points == LS2FM_POISSON_TAIL_POINTS);
    LatticeFrame frame;
    LS2FM_CHECK_ARG(value && density && lattice_frame(origin, voxel, &frame) && (n_points == 0 || (points && normals)));
    Dim dims[kMaxLevels];
    Solver S;
    S.levels = level_dims(Dim{(int)nx, (int)ny, (int)nz}, dims);
    Layout at;
    LS2FM_CHECK_ARG(workspace && ((uintptr_t)workspace & 255) == 0 && workspace_bytes >= (int64_t)layout(workspace, dims, S.levels, &at));
    hipStream_t st = (hipStream_t)stream;
    const size_t total = (size_t)total_of(dims[0]);
    ps_zero<<<blocks_for((int64_t)total), kThreads, 0, st>>>(value, n_points == 0 ? density : nullptr, (int)total);
    if (n_points == 0) return ls2fm_launch_status();          // no cloud: chi = 0 and W = 0 without a sweep
    const int status = splat_finish(points, normals, n_points, dims[0], frame, at.acc, nullptr, at.b0, density, st);
    if (status != LS2FM_OK) return status;
    S.a = screen;
    S.gamma = gamma;
    S.st = st;
    for (int l = 0; l < S.levels; ++l) {
        S.level[l] = l ? Level{dims[l], ldexpf(1.0f, -2 * l), at.coarse[l][0], at.coarse[l][1], at.coarse[l][2]}
                       : Level{dims[0], 1.0f, value, at.b0, density};
        if (l) launch_restrict(S.level[l - 1].W, nullptr, nullptr, dims[l - 1], 0.0f, 0.0f, S.level[l].W, nullptr, st);       // W_l = R W_{l-1}
    }
    if (tail_points)
        for (int l = 0; l < S.levels && S.tail < 0; ++l)
            if (total_of(dims[l]) <= tail_points) S.tail = l;
    if (S.tail >= 0) {
        TailPlan& p = S.plan;
        p = TailPlan{};
        p.levels = S.levels - S.tail;
        int first = 0;
        for (int k = 0; k < p.levels && k < kTailLevels; ++k) {
            p.d[k] = dims[S.tail + k];
            p.total[k] = total_of(p.d[k]);
            p.first[k] = first;
            p.s[k] = S.level[S.tail + k].s;
            first += p.total[k];
        }
        if (p.levels > kTailLevels || first > kTailFloats) return LS2FM_ERR_INVALID_ARGUMENT;      // cannot happen (see kTailFloats)
    }
    for (int c = 0; c < cycles; ++c) S.cycle(0);
    return ls2fm_launch_status();
}

extern "C" int ls2fm_poisson_solve(const float* points, const float* normals, int64_t n_points, int64_t nx, int64_t ny, int64_t nz,
                                   const float* origin, float voxel, float screen, int32_t cycles, int32_t gamma, float* value, float* density,
                                   void* workspace, int64_t workspace_bytes, void* stream) {
    return ls2fm_poisson_solve_plan(points, normals, n_points, nx, ny, nz, origin, voxel, screen, cycles, gamma, LS2FM_POISSON_TAIL_POINTS,
                                    value, density, workspace, workspace_bytes, stream);
}

// ------------------------------------------------------------------------------------------- the stages, one at a time (the tests)
extern "C" int ls2fm_poisson_splat(const float* points, const float* normals, int64_t n_points, int64_t nx, int64_t ny, int64_t nz,
                                   const float* origin, float voxel, float* V, float* b, float* density, void* workspace,
                                   int64_t workspace_bytes, void* stream) {
    LS2FM_CHECK_ARG(n_points >= 0 && n_points < ((int64_t)1 << 31) && dims_ok(nx, ny, nz) && lattice_ok(nx, ny, nz, 2, voxel));
    LatticeFrame frame;
    LS2FM_CHECK_ARG(b && density && lattice_frame(origin, voxel, &frame) && (n_points == 0 || (points && normals)));
    LS2FM_CHECK_ARG(workspace && ((uintptr_t)workspace & 255) == 0 && workspace_bytes >= nx * ny * nz * 32);
    return splat_finish(points, normals, n_points, Dim{(int)nx, (int)ny, (int)nz}, frame, (unsigned long long*)workspace, V, b, density,
                        (hipStream_t)stream);
}

extern "C" int ls2fm_poisson_sweep_colour(float* chi, const float* b, const float* density, int64_t nx, int64_t ny, int64_t nz, float scale,
                                          float screen, int32_t colour, void* stream) {
    LS2FM_CHECK_ARG(chi && b && density && dims_ok(nx, ny, nz) && scale > 0.0f && scale <= 1.0f && screen > 0.0f && screen < INFINITY);
    LS2FM_CHECK_ARG(colour == 0 || colour == 1);
    launch_sweep_colour(chi, b, density, Dim{(int)nx, (int)ny, (int)nz}, scale, screen, colour, (hipStream_t)stream);
    return ls2fm_launch_status();
}

extern "C" int ls2fm_poisson_restrict(const float* chi, const float* b, const float* density, int64_t nx, int64_t ny, int64_t nz, float scale,
                                      float screen, float* coarse, void* stream) {
    LS2FM_CHECK_ARG(chi && coarse && dims_ok(nx, ny, nz) && (b == nullptr) == (density == nullptr));
    LS2FM_CHECK_ARG(!b || (scale > 0.0f && scale <= 1.0f && screen > 0.0f && screen < INFINITY));
    launch_restrict(chi, b, density, Dim{(int)nx, (int)ny, (int)nz}, scale, screen, coarse, nullptr, (hipStream_t)stream);
    return ls2fm_launch_status();
}

extern "C" int ls2fm_poisson_prolong(float* chi, int64_t nx, int64_t ny, int64_t nz, const float* coarse, void* stream) {
    LS2FM_CHECK_ARG(chi && coarse && dims_ok(nx, ny, nz));
    launch_prolong(chi, Dim{(int)nx, (int)ny, (int)nz}, coarse, (hipStream_t)stream);
    return ls2fm_launch_status();
}
