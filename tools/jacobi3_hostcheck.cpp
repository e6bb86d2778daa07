// Stand-alone host build of csrc/pose_math.h's jacobi3_sym (the __host__ __device__ routine cloud_normals.hip runs per lane): 200
// random covariance-like matrices (every fourth of rank 2, every fifth of rank 1), a diagonal one and the zero matrix, inputs and
// results printed as hex floats.  tests/test_cloud_host.py compiles it with the host compiler under -fsanitize=address,undefined
// and -ffp-contract=off and holds every printed result to the bits of tests/cloud_restate.py's jacobi3.
//   g++ -std=c++17 -ffp-contract=off -fsanitize=address,undefined -I level-s2fm_official_amd/csrc tools/jacobi3_hostcheck.cpp
#include <cstdio>
#include <cmath>
#define HD
#include "pose_math.h"

static void run(const double (&c)[6]) {
    double a[6], V[3][3];
    for (int e = 0; e < 6; ++e) a[e] = c[e];
    pose_math::jacobi3_sym(a, V);
    for (int e = 0; e < 6; ++e) printf(" %a", c[e]);
    printf(" %a %a %a", a[pose_math::sidx3(0, 0)], a[pose_math::sidx3(1, 1)], a[pose_math::sidx3(2, 2)]);
    for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) printf(" %a", V[i][j]);
    printf("\n");
}

int main() {
    unsigned long long s = 2024;
    auto rnd = [&]() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (double)(s >> 11) / 9007199254740992.0 * 2.0 - 1.0; };
    for (int it = 0; it < 200; ++it) {
        const int rows = it % 5 == 4 ? 1 : (it % 4 == 3 ? 2 : 16);
        double c[6] = {0, 0, 0, 0, 0, 0};
        for (int r = 0; r < rows; ++r) {
            const double d[3] = {rnd(), rnd(), rnd() * (it % 3 == 0 ? 1e-3 : 1.0)};
            for (int i = 0; i < 3; ++i) for (int j = i; j < 3; ++j) c[pose_math::sidx3(i, j)] += d[i] * d[j];
        }
        run(c);
    }
    const double diagonal[6] = {3.0, 0.0, 0.0, 1.0, 0.0, 2.0}, zero[6] = {0, 0, 0, 0, 0, 0};
    run(diagonal);
    run(zero);
    return 0;
}
