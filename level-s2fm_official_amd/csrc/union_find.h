// Lock-free union-find over int32 node ids, shared by mesh_components.hip (vertices joined by faces) and tracks.hip (key points
// joined by matches).  Every parent pointer points to a SMALLER index, so a root is the minimum of its tree and the final labels
// do not depend on the order of the unions.  Every access to `parent` is an agent-scope atomic: workgroups on other XCDs read and
// move the same pointers inside one launch.  Nothing waits on another workgroup.
#pragma once

#include "ls2fm_device.h"

namespace union_find {

__device__ __forceinline__ int32_t ld_parent(const int32_t* parent, int32_t x) {
    return __hip_atomic_load(parent + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ bool cas_parent(int32_t* parent, int32_t x, int32_t expected, int32_t desired) {
    return __hip_atomic_compare_exchange_strong(parent + x, &expected, desired, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                                __HIP_MEMORY_SCOPE_AGENT);
}

// root of x; halves the path on the way (g, the grandparent, is an ancestor of x, so pointing x at it keeps the forest; a failed
// exchange means x already points higher)
__device__ __forceinline__ int32_t find_root(int32_t* parent, int32_t x) {
    for (;;) {
        const int32_t p = ld_parent(parent, x);
        if (p == x) return x;
        const int32_t g = ld_parent(parent, p);
        if (g == p) return p;
        cas_parent(parent, x, p, g);
        x = g;
    }
}

__device__ __forceinline__ void unite(int32_t* parent, int32_t a, int32_t b) {
    for (;;) {
        a = find_root(parent, a);
        b = find_root(parent, b);
        if (a == b) return;
        if (a > b) {
            const int32_t t = a;
            a = b;
            b = t;
        }
        if (cas_parent(parent, b, b, a)) return;           // the larger root goes under the smaller one
    }
}

}  // namespace union_find
