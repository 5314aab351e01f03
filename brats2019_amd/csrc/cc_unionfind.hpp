// Union-find on voxel indices for the 26-connected labellings (inference.hip: ru_cc_reject; lesion.hip: ru_lesion_metrics).
// parent[v] = v for a root, a smaller index of the same component otherwise, -1 for background; roots are the smallest index of their
// component (atomicMin), which is also the order in which scipy.ndimage.label numbers components.
#pragma once
#include <hip/hip_runtime.h>

namespace ru {

__device__ __forceinline__ int cc_find(const int* parent, int i) {
    int p = __hip_atomic_load(parent + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);          // L2-served: other CUs' links are seen
    while (p != i) { i = p; p = __hip_atomic_load(parent + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }      // parents only ever decrease: terminates
    return i;
}
__device__ __forceinline__ void cc_unite(int* parent, int a, int b) {
    for (;;) {
        a = cc_find(parent, a);
        b = cc_find(parent, b);
        if (a == b) return;
        if (a > b) { const int t = a; a = b; b = t; }     // a < b: hang b under a
        const int old = atomicMin(parent + b, a);
        if (old == b) return;                             // b was still a root: linked
        b = old;                                          // somebody re-parented b meanwhile: continue from there (the atomic's value is never stale)
    }
}
// the 13 neighbours that precede a voxel in linear order
__device__ __forceinline__ bool cc_earlier(int dz, int dy, int dx) { return dz < 0 || (dz == 0 && (dy < 0 || (dy == 0 && dx < 0))); }

}  // namespace ru
