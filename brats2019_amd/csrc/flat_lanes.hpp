// Flat streaming passes over n float32-sized elements (hardcrit.hip, boundary.hip), in optim.hip's lane layout: a lane owns 4 consecutive
// elements moved as 16 bytes, the elements before the first 16-byte boundary and after the last whole quad are taken one by one, the grid
// is capped and strides.  Sums are one float64 slot per workgroup, added in a fixed order by one workgroup: no float atomics.
// Everything here has internal linkage: each translation unit that includes the header gets its own copy of the kernel it launches.
#pragma once
#include "ru_common.h"
#include "pw_helpers.hpp"

#include <stdint.h>

namespace ru {
namespace {

constexpr int FL_BLOCK = 256;
constexpr unsigned FL_GRID_CAP = 2048;           // 256 CUs x 8 workgroups; the rest by grid stride

// [0, head) one by one | nq quads from `head` | the remaining (< 4) elements one by one.  Quads only when every pointer of the call sits at
// the same offset from a 16-byte boundary; otherwise everything goes one by one.
struct Lanes { size_t head, nq; };
template <int N>
inline Lanes lanes_for(size_t n, const void* const (&ptrs)[N]) {
    const uintptr_t a0 = (uintptr_t)ptrs[0] & 15u;
    bool alike = (a0 & 3u) == 0;
    for (int i = 1; i < N; ++i)
        if (ptrs[i] && ((uintptr_t)ptrs[i] & 15u) != a0) alike = false;
    if (!alike) return Lanes{n, 0};
    size_t head = ((16u - a0) & 15u) / 4u;
    if (head > n) head = n;
    return Lanes{head, (n - head) / 4};
}
// an upper bound of the grid for every alignment: the slot count of a sum is a function of n alone
inline unsigned fl_slots(size_t n) { return grid1d((n + 3) / 4 + 3, FL_BLOCK, FL_GRID_CAP); }
inline unsigned fl_grid(const Lanes& l, size_t n) {
    const size_t edge = n - 4 * l.nq;
    return grid1d(l.nq > edge ? l.nq : edge, FL_BLOCK, FL_GRID_CAP);
}
inline bool aligned4(const void* a) { return ((uintptr_t)a & 3u) == 0; }
inline bool overlap(const void* a, const void* b, size_t n) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + 4 * n && y < x + 4 * n;
}

__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ void st4(float* p, const float4& v) { *reinterpret_cast<float4*>(p) = v; }
__device__ __forceinline__ uint4 ld4u(const unsigned* p) { return *reinterpret_cast<const uint4*>(p); }
__device__ __forceinline__ void st4u(unsigned* p, const uint4& v) { *reinterpret_cast<uint4*>(p) = v; }
__device__ __forceinline__ int4 ld4i(const int* p) { return *reinterpret_cast<const int4*>(p); }

// one workgroup: lane t adds its contiguous share of the slots in index order, lane 0 then adds the 256 shares in lane order
__device__ __forceinline__ double sum_slots(const double* __restrict__ slots, size_t n_slots, double* part) {
    const size_t per = (n_slots + FL_BLOCK - 1) / FL_BLOCK;
    const size_t lo = per * threadIdx.x, hi = lo + per < n_slots ? lo + per : n_slots;
    double acc = 0.0;
    for (size_t i = lo; i < hi; ++i) acc += slots[i];
    part[threadIdx.x] = acc;
    __syncthreads();
    double tot = 0.0;
    if (threadIdx.x == 0)
        for (int i = 0; i < FL_BLOCK; ++i) tot += part[i];
    return tot;                                                      // valid in lane 0
}
__global__ __launch_bounds__(FL_BLOCK) void sum_slots_kernel(const double* __restrict__ slots, size_t n_slots, double* __restrict__ out) {
    __shared__ double part[FL_BLOCK];
    const double tot = sum_slots(slots, n_slots, part);
    if (threadIdx.x == 0) *out = tot;
}

}  // namespace
}  // namespace ru
