// Flat streaming passes over n float32-sized elements (optim.hip, hardcrit.hip, boundary.hip): the one home of their lane layout.  A lane owns
// 4 consecutive elements moved as 16 bytes, the elements before the first 16-byte boundary and after the last whole quad are taken one by
// one, the grid is capped and strides.  Sums are one float64 slot per workgroup, added in a fixed order by one workgroup: no float atomics.
// The index arithmetic is written once (fl_walk); stream_kernel and sum_kernel put an op's arithmetic on it, and a kernel with a prologue
// and epilogue of its own calls it between them.  Everything here has internal linkage: each translation unit gets its own copies.
#pragma once
#include "ru_common.h"
#include "pw_helpers.hpp"

#include <stdint.h>
#include <type_traits>
#include <utility>

namespace ru {
namespace {

constexpr int FL_BLOCK = 256;
constexpr unsigned FL_GRID_CAP = 2048;           // 256 CUs x 8 workgroups: one resident wave of workgroups, the rest by grid stride

// [0, head) one by one | nq quads from `head` | the remaining (< 4) elements one by one.  The quads are 16-byte aligned for EVERY pointer of
// the call only if all of them sit at the same offset from a 16-byte boundary (runs of buffers laid out alike do); otherwise everything goes
// one by one.
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

// The walk of one lane: quad(i) for each of its quads [i, i + 4), then one(i) for each of its head and tail elements (at most 6 in the whole
// grid when the quads exist).  Both callables are inlined.
template <class Quad, class One>
__device__ __forceinline__ void fl_walk(const Lanes& l, size_t n, Quad&& quad, One&& one) {
    const size_t t = (size_t)blockIdx.x * FL_BLOCK + threadIdx.x, T = (size_t)gridDim.x * FL_BLOCK;
    for (size_t q = t; q < l.nq; q += T) quad(l.head + 4 * q);
    const size_t edge = n - 4 * l.nq;
    for (size_t e = t; e < edge; e += T) one(e < l.head ? e : e + 4 * l.nq);
}

// Op: `load(i)` fetches elements [i, i + 4) of every operand through 16-byte accesses, `finish(i, q)` updates and stores them; `one(i)` does
// element i; both run the same scalar arithmetic.  (Keeping the loads of two quads in flight per lane measured no faster: every pass on the
// network's runs sits within a few microseconds of its three launches' floor, tools/optim_time.py.)  An op with a `begin()` has it called once
// per lane before the walk: the place to read a scale or a threshold from device memory once, not once per quad.
template <class Op, class = void> struct has_begin : std::false_type {};
template <class Op> struct has_begin<Op, std::void_t<decltype(std::declval<Op&>().begin())>> : std::true_type {};
template <class Op>
__global__ __launch_bounds__(FL_BLOCK) void stream_kernel(Op op, size_t n, Lanes l) {
    if constexpr (has_begin<Op>::value) op.begin();
    fl_walk(l, n, [&](size_t i) { auto a = op.load(i); op.finish(i, a); }, [&](size_t i) { op.one(i); });
}
template <class Op>
inline int stream_launch(const Op& op, size_t n, const Lanes& l, hipStream_t s, const char* what) {
    hipLaunchKernelGGL(stream_kernel<Op>, dim3(fl_grid(l, n)), dim3(FL_BLOCK), 0, s, op, n, l);
    RU_CHECK_LAUNCH(what);
    return RU_OK;
}

// Op: `quad(i)` is the float64 value of elements [i, i + 4), associated as the op writes it; `one(i)` that of element i.
// slots[block] = the workgroup's sum; the grid is fl_slots(n) whatever the alignment, and every workgroup writes its slot, zeros included.
template <class Op>
__global__ __launch_bounds__(FL_BLOCK) void sum_kernel(Op op, size_t n, Lanes l, double* __restrict__ slots) {
    __shared__ double buf[4];
    double acc = 0.0;
    fl_walk(l, n, [&](size_t i) { acc += op.quad(i); }, [&](size_t i) { acc += op.one(i); });
    const double tot = block_sum_d(acc, buf);
    if (threadIdx.x == 0) slots[blockIdx.x] = tot;
}
template <class Op>
inline int sum_launch(const Op& op, size_t n, const Lanes& l, double* slots, hipStream_t s, const char* what) {
    hipLaunchKernelGGL(sum_kernel<Op>, dim3(fl_slots(n)), dim3(FL_BLOCK), 0, s, op, n, l, slots);
    RU_CHECK_LAUNCH(what);
    return RU_OK;
}

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
// *out = the sum of the op over the run: sum_kernel into `slots`, then sum_slots_kernel
template <class Op>
inline int total_launch(const Op& op, size_t n, const Lanes& l, double* slots, double* out, hipStream_t s, const char* what) {
    if (int rc = sum_launch(op, n, l, slots, s, what)) return rc;
    hipLaunchKernelGGL(sum_slots_kernel, dim3(1), dim3(FL_BLOCK), 0, s, (const double*)slots, (size_t)fl_slots(n), out);
    RU_CHECK_LAUNCH("sum_slots_kernel");
    return RU_OK;
}

// a run-time mode in [LO, HI] (anything else counts as HI) as a compile-time constant: f(std::integral_constant<int, mode>())
template <int LO, int HI, class F>
inline int with_mode(int mode, F&& f) {
    if constexpr (LO < HI)
        if (mode != LO) return with_mode<LO + 1, HI>(mode, f);
    return f(std::integral_constant<int, LO>());
}

}  // namespace
}  // namespace ru
