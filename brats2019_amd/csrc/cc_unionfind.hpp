// 26-connected component labelling by union-find on voxel indices (inference.hip: ru_cc_reject; lesion.hip: ru_lesion_metrics;
// postprocess.hip: ru_postprocess_regions, which also labels the background 6-connected -- CONN = 6 below, 3 earlier neighbours instead of 13).
// parent[v] = v for a root, a smaller index of the same component otherwise, -1 for background; roots are the smallest index of their
// component (atomicMin), which is also the order in which scipy.ndimage.label numbers components.  Each voxel is united with its 13
// "earlier" neighbours of the 26-neighbourhood (the other 13 are covered from the neighbour's side), in three passes instead of one
// (the plain form -- every voxel united with its 13 earlier neighbours through uncompressed trees -- took 18 ms on the 4-million-voxel
// noise prediction of a random-init network, bench.py's predict_case):
//   init     : a foreground voxel points at the SMALLEST of its earlier foreground neighbours (itself if none): plain reads of the
//              foreground, no atomics -- most of the component's links exist after this pass, as a forest with decreasing indices;
//   compress : every voxel points at the root of its tree (stale parents read on the way are still ancestors: the pass is race-tolerant);
//   merge    : the remaining equivalences -- a voxel and an earlier neighbour whose trees still differ -- by cc_unite on one- or two-hop paths;
//   compress : again, so that counting and whatever follows find their root in one hop.
// One launch labels gridDim.y * gridDim.z volumes of V voxels: block (., y, z) works on parent + z * zpitch + y * V, and the foreground
// functor is told (y, z).  A single volume is the grid (blocks, 1, 1).  The kernels have internal linkage.
#pragma once
#include "ru_common.h"

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
// the 13 neighbours that precede a voxel in linear order: (dz, dy, dx) with dz = -1, or dz = 0 and dy = -1, or dz = dy = 0 and dx = -1
__device__ __forceinline__ bool cc_earlier(int dz, int dy, int dx) { return dz < 0 || (dz == 0 && (dy < 0 || (dy == 0 && dx < 0))); }

// visit(u, row, x) for every earlier neighbour u = row * W + x of voxel v that lies inside the grid; CONN = 6: the three face neighbours
// (z - 1), (y - 1), (x - 1) only, in the same (ascending) order
template <int CONN = 26, class Visit>
__device__ __forceinline__ void cc_for_earlier(size_t v, int H, int W, Visit visit) {
    static_assert(CONN == 26 || CONN == 6, "cc_for_earlier: 26- or 6-connected");
    const int x = (int)(v % W);
    const size_t r = v / W;
    const int y = (int)(r % H), z = (int)(r / H);
    if constexpr (CONN == 6) {
        if (z > 0) visit(v - (size_t)H * W, r - H, x);
        if (y > 0) visit(v - W, r - 1, x);
        if (x > 0) visit(v - 1, r, x - 1);
        return;
    }
#pragma unroll
    for (int dz = -1; dz <= 0; ++dz)
#pragma unroll
        for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
            for (int dx = -1; dx <= 1; ++dx) {
                if (!cc_earlier(dz, dy, dx)) continue;
                const int zz = z + dz, yy = y + dy, xx = x + dx;
                if (zz < 0 || yy < 0 || yy >= H || xx < 0 || xx >= W) continue;
                const size_t rr = (size_t)zz * H + yy;
                visit(rr * W + xx, rr, xx);
            }
}

namespace {

// Fg: void select(int y, int z) once per block, then bool operator()(size_t row, int x): is voxel x of row (z * H + y) foreground?
// `count` (may be null) holds one array of V per y; the last z clears it.
template <class Fg, int CONN = 26>
__global__ __launch_bounds__(256) void cc_init_kernel(Fg fg, int* __restrict__ parent, size_t zpitch, int* __restrict__ count, int D, int H, int W) {
    const size_t V = (size_t)D * H * W;
    fg.select(blockIdx.y, blockIdx.z);
    parent += blockIdx.z * zpitch + blockIdx.y * V;
    const bool clear = count && blockIdx.z + 1 == gridDim.z;
    for (size_t v = (size_t)blockIdx.x * 256 + threadIdx.x; v < V; v += (size_t)gridDim.x * 256) {
        if (clear) count[blockIdx.y * V + v] = 0;
        if (!fg(v / W, (int)(v % W))) { parent[v] = -1; continue; }
        int m = (int)v;
        cc_for_earlier<CONN>(v, H, W, [&](size_t u, size_t row, int x) {
            if ((int)u < m && fg(row, x)) m = (int)u;
        });
        parent[v] = m;
    }
}

__global__ __launch_bounds__(256) void cc_compress_kernel(int* parent, size_t zpitch, size_t V) {
    parent += blockIdx.z * zpitch + blockIdx.y * V;
    for (size_t v = (size_t)blockIdx.x * 256 + threadIdx.x; v < V; v += (size_t)gridDim.x * 256) {
        if (parent[v] < 0) continue;
        const int root = cc_find(parent, (int)v);
        __hip_atomic_store(parent + v, root, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);          // (an ancestor whatever the other threads do meanwhile)
    }
}

template <int CONN = 26>
__global__ __launch_bounds__(256) void cc_merge_kernel(int* parent, size_t zpitch, int D, int H, int W) {
    const size_t V = (size_t)D * H * W;
    parent += blockIdx.z * zpitch + blockIdx.y * V;
    for (size_t v = (size_t)blockIdx.x * 256 + threadIdx.x; v < V; v += (size_t)gridDim.x * 256) {
        const int pv = parent[v];
        if (pv < 0) continue;
        cc_for_earlier<CONN>(v, H, W, [&](size_t u, size_t, int) {
            const int pu = parent[u];
            if (pu >= 0 && pu != pv) cc_unite(parent, (int)v, (int)u);       // (equal parents: one tree already; a stale read only costs a redundant unite)
        });
    }
}

// count[root] += members, for the volume at `parent`; called by whole 256-thread blocks of a grid over x.  Wave-aggregated: consecutive
// voxels mostly share their root, and atomics on one address serialise (~12 ns each: a 100 000-voxel tumour counted voxel by voxel would
// take over a millisecond) -- the lanes of a wave that hold the same root elect one to add their number ...
__device__ __forceinline__ void cc_count_members(const int* parent, int* count, size_t V) {
    const size_t vend = (V + 255) / 256 * 256;                 // whole waves stay in the loop (the ballots need every lane)
    // ... and a wave carries the (root, number) of its last group across its iterations (wave-uniform), adding it when the root changes: a component
    // that fills the volume -- the noise prediction of a random-init network -- costs one atomic per wave instead of one per 64 voxels (0.72 -> ~0.15 ms)
    int run_root = -1, run_cnt = 0;
    for (size_t v = (size_t)blockIdx.x * 256 + threadIdx.x; v < vend; v += (size_t)gridDim.x * 256) {
        int root = -1;
        if (v < V && parent[v] >= 0) root = cc_find(parent, (int)v);
        unsigned long long todo = __ballot(root >= 0);
        while (todo) {
            const int leader = __builtin_ctzll(todo);
            const int lroot = __shfl(root, leader);
            const unsigned long long same = __ballot(root == lroot) & todo;
            const int n = (int)__builtin_popcountll(same);
            if (lroot == run_root) run_cnt += n;
            else {
                if (run_cnt && (threadIdx.x & 63) == 0) atomicAdd(count + run_root, run_cnt);
                run_root = lroot; run_cnt = n;
            }
            todo &= ~same;
        }
    }
    if (run_cnt && (threadIdx.x & 63) == 0) atomicAdd(count + run_root, run_cnt);
}

// init, compress, merge, compress on stream st; grid = (blocks over V, volumes per z, z); cc_label<6>(...) labels 6-connected
template <int CONN = 26, class Fg>
inline int cc_label(const Fg& fg, int* parent, size_t zpitch, int* count, int D, int H, int W, dim3 grid, hipStream_t st) {
    const size_t V = (size_t)D * H * W;
    hipLaunchKernelGGL((cc_init_kernel<Fg, CONN>), grid, dim3(256), 0, st, fg, parent, zpitch, count, D, H, W);
    RU_CHECK_LAUNCH("cc_init_kernel");
    hipLaunchKernelGGL(cc_compress_kernel, grid, dim3(256), 0, st, parent, zpitch, V);
    RU_CHECK_LAUNCH("cc_compress_kernel");
    hipLaunchKernelGGL(cc_merge_kernel<CONN>, grid, dim3(256), 0, st, parent, zpitch, D, H, W);
    RU_CHECK_LAUNCH("cc_merge_kernel");
    hipLaunchKernelGGL(cc_compress_kernel, grid, dim3(256), 0, st, parent, zpitch, V);
    RU_CHECK_LAUNCH("cc_compress_kernel");
    return RU_OK;
}

}  // namespace
}  // namespace ru
