// Region-wise post-processing of a prediction on the device (include/resunet_hip.h states the definition): per region WT, TC, ET the
// 26-connected components are filtered by volume, by mean probability and by "largest only", enclosed holes are filled and the regions
// are nested.  Everything sits between ru_tta_merge_box / the ensemble finalize and ru_compose_labels, where the masks are in HBM.
//
//   zero2_kernel          : clears the outputs (counts, stats), the arg-max slots and -- with a confidence rule -- the per-root sums.
//   cc_*_kernel<PpRegion> : the union-find labelling of cc_unionfind.hpp for the three regions in one launch sequence (gridDim.y = 3); the
//                           foreground is the mask byte or the BraTS region of the label byte.  Clears the per-root voxel counts.
//   pp_count_kernel<CONF> : vol[root] += members and conf[root] += sum of q(p), wave-aggregated as cc_count_members: the lanes of a wave
//                           that share a root elect one to add, and a wave carries its last (root, sums) across its iterations.
//   pp_decide_kernel      : one thread per root: the volume rule, then the confidence rule (an integer comparison); a survivor of a
//                           keep_largest region enters the arg-max -- one 64-bit atomicMax on (vol << 32) | ~root.  A removed root is
//                           marked in the high bit of its count.
//   pp_apply_kernel       : the filtered masks; counts the survivors that are not the arg-max.
//   cc_*_kernel<PpHoles, 6>: the 6-connected labelling of the background of the filtered masks, for the regions with fill_holes only.
//   pp_face_kernel        : the face voxels of the grid mark their root (integer atomic, skipped once the mark is seen).
//   pp_fill_kernel        : background whose root carries no mark becomes foreground.
//   pp_final_kernel       : nesting, the output masks or the composed label volume, the voxel counts, the invalid label voxels.
// Integer atomics only: the result does not depend on the order of execution.  Nothing synchronises with the host.
#include "ru_common.h"
#include "pw_helpers.hpp"
#include "cc_unionfind.hpp"
#include "mask_bits.hpp"

#include <limits.h>

namespace ru {
namespace {

constexpr int PP_K = RU_POSTPROCESS_REGIONS;
constexpr unsigned PP_REMOVED = 0x80000000u;        // high bit of vol[root]: the component is removed (a volume is below 2^31)

struct PpParams {
    long long min_volume[PP_K];
    u64 conf_thr[PP_K];
    unsigned keep_largest, fill_holes;
    int nest;
};

// workspace slices
struct PpWs {
    u64* best;                  // [3] arg-max keys of keep_largest
    int *parent, *vol;          // [3][V]
    u64* conf;                  // [3][V]
    unsigned char* fm;          // [3][V] filtered masks (kind labels; kind masks filters into `out`)
    size_t bytes;
};

PpWs pp_layout(char* base, int kind, size_t V) {
    PpWs w;
    size_t off = 0;
    auto take = [&](size_t bytes) { char* p = base + off; off += align_up(bytes, 256); return p; };
    w.best = (u64*)take(PP_K * sizeof(u64));
    w.parent = (int*)take(PP_K * V * sizeof(int));
    w.vol = (int*)take(PP_K * V * sizeof(int));
    w.conf = kind == RU_POSTPROCESS_MASKS ? (u64*)take(PP_K * V * sizeof(u64)) : nullptr;      // (labels come without probabilities)
    w.fm = kind == RU_POSTPROCESS_LABELS ? (unsigned char*)take(PP_K * V) : nullptr;
    w.bytes = off;
    return w;
}

// q(p) = floor(clamp(p, 0, 1) * 65536): the product by a power of two is exact, the conversion truncates
__device__ __forceinline__ unsigned pp_q(float p) { return (unsigned)(fminf(fmaxf(p, 0.f), 1.f) * 65536.0f); }

// the foreground of region k = blockIdx.y: a mask byte, or the region of a label byte
template <int KIND>
struct PpRegion {
    const unsigned char* in;
    size_t V;
    int W, k;
    __device__ void select(int y, int) { k = y; if (KIND == RU_POSTPROCESS_MASKS) in += (size_t)y * V; }
    __device__ bool operator()(size_t row, int x) const {
        const unsigned v = in[row * W + x];
        return KIND == RU_POSTPROCESS_MASKS ? v != 0u : brats_region(v, k);
    }
};

// the background of the filtered mask of region slot[y]
struct PpHoles {
    const unsigned char* fm;
    size_t V;
    int W;
    int slot[PP_K];
    __device__ void select(int y, int) { fm += (size_t)slot[y] * V; }
    __device__ bool operator()(size_t row, int x) const { return fm[row * W + x] == 0; }
};

// grid (blocks, 3), whole 256-thread blocks: the scheme of cc_count_members with a second, 64-bit sum.  A wave's q sum is below 2^22.
template <bool CONF>
__global__ __launch_bounds__(256) void pp_count_kernel(const int* __restrict__ parents, int* __restrict__ vols, u64* __restrict__ confs,
                                                       const float* __restrict__ probs, size_t V) {
    const int* __restrict__ parent = parents + blockIdx.y * V;
    int* __restrict__ vol = vols + blockIdx.y * V;
    if (!CONF) { cc_count_members(parent, vol, V); return; }
    u64* __restrict__ conf = confs + blockIdx.y * V;
    const float* __restrict__ p = probs + blockIdx.y * V;
    const size_t vend = (V + 255) / 256 * 256;                 // whole waves stay in the loop (the ballots and shuffles need every lane)
    const bool first = (threadIdx.x & 63) == 0;
    int run_root = -1, run_cnt = 0;
    u64 run_conf = 0;
    for (size_t v = (size_t)blockIdx.x * 256 + threadIdx.x; v < vend; v += (size_t)gridDim.x * 256) {
        int root = -1;
        unsigned q = 0;
        if (v < V && parent[v] >= 0) { root = cc_find(parent, (int)v); q = pp_q(p[v]); }
        u64 todo = __ballot(root >= 0);
        while (todo) {
            const int leader = __builtin_ctzll(todo);
            const int lroot = __shfl(root, leader);
            const u64 same = __ballot(root == lroot) & todo;
            const int n = (int)__builtin_popcountll(same);
            unsigned s = root == lroot ? q : 0u;
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
            if (lroot == run_root) { run_cnt += n; run_conf += s; }
            else {
                if (run_cnt && first) { atomicAdd(vol + run_root, run_cnt); if (run_conf) atomicAdd(conf + run_root, run_conf); }
                run_root = lroot; run_cnt = n; run_conf = s;
            }
            todo &= ~same;
        }
    }
    if (run_cnt && first) { atomicAdd(vol + run_root, run_cnt); if (run_conf) atomicAdd(conf + run_root, run_conf); }
}

// stats[k * RU_POSTPROCESS_STATS + column] += the wave's sum of `local`
__device__ __forceinline__ void pp_stat_add(long long* __restrict__ stats, int k, int column, unsigned local) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) local += __shfl_xor(local, o);
    if ((threadIdx.x & 63) == 0 && local) atomicAdd((u64*)(stats + k * RU_POSTPROCESS_STATS + column), (u64)local);
}

// grid (blocks, 3): the rules at every root
template <bool CONF>
__global__ __launch_bounds__(256) void pp_decide_kernel(const int* __restrict__ parents, int* __restrict__ vols, const u64* __restrict__ confs, PpParams prm,
                                                        u64* __restrict__ best, long long* __restrict__ stats, size_t V) {
    const int k = blockIdx.y;
    const int* __restrict__ parent = parents + k * V;
    unsigned* __restrict__ vol = (unsigned*)(vols + k * V);
    const bool largest = (prm.keep_largest >> k) & 1u;
    unsigned found = 0, by_volume = 0, by_conf = 0;
    for (size_t v = (size_t)blockIdx.x * 256 + threadIdx.x; v < V; v += (size_t)gridDim.x * 256) {
        if (parent[v] != (int)v) continue;
        ++found;
        const unsigned n = vol[v];
        if ((long long)n < prm.min_volume[k]) { ++by_volume; vol[v] = n | PP_REMOVED; continue; }
        if (CONF && prm.conf_thr[k] > 0 && confs[k * V + v] < prm.conf_thr[k] * (u64)n) { ++by_conf; vol[v] = n | PP_REMOVED; continue; }
        if (largest) atomicMax(best + k, ((u64)n << 32) | (u64)(~(unsigned)v));
    }
    pp_stat_add(stats, k, RU_POSTPROCESS_S_FOUND, found);
    pp_stat_add(stats, k, RU_POSTPROCESS_S_VOLUME, by_volume);
    pp_stat_add(stats, k, RU_POSTPROCESS_S_CONFIDENCE, by_conf);
}

// grid (blocks, 3): fm[k][v] = 1 where the voxel's component survives, else 0
__global__ __launch_bounds__(256) void pp_apply_kernel(const int* __restrict__ parents, const int* __restrict__ vols, const u64* __restrict__ best, unsigned keep_largest,
                                                       unsigned char* __restrict__ fm, long long* __restrict__ stats, size_t V) {
    const int k = blockIdx.y;
    const int* __restrict__ parent = parents + k * V;
    const unsigned* __restrict__ vol = (const unsigned*)(vols + k * V);
    unsigned char* __restrict__ m = fm + k * V;
    const bool largest = (keep_largest >> k) & 1u;
    const int winner = largest && best[k] ? (int)~(unsigned)best[k] : -1;
    unsigned not_largest = 0;
    for (size_t v = (size_t)blockIdx.x * 256 + threadIdx.x; v < V; v += (size_t)gridDim.x * 256) {
        const int p = parent[v];
        bool on = false;
        if (p >= 0) {
            const int root = cc_find(parent, (int)v);
            on = !(vol[root] & PP_REMOVED);
            if (on && largest && root != winner) {
                on = false;
                not_largest += root == (int)v ? 1u : 0u;
            }
        }
        m[v] = on ? 1 : 0;
    }
    pp_stat_add(stats, k, RU_POSTPROCESS_S_LARGEST, not_largest);
}

struct PpSlots { int k[PP_K]; };

// grid (blocks, regions with fill_holes): touch[root] = 1 for every background component with a voxel on a face of the grid.  The outside
// is one component with up to 2 (DH + HW + DW) face voxels: they look before they add, so that address sees a handful of atomics
__global__ __launch_bounds__(256) void pp_face_kernel(const int* __restrict__ parents, int* __restrict__ touches, int D, int H, int W) {
    const size_t V = (size_t)D * H * W;
    const int* __restrict__ parent = parents + blockIdx.y * V;
    int* __restrict__ touch = touches + blockIdx.y * V;
    for (size_t v = (size_t)blockIdx.x * 256 + threadIdx.x; v < V; v += (size_t)gridDim.x * 256) {
        const int x = (int)(v % W);
        const size_t r = v / W;
        const int y = (int)(r % H), z = (int)(r / H);
        if (!(x == 0 || x == W - 1 || y == 0 || y == H - 1 || z == 0 || z == D - 1)) continue;
        if (parent[v] < 0) continue;
        const int root = cc_find(parent, (int)v);
        if (__hip_atomic_load(touch + root, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0) atomicOr(touch + root, 1);
    }
}

// grid (blocks, regions with fill_holes)
__global__ __launch_bounds__(256) void pp_fill_kernel(const int* __restrict__ parents, const int* __restrict__ touches, PpSlots slots, unsigned char* __restrict__ fm,
                                                      long long* __restrict__ stats, size_t V) {
    const int k = slots.k[blockIdx.y];
    const int* __restrict__ parent = parents + blockIdx.y * V;
    const int* __restrict__ touch = touches + blockIdx.y * V;
    unsigned char* __restrict__ m = fm + k * V;
    unsigned filled = 0;
    for (size_t v = (size_t)blockIdx.x * 256 + threadIdx.x; v < V; v += (size_t)gridDim.x * 256) {
        if (parent[v] < 0) continue;
        if (touch[cc_find(parent, (int)v)]) continue;
        m[v] = 1;
        ++filled;
    }
    pp_stat_add(stats, k, RU_POSTPROCESS_S_FILLED, filled);
}

// grid (blocks): nesting, the outputs and the counts.  KIND masks: fm == out, rewritten in place; KIND labels: out = 2 where WT, 1 where TC,
// 4 where ET (test.py:155-159), and the label bytes above 4 are counted for every region
template <int KIND>
__global__ __launch_bounds__(256) void pp_final_kernel(const unsigned char* __restrict__ in, const unsigned char* fm, int nest, unsigned char* out,
                                                       u64* __restrict__ counts, long long* __restrict__ stats, size_t V) {
    unsigned c0 = 0, c1 = 0, c2 = 0, bad = 0;
    for (size_t v = (size_t)blockIdx.x * 256 + threadIdx.x; v < V; v += (size_t)gridDim.x * 256) {
        bool m0 = fm[v] != 0, m1 = fm[V + v] != 0, m2 = fm[2 * V + v] != 0;
        if (nest) { m1 = m1 && m0; m2 = m2 && m1; }
        c0 += m0; c1 += m1; c2 += m2;
        if (KIND == RU_POSTPROCESS_MASKS) {
            if (nest) { out[V + v] = m1; out[2 * V + v] = m2; }
        } else {
            out[v] = m2 ? 4 : m1 ? 1 : m0 ? 2 : 0;
            bad += in[v] > 4u;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { c0 += __shfl_xor(c0, o); c1 += __shfl_xor(c1, o); c2 += __shfl_xor(c2, o); }
    if ((threadIdx.x & 63) == 0) {
        if (c0) atomicAdd(counts + 0, (u64)c0);
        if (c1) atomicAdd(counts + 1, (u64)c1);
        if (c2) atomicAdd(counts + 2, (u64)c2);
    }
    if (KIND == RU_POSTPROCESS_LABELS)
        for (int k = 0; k < PP_K; ++k) pp_stat_add(stats, k, RU_POSTPROCESS_S_INVALID, bad);
}

bool pp_shape_ok(int kind, int D, int H, int W) {
    return (kind == RU_POSTPROCESS_MASKS || kind == RU_POSTPROCESS_LABELS) && D >= 1 && H >= 1 && W >= 1 && (size_t)D * H * W < (size_t)INT_MAX;
}

}  // namespace
}  // namespace ru

using namespace ru;

extern "C" size_t ru_postprocess_workspace_bytes(int kind, int D, int H, int W) {
    if (!pp_shape_ok(kind, D, H, W)) return 0;
    return pp_layout(nullptr, kind, (size_t)D * H * W).bytes;
}

extern "C" int ru_postprocess_regions(const void* in, const float* probs, int kind, int D, int H, int W, const long long* min_volume,
                                      const unsigned long long* conf_thr, unsigned keep_largest_bits, unsigned fill_holes_bits, int nest,
                                      unsigned char* out, unsigned long long* counts, long long* stats, void* ws, size_t ws_bytes, ru_stream_t stream) {
    RU_REQUIRE(in && out && counts && stats && min_volume && conf_thr && ws, "ru_postprocess_regions: null argument");
    RU_REQUIRE(kind == RU_POSTPROCESS_MASKS || kind == RU_POSTPROCESS_LABELS, "ru_postprocess_regions: bad kind %d", kind);
    RU_REQUIRE(D >= 1 && H >= 1 && W >= 1, "ru_postprocess_regions: extents %d x %d x %d", D, H, W);
    RU_REQUIRE((size_t)D * H * W < (size_t)INT_MAX, "ru_postprocess_regions: volume too large for 32-bit voxel indices");
    RU_REQUIRE(in != (const void*)out, "ru_postprocess_regions: the input is not written: `out` must be another array");
    PpParams prm;
    bool conf = false;
    for (int k = 0; k < PP_K; ++k) {
        RU_REQUIRE(min_volume[k] >= 0 && conf_thr[k] <= 65536ull, "ru_postprocess_regions: region %d: min_volume %lld must be >= 0, the confidence threshold %llu <= 65536",
                   k, min_volume[k], conf_thr[k]);
        prm.min_volume[k] = min_volume[k];
        prm.conf_thr[k] = conf_thr[k];
        conf = conf || conf_thr[k] > 0;
    }
    RU_REQUIRE(!conf || (probs && kind == RU_POSTPROCESS_MASKS), "ru_postprocess_regions: a confidence threshold needs probabilities (kind masks)");
    RU_REQUIRE(keep_largest_bits < 8u && fill_holes_bits < 8u, "ru_postprocess_regions: the region bit sets have three bits");
    prm.keep_largest = keep_largest_bits;
    prm.fill_holes = fill_holes_bits;
    prm.nest = nest ? 1 : 0;
    const size_t V = (size_t)D * H * W;
    RU_REQUIRE(ws_bytes >= ru_postprocess_workspace_bytes(kind, D, H, W), "ru_postprocess_regions: workspace too small");
    const PpWs w = pp_layout((char*)ws, kind, V);
    hipStream_t st = (hipStream_t)stream;
    const unsigned char* inb = (const unsigned char*)in;
    unsigned char* fm = kind == RU_POSTPROCESS_MASKS ? out : w.fm;
    const unsigned g = grid1d(V, 256 * 4, 4096);

    hipLaunchKernelGGL((zero2_kernel<u64, u64>), dim3(1), dim3(64), 0, st, w.best, (size_t)PP_K, (u64*)counts, (size_t)PP_K);
    RU_CHECK_LAUNCH("zero2_kernel");
    hipLaunchKernelGGL((zero2_kernel<long long, u64>), dim3(conf ? grid1d(PP_K * V, 256 * 4, 4096) : 1), dim3(256), 0, st, stats,
                       (size_t)PP_K * RU_POSTPROCESS_STATS, w.conf, conf ? PP_K * V : (size_t)0);
    RU_CHECK_LAUNCH("zero2_kernel");
    int rl;
    if (kind == RU_POSTPROCESS_MASKS) rl = cc_label(PpRegion<RU_POSTPROCESS_MASKS>{inb, V, W, 0}, w.parent, 0, w.vol, D, H, W, dim3(g, PP_K), st);
    else rl = cc_label(PpRegion<RU_POSTPROCESS_LABELS>{inb, V, W, 0}, w.parent, 0, w.vol, D, H, W, dim3(g, PP_K), st);
    if (rl) return rl;
    if (conf) {
        hipLaunchKernelGGL(pp_count_kernel<true>, dim3(g, PP_K), dim3(256), 0, st, w.parent, w.vol, w.conf, probs, V);
        RU_CHECK_LAUNCH("pp_count_kernel");
        hipLaunchKernelGGL(pp_decide_kernel<true>, dim3(g, PP_K), dim3(256), 0, st, w.parent, w.vol, w.conf, prm, w.best, stats, V);
    } else {
        hipLaunchKernelGGL(pp_count_kernel<false>, dim3(g, PP_K), dim3(256), 0, st, w.parent, w.vol, w.conf, probs, V);
        RU_CHECK_LAUNCH("pp_count_kernel");
        hipLaunchKernelGGL(pp_decide_kernel<false>, dim3(g, PP_K), dim3(256), 0, st, w.parent, w.vol, w.conf, prm, w.best, stats, V);
    }
    RU_CHECK_LAUNCH("pp_decide_kernel");
    hipLaunchKernelGGL(pp_apply_kernel, dim3(g, PP_K), dim3(256), 0, st, w.parent, w.vol, w.best, prm.keep_largest, fm, stats, V);
    RU_CHECK_LAUNCH("pp_apply_kernel");
    if (prm.fill_holes) {
        PpHoles holes = {fm, V, W, {0, 0, 0}};
        PpSlots slots = {{0, 0, 0}};
        int n = 0;
        for (int k = 0; k < PP_K; ++k)
            if ((prm.fill_holes >> k) & 1u) { holes.slot[n] = k; slots.k[n] = k; ++n; }
        // the foreground labelling is spent: its parents and counts hold the background's, the counts as the face marks (cleared by cc_label)
        rl = cc_label<6>(holes, w.parent, 0, w.vol, D, H, W, dim3(g, n), st);
        if (rl) return rl;
        hipLaunchKernelGGL(pp_face_kernel, dim3(g, n), dim3(256), 0, st, w.parent, w.vol, D, H, W);
        RU_CHECK_LAUNCH("pp_face_kernel");
        hipLaunchKernelGGL(pp_fill_kernel, dim3(g, n), dim3(256), 0, st, w.parent, w.vol, slots, fm, stats, V);
        RU_CHECK_LAUNCH("pp_fill_kernel");
    }
    if (kind == RU_POSTPROCESS_MASKS) hipLaunchKernelGGL(pp_final_kernel<RU_POSTPROCESS_MASKS>, dim3(g), dim3(256), 0, st, inb, fm, prm.nest, out, (u64*)counts, stats, V);
    else hipLaunchKernelGGL(pp_final_kernel<RU_POSTPROCESS_LABELS>, dim3(g), dim3(256), 0, st, inb, fm, prm.nest, out, (u64*)counts, stats, V);
    RU_CHECK_LAUNCH("pp_final_kernel");
    return RU_OK;
}
