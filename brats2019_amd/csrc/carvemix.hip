// carvemix.hip -- CarveMix (Zhang et al., MICCAI 2021): carve a region around the donor's lesion, its size drawn from the lesion's volume and its
// shape from the lesion's distance map, and paste voxels and labels into another patch.  The map is ru_signed_sqdist's (boundary.hip), unchanged;
// here are the two passes around it.  Every step is integer or a select of 32-bit words: the numpy restatement (dataloader.carvemix_host) holds
// the device bit for bit.
//
//   threshold   ru_carvemix_threshold: V[k] = |{wt[k] > 0.5f}| (the mask rule of ru_signed_sqdist) counted in the lane layout of flat_lanes.hpp,
//               one integer partial per workgroup; one small launch then adds the partials of donor k in index order and forms
//                   R2 = the largest integer q with q^3 <= V^2                     (64-bit integer search: floor(V^(2/3)), no cbrt, no pow)
//                   outer: T = floor((u u) R2)          inner: T = -ceil(((u u) R2) 0.25)           (float64, plain IEEE multiplies)
//                   V == 0: T = INT32_MIN (nothing is carved)    V == n: T = INT32_MAX (the whole donor)
//               from u[k] and side[k], which travel as kernel arguments.  Nothing waits for the host.
//   mix         ru_carvemix_mix: ONE launch for the batch.  M = s <= T[k]; receiver dst[k] takes the donor's words where M.  A lane owns 4
//               consecutive voxels: s as one int4, T[k] once per lane, 16 bytes per channel; a quad without a selected voxel is neither
//               loaded nor stored, one that is selected whole does not load the receiver.  When the tensors of a donor / receiver pair do not
//               share an offset from a 16-byte boundary (sliced tensors, or a voxel count that is no multiple of 4) the pair goes one by one.
// No float arithmetic on the voxels, no atomics, the same bytes give the same bytes.
#include "ru_common.h"
#include "flat_lanes.hpp"

#include <limits.h>

namespace ru {
namespace {

constexpr size_t CM_MAX_VOXELS = (size_t)1 << 27;                      // V <= 2^27: q^3 <= V^2 <= 2^54 stays inside 64 bits

struct CmCountArgs {
    const float* wt[RU_CARVE_BATCH_MAX];
    Lanes l[RU_CARVE_BATCH_MAX];
};

// grid (fl_slots(n), donors): slots[donor][workgroup] = the workgroup's count, zeros included
__global__ __launch_bounds__(FL_BLOCK) void cm_count_kernel(CmCountArgs a, size_t n, unsigned* __restrict__ slots) {
    __shared__ unsigned buf[4];
    const int k = blockIdx.y;
    const float* __restrict__ x = a.wt[k];
    unsigned acc = 0;
    fl_walk(a.l[k], n,
            [&](size_t i) {
                const float4 v = ld4(x + i);
                acc += (unsigned)(v.x > 0.5f) + (unsigned)(v.y > 0.5f) + (unsigned)(v.z > 0.5f) + (unsigned)(v.w > 0.5f);
            },
            [&](size_t i) { acc += (unsigned)(x[i] > 0.5f); });
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_down(acc, o, 64);
    if ((threadIdx.x & 63) == 0) buf[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) slots[(size_t)k * gridDim.x + blockIdx.x] = (buf[0] + buf[1]) + (buf[2] + buf[3]);
}

struct CmDrawArgs {
    double u[RU_CARVE_BATCH_MAX];
    int side[RU_CARVE_BATCH_MAX];
};

// the largest q with q^3 <= v2, v2 <= 2^54: q <= 2^18
__device__ __forceinline__ unsigned long long cm_icbrt(unsigned long long v2) {
    unsigned long long lo = 0, hi = 1ull << 18;
    while (lo < hi) {
        const unsigned long long mid = (lo + hi + 1) >> 1;
        if (mid * mid * mid <= v2) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

__device__ __forceinline__ int cm_threshold(unsigned long long V, unsigned long long n, double u, int side) {
#pragma clang fp contract(off)
    if (V == 0) return INT_MIN;
    if (V == n) return INT_MAX;
    const double r2 = (double)cm_icbrt(V * V);
    const double uu = u * u;
    const double a = uu * r2;
    if (side == RU_CARVE_OUTER) return (int)floor(a);
    const double b = a * 0.25;
    return -(int)ceil(b);
}

// grid (donors), one workgroup each: lane t adds its contiguous share of the donor's slots, lane 0 the 256 shares
__global__ __launch_bounds__(FL_BLOCK) void cm_threshold_kernel(const unsigned* __restrict__ slots, size_t n_slots, size_t n, CmDrawArgs a,
                                                                int* __restrict__ T, long long* __restrict__ Vout) {
    __shared__ unsigned long long part[FL_BLOCK];
    const int k = blockIdx.x;
    const unsigned* __restrict__ sk = slots + (size_t)k * n_slots;
    const size_t per = (n_slots + FL_BLOCK - 1) / FL_BLOCK;
    const size_t lo = per * threadIdx.x, hi = lo + per < n_slots ? lo + per : n_slots;
    unsigned long long acc = 0;
    for (size_t i = lo; i < hi; ++i) acc += sk[i];
    part[threadIdx.x] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long V = 0;
        for (int i = 0; i < FL_BLOCK; ++i) V += part[i];
        Vout[k] = (long long)V;
        T[k] = cm_threshold(V, (unsigned long long)n, a.u[k], a.side[k]);
    }
}

// one donor / receiver pair of the mix launch
struct CmPair {
    const unsigned* xa;              // donor data [C][n]
    const unsigned* ya;              // donor target [3][n]
    const int* s;                    // the donor's map [n]
    unsigned* xb;                    // receiver data [C][n]
    unsigned* yb;                    // receiver target [3][n]
    unsigned char* mask;             // [n] or null
    Lanes l;
};
struct CmMixArgs { CmPair p[RU_CARVE_BATCH_MAX]; };

__device__ __forceinline__ unsigned sel(bool m, unsigned a, unsigned b) { return m ? a : b; }

// grid (x, pairs).  T is read once per lane.
__global__ __launch_bounds__(FL_BLOCK) void cm_mix_kernel(CmMixArgs a, const int* __restrict__ T, int C, size_t n) {
    const CmPair& p = a.p[blockIdx.y];
    const int t = T[blockIdx.y];
    const unsigned* __restrict__ xa = p.xa;
    const unsigned* __restrict__ ya = p.ya;
    const int* __restrict__ s = p.s;
    unsigned* __restrict__ xb = p.xb;
    unsigned* __restrict__ yb = p.yb;
    unsigned char* __restrict__ mask = p.mask;
    fl_walk(p.l, n,
            [&](size_t i) {
                const int4 sv = ld4i(s + i);
                const bool m0 = sv.x <= t, m1 = sv.y <= t, m2 = sv.z <= t, m3 = sv.w <= t;
                if (mask) {
                    mask[i] = m0;
                    mask[i + 1] = m1;
                    mask[i + 2] = m2;
                    mask[i + 3] = m3;
                }
                if (!(m0 || m1 || m2 || m3)) return;
                const bool all = m0 && m1 && m2 && m3;
                // one channel after the other: keeping the loads of all C + 3 channels in flight before the first store measured slower (39.2 /
                // 46.1 us against 36.3 / 43.9 us at 4 x 4 x 128^3, back to back / after a MALL flush), and so did a capped, striding grid
                // (profiles/carvemix_time.txt)
                for (int c = 0; c < C + 3; ++c) {
                    const unsigned* src = c < C ? xa + (size_t)c * n + i : ya + (size_t)(c - C) * n + i;
                    unsigned* dst = c < C ? xb + (size_t)c * n + i : yb + (size_t)(c - C) * n + i;
                    uint4 w = ld4u(src);
                    if (!all) {
                        const uint4 r = ld4u(dst);
                        w = make_uint4(sel(m0, w.x, r.x), sel(m1, w.y, r.y), sel(m2, w.z, r.z), sel(m3, w.w, r.w));
                    }
                    st4u(dst, w);
                }
            },
            [&](size_t i) {
                const bool m = s[i] <= t;
                if (mask) mask[i] = m;
                if (!m) return;
                for (int c = 0; c < C; ++c) xb[(size_t)c * n + i] = xa[(size_t)c * n + i];
                for (int c = 0; c < 3; ++c) yb[(size_t)c * n + i] = ya[(size_t)c * n + i];
            });
}

inline bool cm_extents_ok(int D, int H, int W) {
    const int cap = (int)CM_MAX_VOXELS;                                 // each factor first: the product of three ints then fits 64 bits
    return D > 0 && H > 0 && W > 0 && D <= cap && H <= cap && W <= cap && (size_t)D * (size_t)H * (size_t)W <= CM_MAX_VOXELS;
}
// runs of na / nb 32-bit words
inline bool cm_overlap(const void* a, size_t na, const void* b, size_t nb) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + 4 * nb && y < x + 4 * na;
}

}  // namespace
}  // namespace ru

using namespace ru;

extern "C" size_t ru_carvemix_workspace_bytes(int K, size_t n) {
    if (K <= 0 || n == 0) return 0;
    const size_t per_launch = K < RU_CARVE_BATCH_MAX ? K : RU_CARVE_BATCH_MAX;
    return per_launch * fl_slots(n) * sizeof(unsigned);
}

extern "C" int ru_carvemix_threshold(const float* wt, int K, size_t n, const double* u, const int* side, int* T_out, long long* V_out, void* ws,
                                     size_t ws_bytes, ru_stream_t stream) {
    RU_REQUIRE(wt && u && side && T_out && V_out && ws && K > 0 && n > 0, "ru_carvemix_threshold: bad argument");
    RU_REQUIRE(n <= CM_MAX_VOXELS, "ru_carvemix_threshold: %zu voxels per donor, at most 2^27", n);
    RU_REQUIRE(aligned4(wt) && aligned4(T_out) && aligned4(ws) && ((uintptr_t)V_out & 7u) == 0, "ru_carvemix_threshold: misaligned pointer");
    RU_REQUIRE(ws_bytes >= ru_carvemix_workspace_bytes(K, n), "ru_carvemix_threshold: workspace too small");
    for (int k = 0; k < K; ++k) {
        RU_REQUIRE(u[k] >= 0.0 && u[k] < 1.0, "ru_carvemix_threshold: u[%d] = %g must lie in [0, 1)", k, u[k]);
        RU_REQUIRE(side[k] == RU_CARVE_OUTER || side[k] == RU_CARVE_INNER, "ru_carvemix_threshold: side[%d] = %d is neither RU_CARVE_OUTER nor RU_CARVE_INNER", k, side[k]);
    }
    hipStream_t s = (hipStream_t)stream;
    const unsigned n_slots = fl_slots(n);
    for (int k0 = 0; k0 < K; k0 += RU_CARVE_BATCH_MAX) {
        const int cnt = K - k0 < RU_CARVE_BATCH_MAX ? K - k0 : RU_CARVE_BATCH_MAX;
        CmCountArgs ca = {};
        CmDrawArgs da = {};
        for (int j = 0; j < cnt; ++j) {
            ca.wt[j] = wt + (size_t)(k0 + j) * n;
            const void* const ptrs[1] = {ca.wt[j]};
            ca.l[j] = lanes_for(n, ptrs);
            da.u[j] = u[k0 + j];
            da.side[j] = side[k0 + j];
        }
        hipLaunchKernelGGL(cm_count_kernel, dim3(n_slots, cnt), dim3(FL_BLOCK), 0, s, ca, n, (unsigned*)ws);
        RU_CHECK_LAUNCH("cm_count_kernel");
        hipLaunchKernelGGL(cm_threshold_kernel, dim3(cnt), dim3(FL_BLOCK), 0, s, (const unsigned*)ws, (size_t)n_slots, n, da, T_out + k0, V_out + k0);
        RU_CHECK_LAUNCH("cm_threshold_kernel");
    }
    return RU_OK;
}

extern "C" int ru_carvemix_mix(const float* donor_data, const float* donor_target, const int* s_map, const int* T, int K, const int* dst, int N, int C,
                               int D, int H, int W, float* data, float* target, unsigned char* mask_out, ru_stream_t stream) {
    RU_REQUIRE(donor_data && donor_target && s_map && T && dst && data && target, "ru_carvemix_mix: null pointer");
    RU_REQUIRE(K > 0 && N > 0 && K <= N, "ru_carvemix_mix: %d donors into %d receivers: 1 <= K <= N", K, N);
    RU_REQUIRE(C >= 1 && C <= RU_AUG_MAXC, "ru_carvemix_mix: %d channels, 1..%d", C, RU_AUG_MAXC);
    RU_REQUIRE(cm_extents_ok(D, H, W), "ru_carvemix_mix: extents %d x %d x %d must be positive and hold at most 2^27 voxels", D, H, W);
    RU_REQUIRE(aligned4(donor_data) && aligned4(donor_target) && aligned4(s_map) && aligned4(T) && aligned4(data) && aligned4(target),
               "ru_carvemix_mix: misaligned pointer");
    const size_t n = (size_t)D * H * W;
    for (int k = 0; k < K; ++k) {
        RU_REQUIRE(dst[k] >= 0 && dst[k] < N, "ru_carvemix_mix: dst[%d] = %d outside the batch of %d", k, dst[k], N);
        for (int j = 0; j < k; ++j) RU_REQUIRE(dst[j] != dst[k], "ru_carvemix_mix: dst[%d] and dst[%d] name the same receiver %d", j, k, dst[k]);
    }
    // the receivers are written in place: nothing that is read may lie inside them
    const size_t nd = (size_t)N * C * n, nt = (size_t)N * 3 * n, kd = (size_t)K * C * n, kt = (size_t)K * 3 * n, ks = (size_t)K * n;
    RU_REQUIRE(!cm_overlap(data, nd, target, nt), "ru_carvemix_mix: data and target overlap");
    const struct { const void* p; size_t len; } reads[4] = {{donor_data, kd}, {donor_target, kt}, {s_map, ks}, {T, (size_t)K}};
    for (const auto& r : reads)
        RU_REQUIRE(!cm_overlap(r.p, r.len, data, nd) && !cm_overlap(r.p, r.len, target, nt), "ru_carvemix_mix: a donor tensor, the map or T overlaps a receiver tensor");
    if (mask_out) {
        RU_REQUIRE(!cm_overlap(mask_out, (ks + 3) / 4, data, nd) && !cm_overlap(mask_out, (ks + 3) / 4, target, nt), "ru_carvemix_mix: mask_out overlaps a receiver tensor");
        for (const auto& r : reads) RU_REQUIRE(!cm_overlap(mask_out, (ks + 3) / 4, r.p, r.len), "ru_carvemix_mix: mask_out overlaps an input");
    }
    hipStream_t s = (hipStream_t)stream;
    for (int k0 = 0; k0 < K; k0 += RU_CARVE_BATCH_MAX) {
        const int cnt = K - k0 < RU_CARVE_BATCH_MAX ? K - k0 : RU_CARVE_BATCH_MAX;
        CmMixArgs a = {};
        unsigned gx = 1;
        for (int j = 0; j < cnt; ++j) {
            const int k = k0 + j;
            CmPair& p = a.p[j];
            p.xa = (const unsigned*)(donor_data + (size_t)k * C * n);
            p.ya = (const unsigned*)(donor_target + (size_t)k * 3 * n);
            p.s = s_map + (size_t)k * n;
            p.xb = (unsigned*)(data + (size_t)dst[k] * C * n);
            p.yb = (unsigned*)(target + (size_t)dst[k] * 3 * n);
            p.mask = mask_out ? mask_out + (size_t)k * n : nullptr;
            // a quad is 16-byte aligned in every channel of the five tensors only if consecutive channels sit alike (n % 4 == 0) and the
            // five bases do; otherwise the pair goes one by one
            const void* const ptrs[5] = {p.s, p.xa, p.ya, p.xb, p.yb};
            p.l = (n & 3u) == 0 ? lanes_for(n, ptrs) : Lanes{n, 0};
            const unsigned g = fl_grid(p.l, n);
            gx = g > gx ? g : gx;
        }
        hipLaunchKernelGGL(cm_mix_kernel, dim3(gx, cnt), dim3(FL_BLOCK), 0, s, a, T + k0, C, n);
        RU_CHECK_LAUNCH("cm_mix_kernel");
    }
    return RU_OK;
}
