// lesion_loss.hip -- the lesion-wise Dice loss (Kofler et al.'s blob loss on the Dice of Dice_loss_joint; include/resunet_hip.h and
// INTEGRATION.md state the definition): the training-side counterpart of lesion.hip's scorer.  Per (sample n, channel c) the target mask
// G = g > 0.5f is grouped into the lesions T_i = G & Z_i, Z_i the 26-connected components of G dilated by the 18-neighbour structure, and the
// Dice of every kept lesion is formed over its own domain: the background and that lesion, the other lesions masked out.
//
//   zero2_kernel           : clears the per-root integer sums and the per-pair records (mask_bits.hpp); the per-root volumes are cleared by
//                            cc_init_kernel's clear slot.
//   ll_pack_kernel         : G as bit rows (mask_bits.hpp, mask_pack_rows).
//   ls_dilate_kernel       : Z = Dil(G), one launch per iteration (mask_dilate.hpp, shared with lesion.hip).
//   cc_*_kernel<LlPlanes>  : the union-find labelling of cc_unionfind.hpp from the plane of Z, every (n, c) in one launch sequence, straight
//                            into labels_out.  After its last compress every voxel of Z holds its root, the smallest index of its component.
//   ll_sum_kernel          : one streaming pass over p, g and the labels.  Per voxel qI = llrint(p g 2^35), qU = llrint(p p 2^35) +
//                            llrint(g 2^35) from exact float64 products.  A voxel outside G adds to the workgroup's background partial (one
//                            atomic per workgroup) and its label becomes -1; a voxel of G adds (1, qI, qU) to the slots of its root, wave-
//                            aggregated and run-carrying as cc_count_members / pp_count_kernel: one atomic per run per wave.  A workgroup
//                            takes a contiguous chunk, so a wave's run lasts across its iterations inside one lesion.  Each lane reads
//                            and writes only its own label, so the rewrite races with nothing.
//   ll_eval_kernel         : grid (blocks, N*C): the roots are the voxels whose volume slot is non-zero (a lesion is never empty).  Per root
//                            Dice_i, a_i, b_i in float64; (a_i, b_i) -- zeros for a dropped lesion -- go to the root's coefficient slot;
//                            a workgroup adds its roots in a fixed order (lane by lane ascending, then the 256 lanes in order) into one
//                            partial.
//   ll_final_kernel        : one workgroup: per pair the partials in block order -> A, B, L and the pair loss; then one lane adds the pair
//                            losses in pair order into totals_out.
//   ll_grad (stream_kernel): flat_lanes.hpp's walk over p, g, labels and dp: s (b p - a g) with (a, b) looked up through the label, (A, B)
//                            on the background, in float64, rounded once to float32.  M is read from the all-reduced totals on the device.
// Integer atomics only: the integer sums do not depend on the order of execution, every float64 sum is taken in an order that is a function
// of the shape alone, so two calls give identical bytes.  Nothing waits for the host.  The number of lesions is not limited: all per-lesion
// storage is indexed by the root's voxel index.
#include "ru_common.h"
#include "pw_helpers.hpp"
#include "cc_unionfind.hpp"
#include "mask_bits.hpp"
#include "mask_dilate.hpp"
#include "flat_lanes.hpp"

#include <limits.h>
#include <math.h>

namespace ru {
namespace {

constexpr double LL_SCALE = 34359738368.0;                 // 2^35: 2^27 voxels x 2 x 2^35 < 2^63
constexpr double LL_UNSCALE = 1.0 / 34359738368.0;
constexpr unsigned LL_EVAL_BLOCKS = 64;                     // workgroups per (n, c) in ll_eval_kernel, at most

// the record of one (n, c), 64 bytes: ops.lesion_loss_table reads it as 8 int64
struct LlPair {
    double A, B, loss;                                      // sum of a_i, of b_i over the kept lesions; 1 - mean Dice_i (0 where L = 0)
    long long L, nles;                                      // kept lesions, lesions
    u64 qI0, qU0;                                           // the background's integer sums
    u64 pad;
};
static_assert(sizeof(LlPair) == 64, "LlPair is read from Python as 8 x 8 bytes");

struct LlPart { double sd, sa, sb; long long kept, nles; };

// state_out: [pairs | vol | qI | qU | ab], every slice 256-byte aligned
struct LlState {
    LlPair* pairs;              // [NK]
    int* vol;                   // [NK][V]   |T_i| at the root of Z_i, 0 elsewhere
    u64 *qI, *qU;               // [NK][V]   the lesion's integer sums at its root; qU follows qI without a gap
    double2* ab;                // [NK][V]   (a_i, b_i) at the root, (0, 0) for a dropped lesion; written at roots only
    size_t off[5], bytes;
};
LlState ll_state(char* base, size_t NK, size_t V) {
    LlState s;
    size_t off = 0;
    int k = 0;
    auto take = [&](size_t bytes) { char* p = base + off; s.off[k++] = off; off += align_up(bytes, 256); return p; };
    s.pairs = (LlPair*)take(NK * sizeof(LlPair));
    s.vol = (int*)take(NK * V * sizeof(int));
    s.qI = (u64*)take(2 * NK * V * sizeof(u64));
    s.qU = s.qI + NK * V;
    s.off[k++] = s.off[2] + NK * V * sizeof(u64);
    s.ab = (double2*)take(NK * V * sizeof(double2));
    s.bytes = off;
    return s;
}

struct LlWs {
    u64* bits;                  // [NK][4][words]: planes 0 and 1 = G, 2 and 3 = the dilation's ping-pong
    LlPart* parts;              // [NK][LL_EVAL_BLOCKS]
    size_t bytes;
};
LlWs ll_ws(char* base, size_t NK, const MaskGeom& g) {
    LlWs w;
    size_t off = 0;
    auto take = [&](size_t bytes) { char* p = base + off; off += align_up(bytes, 256); return p; };
    w.bits = (u64*)take(NK * 4 * g.words * sizeof(u64));
    w.parts = (LlPart*)take(NK * LL_EVAL_BLOCKS * sizeof(LlPart));
    w.bytes = off;
    return w;
}

bool ll_shape_ok(int N, int C, int D, int H, int W) {
    return mask_shape_ok(RU_SURFACE_PROB, N, C, D, H, W) && (size_t)D * H * W < (size_t)INT_MAX && (long long)N * C <= 65535;
}
unsigned ll_eval_blocks(size_t V) { return grid1d(V, 256 * 16, LL_EVAL_BLOCKS); }

// grid (D, N*C), 256 threads: both mask planes of mask_pack_rows are G
__global__ __launch_bounds__(256) void ll_pack_kernel(const float* __restrict__ g, int C, MaskGeom s, u64* __restrict__ bits) {
    u64 c[4];
    mask_pack_rows<0, false>(g, g, C, C, s, bits, c);
}

// the labelling's foreground: plane `zplane` of (n, c) = nk
struct LlPlanes {
    const u64* plane;
    size_t words;
    int WW, zplane;
    __device__ void select(int nk, int) { plane += ((size_t)nk * 4 + zplane) * words; }
    __device__ bool operator()(size_t row, int x) const { return mask_bit(plane, WW, row, x); }
};

__device__ __forceinline__ u64 wave_sum_u64(u64 v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// the voxel's integers: the products are exact in float64 (24 + 24 bits), the scale is a power of two, llrint rounds to nearest even
__device__ __forceinline__ void ll_quant(float p, float g, u64& qi, u64& qu) {
    const double pd = (double)p, gd = (double)g;
    qi = (u64)llrint(pd * gd * LL_SCALE);
    qu = (u64)llrint(pd * pd * LL_SCALE) + (u64)llrint(gd * LL_SCALE);
}

// grid (blocks, N*C), 256 threads
__global__ __launch_bounds__(256) void ll_sum_kernel(const float* __restrict__ p, const float* __restrict__ g, int* labels, size_t V,
                                                     int* __restrict__ vols, u64* __restrict__ qIs, u64* __restrict__ qUs, LlPair* __restrict__ pairs) {
    __shared__ u64 sm[8];
    const size_t base = (size_t)blockIdx.y * V;
    const float* __restrict__ pn = p + base;
    const float* __restrict__ gn = g + base;
    int* lab = labels + base;
    int* __restrict__ vol = vols + base;
    u64* __restrict__ qI = qIs + base;
    u64* __restrict__ qU = qUs + base;
    // a workgroup takes a CONTIGUOUS chunk, a multiple of 256 voxels so that whole waves stay in the loop (the ballots and shuffles need
    // every lane): a wave's successive iterations are 256 voxels apart, mostly inside the same lesion, and the run it carries keeps growing
    const size_t chunk = ((V + gridDim.x - 1) / gridDim.x + 255) / 256 * 256, lo = (size_t)blockIdx.x * chunk;
    const bool first = (threadIdx.x & 63) == 0;
    int run_root = -1, run_cnt = 0;                            // (wave-uniform)
    u64 run_I = 0, run_U = 0, bI = 0, bU = 0;
    for (size_t off = threadIdx.x; off < chunk; off += 256) {
        const size_t v = lo + off;
        int root = -1;
        u64 qi = 0, qu = 0;
        if (v < V) {
            const float gv = gn[v];
            ll_quant(pn[v], gv, qi, qu);
            const int l = lab[v];
            if (gv > 0.5f) root = l;                           // G is inside Z: l is the root of the voxel's component, in [0, V)
            else {
                bI += qi;
                bU += qu;
                if (l >= 0) lab[v] = -1;                       // Z \ G is background
            }
        }
        u64 todo = __ballot(root >= 0);
        while (todo) {
            const int leader = __builtin_ctzll(todo);
            const int lroot = __shfl(root, leader);
            const u64 same = __ballot(root == lroot) & todo;
            const int n = (int)__builtin_popcountll(same);
            const u64 si = wave_sum_u64(root == lroot ? qi : 0ull), su = wave_sum_u64(root == lroot ? qu : 0ull);
            if (lroot == run_root) { run_cnt += n; run_I += si; run_U += su; }
            else {
                if (run_cnt && first) { atomicAdd(vol + run_root, run_cnt); atomicAdd(qI + run_root, run_I); atomicAdd(qU + run_root, run_U); }
                run_root = lroot; run_cnt = n; run_I = si; run_U = su;
            }
            todo &= ~same;
        }
    }
    if (run_cnt && first) { atomicAdd(vol + run_root, run_cnt); atomicAdd(qI + run_root, run_I); atomicAdd(qU + run_root, run_U); }
    bI = wave_sum_u64(bI);
    bU = wave_sum_u64(bU);
    if (first) { sm[(threadIdx.x >> 6) * 2] = bI; sm[(threadIdx.x >> 6) * 2 + 1] = bU; }
    __syncthreads();
    if (threadIdx.x == 0) {
        const u64 tI = sm[0] + sm[2] + sm[4] + sm[6], tU = sm[1] + sm[3] + sm[5] + sm[7];
        if (tI) atomicAdd(&pairs[blockIdx.y].qI0, tI);
        if (tU) atomicAdd(&pairs[blockIdx.y].qU0, tU);
    }
}

// grid (ll_eval_blocks(V), N*C), 256 threads: block x takes the voxels [x * chunk, (x + 1) * chunk)
__global__ __launch_bounds__(256) void ll_eval_kernel(size_t V, const int* __restrict__ vols, const u64* __restrict__ qIs, const u64* __restrict__ qUs,
                                                      const LlPair* __restrict__ pairs, double2* __restrict__ abs, long long min_volume,
                                                      LlPart* __restrict__ parts) {
#pragma clang fp contract(off)
    __shared__ LlPart sm[256];
    const int nk = blockIdx.y;
    const size_t base = (size_t)nk * V;
    const u64 I0 = pairs[nk].qI0, U0 = pairs[nk].qU0;
    const size_t chunk = (V + gridDim.x - 1) / gridDim.x;
    const size_t lo = (size_t)blockIdx.x * chunk, hi = lo + chunk < V ? lo + chunk : V;
    LlPart acc = {0.0, 0.0, 0.0, 0, 0};
    for (size_t v = lo + threadIdx.x; v < hi; v += 256) {
        const int n = vols[base + v];
        if (n <= 0) continue;
        const double I = (double)(I0 + qIs[base + v]) * LL_UNSCALE, U = (double)(U0 + qUs[base + v]) * LL_UNSCALE;
        const double num = I + 1e-6, den = U + 2e-6;
        const double dice = 2.0 * num / den, a = 2.0 / den, b = 4.0 * num / (den * den);
        const bool kept = (long long)n > min_volume;
        abs[base + v] = kept ? make_double2(a, b) : make_double2(0.0, 0.0);
        ++acc.nles;
        if (!kept) continue;
        ++acc.kept;
        acc.sd += dice;
        acc.sa += a;
        acc.sb += b;
    }
    sm[threadIdx.x] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        LlPart t = {0.0, 0.0, 0.0, 0, 0};
        for (int i = 0; i < 256; ++i) {
            t.sd += sm[i].sd; t.sa += sm[i].sa; t.sb += sm[i].sb; t.kept += sm[i].kept; t.nles += sm[i].nles;
        }
        parts[(size_t)nk * LL_EVAL_BLOCKS + blockIdx.x] = t;
    }
}

// one workgroup of 256
__global__ __launch_bounds__(256) void ll_final_kernel(int NK, unsigned blocks, const LlPart* __restrict__ parts, LlPair* pairs,
                                                       long long* __restrict__ stats, double* __restrict__ totals) {
#pragma clang fp contract(off)
    for (int nk = threadIdx.x; nk < NK; nk += 256) {
        LlPart t = {0.0, 0.0, 0.0, 0, 0};
        for (unsigned i = 0; i < blocks; ++i) {
            const LlPart q = parts[(size_t)nk * LL_EVAL_BLOCKS + i];
            t.sd += q.sd; t.sa += q.sa; t.sb += q.sb; t.kept += q.kept; t.nles += q.nles;
        }
        pairs[nk].A = t.sa;
        pairs[nk].B = t.sb;
        pairs[nk].L = t.kept;
        pairs[nk].nles = t.nles;
        pairs[nk].loss = t.kept ? 1.0 - t.sd / (double)t.kept : 0.0;
        stats[(size_t)nk * 2] = t.nles;
        stats[(size_t)nk * 2 + 1] = t.kept;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double sum = 0.0;
        long long M = 0;
        for (int nk = 0; nk < NK; ++nk)
            if (pairs[nk].L >= 1) { sum += pairs[nk].loss; ++M; }
        totals[0] = sum;
        totals[1] = (double)M;
    }
}

// dp = s (b p - a g), s = priority * (*scale) / (M * L) of the voxel's pair (0 where L = 0 or M = 0); (a, b) = the coefficients of the
// voxel's lesion, (A, B) on the background.  A dropped lesion has a = b = 0: its voxels are exact zeros.
struct LlGradOp {
    const float* p; const float* g; const int* lab; const double2* ab; const LlPair* pairs; const double* totals; double k; const float* scale;
    float* dp; size_t V;
    double M;
    __device__ __forceinline__ void begin() {
        M = totals[1];
        if (scale) k *= (double)*scale;
    }
    struct PairCoef { double s, A, B; };
    __device__ __forceinline__ PairCoef pair(size_t nk) const {
#pragma clang fp contract(off)
        const LlPair& r = pairs[nk];
        const long long L = r.L;
        PairCoef c = {(M >= 1.0 && L >= 1) ? k / (M * (double)L) : 0.0, r.A, r.B};
        return c;
    }
    __device__ __forceinline__ float elem(const PairCoef& c, size_t nk, float pv, float gv, int l) const {
#pragma clang fp contract(off)
        double a = c.A, b = c.B;
        if (l >= 0) { const double2 q = ab[nk * V + (size_t)l]; a = q.x; b = q.y; }
        return (float)(c.s * (b * (double)pv - a * (double)gv));
    }
    __device__ __forceinline__ void one(size_t i) const {
        const size_t nk = i / V;
        dp[i] = elem(pair(nk), nk, p[i], g[i], lab[i]);
    }
    struct Q { float4 p, g; int4 l; };
    __device__ __forceinline__ Q load(size_t i) const { return Q{ld4(p + i), ld4(g + i), ld4i(lab + i)}; }
    __device__ __forceinline__ void finish(size_t i, const Q& q) const {
        const size_t nk = i / V;
        if (i + 3 < (nk + 1) * V) {
            const PairCoef c = pair(nk);
            st4(dp + i, make_float4(elem(c, nk, q.p.x, q.g.x, q.l.x), elem(c, nk, q.p.y, q.g.y, q.l.y), elem(c, nk, q.p.z, q.g.z, q.l.z),
                                    elem(c, nk, q.p.w, q.g.w, q.l.w)));
        } else {                                                // the quad straddles two (or, for a tiny volume, more) pairs
            const size_t n1 = (i + 1) / V, n2 = (i + 2) / V, n3 = (i + 3) / V;
            st4(dp + i, make_float4(elem(pair(nk), nk, q.p.x, q.g.x, q.l.x), elem(pair(n1), n1, q.p.y, q.g.y, q.l.y),
                                    elem(pair(n2), n2, q.p.z, q.g.z, q.l.z), elem(pair(n3), n3, q.p.w, q.g.w, q.l.w)));
        }
    }
};

}  // namespace
}  // namespace ru

using namespace ru;

extern "C" size_t ru_lesion_loss_workspace_bytes(int N, int C, int D, int H, int W) {
    if (!ll_shape_ok(N, C, D, H, W)) return 0;
    return ll_ws(nullptr, (size_t)N * C, mask_geom(D, H, W)).bytes;
}

extern "C" size_t ru_lesion_loss_state_bytes(int N, int C, int D, int H, int W, size_t* offsets5) {
    if (!ll_shape_ok(N, C, D, H, W)) return 0;
    const LlState s = ll_state(nullptr, (size_t)N * C, (size_t)D * H * W);
    if (offsets5)
        for (int i = 0; i < 5; ++i) offsets5[i] = s.off[i];
    return s.bytes;
}

// passes: 1 = clears, pack and dilation; 2 = + labelling; 3 = + sum; 4 = + evaluate: the whole forward
extern "C" int ru_lesion_loss_forward_upto(const float* p, const float* g, int N, int C, int D, int H, int W, int dilation, long long min_volume,
                                           int* labels_out, void* state_out, double* totals_out, long long* stats_out, void* ws, size_t ws_bytes,
                                           int passes, ru_stream_t stream) {
    RU_REQUIRE(p && g && labels_out && state_out && totals_out && stats_out && N > 0 && C > 0 && passes >= 1 && passes <= 4,
               "ru_lesion_loss_forward: bad argument");
    RU_REQUIRE(D >= 1 && H >= 1 && W >= 1 && D <= MAX_EXTENT && H <= MAX_EXTENT && W <= MAX_EXTENT,
               "ru_lesion_loss_forward: extents %d x %d x %d: every axis must be in [1, %d]", D, H, W, MAX_EXTENT);
    RU_REQUIRE((size_t)D * H * W < (size_t)INT_MAX, "ru_lesion_loss_forward: volume too large for 32-bit voxel indices");
    RU_REQUIRE(dilation >= 0 && dilation <= MAX_EXTENT && min_volume >= 0, "ru_lesion_loss_forward: dilation %d, min_volume %lld: both must be >= 0",
               dilation, min_volume);
    RU_REQUIRE((long long)N * C <= 65535, "ru_lesion_loss_forward: N * C = %lld: the grid needs N * C <= 65535", (long long)N * C);
    RU_REQUIRE(aligned4(p) && aligned4(g) && aligned4(labels_out) && ((uintptr_t)state_out & 15u) == 0 && ((uintptr_t)totals_out & 7u) == 0 &&
                   ((uintptr_t)stats_out & 7u) == 0 && ((uintptr_t)ws & 7u) == 0,
               "ru_lesion_loss_forward: misaligned pointer");
    const size_t need = ru_lesion_loss_workspace_bytes(N, C, D, H, W);
    RU_REQUIRE(ws && need && ws_bytes >= need, "ru_lesion_loss_forward: workspace too small");
    hipStream_t st = (hipStream_t)stream;
    const MaskGeom s = mask_geom(D, H, W);
    const int NK = N * C;
    const LlWs w = ll_ws((char*)ws, (size_t)NK, s);
    const LlState q = ll_state((char*)state_out, (size_t)NK, s.V);
    const size_t nsum = 2 * (size_t)NK * s.V, npair = (size_t)NK * (sizeof(LlPair) / sizeof(u64));
    hipLaunchKernelGGL((zero2_kernel<u64, u64>), dim3(grid1d(nsum + npair, 256 * 4, 4096)), dim3(256), 0, st, q.qI, nsum, (u64*)q.pairs, npair);
    RU_CHECK_LAUNCH("zero2_kernel");
    hipLaunchKernelGGL(ll_pack_kernel, dim3(D, NK), dim3(256), 0, st, g, C, s, w.bits);
    RU_CHECK_LAUNCH("ll_pack_kernel");
    int zplane = 1;                                              // dilation 0: Z = G
    const unsigned gw = grid1d(s.words, 256, 4096), gv = grid1d(s.V, 256 * 4, 4096);
    for (int it = 0; it < dilation; ++it) {
        const int dst = zplane == 2 ? 3 : 2;
        hipLaunchKernelGGL(ls_dilate_kernel, dim3(gw, NK), dim3(256), 0, st, s, w.bits, zplane, dst);
        RU_CHECK_LAUNCH("ls_dilate_kernel");
        zplane = dst;
    }
    if (passes < 2) return RU_OK;
    const LlPlanes planes = {w.bits, s.words, s.WW, zplane};
    const int rl = cc_label(planes, labels_out, (size_t)0, q.vol, D, H, W, dim3(gv, NK, 1), st);       // (clears vol)
    if (rl) return rl;
    if (passes < 3) return RU_OK;
    hipLaunchKernelGGL(ll_sum_kernel, dim3(grid1d(s.V, 256 * 32, 1024), NK), dim3(256), 0, st, p, g, labels_out, s.V, q.vol, q.qI, q.qU, q.pairs);
    RU_CHECK_LAUNCH("ll_sum_kernel");
    if (passes < 4) return RU_OK;
    const unsigned eb = ll_eval_blocks(s.V);
    hipLaunchKernelGGL(ll_eval_kernel, dim3(eb, NK), dim3(256), 0, st, s.V, (const int*)q.vol, (const u64*)q.qI, (const u64*)q.qU,
                       (const LlPair*)q.pairs, q.ab, min_volume, w.parts);
    RU_CHECK_LAUNCH("ll_eval_kernel");
    hipLaunchKernelGGL(ll_final_kernel, dim3(1), dim3(256), 0, st, NK, eb, (const LlPart*)w.parts, q.pairs, stats_out, totals_out);
    RU_CHECK_LAUNCH("ll_final_kernel");
    return RU_OK;
}

extern "C" int ru_lesion_loss_forward(const float* p, const float* g, int N, int C, int D, int H, int W, int dilation, long long min_volume,
                                      int* labels_out, void* state_out, double* totals_out, long long* stats_out, void* ws, size_t ws_bytes,
                                      ru_stream_t stream) {
    return ru_lesion_loss_forward_upto(p, g, N, C, D, H, W, dilation, min_volume, labels_out, state_out, totals_out, stats_out, ws, ws_bytes, 4, stream);
}

extern "C" int ru_lesion_loss_grad(const float* p, const float* g, const int* labels, const void* state, const double* totals_global,
                                   double priority, const float* scale, float* dp, int N, int C, int D, int H, int W, ru_stream_t stream) {
    RU_REQUIRE(p && g && labels && state && totals_global && dp && N > 0 && C > 0, "ru_lesion_loss_grad: bad argument");
    RU_REQUIRE(ll_shape_ok(N, C, D, H, W), "ru_lesion_loss_grad: bad shape %d x %d x %d x %d x %d", N, C, D, H, W);
    RU_REQUIRE(priority == priority && fabs(priority) <= 1.7e308, "ru_lesion_loss_grad: priority %g is not finite", priority);
    RU_REQUIRE(aligned4(p) && aligned4(g) && aligned4(labels) && aligned4(dp) && ((uintptr_t)state & 15u) == 0 && ((uintptr_t)totals_global & 7u) == 0,
               "ru_lesion_loss_grad: misaligned pointer");
    const size_t V = (size_t)D * H * W, NK = (size_t)N * C, n = NK * V;
    RU_REQUIRE(!overlap(p, dp, n) && !overlap(g, dp, n) && !overlap(labels, dp, n), "ru_lesion_loss_grad: dp overlaps an input");
    const LlState q = ll_state((char*)const_cast<void*>(state), NK, V);
    const void* const ptrs[4] = {p, g, labels, dp};
    return stream_launch(LlGradOp{p, g, labels, q.ab, q.pairs, totals_global, priority, scale, dp, V, 0.0}, n, lanes_for(n, ptrs), (hipStream_t)stream,
                         "lesion_loss_grad_kernel");
}
