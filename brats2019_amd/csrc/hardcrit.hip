// hardcrit.hip -- the criteria for hard voxels and small regions beside the reference's list (criteria.hip): focal loss, Tversky /
// focal-Tversky and top-k cross entropy on the [N, C, V] probability / target pair.
//
//   focal    f = -(a1 g (1-p)^gamma log(p + 1e-6) + a0w (1-g) p^gamma log((1 + 1e-6) - p)), mean over all elements
//            FocalSumOp -> one float64 slot per workgroup, sum_slots_kernel adds the slots in index order; FocalGradOp writes dp
//   Tversky  a closed form in ru_crit_moments' sums (sum pg, sum p, sum g): tversky_eval_kernel writes the value and the per-row
//            coefficients that ru_crit_grad applies
//   top-k    the mean of the K largest l = -(g log(p + 1e-6) + w (1-g) log((1 + 1e-6) - p)).  topk_key_kernel forms l ONCE, stores it as an
//            order-preserving 32-bit key and histograms the key's top 11 bits; two more passes over the stored keys histogram the next 11 and
//            the last 10 bits of the keys that share the prefix found so far (topk_hist_kernel), a one-workgroup scan after each pass picks
//            the bin of the K-th largest key and the rank that remains (topk_scan_kernel).  TopkValueOp sums the l above the threshold
//            into float64 slots, topk_final_kernel adds them in index order; TopkGradOp reads the same stored keys, so every pass
//            sees the same bits of l.
//
// All passes are flat streaming work over n = N*C*V elements in the lane layout of flat_lanes.hpp: the sums are ops of its sum_kernel, the
// gradients ops of its stream_kernel, the two histogram kernels call its walk between their own prologue and epilogue.  No float atomics:
// sums are float64 slots added in a fixed order; the histograms are integers.  Nothing waits for the host.
#include "ru_common.h"
#include "pw_helpers.hpp"
#include "flat_lanes.hpp"

#include <math.h>
#include <stdint.h>

namespace ru {
namespace {

constexpr int HC_BLOCK = FL_BLOCK;             // the lane layout, the grid cap and the slot sums: flat_lanes.hpp
constexpr int HC_BINS = 2048;                    // 11 bits per radix level (the last level uses 10 of them)
constexpr int HC_WAVES = HC_BLOCK / 64;
constexpr int HC_STATE = 4;                      // state[0] key found so far (low bits 0), [1] rank that remains, [2] n_gt, [3] n_eq

// the float32 constants of the reference's BCE expressions (loss.py:77): pred + 1e-6, (1. + 1e-6) - pred
__device__ __forceinline__ float hc_pe(float p) { return p + 1e-6f; }
__device__ __forceinline__ float hc_qe(float p) { return (float)(1.0 + 1e-6) - p; }

// ------------------------------------------------------------------ focal
// MODE 0: gamma == 0 (the gamma x^(gamma-1) terms are dropped, not multiplied by zero), 1: gamma == 1, 2: gamma == 2, 3: any gamma > 1
template <int MODE>
__device__ __forceinline__ void focal_pows(float x, float gamma, float& xg, float& gxg1) {
    if (MODE == 0) { xg = 1.f; gxg1 = 0.f; }
    else if (MODE == 1) { xg = x; gxg1 = 1.f; }
    else if (MODE == 2) { xg = x * x; gxg1 = 2.f * x; }
    else { const float r = powf(x, gamma - 1.f); xg = r * x; gxg1 = gamma * r; }
}
struct FocalP { float gamma, a1, a0w; };

template <int MODE>
__device__ __forceinline__ float focal_value(float p, float g, const FocalP& k) {
    float omg, gomg1, pg, gpg1;
    focal_pows<MODE>(1.f - p, k.gamma, omg, gomg1);
    focal_pows<MODE>(p, k.gamma, pg, gpg1);
    return -(k.a1 * g * omg * logf(hc_pe(p)) + k.a0w * (1.f - g) * pg * logf(hc_qe(p)));
}
template <int MODE>
__device__ __forceinline__ float focal_deriv(float p, float g, const FocalP& k) {
    float omg, gomg1, pg, gpg1;
    focal_pows<MODE>(1.f - p, k.gamma, omg, gomg1);
    focal_pows<MODE>(p, k.gamma, pg, gpg1);
    const float pe = hc_pe(p), qe = hc_qe(p);
    float pos = omg / pe, neg = -pg / qe;
    if (MODE != 0) { pos -= gomg1 * logf(pe); neg += gpg1 * logf(qe); }
    return -k.a1 * g * pos - k.a0w * (1.f - g) * neg;
}

template <int MODE>
struct FocalSumOp {
    const float* p; const float* g; FocalP k;
    __device__ __forceinline__ double quad(size_t i) const {
        const float4 pv = ld4(p + i), gv = ld4(g + i);
        return ((double)focal_value<MODE>(pv.x, gv.x, k) + (double)focal_value<MODE>(pv.y, gv.y, k)) +
               ((double)focal_value<MODE>(pv.z, gv.z, k) + (double)focal_value<MODE>(pv.w, gv.w, k));
    }
    __device__ __forceinline__ double one(size_t i) const { return (double)focal_value<MODE>(p[i], g[i], k); }
};

// dp = df/dp * mult * (*scale if given)
template <int MODE>
struct FocalGradOp {
    const float* p; const float* g; FocalP k; float m; const float* scale; float* dp;      // m = mult, from begin() on times *scale
    __device__ __forceinline__ void begin() { if (scale) m *= *scale; }
    __device__ __forceinline__ void one(size_t i) const { dp[i] = m * focal_deriv<MODE>(p[i], g[i], k); }
    struct Q { float4 p, g; };
    __device__ __forceinline__ Q load(size_t i) const { return Q{ld4(p + i), ld4(g + i)}; }
    __device__ __forceinline__ void finish(size_t i, const Q& q) const {
        st4(dp + i, make_float4(m * focal_deriv<MODE>(q.p.x, q.g.x, k), m * focal_deriv<MODE>(q.p.y, q.g.y, k), m * focal_deriv<MODE>(q.p.z, q.g.z, k),
                                m * focal_deriv<MODE>(q.p.w, q.g.w, k)));
    }
};

inline int focal_mode(float gamma) { return gamma == 0.f ? 0 : gamma == 1.f ? 1 : gamma == 2.f ? 2 : 3; }

// ------------------------------------------------------------------ Tversky
// tot: ru_crit_reduce's (all-reduced) per-channel totals.  value = priority * mean_c (1 - TI_c)^(1/gamma); coef rows: only a and c
__global__ __launch_bounds__(HC_BLOCK) void tversky_eval_kernel(const double* __restrict__ tot, int N, int C, double alpha, double beta, double gamma,
                                                                double smooth, double priority, double* __restrict__ value, float* __restrict__ coef) {
    if (threadIdx.x == 0) {
        double acc = 0.0;
        for (int c = 0; c < C; ++c) {
            const double tp = tot[c * RU_CRIT_MOMENTS + RU_CRIT_M_PG], sp = tot[c * RU_CRIT_MOMENTS + RU_CRIT_M_P], sg = tot[c * RU_CRIT_MOMENTS + RU_CRIT_M_G];
            const double den = tp + alpha * (sp - tp) + beta * (sg - tp) + smooth;
            const double u = 1.0 - (tp + smooth) / den;
            acc += gamma == 1.0 ? u : pow(u, 1.0 / gamma);
        }
        *value = priority * acc / C;
    }
    for (int row = threadIdx.x; row < N * C; row += HC_BLOCK) {
        const int c = row % C;
        const double tp = tot[c * RU_CRIT_MOMENTS + RU_CRIT_M_PG], sp = tot[c * RU_CRIT_MOMENTS + RU_CRIT_M_P], sg = tot[c * RU_CRIT_MOMENTS + RU_CRIT_M_G];
        const double den = tp + alpha * (sp - tp) + beta * (sg - tp) + smooth;
        const double u = 1.0 - (tp + smooth) / den;
        const double o = -priority / C * (gamma == 1.0 ? 1.0 : pow(u, 1.0 / gamma - 1.0) / gamma);
        float* k5 = coef + (size_t)row * 5;
        k5[0] = (float)(o * (den - (tp + smooth) * (1.0 - alpha - beta)) / (den * den));
        k5[1] = 0.f;
        k5[2] = (float)(-o * alpha * (tp + smooth) / (den * den));
        k5[3] = 0.f;
        k5[4] = 0.f;
    }
}

// ------------------------------------------------------------------ top-k
// l formed in float32 as BCE_Loss forms it, then made a key whose unsigned order is the order of l: -0 counts as +0, NaN ranks above all
__device__ __forceinline__ unsigned topk_key(float p, float g, float w) {
    const float l = -(g * logf(hc_pe(p)) + w * (1.f - g) * logf(hc_qe(p))) + 0.f;
    if (l != l) return 0xffffffffu;
    const unsigned b = __float_as_uint(l);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float topk_unkey(unsigned k) {
    if (k == 0xffffffffu) return __uint_as_float(0x7fc00000u);
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}
__device__ __forceinline__ float topk_dl(float p, float g, float w) { return w * (1.f - g) / hc_qe(p) - g / hc_pe(p); }

// The workgroup's histogram lives in LDS, one copy per wave: at the first level the key's top bits are nearly all exponent, about a
// hundred bins are hit, and the four waves would otherwise queue on the same words.  Within a lane, equal bins of a quad are added once.
struct Hist {
    unsigned* h;                                                     // this wave's copy
    __device__ __forceinline__ void add(unsigned bin, unsigned cnt) { atomicAdd(h + bin, cnt); }
    __device__ __forceinline__ void add4(bool ax, bool ay, bool az, bool aw, unsigned bx, unsigned by, unsigned bz, unsigned bw) {
        // run-length over the quad: neighbours in memory are neighbours in value often enough at the first level
        unsigned cur = 0, cnt = 0;
        const bool a[4] = {ax, ay, az, aw};
        const unsigned b[4] = {bx, by, bz, bw};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (!a[j]) continue;
            if (cnt && b[j] == cur) { ++cnt; continue; }
            if (cnt) add(cur, cnt);
            cur = b[j];
            cnt = 1;
        }
        if (cnt) add(cur, cnt);
    }
};
__device__ __forceinline__ void hist_clear(unsigned* lds) {
    for (int i = threadIdx.x; i < HC_WAVES * HC_BINS; i += HC_BLOCK) lds[i] = 0u;
    __syncthreads();
}
// the workgroup's non-zero bins go to the global histogram with integer atomics
__device__ __forceinline__ void hist_flush(const unsigned* lds, unsigned* __restrict__ hist) {
    __syncthreads();
    for (int b = threadIdx.x; b < HC_BINS; b += HC_BLOCK) {
        unsigned c = 0;
#pragma unroll
        for (int w = 0; w < HC_WAVES; ++w) c += lds[w * HC_BINS + b];
        if (c) atomicAdd(hist + b, c);
    }
}

// level 1: l -> key, stored; histogram of key >> 21
__global__ __launch_bounds__(HC_BLOCK) void topk_key_kernel(const float* __restrict__ p, const float* __restrict__ g, size_t n, Lanes l, float w,
                                                            unsigned* __restrict__ keys, unsigned* __restrict__ hist) {
    __shared__ unsigned lds[HC_WAVES * HC_BINS];
    hist_clear(lds);
    Hist H{lds + (threadIdx.x >> 6) * HC_BINS};
    fl_walk(l, n,
            [&](size_t i) {
                const float4 pv = ld4(p + i), gv = ld4(g + i);
                const uint4 k = make_uint4(topk_key(pv.x, gv.x, w), topk_key(pv.y, gv.y, w), topk_key(pv.z, gv.z, w), topk_key(pv.w, gv.w, w));
                st4u(keys + i, k);
                H.add4(true, true, true, true, k.x >> 21, k.y >> 21, k.z >> 21, k.w >> 21);
            },
            [&](size_t i) {
                const unsigned k = topk_key(p[i], g[i], w);
                keys[i] = k;
                H.add(k >> 21, 1u);
            });
    hist_flush(lds, hist);
}

// levels 2 and 3: of the keys whose top `SHIFT + BITS`.. bits equal the prefix found so far, histogram the next BITS bits
template <int SHIFT, int BITS>
__global__ __launch_bounds__(HC_BLOCK) void topk_hist_kernel(const unsigned* __restrict__ keys, size_t n, Lanes l,
                                                             const unsigned long long* __restrict__ state, unsigned* __restrict__ hist) {
    __shared__ unsigned lds[HC_WAVES * HC_BINS];
    hist_clear(lds);
    Hist H{lds + (threadIdx.x >> 6) * HC_BINS};
    const unsigned pre = (unsigned)state[0] >> (SHIFT + BITS);
    constexpr unsigned MASK = (1u << BITS) - 1u;
    fl_walk(l, n,
            [&](size_t i) {
                const uint4 k = ld4u(keys + i);
                H.add4((k.x >> (SHIFT + BITS)) == pre, (k.y >> (SHIFT + BITS)) == pre, (k.z >> (SHIFT + BITS)) == pre, (k.w >> (SHIFT + BITS)) == pre,
                       (k.x >> SHIFT) & MASK, (k.y >> SHIFT) & MASK, (k.z >> SHIFT) & MASK, (k.w >> SHIFT) & MASK);
            },
            [&](size_t i) {
                const unsigned k = keys[i];
                if ((k >> (SHIFT + BITS)) == pre) H.add((k >> SHIFT) & MASK, 1u);
            });
    hist_flush(lds, hist);
}

// one workgroup: walk the bins from the top until the rank that remains falls into one.  state[0] |= bin << shift; state[1] -= the count
// above the bin; state[2] += that count; state[3] = the bin's count (after the last level: the number of keys equal to the threshold)
// first_rank != 0: the first level, the rank is K itself
__global__ __launch_bounds__(HC_BLOCK) void topk_scan_kernel(const unsigned* __restrict__ hist, int shift, unsigned long long first_rank,
                                                             unsigned long long* __restrict__ state) {
    __shared__ unsigned long long part[HC_BLOCK];
    constexpr int PER = HC_BINS / HC_BLOCK;
    // lane j owns bins [HC_BINS - PER*(j+1), HC_BINS - PER*j): lane 0 the highest
    const int top = HC_BINS - 1 - PER * (int)threadIdx.x;
    unsigned long long s = 0;
    for (int j = 0; j < PER; ++j) s += hist[top - j];
    part[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned long long rank = first_rank ? first_rank : state[1];   // 1-based from the largest
        unsigned long long above = 0;
        int lane = 0;
        while (lane < HC_BLOCK - 1 && above + part[lane] < rank) above += part[lane++];
        int bin = HC_BINS - 1 - PER * lane;
        const int last = bin - (PER - 1);
        while (bin > last && above + hist[bin] < rank) above += hist[bin--];
        state[0] |= (unsigned long long)bin << shift;
        state[1] = rank - above;
        state[2] += above;
        state[3] = hist[bin];
    }
}

// the sum of l over the keys above the threshold, float64
struct TopkValueOp {
    const unsigned* keys; const unsigned long long* state;
    __device__ __forceinline__ double above(unsigned k, unsigned tk) const { return k > tk ? (double)topk_unkey(k) : 0.0; }
    __device__ __forceinline__ double quad(size_t i) const {
        const unsigned tk = (unsigned)state[0];
        const uint4 k = ld4u(keys + i);
        return (above(k.x, tk) + above(k.y, tk)) + (above(k.z, tk) + above(k.w, tk));
    }
    __device__ __forceinline__ double one(size_t i) const { return above(keys[i], (unsigned)state[0]); }
};

// out[0] = (sum of the slots + (K - n_gt) * t) / K, out[1] = t
__global__ __launch_bounds__(HC_BLOCK) void topk_final_kernel(const double* __restrict__ slots, size_t n_slots, const unsigned long long* __restrict__ state,
                                                              unsigned long long K, double* __restrict__ out) {
    __shared__ double part[HC_BLOCK];
    const double tot = sum_slots(slots, n_slots, part);
    if (threadIdx.x == 0) {
        const double t = (double)topk_unkey((unsigned)state[0]);
        out[0] = (tot + (double)(K - state[2]) * t) / (double)K;
        out[1] = t;
    }
}

// dp = dl/dp * mult * (*scale) above the threshold, times (K - n_gt) / n_eq at it, 0 below
struct TopkGradOp {
    const float* p; const float* g; const unsigned* keys; float w; const unsigned long long* state; unsigned long long K; double mult;
    const float* scale; float* dp;
    unsigned tk; float m_gt, m_eq;                                   // begin()
    __device__ __forceinline__ void begin() {
        const double m = scale ? mult * (double)*scale : mult;
        tk = (unsigned)state[0];
        m_gt = (float)m;
        m_eq = (float)(m * (double)(K - state[2]) / (double)state[3]);
    }
    __device__ __forceinline__ float dl(float pi, float gi, unsigned k) const {
        return k > tk ? m_gt * topk_dl(pi, gi, w) : k == tk ? m_eq * topk_dl(pi, gi, w) : 0.f;
    }
    __device__ __forceinline__ void one(size_t i) const { dp[i] = dl(p[i], g[i], keys[i]); }
    struct Q { float4 p, g; uint4 k; };
    __device__ __forceinline__ Q load(size_t i) const { return Q{ld4(p + i), ld4(g + i), ld4u(keys + i)}; }
    __device__ __forceinline__ void finish(size_t i, const Q& q) const {
        st4(dp + i, make_float4(dl(q.p.x, q.g.x, q.k.x), dl(q.p.y, q.g.y, q.k.y), dl(q.p.z, q.g.z, q.k.z), dl(q.p.w, q.g.w, q.k.w)));
    }
};

inline bool focal_params_ok(float gamma, float a1, float a0w) { return (gamma == 0.f || gamma >= 1.f) && a1 >= 0.f && a0w >= 0.f; }

// workspace of ru_topk_select: [HC_STATE u64 state | 3 histograms of HC_BINS u32 | slots]
constexpr size_t TOPK_HIST_OFF = HC_STATE * sizeof(unsigned long long);
constexpr size_t TOPK_SLOT_OFF = TOPK_HIST_OFF + 3 * HC_BINS * sizeof(unsigned);

}  // namespace
}  // namespace ru

using namespace ru;

extern "C" size_t ru_focal_workspace_bytes(size_t n) { return n ? fl_slots(n) * sizeof(double) : 0; }

extern "C" int ru_focal_sum(const float* p, const float* g, size_t n, float gamma, float a1, float a0w, double* sum_out, void* ws, size_t ws_bytes,
                            ru_stream_t stream) {
    RU_REQUIRE(p && g && sum_out && ws && n > 0, "ru_focal_sum: bad argument");
    RU_REQUIRE(focal_params_ok(gamma, a1, a0w), "ru_focal_sum: gamma %g must be 0 or at least 1, the weights %g, %g not negative", gamma, a1, a0w);
    RU_REQUIRE(aligned4(p) && aligned4(g) && ((uintptr_t)ws & 7u) == 0 && ((uintptr_t)sum_out & 7u) == 0, "ru_focal_sum: misaligned pointer");
    RU_REQUIRE(ws_bytes >= ru_focal_workspace_bytes(n), "ru_focal_sum: workspace too small");
    hipStream_t s = (hipStream_t)stream;
    const void* const ptrs[2] = {p, g};
    const Lanes l = lanes_for(n, ptrs);
    const FocalP k{gamma, a1, a0w};
    return with_mode<0, 3>(focal_mode(gamma), [&](auto mode) {
        return total_launch(FocalSumOp<mode()>{p, g, k}, n, l, (double*)ws, sum_out, s, "focal_sum_kernel");
    });
}

extern "C" int ru_focal_grad(const float* p, const float* g, size_t n, float gamma, float a1, float a0w, double count, const float* scale, float* dp,
                             ru_stream_t stream) {
    RU_REQUIRE(p && g && dp && n > 0, "ru_focal_grad: bad argument");
    RU_REQUIRE(focal_params_ok(gamma, a1, a0w), "ru_focal_grad: gamma %g must be 0 or at least 1, the weights %g, %g not negative", gamma, a1, a0w);
    RU_REQUIRE(count >= (double)n, "ru_focal_grad: count %g is less than the %zu elements of this shard", count, n);
    RU_REQUIRE(aligned4(p) && aligned4(g) && aligned4(dp), "ru_focal_grad: misaligned pointer");
    RU_REQUIRE(!overlap(p, dp, n) && !overlap(g, dp, n), "ru_focal_grad: dp overlaps an input");
    hipStream_t s = (hipStream_t)stream;
    const void* const ptrs[3] = {p, g, dp};
    const Lanes l = lanes_for(n, ptrs);
    const FocalP k{gamma, a1, a0w};
    const float mult = (float)(1.0 / count);
    return with_mode<0, 3>(focal_mode(gamma), [&](auto mode) {
        return stream_launch(FocalGradOp<mode()>{p, g, k, mult, scale, dp}, n, l, s, "focal_grad_kernel");
    });
}

extern "C" int ru_tversky_eval(const double* totals, int N, int C, double alpha, double beta, double gamma, double smooth, double priority,
                               double* value, float* coef, ru_stream_t stream) {
    RU_REQUIRE(totals && value && coef && N > 0 && C > 0, "ru_tversky_eval: bad argument");
    RU_REQUIRE(alpha >= 0.0 && beta >= 0.0 && gamma >= 1.0 && smooth > 0.0, "ru_tversky_eval: alpha %g, beta %g must not be negative, gamma %g at least 1, smooth %g positive",
               alpha, beta, gamma, smooth);
    hipLaunchKernelGGL(tversky_eval_kernel, dim3(1), dim3(HC_BLOCK), 0, (hipStream_t)stream, totals, N, C, alpha, beta, gamma, smooth, priority, value, coef);
    RU_CHECK_LAUNCH("tversky_eval_kernel");
    return RU_OK;
}

extern "C" size_t ru_topk_workspace_bytes(size_t n) { return n ? TOPK_SLOT_OFF + fl_slots(n) * sizeof(double) : 0; }

extern "C" int ru_topk_select(const float* p, const float* g, size_t n, unsigned long long K, float bg_weight, unsigned* keys, unsigned long long* state,
                              double* out2, void* ws, size_t ws_bytes, ru_stream_t stream) {
    RU_REQUIRE(p && g && keys && state && out2 && ws && n > 0, "ru_topk_select: bad argument");
    RU_REQUIRE(n <= 0xffffffffull, "ru_topk_select: %zu elements, at most 2^32 - 1 (32-bit histogram counts)", n);
    RU_REQUIRE(K >= 1 && K <= n, "ru_topk_select: K = %llu outside 1..%zu", K, n);
    RU_REQUIRE(bg_weight >= 0.f, "ru_topk_select: bg_weight %g is negative", bg_weight);
    RU_REQUIRE(aligned4(p) && aligned4(g) && aligned4(keys) && ((uintptr_t)ws & 7u) == 0 && ((uintptr_t)state & 7u) == 0 && ((uintptr_t)out2 & 7u) == 0,
               "ru_topk_select: misaligned pointer");
    RU_REQUIRE(ws_bytes >= ru_topk_workspace_bytes(n), "ru_topk_select: workspace too small");
    RU_REQUIRE(!overlap(p, keys, n) && !overlap(g, keys, n), "ru_topk_select: keys overlap an input");
    hipStream_t s = (hipStream_t)stream;
    unsigned long long* st = (unsigned long long*)ws;
    unsigned* hist = (unsigned*)((char*)ws + TOPK_HIST_OFF);
    double* slots = (double*)((char*)ws + TOPK_SLOT_OFF);
    if (hipMemsetAsync(ws, 0, TOPK_SLOT_OFF, s) != hipSuccess) return hip_fail(hipGetLastError(), "ru_topk_select: memset");
    const void* const kp[3] = {p, g, keys};
    const Lanes l1 = lanes_for(n, kp);
    const void* const ko[1] = {keys};
    const Lanes l2 = lanes_for(n, ko);
    hipLaunchKernelGGL(topk_key_kernel, dim3(fl_grid(l1, n)), dim3(HC_BLOCK), 0, s, p, g, n, l1, bg_weight, keys, hist);
    RU_CHECK_LAUNCH("topk_key_kernel");
    hipLaunchKernelGGL(topk_scan_kernel, dim3(1), dim3(HC_BLOCK), 0, s, (const unsigned*)hist, 21, K, st);
    RU_CHECK_LAUNCH("topk_scan_kernel");
    hipLaunchKernelGGL((topk_hist_kernel<10, 11>), dim3(fl_grid(l2, n)), dim3(HC_BLOCK), 0, s, (const unsigned*)keys, n, l2,
                       (const unsigned long long*)st, hist + HC_BINS);
    RU_CHECK_LAUNCH("topk_hist_kernel");
    hipLaunchKernelGGL(topk_scan_kernel, dim3(1), dim3(HC_BLOCK), 0, s, (const unsigned*)(hist + HC_BINS), 10, 0ull, st);
    RU_CHECK_LAUNCH("topk_scan_kernel");
    hipLaunchKernelGGL((topk_hist_kernel<0, 10>), dim3(fl_grid(l2, n)), dim3(HC_BLOCK), 0, s, (const unsigned*)keys, n, l2,
                       (const unsigned long long*)st, hist + 2 * HC_BINS);
    RU_CHECK_LAUNCH("topk_hist_kernel");
    hipLaunchKernelGGL(topk_scan_kernel, dim3(1), dim3(HC_BLOCK), 0, s, (const unsigned*)(hist + 2 * HC_BINS), 0, 0ull, st);
    RU_CHECK_LAUNCH("topk_scan_kernel");
    if (int rc = sum_launch(TopkValueOp{keys, st}, n, l2, slots, s, "topk_value_kernel")) return rc;
    hipLaunchKernelGGL(topk_final_kernel, dim3(1), dim3(HC_BLOCK), 0, s, (const double*)slots, (size_t)fl_slots(n), (const unsigned long long*)st, K, out2);
    RU_CHECK_LAUNCH("topk_final_kernel");
    if (hipMemcpyAsync(state, st, HC_STATE * sizeof(unsigned long long), hipMemcpyDeviceToDevice, s) != hipSuccess)
        return hip_fail(hipGetLastError(), "ru_topk_select: copy");
    return RU_OK;
}

extern "C" int ru_topk_grad(const float* p, const float* g, const unsigned* keys, const unsigned long long* state, size_t n, unsigned long long K,
                            float bg_weight, double world, const float* scale, float* dp, ru_stream_t stream) {
    RU_REQUIRE(p && g && keys && state && dp && n > 0, "ru_topk_grad: bad argument");
    RU_REQUIRE(K >= 1 && K <= n && world >= 1.0, "ru_topk_grad: K = %llu outside 1..%zu, or world %g below 1", K, n, world);
    RU_REQUIRE(aligned4(p) && aligned4(g) && aligned4(keys) && aligned4(dp) && ((uintptr_t)state & 7u) == 0, "ru_topk_grad: misaligned pointer");
    RU_REQUIRE(!overlap(p, dp, n) && !overlap(g, dp, n) && !overlap(keys, dp, n), "ru_topk_grad: dp overlaps an input");
    const void* const ptrs[4] = {p, g, keys, dp};
    return stream_launch(TopkGradOp{p, g, keys, bg_weight, state, K, 1.0 / ((double)K * world), scale, dp, 0u, 0.f, 0.f}, n, lanes_for(n, ptrs), (hipStream_t)stream,
                         "topk_grad_kernel");
}
