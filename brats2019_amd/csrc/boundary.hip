// boundary.hip -- criteria that know how far a voxel is from the boundary of a mask: the boundary loss (Kervadec et al.) and the Hausdorff
// distance-transform loss (Karimi & Salehi, in MONAI's HausdorffDTLoss form), both on exact Euclidean distance maps made on the device.
//
//   map      ru_signed_sqdist: per (sample, channel) the mask M = x > 0.5f and s_M as int32, + the squared distance to the nearest voxel of M
//            outside M, - the squared distance to the nearest voxel not in M inside it, 0 everywhere when M is empty or the whole grid.
//              W pass  sd_pass_w_kernel thresholds and ballots each row as hd_pass_w_kernel does (metrics.hip), counts the voxels of M and
//                      hands the row's words to edt_row_pass (the transform towards M, t = 0) and their complement, masked to W in the
//                      last word, to a second edt_row_pass (the transform towards not-M, t = 1): the pair layout f = [items][2][V];
//              H pass  edt_line_kernel<false>, as the scorers run it;
//              D pass  edt_line_kernel<true, SdWrite>: every voxel is a query in exactly one of the two transforms (outside voxels in
//                      t = 0, inside voxels in t = 1), so each output voxel is written once, with its sign, and without atomics.  An
//                      empty or full channel is decided from the count the W pass left on the device: its t = 0 blocks write zeros.
//   losses   phi = F outside, -(F - 1) inside, 0 where s = 0, with F = sqrt(|s|) (Kervadec's one_hot2dist); boundary = sum p phi_G;
//            hddt = sum (p - g)^2 (F_P^alpha + F_G^alpha).  phi and F^alpha are formed from the int32 value where they are used: no float
//            map is stored.  The passes are flat streaming work in the lane layout of flat_lanes.hpp: the sums are ops of its sum_kernel (one
//            float64 slot per workgroup, added in a fixed order by one workgroup), the gradients ops of its stream_kernel.  No float
//            atomics, nothing waits for the host, the same bytes give the same bytes.
#include "ru_common.h"
#include "edt_exact.hpp"
#include "flat_lanes.hpp"

#include <math.h>

namespace ru {
namespace {

// ------------------------------------------------------------------ the map
constexpr size_t SD_COUNT_ALIGN = 256;           // the counts sit in front of f, f starts on a 256-byte boundary
inline size_t sd_count_bytes(int items) { return ((size_t)items * sizeof(u64) + SD_COUNT_ALIGN - 1) / SD_COUNT_ALIGN * SD_COUNT_ALIGN; }

// grid (D, items), 256 threads: wave q takes the rows h = q, q + 4, ... of plane d.  f = [items][2][V]: transform 0 = to M, 1 = to not-M.
// count[item] += |M|.
__global__ __launch_bounds__(256) void sd_pass_w_kernel(const float* __restrict__ x, int D, int H, int W, unsigned* __restrict__ f,
                                                        u64* __restrict__ count) {
    const int d = blockIdx.x, item = blockIdx.y;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const size_t V = (size_t)D * H * W;
    const float* __restrict__ xi = x + (size_t)item * V;
    unsigned* __restrict__ fm = f + ((size_t)item * 2) * V;
    unsigned* __restrict__ fc = fm + V;
    u64 cm = 0;
    for (int h = wave; h < H; h += 4) {
        const size_t row = ((size_t)d * H + h) * W;
        u64 m[MAX_WORDS], c[MAX_WORDS];
#pragma unroll
        for (int k = 0; k < MAX_WORDS; ++k) {
            const int w = k * 64 + lane;
            const bool in = w < W;
            m[k] = __ballot(in && xi[row + w] > 0.5f);
            c[k] = __ballot(in) & ~m[k];                            // the complement within the row: bits at or above W stay zero
            cm += __popcll(m[k]);
        }
        edt_row_pass(m, W, fm + row);
        edt_row_pass(c, W, fc + row);
    }
    if (lane == 0 && cm) atomicAdd(count + item, cm);
}

// The D pass's query.  t = 0 (distances to M) is asked at the voxels outside M and written +, t = 1 (distances to not-M) at the voxels
// inside and written -.  consume() gets no coordinates: a thread's queries of one step share (h, w) and are consumed in the order they
// were asked, so the up to four pending d (9 bits each) wait in a 64-bit queue, 16 bits apart.
struct SdWrite {
    const float* x;
    int* out;
    const u64* count;
    int t, H, W, h, w, npend;
    bool flat;                                                       // the channel is empty or full: zeros
    u64 pend;
    __device__ void begin(const MaskGeom& s, int item, int tt) {
        x += (size_t)item * s.V;
        out += (size_t)item * s.V;
        const u64 n = count[item];
        flat = n == 0 || n == (u64)s.V;
        t = tt;
        H = s.H;
        W = s.W;
        pend = 0;
        npend = 0;
    }
    __device__ bool query(const MaskGeom& s, int d, int hh, int ww) {
        const size_t v = ((size_t)d * s.H + hh) * s.W + ww;
        if (flat) {
            if (t == 0) out[v] = 0;
            return false;
        }
        if ((x[v] > 0.5f) != (t == 1)) return false;
        h = hh;
        w = ww;
        pend |= (u64)d << (16 * npend++);                            // behind the pending ones
        return true;
    }
    __device__ void consume(unsigned sq) {
        const int d = (int)(pend & 0xffffu);
        pend >>= 16;
        --npend;
        out[((size_t)d * H + h) * W + w] = t ? -(int)sq : (int)sq;
    }
    __device__ void finish() {}
};

// ------------------------------------------------------------------ the streaming passes

// Kervadec's level set from the stored integer: F outside, -(F - 1) inside, 0 on a channel without a boundary.  |s| < 2^20 is exact in
// float32 and sqrtf is correctly rounded.
__device__ __forceinline__ float bd_phi(int s) {
    if (s == 0) return 0.f;
    const float F = sqrtf((float)(s < 0 ? -s : s));
    return s > 0 ? F : 1.f - F;
}

// F_P^alpha + F_G^alpha.  MODE 1: alpha == 1, 2: alpha == 2 (the integers themselves, their sum exact), 3: any alpha > 0, half = alpha / 2
template <int MODE>
__device__ __forceinline__ float hd_weight(int sp, int sg, float half) {
    const int a = sp < 0 ? -sp : sp, b = sg < 0 ? -sg : sg;
    if (MODE == 2) return (float)(a + b);
    if (MODE == 1) return sqrtf((float)a) + sqrtf((float)b);
    return (a ? powf((float)a, half) : 0.f) + (b ? powf((float)b, half) : 0.f);
}
inline int hd_mode(float alpha) { return alpha == 1.f ? 1 : alpha == 2.f ? 2 : 3; }

// the term of the sum in float64 from float32 operands: p - g is exact there, the weight carries the float32 roundings
template <int MODE>
__device__ __forceinline__ double hd_term(float p, float g, int sp, int sg, float half) {
    const double d = (double)p - (double)g;
    return d * d * (double)hd_weight<MODE>(sp, sg, half);
}
template <int MODE>
__device__ __forceinline__ float hd_deriv(float p, float g, int sp, int sg, float half) {
    return 2.f * (p - g) * hd_weight<MODE>(sp, sg, half);
}

struct BoundarySumOp {
    const float* p; const int* s;
    __device__ __forceinline__ double quad(size_t i) const {
        const float4 pv = ld4(p + i);
        const int4 sv = ld4i(s + i);
        return ((double)pv.x * (double)bd_phi(sv.x) + (double)pv.y * (double)bd_phi(sv.y)) +
               ((double)pv.z * (double)bd_phi(sv.z) + (double)pv.w * (double)bd_phi(sv.w));
    }
    __device__ __forceinline__ double one(size_t i) const { return (double)p[i] * (double)bd_phi(s[i]); }
};

// dp = phi * mult * (*scale if given)
struct BoundaryGradOp {
    const int* s; float m; const float* scale; float* dp;           // m = mult, from begin() on times *scale
    __device__ __forceinline__ void begin() { if (scale) m *= *scale; }
    __device__ __forceinline__ void one(size_t i) const { dp[i] = m * bd_phi(s[i]); }
    __device__ __forceinline__ int4 load(size_t i) const { return ld4i(s + i); }
    __device__ __forceinline__ void finish(size_t i, const int4& sv) const {
        st4(dp + i, make_float4(m * bd_phi(sv.x), m * bd_phi(sv.y), m * bd_phi(sv.z), m * bd_phi(sv.w)));
    }
};

template <int MODE>
struct HddtSumOp {
    const float* p; const float* g; const int* sp; const int* sg; float half;
    __device__ __forceinline__ double quad(size_t i) const {
        const float4 pv = ld4(p + i), gv = ld4(g + i);
        const int4 a = ld4i(sp + i), b = ld4i(sg + i);
        return (hd_term<MODE>(pv.x, gv.x, a.x, b.x, half) + hd_term<MODE>(pv.y, gv.y, a.y, b.y, half)) +
               (hd_term<MODE>(pv.z, gv.z, a.z, b.z, half) + hd_term<MODE>(pv.w, gv.w, a.w, b.w, half));
    }
    __device__ __forceinline__ double one(size_t i) const { return hd_term<MODE>(p[i], g[i], sp[i], sg[i], half); }
};

// dp = 2 (p - g) (F_P^alpha + F_G^alpha) * mult * (*scale if given)
template <int MODE>
struct HddtGradOp {
    const float* p; const float* g; const int* sp; const int* sg; float half, m; const float* scale; float* dp;     // m as BoundaryGradOp's
    __device__ __forceinline__ void begin() { if (scale) m *= *scale; }
    __device__ __forceinline__ void one(size_t i) const { dp[i] = m * hd_deriv<MODE>(p[i], g[i], sp[i], sg[i], half); }
    struct Q { float4 p, g; int4 a, b; };
    __device__ __forceinline__ Q load(size_t i) const { return Q{ld4(p + i), ld4(g + i), ld4i(sp + i), ld4i(sg + i)}; }
    __device__ __forceinline__ void finish(size_t i, const Q& q) const {
        st4(dp + i, make_float4(m * hd_deriv<MODE>(q.p.x, q.g.x, q.a.x, q.b.x, half), m * hd_deriv<MODE>(q.p.y, q.g.y, q.a.y, q.b.y, half),
                                m * hd_deriv<MODE>(q.p.z, q.g.z, q.a.z, q.b.z, half), m * hd_deriv<MODE>(q.p.w, q.g.w, q.a.w, q.b.w, half)));
    }
};

inline bool alpha_ok(float alpha) { return alpha > 0.f && alpha <= 3.4e38f; }      // NaN fails the first comparison

}  // namespace
}  // namespace ru

using namespace ru;

extern "C" size_t ru_signed_sqdist_workspace_bytes(int items, int D, int H, int W) {
    if (items <= 0 || D <= 0 || H <= 0 || W <= 0) return 0;
    return sd_count_bytes(items) + (size_t)items * 2 * ((size_t)D * H * W) * sizeof(unsigned);
}

extern "C" int ru_signed_sqdist(const float* x, int items, int D, int H, int W, int* out, void* ws, size_t ws_bytes, ru_stream_t stream) {
    RU_REQUIRE(x && out && items > 0, "ru_signed_sqdist: bad argument");
    RU_REQUIRE(D > 0 && H > 0 && W > 0 && D <= MAX_EXTENT && H <= MAX_EXTENT && W <= MAX_EXTENT,
               "ru_signed_sqdist: extents %d x %d x %d: every axis must be in [1, %d]", D, H, W, MAX_EXTENT);
    RU_REQUIRE((long long)items * 2 <= 65535, "ru_signed_sqdist: %d channels, at most 32767 in one call", items);
    RU_REQUIRE(aligned4(x) && aligned4(out), "ru_signed_sqdist: misaligned pointer");
    const size_t V = (size_t)D * H * W;
    RU_REQUIRE(!overlap(x, out, (size_t)items * V), "ru_signed_sqdist: out overlaps the input");
    RU_REQUIRE(ws && ((uintptr_t)ws & 7u) == 0 && ws_bytes >= ru_signed_sqdist_workspace_bytes(items, D, H, W), "ru_signed_sqdist: workspace too small");
    hipStream_t s = (hipStream_t)stream;
    u64* count = (u64*)ws;
    unsigned* f = (unsigned*)((char*)ws + sd_count_bytes(items));
    hipLaunchKernelGGL((zero2_kernel<u64, u64>), dim3(cdiv(items, 256)), dim3(256), 0, s, count, (size_t)items, (u64*)nullptr, (size_t)0);
    RU_CHECK_LAUNCH("zero2_kernel");
    hipLaunchKernelGGL(sd_pass_w_kernel, dim3(D, items), dim3(256), 0, s, x, D, H, W, f, count);
    RU_CHECK_LAUNCH("sd_pass_w_kernel");
    const SdWrite q = {x, out, count, 0, 0, 0, 0, 0, 0, false, 0ull};
    return edt_line_passes(f, mask_geom(D, H, W), items, q, s);
}

extern "C" size_t ru_boundary_workspace_bytes(size_t n) { return n ? fl_slots(n) * sizeof(double) : 0; }

extern "C" int ru_boundary_sum(const float* p, const int* s_g, size_t n, double* sum_out, void* ws, size_t ws_bytes, ru_stream_t stream) {
    RU_REQUIRE(p && s_g && sum_out && ws && n > 0, "ru_boundary_sum: bad argument");
    RU_REQUIRE(aligned4(p) && aligned4(s_g) && ((uintptr_t)ws & 7u) == 0 && ((uintptr_t)sum_out & 7u) == 0, "ru_boundary_sum: misaligned pointer");
    RU_REQUIRE(ws_bytes >= ru_boundary_workspace_bytes(n), "ru_boundary_sum: workspace too small");
    const void* const ptrs[2] = {p, s_g};
    return total_launch(BoundarySumOp{p, s_g}, n, lanes_for(n, ptrs), (double*)ws, sum_out, (hipStream_t)stream, "boundary_sum_kernel");
}

extern "C" int ru_boundary_grad(const int* s_g, size_t n, float coef, const float* scale, float* dp, ru_stream_t stream) {
    RU_REQUIRE(s_g && dp && n > 0, "ru_boundary_grad: bad argument");
    RU_REQUIRE(coef == coef && fabsf(coef) <= 3.4e38f, "ru_boundary_grad: coef %g is not finite", coef);
    RU_REQUIRE(aligned4(s_g) && aligned4(dp), "ru_boundary_grad: misaligned pointer");
    RU_REQUIRE(!overlap(s_g, dp, n), "ru_boundary_grad: dp overlaps the map");
    const void* const ptrs[2] = {s_g, dp};
    return stream_launch(BoundaryGradOp{s_g, coef, scale, dp}, n, lanes_for(n, ptrs), (hipStream_t)stream, "boundary_grad_kernel");
}

extern "C" int ru_hddt_sum(const float* p, const float* g, const int* s_p, const int* s_g, size_t n, float alpha, double* sum_out, void* ws,
                           size_t ws_bytes, ru_stream_t stream) {
    RU_REQUIRE(p && g && s_p && s_g && sum_out && ws && n > 0, "ru_hddt_sum: bad argument");
    RU_REQUIRE(alpha_ok(alpha), "ru_hddt_sum: alpha %g must be positive and finite", alpha);
    RU_REQUIRE(aligned4(p) && aligned4(g) && aligned4(s_p) && aligned4(s_g) && ((uintptr_t)ws & 7u) == 0 && ((uintptr_t)sum_out & 7u) == 0,
               "ru_hddt_sum: misaligned pointer");
    RU_REQUIRE(ws_bytes >= ru_boundary_workspace_bytes(n), "ru_hddt_sum: workspace too small");
    hipStream_t s = (hipStream_t)stream;
    const void* const ptrs[4] = {p, g, s_p, s_g};
    const Lanes l = lanes_for(n, ptrs);
    const float half = 0.5f * alpha;
    return with_mode<1, 3>(hd_mode(alpha), [&](auto mode) {
        return total_launch(HddtSumOp<mode()>{p, g, s_p, s_g, half}, n, l, (double*)ws, sum_out, s, "hddt_sum_kernel");
    });
}

extern "C" int ru_hddt_grad(const float* p, const float* g, const int* s_p, const int* s_g, size_t n, float alpha, float coef, const float* scale,
                            float* dp, ru_stream_t stream) {
    RU_REQUIRE(p && g && s_p && s_g && dp && n > 0, "ru_hddt_grad: bad argument");
    RU_REQUIRE(alpha_ok(alpha), "ru_hddt_grad: alpha %g must be positive and finite", alpha);
    RU_REQUIRE(coef == coef && fabsf(coef) <= 3.4e38f, "ru_hddt_grad: coef %g is not finite", coef);
    RU_REQUIRE(aligned4(p) && aligned4(g) && aligned4(s_p) && aligned4(s_g) && aligned4(dp), "ru_hddt_grad: misaligned pointer");
    RU_REQUIRE(!overlap(p, dp, n) && !overlap(g, dp, n) && !overlap(s_p, dp, n) && !overlap(s_g, dp, n), "ru_hddt_grad: dp overlaps an input");
    hipStream_t s = (hipStream_t)stream;
    const void* const ptrs[5] = {p, g, s_p, s_g, dp};
    const Lanes l = lanes_for(n, ptrs);
    const float half = 0.5f * alpha;
    return with_mode<1, 3>(hd_mode(alpha), [&](auto mode) {
        return stream_launch(HddtGradOp<mode()>{p, g, s_p, s_g, half, coef, scale, dp}, n, l, s, "hddt_grad_kernel");
    });
}
