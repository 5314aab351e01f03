// optim.hip -- the rest of the optimisation recipe beside ru_adam_step (pointwise.hip): the global gradient norm and its clipping
// coefficient, SGD with (Nesterov) momentum, AdamW, an exponential moving average of the weights and an in-place exchange of two buffers.
//
//   torch.nn.utils.clip_grad_norm_   norm over any number of runs, coef = min(1, max_norm / (norm + 1e-6))  -> gradnorm_partial_kernel,
//                                                                                                             gradnorm_finalize_kernel
//   torch.optim.SGD                  d = coef*g + wd*w; buf = first ? d : mom*buf + (1-damp)*d; u = nesterov ? d + mom*buf : buf; w -= lr*u
//   torch.optim.AdamW / Adam         decoupled: w *= 1 - lr*wd first; else adam_kernel's arithmetic on coef*g
//
// All of it is streaming work over runs of the flat parameter / gradient bucket, which start at arbitrary ELEMENT offsets.  One lane
// layout serves every kernel (stream_kernel): a lane owns 4 consecutive floats and moves them as 16 bytes; the elements before the run's
// first 16-byte boundary and those after its last whole quad are taken one float at a time by the first lanes of the grid.  The grid is
// capped at OPT_GRID_CAP workgroups and strides.  The coefficient stays on the device (a float the finalize wrote): nothing here waits
// for the host.  No float atomics: the norm's partial sums are float64, one slot per workgroup, added in slot order by one workgroup.
#include "ru_common.h"
#include "pw_helpers.hpp"

#include <math.h>
#include <stdint.h>

namespace ru {

constexpr int OPT_BLOCK = 256;
constexpr unsigned OPT_GRID_CAP = 2048;          // 256 CUs x 8 workgroups: one resident wave of workgroups, the rest by grid stride

// [0, head) scalar | nq quads from `head` | the remaining (< 4) elements scalar.  The quads are 16-byte aligned for EVERY pointer of the
// call only if all of them sit at the same offset from a 16-byte boundary (runs of buffers laid out alike do); otherwise all is scalar.
struct Lanes { size_t head, nq; };
template <int N>
static inline Lanes lanes_for(size_t n, const void* const (&ptrs)[N]) {
    const uintptr_t a0 = (uintptr_t)ptrs[0] & 15u;
    bool alike = (a0 & 3u) == 0;
    for (int i = 1; i < N; ++i)
        if (ptrs[i] && ((uintptr_t)ptrs[i] & 15u) != a0) alike = false;
    if (!alike) return Lanes{n, 0};
    size_t head = ((16u - a0) & 15u) / 4u;
    if (head > n) head = n;
    return Lanes{head, (n - head) / 4};
}
static inline unsigned opt_grid(const Lanes& l, size_t n) {
    const size_t edge = n - 4 * l.nq;
    return grid1d(l.nq > edge ? l.nq : edge, OPT_BLOCK, OPT_GRID_CAP);
}

__device__ __forceinline__ float mul_rn(float a, float b) {        // a product that is rounded on its own, never folded into an fma
#pragma clang fp contract(off)
    return a * b;
}

// Op: `load(i)` fetches elements [i, i + 4) of every operand through 16-byte accesses, `finish(i, q)` updates and stores them; `one(i)` does
// element i; both run the same scalar arithmetic.  (Keeping the loads of two quads in flight per lane measured no faster: every pass on the
// network's runs sits within a few microseconds of its three launches' floor, tools/optim_time.py.)
template <class Op>
__global__ __launch_bounds__(OPT_BLOCK) void stream_kernel(Op op, size_t n, size_t head, size_t nq) {
    const size_t t = (size_t)blockIdx.x * OPT_BLOCK + threadIdx.x, T = (size_t)gridDim.x * OPT_BLOCK;
    for (size_t q = t; q < nq; q += T) {
        auto a = op.load(head + 4 * q);
        op.finish(head + 4 * q, a);
    }
    const size_t edge = n - 4 * nq;                                  // head + tail: at most 6 elements when the quads exist
    for (size_t e = t; e < edge; e += T) op.one(e < head ? e : e + 4 * nq);
}
template <class Op>
static int stream_launch(const Op& op, size_t n, const Lanes& l, hipStream_t s, const char* what) {
    hipLaunchKernelGGL(stream_kernel<Op>, dim3(opt_grid(l, n)), dim3(OPT_BLOCK), 0, s, op, n, l.head, l.nq);
    RU_CHECK_LAUNCH(what);
    return RU_OK;
}

__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ void st4(float* p, const float4& v) { *reinterpret_cast<float4*>(p) = v; }

// ------------------------------------------------------------------ global L2 norm, float64
__global__ __launch_bounds__(OPT_BLOCK) void gradnorm_partial_kernel(const float* __restrict__ g, size_t n, size_t head, size_t nq, double* __restrict__ slots) {
    __shared__ double buf[4];
    const size_t t = (size_t)blockIdx.x * OPT_BLOCK + threadIdx.x, T = (size_t)gridDim.x * OPT_BLOCK;
    double acc = 0.0;
    auto sq = [](const float4& v) {
        const double x = v.x, y = v.y, z = v.z, w = v.w;
        return (x * x + y * y) + (z * z + w * w);
    };
    for (size_t q = t; q < nq; q += T) acc += sq(ld4(g + head + 4 * q));
    const size_t edge = n - 4 * nq;
    for (size_t e = t; e < edge; e += T) {
        const double x = g[e < head ? e : e + 4 * nq];
        acc += x * x;
    }
    const double tot = block_sum_d(acc, buf);
    if (threadIdx.x == 0) slots[blockIdx.x] = tot;                   // every workgroup of the grid writes its own slot, zeros included
}

// one workgroup: lane t adds its contiguous share of the slots in index order, lane 0 then adds the 256 shares in lane order
__global__ __launch_bounds__(OPT_BLOCK) void gradnorm_finalize_kernel(const double* __restrict__ slots, size_t n_slots, double max_norm,
                                                                      double* __restrict__ norm_out, float* __restrict__ coef_out) {
    __shared__ double part[OPT_BLOCK];
    const size_t per = (n_slots + OPT_BLOCK - 1) / OPT_BLOCK;
    const size_t lo = per * threadIdx.x, hi = lo + per < n_slots ? lo + per : n_slots;
    double acc = 0.0;
    for (size_t i = lo; i < hi; ++i) acc += slots[i];
    part[threadIdx.x] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double tot = 0.0;
        for (int i = 0; i < OPT_BLOCK; ++i) tot += part[i];
        const double norm = sqrt(tot);
        const double c = max_norm / (norm + 1e-6);                   // clip_grad_norm_: clamp(max_norm / (norm + 1e-6), max=1.0); NaN stays NaN
        *norm_out = norm;
        *coef_out = (float)(c > 1.0 ? 1.0 : c);
    }
}

// ------------------------------------------------------------------ g *= *coef
struct ScaleOp {
    float* g; const float* coef;
    __device__ __forceinline__ void one(size_t i) const { g[i] = mul_rn(*coef, g[i]); }
    __device__ __forceinline__ float4 load(size_t i) const { return ld4(g + i); }
    __device__ __forceinline__ void finish(size_t i, float4& v) const {
        const float c = *coef;
        v.x = mul_rn(c, v.x); v.y = mul_rn(c, v.y); v.z = mul_rn(c, v.z); v.w = mul_rn(c, v.w);
        st4(g + i, v);
    }
};

// ------------------------------------------------------------------ torch.optim.SGD
struct SgdOp {
    float* w; const float* g; float* buf; const float* coef;
    float lr, momentum, undamp, wd;                                  // undamp = 1 - dampening
    int nesterov, first;
    __device__ __forceinline__ void upd(float& wi, float gi, float& bi, bool has_c, float c) const {
        // every product-sum is spelled out as one fma, so that the 16-byte lanes and the one-float lanes round alike whatever the compiler would fuse
        const float gc = has_c ? mul_rn(c, gi) : gi;                // rounded on its own: a coefficient of exactly 1 changes no bit below
        const float d = fmaf(wd, wi, gc);
        float u = d;
        if (buf) {
            bi = first ? d : fmaf(momentum, bi, mul_rn(undamp, d));
            u = nesterov ? fmaf(momentum, bi, d) : bi;
        }
        wi = fmaf(-lr, u, wi);
    }
    __device__ __forceinline__ void one(size_t i) const {
        float wi = w[i], bi = (buf && !first) ? buf[i] : 0.f;
        upd(wi, g[i], bi, coef != nullptr, coef ? *coef : 1.f);
        w[i] = wi;
        if (buf) buf[i] = bi;
    }
    struct Q { float4 w, g, b; };
    __device__ __forceinline__ Q load(size_t i) const { return Q{ld4(w + i), ld4(g + i), (buf && !first) ? ld4(buf + i) : make_float4(0.f, 0.f, 0.f, 0.f)}; }
    __device__ __forceinline__ void finish(size_t i, Q& q) const {
        const bool has_c = coef != nullptr;
        const float c = has_c ? *coef : 1.f;
        float4& wv = q.w;
        const float4& gv = q.g;
        float4& bv = q.b;
        upd(wv.x, gv.x, bv.x, has_c, c); upd(wv.y, gv.y, bv.y, has_c, c); upd(wv.z, gv.z, bv.z, has_c, c); upd(wv.w, gv.w, bv.w, has_c, c);
        st4(w + i, wv);
        if (buf) st4(buf + i, bv);
    }
};

// ------------------------------------------------------------------ torch.optim.AdamW (DEC) / adam_kernel's arithmetic on coef * g (!DEC)
template <bool AMS, bool DEC>
struct AdamWOp {
    float* w; const float* g; float* m; float* v; float* vmax; const float* coef;
    float step_size, b1, b2, eps, wd, bc2_sqrt, decay;              // decay = 1 - lr * wd (DEC)
    __device__ __forceinline__ void upd(float& wr, float gr, float& mr, float& vr, float& vmr, bool has_c, float c) const {
        const float gc = has_c ? mul_rn(c, gr) : gr;
        const float wi = DEC ? mul_rn(wr, decay) : wr;              // param.mul_(1 - lr * weight_decay)
        // adam_kernel's lines with the fusions its build makes spelled out (tests/test_optim_recipe.py holds the two to equal bytes), so that
        // the 16-byte lanes and the one-float lanes round alike
        const float gi = DEC ? gc : fmaf(wd, wi, gc);               // g[i] + wd * wi
        const float mi = fmaf(gi - mr, 1.f - b1, mr);               // m[i] + (gi - m[i]) * (1.f - b1): exp_avg.lerp_(grad, 1 - beta1)
        const float vi = fmaf(vr, b2, mul_rn(mul_rn(1.f - b2, gi), gi));   // v[i] * b2 + (1.f - b2) * gi * gi: exp_avg_sq.mul_(beta2).addcmul_(grad, grad, 1 - beta2)
        float vm = vi;
        if (AMS) { vm = fmaxf(vmr, vi); vmr = vm; }
        const float denom = sqrtf(vm) / bc2_sqrt + eps;
        mr = mi; vr = vi;
        wr = fmaf(-step_size, mi / denom, wi);                      // wi - step_size * (mi / denom)
    }
    __device__ __forceinline__ void one(size_t i) const {
        float wi = w[i], mi = m[i], vi = v[i], vm = AMS ? vmax[i] : 0.f;
        upd(wi, g[i], mi, vi, vm, coef != nullptr, coef ? *coef : 1.f);
        w[i] = wi; m[i] = mi; v[i] = vi;
        if (AMS) vmax[i] = vm;
    }
    struct Q { float4 w, g, m, v, x; };
    __device__ __forceinline__ Q load(size_t i) const { return Q{ld4(w + i), ld4(g + i), ld4(m + i), ld4(v + i), AMS ? ld4(vmax + i) : make_float4(0.f, 0.f, 0.f, 0.f)}; }
    __device__ __forceinline__ void finish(size_t i, Q& q) const {
        const bool has_c = coef != nullptr;
        const float c = has_c ? *coef : 1.f;
        float4 &wv = q.w, &mv = q.m, &vv = q.v, &xv = q.x;
        const float4& gv = q.g;
        upd(wv.x, gv.x, mv.x, vv.x, xv.x, has_c, c); upd(wv.y, gv.y, mv.y, vv.y, xv.y, has_c, c);
        upd(wv.z, gv.z, mv.z, vv.z, xv.z, has_c, c); upd(wv.w, gv.w, mv.w, vv.w, xv.w, has_c, c);
        st4(w + i, wv); st4(m + i, mv); st4(v + i, vv);
        if (AMS) st4(vmax + i, xv);
    }
};

// ------------------------------------------------------------------ ema = fmaf(decay, ema, (1 - decay) * w)
struct EmaOp {
    float* ema; const float* w; float decay, rest;
    __device__ __forceinline__ float upd(float e, float x) const { return fmaf(decay, e, mul_rn(rest, x)); }
    __device__ __forceinline__ void one(size_t i) const { ema[i] = upd(ema[i], w[i]); }
    struct Q { float4 e, x; };
    __device__ __forceinline__ Q load(size_t i) const { return Q{ld4(ema + i), ld4(w + i)}; }
    __device__ __forceinline__ void finish(size_t i, Q& q) const {
        float4& e = q.e;
        const float4& x = q.x;
        e.x = upd(e.x, x.x); e.y = upd(e.y, x.y); e.z = upd(e.z, x.z); e.w = upd(e.w, x.w);
        st4(ema + i, e);
    }
};

struct SwapOp {
    float* a; float* b;
    __device__ __forceinline__ void one(size_t i) const { const float x = a[i]; a[i] = b[i]; b[i] = x; }
    struct Q { float4 x, y; };
    __device__ __forceinline__ Q load(size_t i) const { return Q{ld4(a + i), ld4(b + i)}; }
    __device__ __forceinline__ void finish(size_t i, Q& q) const { st4(a + i, q.y); st4(b + i, q.x); }
};

template <bool AMS, bool DEC>
static int adamw_launch(float* w, const float* g, float* m, float* v, float* vmax, const float* coef, size_t n, float lr, float b1, float b2, float eps,
                        float wd, int step, const Lanes& l, hipStream_t s) {
    const double bc1 = 1.0 - pow((double)b1, (double)step), bc2 = 1.0 - pow((double)b2, (double)step);       // as adam_launch
    AdamWOp<AMS, DEC> op{w, g, m, v, vmax, coef, (float)((double)lr / bc1), b1, b2, eps, wd, (float)sqrt(bc2), (float)(1.0 - (double)lr * (double)wd)};
    return stream_launch(op, n, l, s, "adamw_kernel");
}

static inline bool overlap(const void* a, const void* b, size_t n) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + 4 * n && y < x + 4 * n;
}

}  // namespace ru

using namespace ru;

extern "C" size_t ru_gradnorm_slots(size_t n) {
    if (n == 0) return 0;
    return grid1d((n + 3) / 4 + 3, OPT_BLOCK, OPT_GRID_CAP);         // an upper bound of the grid for every alignment of the run
}

extern "C" size_t ru_gradnorm_workspace_bytes(size_t n_total, size_t n_runs) {
    // at least the sum of ru_gradnorm_slots over any split of n_total elements into n_runs runs: a run of n elements takes
    // ceil((ceil(n / 4) + 3) / 256) <= (n / 4 + 1) / 256 + 2 slots
    return sizeof(double) * ((n_total / 4 + n_runs) / OPT_BLOCK + 2 * n_runs + 1);
}

extern "C" int ru_gradnorm_partial(const float* g, size_t n, size_t first_slot, double* ws, size_t ws_bytes, ru_stream_t stream) {
    RU_REQUIRE(g && ws, "ru_gradnorm_partial: null argument");
    RU_REQUIRE(((uintptr_t)g & 3u) == 0 && ((uintptr_t)ws & 7u) == 0, "ru_gradnorm_partial: misaligned pointer");
    if (n == 0) return RU_OK;
    const void* const ptrs[1] = {g};
    const Lanes l = lanes_for(n, ptrs);
    const unsigned grid = (unsigned)ru_gradnorm_slots(n);             // the slot count is a function of n alone: lanes past the work write 0
    RU_REQUIRE((first_slot + grid) * sizeof(double) <= ws_bytes, "ru_gradnorm_partial: workspace too small for slots [%zu, %zu)", first_slot, first_slot + grid);
    hipLaunchKernelGGL(gradnorm_partial_kernel, dim3(grid), dim3(OPT_BLOCK), 0, (hipStream_t)stream, g, n, l.head, l.nq, ws + first_slot);
    RU_CHECK_LAUNCH("gradnorm_partial_kernel");
    return RU_OK;
}

extern "C" int ru_gradnorm_finalize(const double* ws, size_t n_slots, double max_norm, double* norm_out, float* coef_out, ru_stream_t stream) {
    RU_REQUIRE(ws && norm_out && coef_out, "ru_gradnorm_finalize: null argument");
    RU_REQUIRE(!(max_norm < 0.0), "ru_gradnorm_finalize: max_norm must not be negative");
    hipLaunchKernelGGL(gradnorm_finalize_kernel, dim3(1), dim3(OPT_BLOCK), 0, (hipStream_t)stream, ws, n_slots, max_norm, norm_out, coef_out);
    RU_CHECK_LAUNCH("gradnorm_finalize_kernel");
    return RU_OK;
}

extern "C" int ru_scale_by(float* g, size_t n, const float* coef, ru_stream_t stream) {
    RU_REQUIRE(g && coef, "ru_scale_by: null argument");
    RU_REQUIRE(((uintptr_t)g & 3u) == 0, "ru_scale_by: misaligned pointer");
    if (n == 0) return RU_OK;
    const void* const ptrs[1] = {g};
    return stream_launch(ScaleOp{g, coef}, n, lanes_for(n, ptrs), (hipStream_t)stream, "scale_kernel");
}

extern "C" int ru_sgd_step(float* w, const float* g, float* buf_or_null, size_t n, float lr, float momentum, float dampening, float weight_decay,
                           int nesterov, int first, const float* coef_or_null, ru_stream_t stream) {
    RU_REQUIRE(w && g, "ru_sgd_step: null argument");
    RU_REQUIRE((momentum != 0.f) == (buf_or_null != nullptr), "ru_sgd_step: a momentum buffer goes with momentum != 0, and only with it");
    RU_REQUIRE(!nesterov || (momentum > 0.f && dampening == 0.f), "ru_sgd_step: Nesterov momentum requires a momentum and zero dampening");
    RU_REQUIRE((((uintptr_t)w | (uintptr_t)g | (uintptr_t)buf_or_null) & 3u) == 0, "ru_sgd_step: misaligned pointer");
    if (n == 0) return RU_OK;
    RU_REQUIRE(!overlap(w, g, n) && (!buf_or_null || (!overlap(w, buf_or_null, n) && !overlap(g, buf_or_null, n))), "ru_sgd_step: buffers overlap");
    const void* const ptrs[3] = {w, g, buf_or_null};
    SgdOp op{w, g, buf_or_null, coef_or_null, lr, momentum, 1.f - dampening, weight_decay, nesterov != 0, first != 0};
    return stream_launch(op, n, lanes_for(n, ptrs), (hipStream_t)stream, "sgd_kernel");
}

extern "C" int ru_adamw_step(float* w, const float* g, float* m, float* v, float* vmax_or_null, size_t n, float lr, float beta1, float beta2, float eps,
                             float weight_decay, int decoupled, int step, const float* coef_or_null, ru_stream_t stream) {
    RU_REQUIRE(w && g && m && v, "ru_adamw_step: null argument");
    RU_REQUIRE(step >= 1, "ru_adamw_step: step is 1-based");
    RU_REQUIRE((((uintptr_t)w | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v | (uintptr_t)vmax_or_null) & 3u) == 0, "ru_adamw_step: misaligned pointer");
    if (n == 0) return RU_OK;
    const void* const ptrs[5] = {w, g, m, v, vmax_or_null};
    for (int i = 0; i < 5; ++i)
        for (int j = i + 1; j < 5; ++j) RU_REQUIRE(!ptrs[i] || !ptrs[j] || !overlap(ptrs[i], ptrs[j], n), "ru_adamw_step: buffers overlap");
    const Lanes l = lanes_for(n, ptrs);
    hipStream_t s = (hipStream_t)stream;
    if (vmax_or_null) return decoupled ? adamw_launch<true, true>(w, g, m, v, vmax_or_null, coef_or_null, n, lr, beta1, beta2, eps, weight_decay, step, l, s)
                                       : adamw_launch<true, false>(w, g, m, v, vmax_or_null, coef_or_null, n, lr, beta1, beta2, eps, weight_decay, step, l, s);
    return decoupled ? adamw_launch<false, true>(w, g, m, v, nullptr, coef_or_null, n, lr, beta1, beta2, eps, weight_decay, step, l, s)
                     : adamw_launch<false, false>(w, g, m, v, nullptr, coef_or_null, n, lr, beta1, beta2, eps, weight_decay, step, l, s);
}

extern "C" int ru_ema_update(float* ema, const float* w, size_t n, float decay, ru_stream_t stream) {
    RU_REQUIRE(ema && w, "ru_ema_update: null argument");
    RU_REQUIRE(decay >= 0.f && decay <= 1.f, "ru_ema_update: decay must lie in [0, 1]");
    RU_REQUIRE((((uintptr_t)ema | (uintptr_t)w) & 3u) == 0, "ru_ema_update: misaligned pointer");
    if (n == 0) return RU_OK;
    RU_REQUIRE(!overlap(ema, w, n), "ru_ema_update: buffers overlap");
    const void* const ptrs[2] = {ema, w};
    return stream_launch(EmaOp{ema, w, decay, 1.f - decay}, n, lanes_for(n, ptrs), (hipStream_t)stream, "ema_kernel");
}

extern "C" int ru_swap_f32(float* a, float* b, size_t n, ru_stream_t stream) {
    RU_REQUIRE(a && b, "ru_swap_f32: null argument");
    RU_REQUIRE((((uintptr_t)a | (uintptr_t)b) & 3u) == 0, "ru_swap_f32: misaligned pointer");
    if (n == 0) return RU_OK;
    RU_REQUIRE(!overlap(a, b, n), "ru_swap_f32: buffers overlap");
    const void* const ptrs[2] = {a, b};
    return stream_launch(SwapOp{a, b}, n, lanes_for(n, ptrs), (hipStream_t)stream, "swap_kernel");
}
