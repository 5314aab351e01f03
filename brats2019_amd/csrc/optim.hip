// optim.hip -- the rest of the optimisation recipe beside ru_adam_step (pointwise.hip): the global gradient norm and its clipping
// coefficient, SGD with (Nesterov) momentum, AdamW, an exponential moving average of the weights and an in-place exchange of two buffers.
//
//   torch.nn.utils.clip_grad_norm_   norm over any number of runs, coef = min(1, max_norm / (norm + 1e-6))  -> SquareOp, gradnorm_finalize_kernel
//   torch.optim.SGD                  d = coef*g + wd*w; buf = first ? d : mom*buf + (1-damp)*d; u = nesterov ? d + mom*buf : buf; w -= lr*u
//   torch.optim.AdamW / Adam         decoupled: w *= 1 - lr*wd first; else adam_kernel's arithmetic on coef*g
//
// All of it is streaming work over runs of the flat parameter / gradient bucket, which start at arbitrary ELEMENT offsets, in the lane
// layout of flat_lanes.hpp: the update kernels are ops of its stream_kernel, the norm's partial sums an op of its sum_kernel.  The coefficient
// stays on the device (a float the finalize wrote): nothing here waits for the host.  No float atomics: the norm's partial sums are float64,
// one slot per workgroup, added in slot order by one workgroup.
#include "ru_common.h"
#include "pw_helpers.hpp"
#include "flat_lanes.hpp"

#include <math.h>
#include <stdint.h>

namespace ru {
namespace {

__device__ __forceinline__ float mul_rn(float a, float b) {        // a product that is rounded on its own, never folded into an fma
#pragma clang fp contract(off)
    return a * b;
}

// ------------------------------------------------------------------ global L2 norm, float64
struct SquareOp {
    const float* g;
    __device__ __forceinline__ double quad(size_t i) const {
        const float4 v = ld4(g + i);
        const double x = v.x, y = v.y, z = v.z, w = v.w;
        return (x * x + y * y) + (z * z + w * w);
    }
    __device__ __forceinline__ double one(size_t i) const { const double x = g[i]; return x * x; }
};

__global__ __launch_bounds__(FL_BLOCK) void gradnorm_finalize_kernel(const double* __restrict__ slots, size_t n_slots, double max_norm,
                                                                     double* __restrict__ norm_out, float* __restrict__ coef_out) {
    __shared__ double part[FL_BLOCK];
    const double tot = sum_slots(slots, n_slots, part);
    if (threadIdx.x == 0) {
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
int adamw_launch(float* w, const float* g, float* m, float* v, float* vmax, const float* coef, size_t n, float lr, float b1, float b2, float eps,
                        float wd, int step, const Lanes& l, hipStream_t s) {
    const double bc1 = 1.0 - pow((double)b1, (double)step), bc2 = 1.0 - pow((double)b2, (double)step);       // as adam_launch
    AdamWOp<AMS, DEC> op{w, g, m, v, vmax, coef, (float)((double)lr / bc1), b1, b2, eps, wd, (float)sqrt(bc2), (float)(1.0 - (double)lr * (double)wd)};
    return stream_launch(op, n, l, s, "adamw_kernel");
}

}  // namespace
}  // namespace ru

using namespace ru;

extern "C" size_t ru_gradnorm_slots(size_t n) {
    return n ? fl_slots(n) : 0;
}

extern "C" size_t ru_gradnorm_workspace_bytes(size_t n_total, size_t n_runs) {
    // at least the sum of ru_gradnorm_slots over any split of n_total elements into n_runs runs: a run of n elements takes
    // ceil((ceil(n / 4) + 3) / 256) <= (n / 4 + 1) / 256 + 2 slots
    return sizeof(double) * ((n_total / 4 + n_runs) / FL_BLOCK + 2 * n_runs + 1);
}

extern "C" int ru_gradnorm_partial(const float* g, size_t n, size_t first_slot, double* ws, size_t ws_bytes, ru_stream_t stream) {
    RU_REQUIRE(g && ws, "ru_gradnorm_partial: null argument");
    RU_REQUIRE(((uintptr_t)g & 3u) == 0 && ((uintptr_t)ws & 7u) == 0, "ru_gradnorm_partial: misaligned pointer");
    if (n == 0) return RU_OK;
    const void* const ptrs[1] = {g};
    const size_t grid = fl_slots(n);                                 // the slot count is a function of n alone: lanes past the work write 0
    RU_REQUIRE((first_slot + grid) * sizeof(double) <= ws_bytes, "ru_gradnorm_partial: workspace too small for slots [%zu, %zu)", first_slot, first_slot + grid);
    return sum_launch(SquareOp{g}, n, lanes_for(n, ptrs), ws + first_slot, (hipStream_t)stream, "gradnorm_partial_kernel");
}

extern "C" int ru_gradnorm_finalize(const double* ws, size_t n_slots, double max_norm, double* norm_out, float* coef_out, ru_stream_t stream) {
    RU_REQUIRE(ws && norm_out && coef_out, "ru_gradnorm_finalize: null argument");
    RU_REQUIRE(!(max_norm < 0.0), "ru_gradnorm_finalize: max_norm must not be negative");
    hipLaunchKernelGGL(gradnorm_finalize_kernel, dim3(1), dim3(FL_BLOCK), 0, (hipStream_t)stream, ws, n_slots, max_norm, norm_out, coef_out);
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
