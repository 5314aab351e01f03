// The reference's training criteria (loss.py:15-195) on the device, as closed forms in per-row moments.  A row is one (n, c) of the
// [N, C, V] probability / target pair.  Every criterion's value is a function of a few sums over rows, and its gradient has the form
//     dL/dp = a*g + b*p + c + d * g/(p + 1e-6) + e * (1-g)/((1+1e-6) - p)
// with a..e constant per row.  Four launches:
//   crit_moments_kernel + crit_moments_final_kernel : one streaming pass, float64 moments [N, C, M] (float per chunk, double across chunks)
//   crit_reduce_kernel   : what crosses ranks -- per-channel totals over the shard's samples, and the Dice_loss_separate sum over them
//   crit_eval_kernel     : the float64 value of every term and of the weighted total, and the per-row coefficient table [N, C, 5]
//   crit_apply_kernel    : one streaming pass, dp = f(p, g, coef[row]) (times an optional device scale: autograd's incoming gradient)
// The Dice_loss_joint + BCE pair of the training step keeps its own kernels (pointwise.hip, crit_*); this unit serves criterion lists.
#include "pw_helpers.hpp"

#include <stdint.h>

namespace ru {
namespace {

constexpr int CM_CHUNK = 8192;                    // voxels of one row per moments block
constexpr int CM = RU_CRIT_MOMENTS;
constexpr unsigned CM_LOG_BITS = (1u << RU_CRIT_M_GLOGP) | (1u << RU_CRIT_M_QLOGQ);

int cm_tiles(size_t V) { return (int)((V + CM_CHUNK - 1) / CM_CHUNK); }

// the float32 constants of the reference's expressions: pred + 1e-6, (1. + 1e-6) - pred
__device__ __forceinline__ float ce_log_p(float p) { return logf(p + 1e-6f); }
__device__ __forceinline__ float ce_log_q(float p) { return logf((float)(1.0 + 1e-6) - p); }

template <bool LOGS>
__device__ __forceinline__ void cm_add(float (&s)[CM], float p, float g) {
    s[RU_CRIT_M_PG] += p * g;
    s[RU_CRIT_M_PP] += p * p;
    s[RU_CRIT_M_P] += p;
    s[RU_CRIT_M_G] += g;
    if (LOGS) {
        s[RU_CRIT_M_GLOGP] += g * ce_log_p(p);
        s[RU_CRIT_M_QLOGQ] += (1.f - g) * ce_log_q(p);
    }
    const float d = p - g;
    s[RU_CRIT_M_D2] += d * d;
}

// grid (tiles, N*C), 256 threads: block (t, row) sums voxels [t*CM_CHUNK, (t+1)*CM_CHUNK) of the row.  VEC4: float4 loads; the launcher takes it only when
// V % 4 == 0 AND p and g are 16-byte aligned (vec4_ok) -- every row start and every tile start is then 16-byte aligned too.  part[(row*nblk + t)*CM + m]
template <bool LOGS, bool VEC4>
__global__ __launch_bounds__(256) void crit_moments_kernel(const float* __restrict__ p, const float* __restrict__ g, float* __restrict__ part,
                                                           size_t V, int nblk) {
    __shared__ float buf[4];
    const size_t row = blockIdx.y;
    const size_t v0 = (size_t)blockIdx.x * CM_CHUNK;
    const size_t v1 = v0 + CM_CHUNK < V ? v0 + CM_CHUNK : V;
    const float* __restrict__ pr = p + row * V;
    const float* __restrict__ gr = g + row * V;
    float s[CM];
#pragma unroll
    for (int m = 0; m < CM; ++m) s[m] = 0.f;
    if (VEC4) {
        for (size_t v = v0 + 4 * threadIdx.x; v < v1; v += 4 * 256) {
            const float4 pv = *reinterpret_cast<const float4*>(pr + v), gv = *reinterpret_cast<const float4*>(gr + v);
            cm_add<LOGS>(s, pv.x, gv.x);
            cm_add<LOGS>(s, pv.y, gv.y);
            cm_add<LOGS>(s, pv.z, gv.z);
            cm_add<LOGS>(s, pv.w, gv.w);
        }
    } else {
        for (size_t v = v0 + threadIdx.x; v < v1; v += 256) cm_add<LOGS>(s, pr[v], gr[v]);
    }
    float* q = part + (row * nblk + blockIdx.x) * CM;
#pragma unroll
    for (int m = 0; m < CM; ++m) {
        const float t = block_sum(s[m], buf);
        if (threadIdx.x == 0) q[m] = t;
    }
}

// one block per row: moments[row*CM + m] = sum over the row's tiles in float64, tiles in a fixed order
__global__ __launch_bounds__(256) void crit_moments_final_kernel(const float* __restrict__ part, double* __restrict__ moments, int nblk) {
    __shared__ double buf[4];
    const size_t row = blockIdx.x;
    for (int m = 0; m < CM; ++m) {
        double t = 0.0;
        for (int b = threadIdx.x; b < nblk; b += 256) t += (double)part[(row * nblk + b) * CM + m];
        t = block_sum_d(t, buf);
        if (threadIdx.x == 0) moments[row * CM + m] = t;
    }
}

// Dice_loss_separate's per-sample term for row (n, c >= 1): (2 sum pg + 1) / (sum (p^2 + g) + 1) (loss.py:187-193)
__device__ __forceinline__ double sep_term(const double* __restrict__ s) {
    return (2.0 * s[RU_CRIT_M_PG] + 1.0) / (s[RU_CRIT_M_PP] + s[RU_CRIT_M_G] + 1.0);
}

// one block: out[c*CM + m] = sum over the shard's samples (in order) of moments[n, c, m]; out[C*CM] = sum over n, c >= 1 of sep_term
__global__ __launch_bounds__(256) void crit_reduce_kernel(const double* __restrict__ moments, int N, int C, double* __restrict__ out) {
    for (int i = threadIdx.x; i < C * CM; i += 256) {
        double t = 0.0;
        for (int n = 0; n < N; ++n) t += moments[(size_t)n * C * CM + i];
        out[i] = t;
    }
    if (threadIdx.x == 0) {
        double t = 0.0;
        for (int n = 0; n < N; ++n)
            for (int c = 1; c < C; ++c) t += sep_term(moments + ((size_t)n * C + c) * CM);
        out[C * CM] = t;
    }
}

struct CritTerms {
    ru_crit_term_t t[RU_CRIT_MAX_TERMS];
    int n;
};

// values[0] = sum_t weight_t * L_t, values[1 + t] = L_t.  coef[(n*C + c)*5 + {a,b,c,d,e}] = sum_t weight_t * (coefficients of dL_t/dp).
// tot: the global per-channel totals and the Dice_loss_separate slot (crit_reduce_kernel's output, all-reduced); local: this shard's moments.
__global__ __launch_bounds__(256) void crit_eval_kernel(const double* __restrict__ tot, const double* __restrict__ local, int N, int C, double count,
                                                        double n_global, CritTerms terms, double* __restrict__ values, float* __restrict__ coef) {
    __shared__ double gdl_i[RU_CRIT_MAX_TERMS], gdl_u[RU_CRIT_MAX_TERMS];
#define T_(c, m) tot[(c) * CM + (m)]
    if (threadIdx.x == 0) {
        double total = 0.0;
        for (int k = 0; k < terms.n; ++k) {
            const ru_crit_term_t& t = terms.t[k];
            const double pr = t.priority;
            double L = 0.0, a = 0.0, b = 0.0;
            switch (t.kind) {
            case RU_CRIT_DICE_JOINT:                                     // loss.py:112-122
                for (int c = 0; c < C; ++c) a += 2.0 * (T_(c, RU_CRIT_M_PG) + 1e-6) / (T_(c, RU_CRIT_M_PP) + T_(c, RU_CRIT_M_G) + 2e-6);
                L = pr * (1.0 - a / C);
                break;
            case RU_CRIT_BCE:                                            // loss.py:76-79
                for (int c = 0; c < C; ++c) { a += T_(c, RU_CRIT_M_GLOGP); b += T_(c, RU_CRIT_M_QLOGQ); }
                L = -(a + t.bg_weight * b) / count;
                break;
            case RU_CRIT_MSE:                                            // loss.py:24-29
                for (int c = 0; c < C; ++c) a += T_(c, RU_CRIT_M_D2);
                L = pr * a / count;
                break;
            case RU_CRIT_CE:                                             // loss.py:59-61
                for (int c = 0; c < C; ++c) a += T_(c, RU_CRIT_M_GLOGP);
                L = -a / count;
                break;
            case RU_CRIT_DICE1D:                                         // loss.py:90-96
                for (int c = 0; c < C; ++c) a += (T_(c, RU_CRIT_M_PG) + 1.0) / (T_(c, RU_CRIT_M_P) + T_(c, RU_CRIT_M_G) + 2.0);
                L = 1.0 - 2.0 * (a / C);
                break;
            case RU_CRIT_GDL_JOINT:                                      // loss.py:135-150: channels 1.., w_c = 1 / sum g (inf for an absent class)
                for (int c = 1; c < C; ++c) {
                    const double w = 1.0 / T_(c, RU_CRIT_M_G);
                    a += w * (T_(c, RU_CRIT_M_PG) + 1.0);
                    b += w * (T_(c, RU_CRIT_M_PP) + T_(c, RU_CRIT_M_G) + 1.0);
                }
                gdl_i[k] = a;
                gdl_u[k] = b;
                L = pr * (1.0 - 2.0 * a / b);
                break;
            case RU_CRIT_SENS_JOINT:                                     // loss.py:162-174, all channels
                for (int c = 0; c < C; ++c) a += (T_(c, RU_CRIT_M_PG) + 1.0) / (T_(c, RU_CRIT_M_G) + 1.0);
                L = pr * (1.0 - a / C);
                break;
            case RU_CRIT_DICE_SEPARATE:                                  // loss.py:184-195: channels 1.., priority unused
                L = 1.0 - tot[C * CM] / (n_global * (C - 1));
                break;
            }
            values[1 + k] = L;
            total += t.weight * L;
        }
        values[0] = total;
    }
    __syncthreads();
    for (int row = threadIdx.x; row < N * C; row += 256) {
        const int c = row % C;
        const double* s = local + (size_t)row * CM;
        double k5[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
        for (int k = 0; k < terms.n; ++k) {
            const ru_crit_term_t& t = terms.t[k];
            const double w = t.weight, pr = t.priority;
            switch (t.kind) {
            case RU_CRIT_DICE_JOINT: {
                const double I = T_(c, RU_CRIT_M_PG) + 1e-6, U = T_(c, RU_CRIT_M_PP) + T_(c, RU_CRIT_M_G) + 2e-6, q = 2.0 * pr / C;
                k5[0] -= w * q / U;
                k5[1] += w * 2.0 * q * I / (U * U);
                break;
            }
            case RU_CRIT_BCE:
                k5[3] -= w / count;
                k5[4] += w * t.bg_weight / count;
                break;
            case RU_CRIT_MSE:
                k5[0] -= w * 2.0 * pr / count;
                k5[1] += w * 2.0 * pr / count;
                break;
            case RU_CRIT_CE:
                k5[3] -= w / count;
                break;
            case RU_CRIT_DICE1D: {
                const double I = T_(c, RU_CRIT_M_PG) + 1.0, U = T_(c, RU_CRIT_M_P) + T_(c, RU_CRIT_M_G) + 2.0;
                k5[0] -= w * 2.0 / (C * U);
                k5[2] += w * 2.0 * I / (C * U * U);
                break;
            }
            case RU_CRIT_GDL_JOINT:
                if (c > 0) {
                    const double wc = 1.0 / T_(c, RU_CRIT_M_G), I = gdl_i[k], U = gdl_u[k];
                    k5[0] -= w * 2.0 * pr * wc / U;
                    k5[1] += w * 4.0 * pr * wc * I / (U * U);
                }
                break;
            case RU_CRIT_SENS_JOINT:
                k5[0] -= w * pr / (C * (T_(c, RU_CRIT_M_G) + 1.0));
                break;
            case RU_CRIT_DICE_SEPARATE:
                if (c > 0) {
                    const double K = 1.0 / (n_global * (C - 1)), I = s[RU_CRIT_M_PG], U = s[RU_CRIT_M_PP] + s[RU_CRIT_M_G] + 1.0;
                    k5[0] -= w * 2.0 * K / U;
                    k5[1] += w * 2.0 * K * (2.0 * I + 1.0) / (U * U);
                }
                break;
            }
        }
        for (int j = 0; j < 5; ++j) coef[(size_t)row * 5 + j] = (float)k5[j];
    }
#undef T_
}

template <bool LOGS>
__device__ __forceinline__ float crit_f(float p, float g, float a, float b, float c, float d, float e) {
    float r = (a * g + b * p) + c;
    if (LOGS) r += d * (g / (p + 1e-6f)) + e * ((1.f - g) / ((float)(1.0 + 1e-6) - p));
    return r;
}

// grid (x, N*C): dp = f(p, g, coef[row]) * (*scale if given).  LOGS = false when no term has d or e (no division).  VEC4 under vec4_ok(V, p, g, dp)
template <bool LOGS, bool VEC4>
__global__ __launch_bounds__(256) void crit_apply_kernel(const float* __restrict__ p, const float* __restrict__ g, const float* __restrict__ coef,
                                                         const float* __restrict__ scale, float* __restrict__ dp, size_t V) {
    const size_t row = blockIdx.y;
    const float sc = scale ? *scale : 1.f;
    const float a = coef[row * 5 + 0] * sc, b = coef[row * 5 + 1] * sc, c = coef[row * 5 + 2] * sc;
    const float d = coef[row * 5 + 3] * sc, e = coef[row * 5 + 4] * sc;
    const float* __restrict__ pr = p + row * V;
    const float* __restrict__ gr = g + row * V;
    float* __restrict__ o = dp + row * V;
    const size_t step = (size_t)gridDim.x * 256;
    if (VEC4) {
        for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < V / 4; i += step) {
            const float4 pv = reinterpret_cast<const float4*>(pr)[i], gv = reinterpret_cast<const float4*>(gr)[i];
            reinterpret_cast<float4*>(o)[i] = make_float4(crit_f<LOGS>(pv.x, gv.x, a, b, c, d, e), crit_f<LOGS>(pv.y, gv.y, a, b, c, d, e),
                                                          crit_f<LOGS>(pv.z, gv.z, a, b, c, d, e), crit_f<LOGS>(pv.w, gv.w, a, b, c, d, e));
        }
    } else {
        for (size_t v = (size_t)blockIdx.x * 256 + threadIdx.x; v < V; v += step) o[v] = crit_f<LOGS>(pr[v], gr[v], a, b, c, d, e);
    }
}

// the float4 forms: rows of a multiple of 4 elements that start on a 16-byte boundary, for every pointer the kernel accesses 16 bytes at a time
bool vec4_ok(size_t V, const void* a, const void* b, const void* c = nullptr) {
    return V % 4 == 0 && (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c) & 15u) == 0;
}

dim3 apply_grid(size_t V, int vec, int rows) {
    size_t bx = (V / vec + 255) / 256;
    if (bx > 4096) bx = 4096;
    if (bx < 1) bx = 1;
    return dim3((unsigned)bx, (unsigned)rows);
}

}  // namespace
}  // namespace ru

using namespace ru;

extern "C" size_t ru_crit_moments_workspace_bytes(int N, int C, size_t V) {
    if (N <= 0 || C <= 0 || V == 0) return 0;
    return (size_t)N * C * cm_tiles(V) * CM * sizeof(float);
}

extern "C" int ru_crit_moments(const float* p, const float* g, int N, int C, size_t V, unsigned mask, double* moments,
                               void* ws, size_t ws_bytes, ru_stream_t stream) {
    RU_REQUIRE(p && g && moments && N > 0 && C > 0 && V > 0, "ru_crit_moments: bad argument");
    RU_REQUIRE((long long)N * C <= 65535, "ru_crit_moments: N * C = %lld rows, at most 65535", (long long)N * C);
    RU_REQUIRE((mask & ~(unsigned)RU_CRIT_MASK_ALL) == 0, "ru_crit_moments: mask 0x%x has bits outside RU_CRIT_MASK_ALL", mask);
    RU_REQUIRE(ws && ws_bytes >= ru_crit_moments_workspace_bytes(N, C, V), "ru_crit_moments: workspace too small");
    hipStream_t s = (hipStream_t)stream;
    const int nblk = cm_tiles(V);
    const bool logs = (mask & CM_LOG_BITS) != 0, vec = vec4_ok(V, p, g);
    const dim3 grid(nblk, N * C);
    float* part = (float*)ws;
    if (logs && vec) hipLaunchKernelGGL((crit_moments_kernel<true, true>), grid, dim3(256), 0, s, p, g, part, V, nblk);
    else if (logs) hipLaunchKernelGGL((crit_moments_kernel<true, false>), grid, dim3(256), 0, s, p, g, part, V, nblk);
    else if (vec) hipLaunchKernelGGL((crit_moments_kernel<false, true>), grid, dim3(256), 0, s, p, g, part, V, nblk);
    else hipLaunchKernelGGL((crit_moments_kernel<false, false>), grid, dim3(256), 0, s, p, g, part, V, nblk);
    RU_CHECK_LAUNCH("crit_moments_kernel");
    hipLaunchKernelGGL(crit_moments_final_kernel, dim3(N * C), dim3(256), 0, s, (const float*)part, moments, nblk);
    RU_CHECK_LAUNCH("crit_moments_final_kernel");
    return RU_OK;
}

extern "C" int ru_crit_reduce(const double* moments, int N, int C, double* out, ru_stream_t stream) {
    RU_REQUIRE(moments && out && N > 0 && C > 0, "ru_crit_reduce: bad argument");
    hipLaunchKernelGGL(crit_reduce_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, moments, N, C, out);
    RU_CHECK_LAUNCH("crit_reduce_kernel");
    return RU_OK;
}

extern "C" int ru_crit_eval(const double* totals, const double* moments, int N, int C, double count, double n_global,
                            const ru_crit_term_t* terms, int nterms, double* values, float* coef, ru_stream_t stream) {
    RU_REQUIRE(totals && moments && values && coef && terms && N > 0 && C > 0, "ru_crit_eval: bad argument");
    RU_REQUIRE(nterms >= 1 && nterms <= RU_CRIT_MAX_TERMS, "ru_crit_eval: %d terms, 1..%d", nterms, RU_CRIT_MAX_TERMS);
    RU_REQUIRE(count > 0.0 && n_global >= N, "ru_crit_eval: count %g, n_global %g (at least N = %d)", count, n_global, N);
    CritTerms t{};
    for (int k = 0; k < nterms; ++k) {
        RU_REQUIRE(terms[k].kind >= 0 && terms[k].kind < RU_CRIT_NUM_KINDS, "ru_crit_eval: term %d has unknown kind %d", k, terms[k].kind);
        t.t[k] = terms[k];
    }
    t.n = nterms;
    hipLaunchKernelGGL(crit_eval_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, totals, moments, N, C, count, n_global, t, values, coef);
    RU_CHECK_LAUNCH("crit_eval_kernel");
    return RU_OK;
}

extern "C" int ru_crit_grad(const float* p, const float* g, const float* coef, const float* scale, int N, int C, size_t V, int with_logs,
                            float* dp, ru_stream_t stream) {
    RU_REQUIRE(p && g && coef && dp && N > 0 && C > 0 && V > 0, "ru_crit_grad: bad argument");
    RU_REQUIRE((long long)N * C <= 65535, "ru_crit_grad: N * C = %lld rows, at most 65535", (long long)N * C);
    hipStream_t s = (hipStream_t)stream;
    const bool vec = vec4_ok(V, p, g, dp);
    const dim3 grid = apply_grid(V, vec ? 4 : 1, N * C);
    if (with_logs && vec) hipLaunchKernelGGL((crit_apply_kernel<true, true>), grid, dim3(256), 0, s, p, g, coef, scale, dp, V);
    else if (with_logs) hipLaunchKernelGGL((crit_apply_kernel<true, false>), grid, dim3(256), 0, s, p, g, coef, scale, dp, V);
    else if (vec) hipLaunchKernelGGL((crit_apply_kernel<false, true>), grid, dim3(256), 0, s, p, g, coef, scale, dp, V);
    else hipLaunchKernelGGL((crit_apply_kernel<false, false>), grid, dim3(256), 0, s, p, g, coef, scale, dp, V);
    RU_CHECK_LAUNCH("crit_apply_kernel");
    return RU_OK;
}
