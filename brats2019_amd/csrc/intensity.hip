// intensity.hip -- intensity augmentation of a training patch (ru_intensity_augment): the transforms nnU-Net made standard, per channel and in
// this fixed order (include/resunet_hip.h holds the definitions; dataloader.intensity_augment_host is the float64 restatement):
//
//   1 blur        gaussian_filter(x, sigma, mode='reflect'), radius <= 8     -> int_blur_d_kernel (axis 0), int_blur_hw_kernel (axes 1, 2 in one tile)
//   2 low-res     nearest down, trilinear up: 8 reads per output voxel      -> the LOAD of int_pointwise_kernel (index tables: int_lowres_table_kernel)
//   3 noise       x + sqrt(variance) * n(seed, channel, voxel)               \
//   4 brightness  x * b                                                       |  int_pointwise_kernel: one kernel, evaluated up to a `level`
//   5 contrast    clip((x - mean) * f + mean, min, max)                       |
//   6 gamma       ((x - min) / (range + 1e-7))^g * range + min, +- invert, retain-stats /
//
// Passes.  Contrast, gamma and retain-stats each need statistics of the WHOLE channel as it enters them, so each is a device-wide
// dependency: one launch of int_pointwise_kernel per statistic (`level` 0, 1, 2: per-workgroup partials -> int_stats_final_kernel) and a final
// launch that writes.  A pass is bytes, and the chain behind the statistics-free head (low-res load, noise, brightness) is cheap, so no
// launch stores an intermediate for the next one: each evaluates the chain again, up to its level, from the value that enters contrast.
// That value is the spatial stage's output itself, or -- where the head holds the low-res load or the noise, which cost more than a
// read and a write -- a copy kept in the (by then free) first blur buffer by the launch that takes the channel's first statistic.  Every
// launch runs the same machine code on the same stored values without contraction, so a value formed again is bit-identical (the exact
// min stays a lower bound of what gamma sees).  Per channel, in units of one read or one write of the channel (V * 4 bytes):
//     no stage                 R + W                      (the copy: the final launch with an empty mask)
//     blur only                2 (R + W)                  (the tile pass writes `out` directly; the final launch skips the channel)
//     any of 2 3 4             R + W                      (low-res is a launch's load: no pass and no array of its own)
//     each of contrast, gamma, retain-stats   + R         (one statistics launch each), + W once if low-res or noise is on (the kept copy)
//     all stages               4 (R + W) + 2 R = 10 units (blur 2, first statistic + copy 1, final 1, two more statistics); 4 x 128^3: 336 MB
// The low-res load reads 8 source voxels per output, but they are the coarse grid's: at zoom z about z^3 of the channel is touched at all.
//
// Blur.  The taps are a fixed 17 (radius 8) with the weights beyond the channel's radius set to zero -- adding +0 * x changes no finite sum --
// so every window index is a compile-time constant and the weights sit in scalar registers (kernel arguments).  Axis 0 has no sharing
// between lanes: a thread keeps a 16-byte column of 32 inputs in registers and writes 16 outputs.  Axes 1 and 2 share one LDS tile with
// an 8-voxel halo: 48 x 144 staged, axis 1 into 32 x 144, axis 2 into 32 x 128, in scipy's axis order.  Every index goes through the
// periodic reflection, so a radius beyond the extent is the same code.
#include "ru_common.h"
#include "pw_helpers.hpp"

#include <limits.h>
#include <math.h>

namespace ru {

static_assert(RU_AUG_MAXC == 8, "ru_intensity_params holds 8 channels");
constexpr int IN_R = 8;                    // largest radius: int(4 * 2.0 + 0.5)
constexpr int IN_TAPS = 2 * IN_R + 1;
constexpr int IN_TD = 16;                  // outputs per thread along axis 0
constexpr int IN_TH = 32, IN_TW = 128;     // output tile of the axis 1 + 2 pass
constexpr int IN_SH = IN_TH + 2 * IN_R, IN_SW = IN_TW + 2 * IN_R;     // 48 x 144 staged
constexpr int IN_CHUNK = 8192;             // voxels per workgroup of the pointwise kernel = one partial

// the generator of csrc/elastic.hip (el_mix64: splitmix64's finalizer), restated: that unit keeps it to itself
__host__ __device__ __forceinline__ unsigned long long in_mix64(unsigned long long z) {
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
__device__ __forceinline__ int in_reflect(int i, int n) {      // el_reflect: half-sample symmetric, periodic in 2 n
    if ((unsigned)i < (unsigned)n) return i;
    int m = i % (2 * n);
    if (m < 0) m += 2 * n;
    return m < n ? m : 2 * n - 1 - m;
}

__device__ __forceinline__ float in_fma(float w, float x, float a) { return fmaf(w, x, a); }
__device__ __forceinline__ float4 in_fma(float w, float4 x, float4 a) { return make_float4(fmaf(w, x.x, a.x), fmaf(w, x.y, a.y), fmaf(w, x.z, a.z), fmaf(w, x.w, a.w)); }
template <class T> __device__ __forceinline__ T in_zero();
template <> __device__ __forceinline__ float in_zero<float>() { return 0.f; }
template <> __device__ __forceinline__ float4 in_zero<float4>() { return make_float4(0.f, 0.f, 0.f, 0.f); }

struct IntLrEntry { int s0, s1; float t, pad; };               // low-res, one axis: out = (1 - t) * x[s0] + t * x[s1]

struct IntArgs {
    const float* in;             // [C][P0][P1][P2]
    float* out;
    float* tmp_a;                // axis-0 pass of the blur
    float* tmp_b;                // blurred channels that have further stages
    const IntLrEntry* table;     // [C][P0 + P1 + P2]
    double* partials;            // [3][C][nblk][4]: sum, sum of squares, min, max
    double* stats;               // [3][C][4]: mean, std, min, max as the channel enters contrast / gamma / the retain-stats rescale
    int C, P0, P1, P2, nblk, vec;
    unsigned V;
    int mask[RU_AUG_MAXC];
    float w[RU_AUG_MAXC][IN_TAPS];
    float sd[RU_AUG_MAXC], bright[RU_AUG_MAXC], contrast[RU_AUG_MAXC], gamma[RU_AUG_MAXC];
    unsigned long long key[RU_AUG_MAXC];
};

// ---------------------------------------------------------------------------------------------------------------- blur, axis 0
// in [P0][inner], inner = P1 * P2 contiguous, T = float4 where inner % 4 == 0.  grid (inner / 256, P0 / 16, C).
template <class T>
__global__ __launch_bounds__(256) void int_blur_d_kernel(const IntArgs a) {
    const int c = blockIdx.z;
    if (!(a.mask[c] & RU_INT_BLUR)) return;
    const unsigned inner = (unsigned)a.P1 * a.P2 / (unsigned)(sizeof(T) / 4);
    const unsigned col = blockIdx.x * 256u + threadIdx.x;
    if (col >= inner) return;
    const int i0 = (int)blockIdx.y * IN_TD;
    const T* src = (const T*)(a.in + (size_t)c * a.V);
    T* dst = (T*)(a.tmp_a + (size_t)c * a.V);
    float w[IN_TAPS];
#pragma unroll
    for (int k = 0; k < IN_TAPS; ++k) w[k] = a.w[c][k];
    T x[IN_TD + 2 * IN_R];
#pragma unroll
    for (int k = 0; k < IN_TD + 2 * IN_R; ++k) x[k] = src[(size_t)in_reflect(i0 - IN_R + k, a.P0) * inner + col];
#pragma unroll
    for (int t = 0; t < IN_TD; ++t) {
        T acc = in_zero<T>();
#pragma unroll
        for (int k = 0; k < IN_TAPS; ++k) acc = in_fma(w[k], x[t + k], acc);
        if (i0 + t < a.P0) dst[(size_t)(i0 + t) * inner + col] = acc;
    }
}

// ---------------------------------------------------------------------------------------------------------------- blur, axes 1 and 2
// One [P1][P2] slice per blockIdx.y, tiles of 32 x 128 outputs.  grid (tiles, P0, C).  Rows and columns of a tile beyond the extent are
// computed from reflected (valid) indices and not stored.
__global__ __launch_bounds__(256) void int_blur_hw_kernel(const IntArgs a) {
    __shared__ float4 S[IN_SH][IN_SW / 4];
    __shared__ float4 M[IN_TH][IN_SW / 4];
    const int c = blockIdx.z;
    const int m = a.mask[c];
    if (!(m & RU_INT_BLUR)) return;
    const int P1 = a.P1, P2 = a.P2;
    const int tw = (P2 + IN_TW - 1) / IN_TW;
    const int h0 = ((int)blockIdx.x / tw) * IN_TH, w0 = ((int)blockIdx.x % tw) * IN_TW;
    const float* src = a.tmp_a + (size_t)c * a.V + (size_t)blockIdx.y * P1 * P2;
    float* dst = (m == RU_INT_BLUR ? a.out : a.tmp_b) + (size_t)c * a.V + (size_t)blockIdx.y * P1 * P2;
    float w[IN_TAPS];
#pragma unroll
    for (int k = 0; k < IN_TAPS; ++k) w[k] = a.w[c][k];
    for (int idx = threadIdx.x; idx < IN_SH * (IN_SW / 4); idx += 256) {
        const int row = idx / (IN_SW / 4), g = idx % (IN_SW / 4);
        const int h = in_reflect(h0 - IN_R + row, P1);
        const int wq = w0 - IN_R + 4 * g;
        const float* r = src + (size_t)h * P2;
        float4 v;
        if (a.vec && wq >= 0 && wq + 4 <= P2) v = *(const float4*)(r + wq);
        else v = make_float4(r[in_reflect(wq, P2)], r[in_reflect(wq + 1, P2)], r[in_reflect(wq + 2, P2)], r[in_reflect(wq + 3, P2)]);
        S[row][g] = v;
    }
    __syncthreads();
    if (threadIdx.x < (IN_SW / 4) * (IN_TH / 8)) {             // axis 1: 36 column groups x 4 chunks of 8 rows
        const int g = threadIdx.x % (IN_SW / 4), r0 = (threadIdx.x / (IN_SW / 4)) * 8;
        float4 x[8 + 2 * IN_R];
#pragma unroll
        for (int k = 0; k < 8 + 2 * IN_R; ++k) x[k] = S[r0 + k][g];
#pragma unroll
        for (int t = 0; t < 8; ++t) {
            float4 acc = in_zero<float4>();
#pragma unroll
            for (int k = 0; k < IN_TAPS; ++k) acc = in_fma(w[k], x[t + k], acc);
            M[r0 + t][g] = acc;
        }
    }
    __syncthreads();
#pragma unroll 1
    for (int item = threadIdx.x; item < IN_TH * (IN_TW / 4); item += 256) {      // axis 2: 4 outputs from 20 inputs
        const int row = item / (IN_TW / 4), g = item % (IN_TW / 4);
        float x[4 + 2 * IN_R];
#pragma unroll
        for (int q = 0; q < 5; ++q) {
            const float4 v = M[row][g + q];
            x[4 * q] = v.x; x[4 * q + 1] = v.y; x[4 * q + 2] = v.z; x[4 * q + 3] = v.w;
        }
        float o[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float acc = 0.f;
#pragma unroll
            for (int k = 0; k < IN_TAPS; ++k) acc = fmaf(w[k], x[j + k], acc);
            o[j] = acc;
        }
        const int h = h0 + row, wq = w0 + 4 * g;
        if (h >= P1 || wq >= P2) continue;
        float* r = dst + (size_t)h * P2 + wq;
        if (a.vec && wq + 4 <= P2) *(float4*)r = make_float4(o[0], o[1], o[2], o[3]);
        else
            for (int j = 0; j < 4 && wq + j < P2; ++j) r[j] = o[j];
    }
}

// ---------------------------------------------------------------------------------------------------------------- low-res index tables
// Per channel and axis (extent P, zoom z): n_c = max(1, floor(P z + 0.5)) comes from the host; in exact integer arithmetic
//   c = clamp((i + 0.5) n_c / P - 0.5, 0, n_c - 1) = clamp(((2 i + 1) n_c - P) / (2 P), ..),  j0 = floor(c), t = c - j0, j1 = min(j0 + 1, n_c - 1),
//   coarse sample j = source voxel min(floor((2 j + 1) P / (2 n_c)), P - 1).   grid (C), entries [P0 | P1 | P2].
struct IntLrArgs { IntLrEntry* table; int P[3]; int nc[RU_AUG_MAXC][3]; int mask[RU_AUG_MAXC]; };
__global__ __launch_bounds__(256) void int_lowres_table_kernel(const IntLrArgs a) {
    const int c = blockIdx.x;
    if (!(a.mask[c] & RU_INT_LOWRES)) return;
    const int total = a.P[0] + a.P[1] + a.P[2];
    for (int e = threadIdx.x; e < total; e += 256) {
        const int ax = e < a.P[0] ? 0 : (e < a.P[0] + a.P[1] ? 1 : 2);
        const int i = e - (ax == 0 ? 0 : (ax == 1 ? a.P[0] : a.P[0] + a.P[1]));
        const long long P = a.P[ax], nc = a.nc[c][ax];
        const long long num = (2ll * i + 1) * nc - P;
        long long j0 = 0, rem = 0;
        if (num > 0) { j0 = num / (2 * P); rem = num % (2 * P); }
        if (j0 >= nc - 1) { j0 = nc - 1; rem = 0; }
        const long long j1 = j0 + 1 < nc ? j0 + 1 : nc - 1;
        IntLrEntry t;
        t.s0 = (int)min(((2 * j0 + 1) * P) / (2 * nc), P - 1);
        t.s1 = (int)min(((2 * j1 + 1) * P) / (2 * nc), P - 1);
        t.t = (float)((double)rem / (double)(2 * P));
        t.pad = 0.f;
        a.table[(size_t)c * total + e] = t;
    }
}

// ---------------------------------------------------------------------------------------------------------------- the pointwise chain
// n(seed, channel, v): key = mix64(seed + (channel + 1) G), z1 = mix64(key + (2 v + 1) G), z2 = mix64(key + (2 v + 2) G), G = 0x9E3779B97F4A7C15;
// u1 = ((z1 >> 11) + 1) 2^-53 in (0, 1], u2 = (z2 >> 11) 2^-53 in [0, 1); n = sqrt(-2 ln u1) cos(2 pi u2).  The angle is reduced to
// [-pi, pi) in float64 before it is rounded to float32 (cos has period 1 in u2).  ln u1 keeps a RELATIVE error: with h = float32(u1),
// ln u1 = ln h + ln(1 + (u1 - h) / h) = logf(h) + (u1 - h) / h up to 2^-51, the difference exact in float64 -- one logf, no branch.  logf(h)
// alone leaves -ln u1 an absolute error of 3e-8 where it is about 1e-7 and turns every u1 in (1 - 2^-25, 1] into n = 0 (7.5e-5 off in n
// among 2 10^6 voxels).
__device__ __forceinline__ float in_normal(unsigned long long key, unsigned v) {
#pragma clang fp contract(off)
    const unsigned long long z1 = in_mix64(key + (2ull * v + 1ull) * 0x9E3779B97F4A7C15ull);
    const unsigned long long z2 = in_mix64(key + (2ull * v + 2ull) * 0x9E3779B97F4A7C15ull);
    const double u1 = (double)((z1 >> 11) + 1ull) * (1.0 / 9007199254740992.0);
    const float h = (float)u1;
    const float ln1 = logf(h) + (float)(u1 - (double)h) / h;
    double u2 = (double)(z2 >> 11) * (1.0 / 9007199254740992.0);
    if (u2 >= 0.5) u2 -= 1.0;
    const float ang = (float)(u2 * 6.283185307179586476925);
    return sqrtf(-2.f * ln1) * cosf(ang);
}

struct IntChan {                 // one channel's constants, in registers
    int m;
    float sd, bright, f, g;
    unsigned long long key;
    float c_mean, c_min, c_max;                  // contrast
    float g_min, g_range, g_inv;                 // gamma: min, max - min, 1 / (range + 1e-7)
    float r_mean_y, r_scale, r_mean;             // retain-stats
};
// noise and brightness: the part of the chain that needs no statistics
__device__ __forceinline__ float in_head(const IntChan& k, float x, unsigned v) {
#pragma clang fp contract(off)
    if (k.m & RU_INT_NOISE) x = x + k.sd * in_normal(k.key, v);
    if (k.m & RU_INT_BRIGHTNESS) x = x * k.bright;
    return x;
}
// from the value that enters contrast to the value at `level`: 0 = that value, 1 = as it enters gamma (negated if inverted), 2 = gamma's y
// before the retain-stats rescale, 3 = final.  No contraction, so a value is rounded the same way at whatever level it is formed again.
// t^g = exp2(g log2 t) on v_exp_f32 / v_log_f32 (measured 1.41 and 1.97 units of 2^-24 |result|, tools/libm_ulp.py; a denormal t counts as 0): the error
// of y is range t^g ln2 |g log2 t| times a few 2^-24 -- it grows with g, and tests/intensity_inputs.py carries that term per voxel.
__device__ __forceinline__ float in_tail(const IntChan& k, float x, int level) {
#pragma clang fp contract(off)
    if (level == 0) return x;
    if (k.m & RU_INT_CONTRAST) x = fminf(fmaxf((x - k.c_mean) * k.f + k.c_mean, k.c_min), k.c_max);
    if (!(k.m & RU_INT_GAMMA)) return x;
    const bool inv = (k.m & RU_INT_GAMMA_INVERT) != 0;
    if (inv) x = -x;
    if (level == 1) return x;
    const float t = fmaxf((x - k.g_min) * k.g_inv, 0.f);
    float y = __builtin_amdgcn_exp2f(k.g * __builtin_amdgcn_logf(t)) * k.g_range + k.g_min;
    if (level == 2) return y;
    if (k.m & RU_INT_GAMMA_RETAIN) y = (y - k.r_mean_y) * k.r_scale + k.r_mean;
    return inv ? -y : y;
}
// the low-res load of voxel (i, j, k): trilinear over the 8 coarse samples, read from the source directly
__device__ __forceinline__ float in_lowres(const float* __restrict__ src, const IntLrEntry& e0, const IntLrEntry& e1, const IntLrEntry& e2, int P1, int P2) {
    const size_t r00 = ((size_t)e0.s0 * P1 + e1.s0) * P2, r01 = ((size_t)e0.s0 * P1 + e1.s1) * P2;
    const size_t r10 = ((size_t)e0.s1 * P1 + e1.s0) * P2, r11 = ((size_t)e0.s1 * P1 + e1.s1) * P2;
    const float a00 = src[r00 + e2.s0] + e2.t * (src[r00 + e2.s1] - src[r00 + e2.s0]);
    const float a01 = src[r01 + e2.s0] + e2.t * (src[r01 + e2.s1] - src[r01 + e2.s0]);
    const float a10 = src[r10 + e2.s0] + e2.t * (src[r10 + e2.s1] - src[r10 + e2.s0]);
    const float a11 = src[r11 + e2.s0] + e2.t * (src[r11 + e2.s1] - src[r11 + e2.s0]);
    const float b0 = a00 + e1.t * (a01 - a00), b1 = a10 + e1.t * (a11 - a10);
    return b0 + e0.t * (b1 - b0);
}

struct IntAcc {                  // a thread's share of a channel statistic
    double s1 = 0.0, s2 = 0.0;
    float mn = INFINITY, mx = -INFINITY;
    __device__ __forceinline__ void add(float x) { s1 += (double)x; s2 += (double)x * (double)x; mn = fminf(mn, x); mx = fmaxf(mx, x); }
};

// grid (nblk, C); level 0..2: one partial per workgroup of the statistic taken at that level; level 3: writes `out`.  A channel that does not
// need the launch leaves at once.  A channel whose chain starts with the low-res load or the noise keeps the value that enters contrast in
// `tmp_a` when its first statistic is taken, and later launches start from there.
__global__ __launch_bounds__(256) void int_pointwise_kernel(const IntArgs a, int level) {
    __shared__ double sbuf[4][4];
    const int c = blockIdx.y;
    IntChan k;
    k.m = a.mask[c];
    const bool gam = (k.m & RU_INT_GAMMA) != 0;
    const bool wanted = level == 0 ? (k.m & RU_INT_CONTRAST) != 0 : level == 1 ? gam : level == 2 ? (gam && (k.m & RU_INT_GAMMA_RETAIN)) : k.m != RU_INT_BLUR;
    if (!wanted) return;
    k.sd = a.sd[c]; k.bright = a.bright[c]; k.f = a.contrast[c]; k.g = a.gamma[c]; k.key = a.key[c];
    k.c_mean = k.c_min = k.c_max = k.g_min = k.g_range = k.g_inv = k.r_mean_y = k.r_scale = k.r_mean = 0.f;
    if (level > 0 && (k.m & RU_INT_CONTRAST)) {
        const double* s = a.stats + (size_t)(0 * a.C + c) * 4;
        k.c_mean = (float)s[0]; k.c_min = (float)s[2]; k.c_max = (float)s[3];
    }
    if (level > 1 && gam) {
        const double* s = a.stats + (size_t)(1 * a.C + c) * 4;
        k.g_min = (float)s[2]; k.g_range = (float)(s[3] - s[2]); k.g_inv = 1.f / (k.g_range + 1e-7f);
        k.r_mean = (float)s[0];
        if (level > 2 && (k.m & RU_INT_GAMMA_RETAIN)) {
            const double* y = a.stats + (size_t)(2 * a.C + c) * 4;
            k.r_mean_y = (float)y[0];
            k.r_scale = (float)(s[1] / (y[1] >= 1e-8 ? y[1] : 1e-8));
        }
    }
    const int first = (k.m & RU_INT_CONTRAST) ? 0 : (gam ? 1 : 3);              // the first launch this channel takes part in
    const bool heavy = (k.m & (RU_INT_LOWRES | RU_INT_NOISE)) != 0;
    const bool from_keep = heavy && level > first, to_keep = heavy && level == first && first < 3;
    const bool gather = (k.m & RU_INT_LOWRES) != 0 && !from_keep;
    float* keep = a.tmp_a + (size_t)c * a.V;
    const float* src = from_keep ? keep : ((k.m & RU_INT_BLUR) ? a.tmp_b : a.in) + (size_t)c * a.V;
    float* dst = a.out + (size_t)c * a.V;
    const IntLrEntry* tab = a.table + (size_t)c * (a.P0 + a.P1 + a.P2);
    const unsigned v0 = blockIdx.x * (unsigned)IN_CHUNK, v1 = min(v0 + (unsigned)IN_CHUNK, a.V);
    IntAcc acc;
    const unsigned P2 = (unsigned)a.P2, P1 = (unsigned)a.P1;
    if (a.vec && !gather) {                                    // V a multiple of 4 and 16-byte aligned pointers
        for (unsigned v = v0 + 4u * threadIdx.x; v < v1; v += 1024u) {
            const float4 t = *(const float4*)(src + v);
            float x[4] = {t.x, t.y, t.z, t.w};
            if (!from_keep) {
#pragma unroll
                for (int q = 0; q < 4; ++q) x[q] = in_head(k, x[q], v + q);
            }
            if (to_keep) *(float4*)(keep + v) = make_float4(x[0], x[1], x[2], x[3]);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                x[q] = in_tail(k, x[q], level);
                acc.add(x[q]);
            }
            if (level == 3) *(float4*)(dst + v) = make_float4(x[0], x[1], x[2], x[3]);
        }
    } else {                                                   // one voxel per lane: a wave's low-res loads fall into a few cache lines per corner
        for (unsigned v = v0 + threadIdx.x; v < v1; v += 256u) {
            float x;
            if (gather) {
                const unsigned kk = v % P2, rr = v / P2;
                x = in_lowres(src, tab[rr / P1], tab[a.P0 + rr % P1], tab[a.P0 + a.P1 + kk], a.P1, a.P2);
            } else x = src[v];
            if (!from_keep) x = in_head(k, x, v);
            if (to_keep) keep[v] = x;
            x = in_tail(k, x, level);
            acc.add(x);
            if (level == 3) dst[v] = x;
        }
    }
    if (level == 3) return;
    double s1 = wave_sum_d(acc.s1), s2 = wave_sum_d(acc.s2);   // xor butterflies: every lane holds the same bits, the order is fixed
    float mn = acc.mn, mx = acc.mx;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { mn = fminf(mn, __shfl_xor(mn, o)); mx = fmaxf(mx, __shfl_xor(mx, o)); }
    if ((threadIdx.x & 63) == 0) { double* b = sbuf[threadIdx.x >> 6]; b[0] = s1; b[1] = s2; b[2] = (double)mn; b[3] = (double)mx; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double* p = a.partials + ((size_t)(level * a.C + c) * a.nblk + blockIdx.x) * 4;
        p[0] = ((sbuf[0][0] + sbuf[1][0]) + sbuf[2][0]) + sbuf[3][0];
        p[1] = ((sbuf[0][1] + sbuf[1][1]) + sbuf[2][1]) + sbuf[3][1];
        p[2] = fmin(fmin(sbuf[0][2], sbuf[1][2]), fmin(sbuf[2][2], sbuf[3][2]));
        p[3] = fmax(fmax(sbuf[0][3], sbuf[1][3]), fmax(sbuf[2][3], sbuf[3][3]));
    }
}
// partials -> (mean, std, min, max) in float64.  grid (C), 256 threads: thread t takes partials t, t + 256, .. in order, then a tree over the
// threads with fixed pairs -- the order of the additions depends on nothing but the number of partials.
__global__ __launch_bounds__(256) void int_stats_final_kernel(const IntArgs a, int level) {
    __shared__ double r[4][256];
    const int c = blockIdx.x, t = threadIdx.x;
    const int m = a.mask[c];
    if (!(level == 0 ? (m & RU_INT_CONTRAST) != 0 : level == 1 ? (m & RU_INT_GAMMA) != 0 : (m & RU_INT_GAMMA) && (m & RU_INT_GAMMA_RETAIN))) return;
    const double* p = a.partials + (size_t)(level * a.C + c) * a.nblk * 4;
    double s1 = 0.0, s2 = 0.0, mn = INFINITY, mx = -INFINITY;
    for (int i = t; i < a.nblk; i += 256) {
        const double* q = p + (size_t)i * 4;
        s1 += q[0]; s2 += q[1]; mn = fmin(mn, q[2]); mx = fmax(mx, q[3]);
    }
    r[0][t] = s1; r[1][t] = s2; r[2][t] = mn; r[3][t] = mx;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (t < o) { r[0][t] += r[0][t + o]; r[1][t] += r[1][t + o]; r[2][t] = fmin(r[2][t], r[2][t + o]); r[3][t] = fmax(r[3][t], r[3][t + o]); }
        __syncthreads();
    }
    if (t == 0) {
        double* s = a.stats + (size_t)(level * a.C + c) * 4;
        const double mean = r[0][0] / (double)a.V, var = r[1][0] / (double)a.V - mean * mean;
        s[0] = mean; s[1] = sqrt(var > 0.0 ? var : 0.0); s[2] = r[2][0]; s[3] = r[3][0];
    }
}

static int intensity_shape_ok(int C, int P0, int P1, int P2) {
    RU_REQUIRE(C >= 1 && C <= RU_AUG_MAXC, "ru_intensity_augment: 1..%d channels (got %d)", RU_AUG_MAXC, C);
    RU_REQUIRE(P0 > 0 && P1 > 0 && P2 > 0, "ru_intensity_augment: the patch extents must be positive");
    RU_REQUIRE((size_t)P0 * P1 * P2 * 2 < (size_t)INT_MAX && P0 <= 65535, "ru_intensity_augment: patch too large for 32-bit voxel indices");
    return RU_OK;
}
static inline int int_nblk(size_t V) { return (int)((V + IN_CHUNK - 1) / IN_CHUNK); }

}  // namespace ru

using namespace ru;

// workspace: two [C][V] float32 intermediates of the blur, the low-res tables, the partials and the statistics
extern "C" size_t ru_intensity_workspace_bytes(int C, int P0, int P1, int P2) {
    if (C < 1 || C > RU_AUG_MAXC || P0 <= 0 || P1 <= 0 || P2 <= 0) return 0;
    const size_t V = (size_t)P0 * P1 * P2;
    return 256 + 2 * align_up((size_t)C * V * sizeof(float), 256) + align_up((size_t)C * ((size_t)P0 + P1 + P2) * sizeof(IntLrEntry), 256) +
           align_up((size_t)3 * C * int_nblk(V) * 4 * sizeof(double), 256) + align_up((size_t)3 * C * 4 * sizeof(double), 256);
}

extern "C" int ru_intensity_augment(const float* in, float* out, int C, int P0, int P1, int P2, const ru_intensity_params* p, void* ws, size_t ws_bytes,
                                    ru_stream_t stream) {
    RU_REQUIRE(in && out && p, "ru_intensity_augment: null argument");
    if (int rc = intensity_shape_ok(C, P0, P1, P2)) return rc;
    const size_t V = (size_t)P0 * P1 * P2;
    RU_REQUIRE(in + (size_t)C * V <= out || out + (size_t)C * V <= in, "ru_intensity_augment: `out` may not alias `in`");
    RU_REQUIRE(ws && ws_bytes >= ru_intensity_workspace_bytes(C, P0, P1, P2), "ru_intensity_augment: workspace too small");
    IntArgs a{};
    IntLrArgs lr{};
    const int all_bits = RU_INT_BLUR | RU_INT_LOWRES | RU_INT_NOISE | RU_INT_BRIGHTNESS | RU_INT_CONTRAST | RU_INT_GAMMA | RU_INT_GAMMA_INVERT | RU_INT_GAMMA_RETAIN;
    bool any_blur = false, any_lowres = false, need[3] = {false, false, false}, any_final = false;
    const int ext[3] = {P0, P1, P2};
    for (int c = 0; c < C; ++c) {
        int m = p->mask[c];
        RU_REQUIRE((m & ~all_bits) == 0, "ru_intensity_augment: channel %d: unknown stage bits 0x%x", c, m);
        if (!(m & RU_INT_GAMMA)) m &= ~(RU_INT_GAMMA_INVERT | RU_INT_GAMMA_RETAIN);      // modifiers of the gamma stage only
        a.mask[c] = lr.mask[c] = m;
        if (m & RU_INT_BLUR) {
            const double sigma = p->blur_sigma[c];
            RU_REQUIRE(sigma > 0.0 && sigma < 1.0e6, "ru_intensity_augment: channel %d: blur sigma must be positive and finite (got %g)", c, sigma);
            const int r = (int)(4.0 * sigma + 0.5);              // scipy: lw = int(truncate * sd + 0.5), truncate = 4
            RU_REQUIRE(r <= IN_R, "ru_intensity_augment: channel %d: radius int(4 sigma + 0.5) = %d exceeds %d", c, r, IN_R);
            double e[IN_TAPS], total = 0.0;
            for (int d = -r; d <= r; ++d) total += (e[d + r] = exp(-0.5 / (sigma * sigma) * (double)(d * d)));
            for (int k = 0; k < IN_TAPS; ++k) a.w[c][k] = (k >= IN_R - r && k <= IN_R + r) ? (float)(e[k - IN_R + r] / total) : 0.f;
            any_blur = true;
        }
        if (m & RU_INT_LOWRES) {
            const double z = p->lowres_zoom[c];
            RU_REQUIRE(z > 0.0 && z <= 1.0, "ru_intensity_augment: channel %d: low-res zoom must lie in (0, 1] (got %g)", c, z);
            for (int ax = 0; ax < 3; ++ax) {
                const int nc = (int)floor(ext[ax] * z + 0.5);
                lr.nc[c][ax] = nc < 1 ? 1 : nc;
            }
            any_lowres = true;
        }
        if (m & RU_INT_NOISE) {
            const double var = p->noise_variance[c];
            RU_REQUIRE(var >= 0.0 && var < 1.0e30, "ru_intensity_augment: channel %d: noise variance must be non-negative and finite (got %g)", c, var);
            a.sd[c] = (float)sqrt(var);
            a.key[c] = in_mix64(p->noise_seed[c] + (unsigned long long)(c + 1) * 0x9E3779B97F4A7C15ull);
        }
        if (m & RU_INT_BRIGHTNESS) {
            RU_REQUIRE(fabs(p->brightness[c]) < 1.0e30, "ru_intensity_augment: channel %d: brightness must be finite", c);
            a.bright[c] = (float)p->brightness[c];
        }
        if (m & RU_INT_CONTRAST) {
            RU_REQUIRE(fabs(p->contrast[c]) < 1.0e30, "ru_intensity_augment: channel %d: contrast must be finite", c);
            a.contrast[c] = (float)p->contrast[c];
            need[0] = true;
        }
        if (m & RU_INT_GAMMA) {
            RU_REQUIRE(p->gamma[c] > 0.0 && p->gamma[c] < 1.0e6, "ru_intensity_augment: channel %d: gamma must be positive and finite (got %g)", c, p->gamma[c]);
            a.gamma[c] = (float)p->gamma[c];
            need[1] = true;
            if (m & RU_INT_GAMMA_RETAIN) need[2] = true;
        }
        if (m != RU_INT_BLUR) any_final = true;
    }
    char* base = (char*)align_up((size_t)ws, 256);
    const size_t tmp_bytes = align_up((size_t)C * V * sizeof(float), 256);
    a.in = in; a.out = out;
    a.tmp_a = (float*)base;
    a.tmp_b = (float*)(base + tmp_bytes);
    IntLrEntry* table = (IntLrEntry*)(base + 2 * tmp_bytes);
    a.table = table;
    a.nblk = int_nblk(V);
    a.partials = (double*)((char*)table + align_up((size_t)C * ((size_t)P0 + P1 + P2) * sizeof(IntLrEntry), 256));
    a.stats = (double*)((char*)a.partials + align_up((size_t)3 * C * a.nblk * 4 * sizeof(double), 256));
    a.C = C; a.P0 = P0; a.P1 = P1; a.P2 = P2; a.V = (unsigned)V;
    a.vec = (P2 % 4 == 0) && (((size_t)in | (size_t)out) % 16 == 0);       // then V % 4 == 0 too: every channel and every W row starts 16-byte aligned
    hipStream_t s = (hipStream_t)stream;
    if (any_blur) {
        const unsigned inner = (unsigned)P1 * P2;
        if (a.vec) hipLaunchKernelGGL(int_blur_d_kernel<float4>, dim3(cdiv((int)(inner / 4), 256), cdiv(P0, IN_TD), C), dim3(256), 0, s, a);
        else hipLaunchKernelGGL(int_blur_d_kernel<float>, dim3(cdiv((int)inner, 256), cdiv(P0, IN_TD), C), dim3(256), 0, s, a);
        RU_CHECK_LAUNCH("int_blur_d_kernel");
        hipLaunchKernelGGL(int_blur_hw_kernel, dim3(cdiv(P1, IN_TH) * cdiv(P2, IN_TW), P0, C), dim3(256), 0, s, a);
        RU_CHECK_LAUNCH("int_blur_hw_kernel");
    }
    if (any_lowres) {
        lr.table = table; lr.P[0] = P0; lr.P[1] = P1; lr.P[2] = P2;
        hipLaunchKernelGGL(int_lowres_table_kernel, dim3(C), dim3(256), 0, s, lr);
        RU_CHECK_LAUNCH("int_lowres_table_kernel");
    }
    for (int level = 0; level < 3; ++level) {
        if (!need[level]) continue;
        hipLaunchKernelGGL(int_pointwise_kernel, dim3(a.nblk, C), dim3(256), 0, s, a, level);
        RU_CHECK_LAUNCH("int_pointwise_kernel");
        hipLaunchKernelGGL(int_stats_final_kernel, dim3(C), dim3(256), 0, s, a, level);
        RU_CHECK_LAUNCH("int_stats_final_kernel");
    }
    if (any_final) {
        hipLaunchKernelGGL(int_pointwise_kernel, dim3(a.nblk, C), dim3(256), 0, s, a, 3);
        RU_CHECK_LAUNCH("int_pointwise_kernel");
    }
    return RU_OK;
}
