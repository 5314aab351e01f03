// Calibration scoring and the per-region threshold search (include/resunet_hip.h, "calibration"): one integer pass over (probability, target)
// that bins the probability, and three small launches that read the tables.
//   calib_histogram_kernel : per (sample, channel) plane hist[k][y], conf[k][y] (sum of the 24-bit fixed-point confidence r), sq[y] (sum of r*r as
//                            {low, high} 32-bit halves) and the invalid count.  Everything is an integer: k = ceil(p * NB) and r = floor(p * 2^24)
//                            are formed from float32 products with a power of two, which are exact, and validity is decided on the bit pattern.
//   calib_accumulate_kernel: pooled tables += the per-sample tables; the Dice / sensitivity / specificity curves at every threshold b / NB from
//                            suffix sums of hist, one float64 division each.
//   calib_summary_kernel   : ECE, MCE, Brier, mean confidence, prevalence and the reliability table from the pooled tables.
//   threshold_kernel       : mask = p > t[c], exact counts (one integer atomic per workgroup and channel, as the merge family's).
// Contention: a trained network puts well over 90 % of a case into the bins 0, 1 and NB with y = 0.  An LDS histogram alone would serialise on
// those addresses, so the three extreme bins of both classes never touch LDS per voxel: every lane keeps their counts and sums in registers
// (selects, no branch), a wave adds them up by shuffles at the end of its walk, and one lane per wave adds them to the table.  Only the voxels of
// the bins 2 .. NB-1 take the two LDS atomics (a 32-bit count, a 64-bit sum), and those spread over the table.  The sums of r*r are per-lane
// registers for every voxel.  The workgroup's table then goes to global memory with one integer atomic per non-empty entry.
// Counter widths: V <= 2^31 per plane, so a lane's or a workgroup's 32-bit count (<= V < 2^32) and 64-bit sums (r <= 2^24: <= 2^55; the low halves
// of r*r: < 2^32 * 2^31 = 2^63) cannot overflow before the single flush at the end of the walk: no flush in between is needed.
// The outputs are cleared by a kernel of the same call (mask_bits.hpp, zero2_kernel: the calls capture into a hipGraph).
#include "ru_common.h"
#include "mask_bits.hpp"
#include "pw_helpers.hpp"

namespace ru {
namespace {

constexpr int CAL_THREADS = 512;                  // 8 waves
constexpr int CAL_TARGET_BLOCKS = 1024;           // ~4 workgroups per CU over all planes
constexpr int CAL_MAX_BLOCKS_PER_PLANE = 512;     // bounds the flush: <= 512 atomics per table entry and plane
constexpr int CAL_SMALL_THREADS = 256;
constexpr unsigned CAL_ONE_BITS = 0x3f800000u;    // 1.0f
constexpr float CAL_R_SCALE = 16777216.f;         // 2^24

// p as its bit pattern: valid iff 0 <= p <= 1 (-0.0 is valid; NaN, negatives, > 1 and infinities are not).  Integer compares, so that a
// subnormal is what it is whatever the denormal mode.
__device__ __forceinline__ bool cal_valid(unsigned u) { return u == 0x80000000u || u <= CAL_ONE_BITS; }
// k = ceil(p * NB) in 0..NB; bin 0 holds exactly p == 0.  p * NB is exact (NB is a power of two), and a product flushed to zero still lands in bin 1.
__device__ __forceinline__ unsigned cal_bin(unsigned u, float nbf) {
    if ((u & 0x7fffffffu) == 0u) return 0u;
    const unsigned k = (unsigned)ceilf(__builtin_bit_cast(float, u) * nbf);
    return k < 1u ? 1u : k;
}
// r = floor(p * 2^24) in 0..2^24: the product is exact
__device__ __forceinline__ unsigned cal_fixed(unsigned u) { return (unsigned)(__builtin_bit_cast(float, u & 0x7fffffffu) * CAL_R_SCALE); }

__device__ __forceinline__ unsigned wave_sum_u32(unsigned v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ u64 wave_sum_u64(u64 v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned lo = __shfl_xor((unsigned)v, o), hi = __shfl_xor((unsigned)(v >> 32), o);
        v += ((u64)hi << 32) | lo;
    }
    return v;
}

// a lane's registers: the three extreme bins of both classes, the sums of r*r, the invalid count
struct CalLane {
    unsigned c0[2], c1[2], cn[2], inv;
    u64 s1[2], sn[2], qlo[2], qhi[2];
};

// one voxel: u = the probability's bits, y = its class, ok = the target is valid
__device__ __forceinline__ void cal_voxel(unsigned u, bool y, bool ok, unsigned NB, float nbf, CalLane& a, unsigned* __restrict__ lh, u64* __restrict__ lc) {
    ok = ok && cal_valid(u);
    const unsigned k = cal_bin(u, nbf), r = cal_fixed(u);
    const u64 r2 = (u64)r * r;
    const unsigned lo = (unsigned)r2, hi = (unsigned)(r2 >> 32);
    a.inv += ok ? 0u : 1u;
#pragma unroll
    for (int yy = 0; yy < 2; ++yy) {
        const bool m = ok && y == (yy == 1);
        const bool m1 = m && k == 1u, mn = m && k == NB;
        a.c0[yy] += (m && k == 0u) ? 1u : 0u;
        a.c1[yy] += m1 ? 1u : 0u;
        a.cn[yy] += mn ? 1u : 0u;
        a.s1[yy] += m1 ? r : 0u;
        a.sn[yy] += mn ? r : 0u;
        a.qlo[yy] += m ? lo : 0u;
        a.qhi[yy] += m ? hi : 0u;
    }
    if (ok && k > 1u && k < NB) {
        const unsigned e = 2u * k + (y ? 1u : 0u);
        atomicAdd(lh + e, 1u);
        atomicAdd(lc + e, (u64)r);
    }
}

// KIND RU_CALIB_TARGET_REGIONS: target float32 [N][C][V].  RU_CALIB_TARGET_LABELS: uint8 [N][V], C = 3.  grid (blocks per plane, N * C).
// A plane's walk is flat_lanes.hpp's: the elements before the first 16-byte boundary of the prediction plane one by one, then quads as 16
// bytes (the target's quad as 16 bytes, or 4 label bytes as one word), then the tail one by one; if the target plane does not sit at the
// same offset from its boundary, everything goes one by one.  Dynamic LDS: lc u64 [2 * (NB + 1)], lq u64 [4], lh u32 [2 * (NB + 1)], linv.
template <int KIND>
__global__ __launch_bounds__(CAL_THREADS) void calib_histogram_kernel(const float* __restrict__ pred, const void* __restrict__ target, int C, size_t V, unsigned NB,
                                                                      u64* __restrict__ hist, u64* __restrict__ conf, u64* __restrict__ sq,
                                                                      u64* __restrict__ invalid) {
    extern __shared__ u64 cal_lds[];
    const unsigned E = 2u * (NB + 1u);
    u64* __restrict__ lc = cal_lds;
    u64* __restrict__ lq = lc + E;
    unsigned* __restrict__ lh = reinterpret_cast<unsigned*>(lq + 4);
    unsigned* __restrict__ linv = lh + E;
    for (unsigned i = threadIdx.x; i < E; i += CAL_THREADS) { lc[i] = 0; lh[i] = 0; }
    if (threadIdx.x < 4) lq[threadIdx.x] = 0;
    if (threadIdx.x == 0) *linv = 0;
    __syncthreads();

    const size_t plane = blockIdx.y, n = plane / (size_t)C;
    const int c = (int)(plane - n * C);
    const float* __restrict__ pp = pred + plane * V;
    const float* __restrict__ gp = KIND == RU_CALIB_TARGET_REGIONS ? static_cast<const float*>(target) + plane * V : nullptr;
    const unsigned char* __restrict__ gl = KIND == RU_CALIB_TARGET_LABELS ? static_cast<const unsigned char*>(target) + n * V : nullptr;
    const float nbf = (float)NB;

    const uintptr_t a0 = (uintptr_t)pp & 15u;
    size_t head = ((16u - a0) & 15u) / 4u;
    if (head > V) head = V;
    const bool alike = KIND == RU_CALIB_TARGET_REGIONS ? ((uintptr_t)gp & 15u) == a0 : ((uintptr_t)(gl + head) & 3u) == 0;
    const size_t nq = alike ? (V - head) / 4 : 0;
    if (!alike) head = V;
    const size_t edge = V - 4 * nq;

    CalLane a = {};
    auto one = [&](size_t i) {
        const unsigned u = __builtin_bit_cast(unsigned, pp[i]);
        if (KIND == RU_CALIB_TARGET_REGIONS) {
            const float g = gp[i];
            cal_voxel(u, g > 0.5f, g == g, NB, nbf, a, lh, lc);
        } else {
            const unsigned v = gl[i];
            cal_voxel(u, brats_region(v, c), v <= 4u, NB, nbf, a, lh, lc);
        }
    };
    const size_t t = (size_t)blockIdx.x * CAL_THREADS + threadIdx.x, T = (size_t)gridDim.x * CAL_THREADS;
    for (size_t q = t; q < nq; q += T) {
        const size_t i = head + 4 * q;
        const uint4 p4 = *reinterpret_cast<const uint4*>(pp + i);
        const unsigned pu[4] = {p4.x, p4.y, p4.z, p4.w};
        if (KIND == RU_CALIB_TARGET_REGIONS) {
            const float4 g4 = *reinterpret_cast<const float4*>(gp + i);
            const float g[4] = {g4.x, g4.y, g4.z, g4.w};
#pragma unroll
            for (int j = 0; j < 4; ++j) cal_voxel(pu[j], g[j] > 0.5f, g[j] == g[j], NB, nbf, a, lh, lc);
        } else {
            const unsigned w = *reinterpret_cast<const unsigned*>(gl + i);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const unsigned v = (w >> (8 * j)) & 0xffu;
                cal_voxel(pu[j], brats_region(v, c), v <= 4u, NB, nbf, a, lh, lc);
            }
        }
    }
    for (size_t e = t; e < edge; e += T) one(e < head ? e : e + 4 * nq);

    // the lanes' registers -> the wave's sums -> the workgroup's table (one lane per wave)
    unsigned inv = wave_sum_u32(a.inv);
#pragma unroll
    for (int yy = 0; yy < 2; ++yy) {
        const unsigned c0 = wave_sum_u32(a.c0[yy]), c1 = wave_sum_u32(a.c1[yy]), cn = wave_sum_u32(a.cn[yy]);
        const u64 s1 = wave_sum_u64(a.s1[yy]), sn = wave_sum_u64(a.sn[yy]), qlo = wave_sum_u64(a.qlo[yy]), qhi = wave_sum_u64(a.qhi[yy]);
        if ((threadIdx.x & 63) == 0) {
            if (c0) atomicAdd(lh + yy, c0);
            if (c1) { atomicAdd(lh + 2 + yy, c1); atomicAdd(lc + 2 + yy, s1); }
            if (cn) { atomicAdd(lh + 2 * NB + yy, cn); atomicAdd(lc + 2 * NB + yy, sn); }
            if (qlo) atomicAdd(lq + 2 * yy, qlo);
            if (qhi) atomicAdd(lq + 2 * yy + 1, qhi);
        }
    }
    if ((threadIdx.x & 63) == 0 && inv) atomicAdd(linv, inv);
    __syncthreads();

    u64* __restrict__ gh = hist + plane * E;
    u64* __restrict__ gc = conf + plane * E;
    for (unsigned i = threadIdx.x; i < E; i += CAL_THREADS) {
        const unsigned h = lh[i];
        const u64 s = lc[i];
        if (h) atomicAdd(gh + i, (u64)h);
        if (s) atomicAdd(gc + i, s);
    }
    if (threadIdx.x < 4 && lq[threadIdx.x]) atomicAdd(sq + plane * 4 + threadIdx.x, lq[threadIdx.x]);
    if (threadIdx.x == 0 && *linv) atomicAdd(invalid + plane, (u64)*linv);
}

__global__ void calib_zero_kernel(u64* __restrict__ hist, u64* __restrict__ conf, size_t ne, u64* __restrict__ sq, size_t nsq, u64* __restrict__ invalid, size_t ninv) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < ne; i += stride) {
        hist[i] = 0;
        conf[i] = 0;
        if (i < nsq) sq[i] = 0;
        if (i < ninv) invalid[i] = 0;
    }
}

// ---------------------------------------------------------------- accumulate: one workgroup per channel, the samples in order
// Pooled tables: pool += the sum over n (integers).  pool_sq is kept carried: {low, high} with low < 2^32, the same S2 = high * 2^32 + low.
// Curves: lane t owns the thresholds b of its contiguous segment.  With P, Q the totals of y = 1, y = 0 and TP_b, FP_b the suffix sums over
// k > b (a lane's suffix = the sum of the segment totals of the lanes above it, added in lane order, then its own bins from the top):
//   Dice_b = (double)(2 TP) / (double)(2 TP + FP + FN), Sens_b = (double)TP / (double)P, Spec_b = (double)TN / (double)Q, 1 for a zero denominator
// -- exact integers, exact conversions below 2^53, one division.  curve_acc[c][j][b] += ((v_0 + v_1) + ...) + v_(N-1), in that order.
__global__ __launch_bounds__(CAL_SMALL_THREADS) void calib_accumulate_kernel(const u64* __restrict__ hist, const u64* __restrict__ conf, const u64* __restrict__ sq, int N,
                                                                             int C, int NB, u64* __restrict__ pool_hist, u64* __restrict__ pool_conf,
                                                                             u64* __restrict__ pool_sq, double* __restrict__ curve_acc,
                                                                             double* __restrict__ curves_out) {
#pragma clang fp contract(off)
    __shared__ u64 part[CAL_SMALL_THREADS][2];
    const int c = blockIdx.x, tid = threadIdx.x, K = NB + 1, E = 2 * K;
    for (int i = tid; i < E; i += CAL_SMALL_THREADS) {
        u64 h = 0, s = 0;
        for (int n = 0; n < N; ++n) {
            h += hist[((size_t)n * C + c) * E + i];
            s += conf[((size_t)n * C + c) * E + i];
        }
        pool_hist[(size_t)c * E + i] += h;
        pool_conf[(size_t)c * E + i] += s;
    }
    if (tid < 2) {
        u64 lo = pool_sq[c * 4 + 2 * tid], hi = pool_sq[c * 4 + 2 * tid + 1];
        for (int n = 0; n < N; ++n) {
            const u64 l = sq[((size_t)n * C + c) * 4 + 2 * tid];
            hi += sq[((size_t)n * C + c) * 4 + 2 * tid + 1] + (l >> 32);
            lo += l & 0xffffffffull;
        }
        pool_sq[c * 4 + 2 * tid] = lo & 0xffffffffull;
        pool_sq[c * 4 + 2 * tid + 1] = hi + (lo >> 32);
    }
    const int per = (K + CAL_SMALL_THREADS - 1) / CAL_SMALL_THREADS;
    const int lo = tid * per < K ? tid * per : K, hi = lo + per < K ? lo + per : K;
    double sum[5][3];                                              // per <= 5 for NB <= 1024
#pragma unroll
    for (int j = 0; j < 5; ++j) sum[j][0] = sum[j][1] = sum[j][2] = 0.0;
    for (int n = 0; n < N; ++n) {
        const u64* __restrict__ h = hist + ((size_t)n * C + c) * E;
        u64 s0 = 0, s1 = 0;
        for (int k = lo; k < hi; ++k) { s0 += h[2 * k]; s1 += h[2 * k + 1]; }
        __syncthreads();
        part[tid][0] = s0;
        part[tid][1] = s1;
        __syncthreads();
        u64 Q = 0, P = 0, fp = 0, tp = 0;
        for (int t = 0; t < CAL_SMALL_THREADS; ++t) {
            Q += part[t][0];
            P += part[t][1];
            if (t > tid) { fp += part[t][0]; tp += part[t][1]; }
        }
        u64 hk0[5], hk1[5];
#pragma unroll
        for (int j = 0; j < 5; ++j) {
            const int k = lo + j;
            hk0[j] = k < hi ? h[2 * k] : 0;
            hk1[j] = k < hi ? h[2 * k + 1] : 0;
        }
#pragma unroll
        for (int j = 4; j >= 0; --j) {                             // from the top of the segment: (tp, fp) = the sums over k > b
            const int b = lo + j;
            if (b < hi) {
                const u64 fn = P - tp, tn = Q - fp, den = 2 * tp + fp + fn;
                const double v[3] = {den ? (double)(2 * tp) / (double)den : 1.0, P ? (double)tp / (double)P : 1.0, Q ? (double)tn / (double)Q : 1.0};
#pragma unroll
                for (int m = 0; m < 3; ++m) {
                    if (curves_out) curves_out[(((size_t)n * C + c) * 3 + m) * K + b] = v[m];
                    sum[j][m] = n == 0 ? v[m] : sum[j][m] + v[m];
                }
                fp += hk0[j];
                tp += hk1[j];
            }
        }
    }
#pragma unroll
    for (int j = 0; j < 5; ++j) {
        const int b = lo + j;
        if (b < hi) {
#pragma unroll
            for (int m = 0; m < 3; ++m) curve_acc[((size_t)c * 3 + m) * K + b] += sum[j][m];
        }
    }
}

// ---------------------------------------------------------------- summary: one workgroup per channel
// Coarse bin m = (max(k, 1) - 1) / (NB / M).  Integers: n_m = n_m(0) + n_m(1), R_m = the sum of r, n = the sum of n_m.  Float64, in this order:
//   conf_m = (double)R_m / ((double)n_m * 2^24), freq_m = (double)n_m(1) / (double)n_m, gap_m = |freq_m - conf_m|, w_m = (double)n_m / (double)n,
//   ECE = ((0 + w_0 * gap_0) + w_1 * gap_1) + ... over the non-empty bins in order of m (product rounded, then the sum), MCE = the largest gap_m,
//   mean confidence = (double)R / ((double)n * 2^24), prevalence = (double)n(1) / (double)n,
//   Brier = T / ((double)n * 2^48) with the exact 128-bit integer T = S2(0) + S2(1) + n(1) * 2^48 - 2^25 * R(1) converted as
//   (double)(T >> 64) * 2^64 + (double)(T & (2^64 - 1)).
// An empty channel gives zeros.  out[c] = {ECE, MCE, Brier, mean confidence, prevalence, n, non-empty coarse bins}; table[c][m] = {n_m, conf_m, freq_m}.
__global__ __launch_bounds__(CAL_SMALL_THREADS) void calib_summary_kernel(const u64* __restrict__ pool_hist, const u64* __restrict__ pool_conf,
                                                                          const u64* __restrict__ pool_sq, int NB, int M, double* __restrict__ out,
                                                                          double* __restrict__ table) {
#pragma clang fp contract(off)
    __shared__ u64 s_n[RU_CALIB_MAX_NB], s_n1[RU_CALIB_MAX_NB], s_r[RU_CALIB_MAX_NB], s_r1[RU_CALIB_MAX_NB];
    const int c = blockIdx.x, K = NB + 1, width = NB / M;
    const u64* __restrict__ h = pool_hist + (size_t)c * 2 * K;
    const u64* __restrict__ s = pool_conf + (size_t)c * 2 * K;
    for (int m = threadIdx.x; m < M; m += CAL_SMALL_THREADS) {
        u64 n0 = 0, n1 = 0, r0 = 0, r1 = 0;
        for (int k = m == 0 ? 0 : m * width + 1; k <= (m + 1) * width; ++k) {
            n0 += h[2 * k]; n1 += h[2 * k + 1];
            r0 += s[2 * k]; r1 += s[2 * k + 1];
        }
        s_n[m] = n0 + n1; s_n1[m] = n1; s_r[m] = r0 + r1; s_r1[m] = r1;
        const u64 nm = n0 + n1;
        double* __restrict__ row = table + ((size_t)c * M + m) * 3;
        row[0] = (double)nm;
        row[1] = nm ? (double)(r0 + r1) / ((double)nm * 16777216.0) : 0.0;
        row[2] = nm ? (double)n1 / (double)nm : 0.0;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    u64 n = 0, n1 = 0, R = 0, R1 = 0;
    for (int m = 0; m < M; ++m) { n += s_n[m]; n1 += s_n1[m]; R += s_r[m]; R1 += s_r1[m]; }
    double ece = 0.0, mce = 0.0, brier = 0.0, meanc = 0.0, prev = 0.0;
    int used = 0;
    if (n) {
        for (int m = 0; m < M; ++m) {
            const u64 nm = s_n[m];
            if (!nm) continue;
            const double cf = (double)s_r[m] / ((double)nm * 16777216.0), fr = (double)s_n1[m] / (double)nm;
            const double gap = fabs(fr - cf), w = (double)nm / (double)n;
            const double term = w * gap;
            ece = ece + term;
            mce = gap > mce ? gap : mce;
            ++used;
        }
        typedef unsigned __int128 u128;
        const u64* __restrict__ q = pool_sq + c * 4;
        const u128 T = (((u128)q[1] << 32) + q[0]) + (((u128)q[3] << 32) + q[2]) + ((u128)n1 << 48) - ((u128)R1 << 25);
        const double num = (double)(u64)(T >> 64) * 18446744073709551616.0 + (double)(u64)T;
        brier = num / ((double)n * 281474976710656.0);
        meanc = (double)R / ((double)n * 16777216.0);
        prev = (double)n1 / (double)n;
    }
    double* __restrict__ o = out + c * 7;
    o[0] = ece; o[1] = mce; o[2] = brier; o[3] = meanc; o[4] = prev; o[5] = (double)n; o[6] = (double)used;
}

// ---------------------------------------------------------------- mask = p > t[c]
struct CalThresholds { float t[RU_CALIB_MAX_C]; };

template <bool VEC4>
__global__ __launch_bounds__(256) void threshold_kernel(const float* __restrict__ p, size_t V, CalThresholds th, unsigned char* __restrict__ mask,
                                                        u64* __restrict__ counts) {
    __shared__ unsigned sm[4];
    const int c = blockIdx.y;
    const float t = th.t[c];
    const float* __restrict__ pc = p + (size_t)c * V;
    unsigned char* __restrict__ mc = mask + (size_t)c * V;
    const size_t stride = (size_t)gridDim.x * 256;
    unsigned local = 0;
    if (VEC4) {
        for (size_t q = (size_t)blockIdx.x * 256 + threadIdx.x; q < V / 4; q += stride) {
            const float4 a = reinterpret_cast<const float4*>(pc)[q];
            const unsigned b0 = a.x > t, b1 = a.y > t, b2 = a.z > t, b3 = a.w > t;
            reinterpret_cast<unsigned*>(mc)[q] = b0 | (b1 << 8) | (b2 << 16) | (b3 << 24);
            local += b0 + b1 + b2 + b3;
        }
    } else {
        for (size_t v = (size_t)blockIdx.x * 256 + threadIdx.x; v < V; v += stride) {
            const unsigned b = pc[v] > t;
            mc[v] = (unsigned char)b;
            local += b;
        }
    }
    wg_count_add(local, sm, counts + c);
}

bool cal_pow2(int v) { return v > 0 && (v & (v - 1)) == 0; }
bool cal_nb_ok(int NB) { return cal_pow2(NB) && NB >= RU_CALIB_MIN_NB && NB <= RU_CALIB_MAX_NB; }

}  // namespace
}  // namespace ru

using namespace ru;

extern "C" int ru_calib_histogram(const float* pred, const void* target, int kind, int N, int C, size_t V, int NB, unsigned long long* hist,
                                  unsigned long long* conf, unsigned long long* sq, unsigned long long* invalid, ru_stream_t stream) {
    RU_REQUIRE(pred && target && hist && conf && sq && invalid, "ru_calib_histogram: null argument");
    RU_REQUIRE(kind == RU_CALIB_TARGET_REGIONS || kind == RU_CALIB_TARGET_LABELS, "ru_calib_histogram: kind %d is neither RU_CALIB_TARGET_REGIONS nor RU_CALIB_TARGET_LABELS", kind);
    RU_REQUIRE(N > 0 && N <= 65535 / RU_CALIB_MAX_C && C >= 1 && C <= RU_CALIB_MAX_C && V > 0 && V <= (1ull << 31),
               "ru_calib_histogram: needs 1 <= N <= %d, 1 <= C <= %d, 1 <= V <= 2^31", 65535 / RU_CALIB_MAX_C, RU_CALIB_MAX_C);
    RU_REQUIRE(kind == RU_CALIB_TARGET_REGIONS || C == 3, "ru_calib_histogram: label targets have C = 3 regions, got %d", C);
    RU_REQUIRE(cal_nb_ok(NB), "ru_calib_histogram: NB = %d is no power of two in %d..%d", NB, RU_CALIB_MIN_NB, RU_CALIB_MAX_NB);
    RU_REQUIRE(((uintptr_t)pred & 3u) == 0 && (kind == RU_CALIB_TARGET_LABELS || ((uintptr_t)target & 3u) == 0), "ru_calib_histogram: float32 tensors must be 4-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    const size_t planes = (size_t)N * C, E = 2 * ((size_t)NB + 1);
    hipLaunchKernelGGL(calib_zero_kernel, dim3(grid1d(planes * E, 256, 1024)), dim3(256), 0, s, hist, conf, planes * E, sq, planes * 4, invalid, planes);
    RU_CHECK_LAUNCH("calib_zero_kernel");
    int want = (CAL_TARGET_BLOCKS + (int)planes - 1) / (int)planes;
    want = want < CAL_MAX_BLOCKS_PER_PLANE ? want : CAL_MAX_BLOCKS_PER_PLANE;
    const unsigned bx = grid1d((V + 3) / 4 + 3, CAL_THREADS, (unsigned)want);
    const size_t lds = (E + 4) * 8 + (E + 2) * 4;
    if (kind == RU_CALIB_TARGET_REGIONS)
        hipLaunchKernelGGL(calib_histogram_kernel<RU_CALIB_TARGET_REGIONS>, dim3(bx, (unsigned)planes), dim3(CAL_THREADS), lds, s, pred, target, C, V, (unsigned)NB, hist,
                           conf, sq, invalid);
    else
        hipLaunchKernelGGL(calib_histogram_kernel<RU_CALIB_TARGET_LABELS>, dim3(bx, (unsigned)planes), dim3(CAL_THREADS), lds, s, pred, target, C, V, (unsigned)NB, hist,
                           conf, sq, invalid);
    RU_CHECK_LAUNCH("calib_histogram_kernel");
    return RU_OK;
}

extern "C" int ru_calib_accumulate(const unsigned long long* hist, const unsigned long long* conf, const unsigned long long* sq, int N, int C, int NB,
                                   unsigned long long* pool_hist, unsigned long long* pool_conf, unsigned long long* pool_sq, double* curve_acc,
                                   double* curves_out, ru_stream_t stream) {
    RU_REQUIRE(hist && conf && sq && pool_hist && pool_conf && pool_sq && curve_acc, "ru_calib_accumulate: null argument");
    RU_REQUIRE(N > 0 && C >= 1 && C <= RU_CALIB_MAX_C && cal_nb_ok(NB), "ru_calib_accumulate: needs N >= 1, 1 <= C <= %d and NB a power of two in %d..%d",
               RU_CALIB_MAX_C, RU_CALIB_MIN_NB, RU_CALIB_MAX_NB);
    hipLaunchKernelGGL(calib_accumulate_kernel, dim3(C), dim3(CAL_SMALL_THREADS), 0, (hipStream_t)stream, hist, conf, sq, N, C, NB, pool_hist, pool_conf, pool_sq, curve_acc,
                       curves_out);
    RU_CHECK_LAUNCH("calib_accumulate_kernel");
    return RU_OK;
}

extern "C" int ru_calib_summary(const unsigned long long* pool_hist, const unsigned long long* pool_conf, const unsigned long long* pool_sq, int C, int NB, int M,
                                double* out, double* table, ru_stream_t stream) {
    RU_REQUIRE(pool_hist && pool_conf && pool_sq && out && table, "ru_calib_summary: null argument");
    RU_REQUIRE(C >= 1 && C <= RU_CALIB_MAX_C && cal_nb_ok(NB), "ru_calib_summary: needs 1 <= C <= %d and NB a power of two in %d..%d", RU_CALIB_MAX_C, RU_CALIB_MIN_NB,
               RU_CALIB_MAX_NB);
    RU_REQUIRE(M >= 1 && M <= NB && NB % M == 0, "ru_calib_summary: M = %d coarse bins must divide NB = %d", M, NB);
    hipLaunchKernelGGL(calib_summary_kernel, dim3(C), dim3(CAL_SMALL_THREADS), 0, (hipStream_t)stream, pool_hist, pool_conf, pool_sq, NB, M, out, table);
    RU_CHECK_LAUNCH("calib_summary_kernel");
    return RU_OK;
}

extern "C" int ru_threshold_regions(const float* probs, int C, size_t V, const float* thresholds, unsigned char* mask, unsigned long long* counts,
                                    ru_stream_t stream) {
    RU_REQUIRE(probs && thresholds && mask && counts, "ru_threshold_regions: null argument");
    RU_REQUIRE(C >= 1 && C <= RU_CALIB_MAX_C && V > 0 && V < (1ull << 32), "ru_threshold_regions: needs 1 <= C <= %d and 1 <= V < 2^32", RU_CALIB_MAX_C);
    CalThresholds th = {};
    for (int c = 0; c < C; ++c) {
        RU_REQUIRE(thresholds[c] == thresholds[c], "ru_threshold_regions: threshold %d is NaN", c);
        th.t[c] = thresholds[c];
    }
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL((zero2_kernel<u64, u64>), dim3(1), dim3(64), 0, s, counts, (size_t)C, (u64*)nullptr, (size_t)0);
    RU_CHECK_LAUNCH("zero2_kernel");
    const bool vec = V % 4 == 0 && ((uintptr_t)probs & 15u) == 0 && ((uintptr_t)mask & 3u) == 0;
    if (vec) hipLaunchKernelGGL(threshold_kernel<true>, dim3(grid1d(V / 4, 256, 1024), C), dim3(256), 0, s, probs, V, th, mask, counts);
    else hipLaunchKernelGGL(threshold_kernel<false>, dim3(grid1d(V, 256, 1024), C), dim3(256), 0, s, probs, V, th, mask, counts);
    RU_CHECK_LAUNCH("threshold_kernel");
    return RU_OK;
}
