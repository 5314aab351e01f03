// uncertainty.hip -- the third BraTS 2019 task, quantification of uncertainty in segmentation, on the device: per case three uint8 maps
// (whole tumour, tumour core, enhancing tumour; 0 = certain .. 100 = uncertain) made from the M models x K flips an ensemble predicts
// anyway (ensemble.hip), and the challenge's score of such maps.
//
//   unc_accumulate_kernel  : ens_accumulate_kernel plus the second-moment sum acc2, in the SAME pass over the predictions
//                            (ru_unc_accumulate); its FINAL form also forms mean / mask / counts and the map (ru_unc_accumulate_finalize)
//   unc_finalize_kernel    : the same finalize from stored sums (ru_unc_finalize: saved predictions, tests)
//   unc_histogram_kernel   : one pass over (prediction labels, target labels, three maps) -> exact counts hist[region][map value][TP FP FN TN]
//   unc_score_kernel       : cumulative sums over the map value, the filtered Dice / FTP / FTN curves, their AUCs and the score, float64
//   paste_u8c_kernel       : the maps in the case's own frame (ru_paste_u8c)
//
// The arithmetic is fixed so that a map can be compared with numpy exactly:
//   mean      as ensemble.hip: p_m = (((o0 + o1) + o2) + o3) / K, S_m = S_(m-1) + p_m, mean = S_M / (float)M
//   moment    q_m = ((o0*o0 + o1*o1) + o2*o2) + o3*o3, T_1 = q_1, T_m = T_(m-1) + q_m: float32, every product and sum rounded (no fma)
//   std       e2 = (double)T_M / (double)(M*K), mu = (double)mean, var = max(e2 - mu*mu, 0), u = floor(min(200*sqrt(var), 100) + 0.5)
//   entropy   H = -(mu*log2(mu) + (1-mu)*log2(1-mu)), a term is 0 unless its argument lies inside (0, 1); u = floor(100*H + 0.5)
// Contraction is switched off where these are formed.  All passes are HBM streams: 256-thread workgroups, a lane takes 4 consecutive
// voxels of the box (16-byte loads and stores; the hardware takes them at dword alignment, which a box row at an odd offset needs).
#include "ru_common.h"
#include "pw_helpers.hpp"
#include "mask_bits.hpp"

#include <limits.h>

namespace ru {
namespace {

typedef float unc_f4 __attribute__((ext_vector_type(4), aligned(4)));      // 4 floats at dword alignment: one global_load/store_dwordx4

constexpr int UNC_REGIONS = 3, UNC_LEVELS = 101, UNC_CLASSES = 4;
constexpr int UNC_BINS = UNC_REGIONS * UNC_LEVELS * UNC_CLASSES;
constexpr int UNC_HIST_THREADS = 256, UNC_HIST_WAVES = UNC_HIST_THREADS / 64;
constexpr int UNC_HIST_MAX_BLOCKS = 512;                                   // bounds the same-address atomics: <= 512 per bin
constexpr int UNC_MAX_THRESHOLDS = 101;
// labels of the three regions as bit sets over the label value: WT = {1,2,3,4}, TC = {1,3,4}, ET = {3,4} (mask_bits.hpp, brats_region)
constexpr unsigned UNC_REGION_BITS[UNC_REGIONS] = {0x1eu, 0x1au, 0x18u};

struct UncThresholds { int t[UNC_MAX_THRESHOLDS]; };

__device__ __forceinline__ unsigned unc_std_value(float T, float mean, double MK) {
#pragma clang fp contract(off)
    const double e2 = (double)T / MK, mu = (double)mean;
    double var = e2 - mu * mu;
    var = var > 0.0 ? var : 0.0;
    double u = 200.0 * __builtin_sqrt(var);
    u = u < 100.0 ? u : 100.0;
    return (unsigned)__builtin_floor(u + 0.5);
}

__device__ __forceinline__ unsigned unc_entropy_value(float mean) {
#pragma clang fp contract(off)
    const double mu = (double)mean, nu = 1.0 - mu;
    const double a = mu > 0.0 && mu < 1.0 ? mu * log2(mu) : 0.0;
    const double b = nu > 0.0 && nu < 1.0 ? nu * log2(nu) : 0.0;
    const double h = -(a + b);
    const double u = __builtin_floor(100.0 * h + 0.5);
    return (unsigned)(u < 100.0 ? u : 100.0);
}

__device__ __forceinline__ unsigned unc_value(int measure, float T, float mean, double MK) {
    return measure == RU_UNC_STD ? unc_std_value(T, mean, MK) : unc_entropy_value(mean);
}

// 4 bytes at p: one dword store where p allows it (a channel of an odd box starts at any byte)
__device__ __forceinline__ void unc_store_u8x4(unsigned char* p, const unsigned (&b)[4]) {
    if (((uintptr_t)p & 3) == 0) {
        *reinterpret_cast<unsigned*>(p) = b[0] | (b[1] << 8) | (b[2] << 16) | (b[3] << 24);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) p[j] = (unsigned char)b[j];
    }
}

// One streaming pass per model; a lane takes the box voxels v .. v+3 of channel blockIdx.y.  S, mean as ens_accumulate_kernel<FIRST, FINAL>;
// T = FIRST ? q_m : acc2 + q_m.  !FINAL: acc = S, acc2 = T.  FINAL: mean_out / mask / counts / unc from (S, T); acc, acc2 are not written,
// and with the entropy measure acc2 is not read either.
template <bool FIRST, bool FINAL>
__global__ __launch_bounds__(256) void unc_accumulate_kernel(const float* __restrict__ p, int K, unsigned flips, float* __restrict__ acc, float* __restrict__ acc2,
                                                             float M, double MK, int measure, float* __restrict__ mean_out, unsigned char* __restrict__ mask,
                                                             unsigned long long* __restrict__ counts, unsigned char* __restrict__ unc, int C, int D, int H, int W,
                                                             Box3 b) {
#pragma clang fp contract(off)
    __shared__ unsigned sm[4];
    const unsigned sx = (unsigned)b.size[2], sy = (unsigned)b.size[1];
    const unsigned Vb = (unsigned)b.size[0] * sy * sx, n4 = (Vb + 3u) >> 2;
    const int c = blockIdx.y;
    const size_t HW = (size_t)H * W, DHW = (size_t)D * HW, cb = (size_t)c * Vb;
    const bool moment = !FINAL || measure == RU_UNC_STD;
    unsigned local = 0;
    for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < n4; i += gridDim.x * 256u) {
        const unsigned v = i << 2, n = Vb - v < 4u ? Vb - v : 4u;
        const unsigned r = v / sx, x0 = v - r * sx;
        const bool row = n == 4u && x0 + 3u < sx;                      // the four voxels lie in one box row: one 16-byte load per copy
        float s[4], q[4];
        for (int k = 0; k < K; ++k) {
            const unsigned f = (flips >> (3 * k)) & 7u;
            const float* pk = p + ((size_t)k * C + c) * DHW;
            float t[4] = {0.f, 0.f, 0.f, 0.f};
            if (row) {
                const unsigned zq = r / sy;
                const int x = (int)x0 + b.lo[2], y = (int)(r - zq * sy) + b.lo[1], z = (int)zq + b.lo[0];
                const int zz = (f & 1u) ? D - 1 - z : z, yy = (f & 2u) ? H - 1 - y : y;
                const float* line = pk + (size_t)zz * HW + (size_t)yy * W;
                if (f & 4u) {                                          // an x-flipped row is read backwards: the same 16 bytes, reversed
                    const unc_f4 a = *reinterpret_cast<const unc_f4*>(line + (W - 1 - x - 3));
                    t[0] = a.w; t[1] = a.z; t[2] = a.y; t[3] = a.x;
                } else {
                    const unc_f4 a = *reinterpret_cast<const unc_f4*>(line + x);
                    t[0] = a.x; t[1] = a.y; t[2] = a.z; t[3] = a.w;
                }
            } else {
                for (unsigned j = 0; j < n; ++j) {
                    const unsigned rj = (v + j) / sx, zq = rj / sy;
                    const int x = (int)(v + j - rj * sx) + b.lo[2], y = (int)(rj - zq * sy) + b.lo[1], z = (int)zq + b.lo[0];
                    const int zz = (f & 1u) ? D - 1 - z : z, yy = (f & 2u) ? H - 1 - y : y, xx = (f & 4u) ? W - 1 - x : x;
                    t[j] = pk[(size_t)zz * HW + (size_t)yy * W + xx];
                }
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float tt = t[j] * t[j];
                s[j] = k == 0 ? t[j] : s[j] + t[j];
                q[j] = k == 0 ? tt : q[j] + tt;
            }
        }
        float S[4], T[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) { S[j] = s[j] / (float)K; T[j] = q[j]; }
        if (!FIRST) {
            if (n == 4u) {
                const unc_f4 a = *reinterpret_cast<const unc_f4*>(acc + cb + v);
                S[0] = a.x + S[0]; S[1] = a.y + S[1]; S[2] = a.z + S[2]; S[3] = a.w + S[3];
                if (moment) {
                    const unc_f4 a2 = *reinterpret_cast<const unc_f4*>(acc2 + cb + v);
                    T[0] = a2.x + T[0]; T[1] = a2.y + T[1]; T[2] = a2.z + T[2]; T[3] = a2.w + T[3];
                }
            } else {
                for (unsigned j = 0; j < n; ++j) {
                    S[j] = acc[cb + v + j] + S[j];
                    if (moment) T[j] = acc2[cb + v + j] + T[j];
                }
            }
        }
        if (!FINAL) {
            if (n == 4u) {
                unc_f4 o, o2;
                o.x = S[0]; o.y = S[1]; o.z = S[2]; o.w = S[3];
                o2.x = T[0]; o2.y = T[1]; o2.z = T[2]; o2.w = T[3];
                *reinterpret_cast<unc_f4*>(acc + cb + v) = o;
                *reinterpret_cast<unc_f4*>(acc2 + cb + v) = o2;
            } else {
                for (unsigned j = 0; j < n; ++j) { acc[cb + v + j] = S[j]; acc2[cb + v + j] = T[j]; }
            }
        } else {
            float m[4];
            unsigned on[4], u[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                m[j] = S[j] / M;
                on[j] = m[j] > 0.5f ? 1u : 0u;
                u[j] = (unsigned)j < n ? unc_value(measure, T[j], m[j], MK) : 0u;
                local += (unsigned)j < n ? on[j] : 0u;
            }
            if (n == 4u) {
                if (mean_out) {
                    unc_f4 o;
                    o.x = m[0]; o.y = m[1]; o.z = m[2]; o.w = m[3];
                    *reinterpret_cast<unc_f4*>(mean_out + cb + v) = o;
                }
                unc_store_u8x4(mask + cb + v, on);
                unc_store_u8x4(unc + cb + v, u);
            } else {
                for (unsigned j = 0; j < n; ++j) {
                    if (mean_out) mean_out[cb + v + j] = m[j];
                    mask[cb + v + j] = (unsigned char)on[j];
                    unc[cb + v + j] = (unsigned char)u[j];
                }
            }
        }
    }
    if (FINAL) wg_count_add(local, sm, counts + c);
}

// stored sums -> mean = S_M / (float)M, mask, counts and the map; acc2 may be null with the entropy measure
__global__ __launch_bounds__(256) void unc_finalize_kernel(const float* __restrict__ acc, const float* __restrict__ acc2, float M, double MK, int measure,
                                                           float* __restrict__ mean_out, unsigned char* __restrict__ mask,
                                                           unsigned long long* __restrict__ counts, unsigned char* __restrict__ unc, unsigned Vb) {
    __shared__ unsigned sm[4];
    const int c = blockIdx.y;
    const size_t cb = (size_t)c * Vb;
    const unsigned n4 = (Vb + 3u) >> 2;
    const bool moment = measure == RU_UNC_STD;
    unsigned local = 0;
    for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < n4; i += gridDim.x * 256u) {
        const unsigned v = i << 2, n = Vb - v < 4u ? Vb - v : 4u;
        float S[4] = {0.f, 0.f, 0.f, 0.f}, T[4] = {0.f, 0.f, 0.f, 0.f};
        if (n == 4u) {
            const unc_f4 a = *reinterpret_cast<const unc_f4*>(acc + cb + v);
            S[0] = a.x; S[1] = a.y; S[2] = a.z; S[3] = a.w;
            if (moment) {
                const unc_f4 a2 = *reinterpret_cast<const unc_f4*>(acc2 + cb + v);
                T[0] = a2.x; T[1] = a2.y; T[2] = a2.z; T[3] = a2.w;
            }
        } else {
            for (unsigned j = 0; j < n; ++j) {
                S[j] = acc[cb + v + j];
                if (moment) T[j] = acc2[cb + v + j];
            }
        }
        float m[4];
        unsigned on[4], u[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            m[j] = S[j] / M;
            on[j] = m[j] > 0.5f ? 1u : 0u;
            u[j] = (unsigned)j < n ? unc_value(measure, T[j], m[j], MK) : 0u;
            local += (unsigned)j < n ? on[j] : 0u;
        }
        if (n == 4u) {
            if (mean_out) {
                unc_f4 o;
                o.x = m[0]; o.y = m[1]; o.z = m[2]; o.w = m[3];
                *reinterpret_cast<unc_f4*>(mean_out + cb + v) = o;
            }
            unc_store_u8x4(mask + cb + v, on);
            unc_store_u8x4(unc + cb + v, u);
        } else {
            for (unsigned j = 0; j < n; ++j) {
                if (mean_out) mean_out[cb + v + j] = m[j];
                mask[cb + v + j] = (unsigned char)on[j];
                unc[cb + v + j] = (unsigned char)u[j];
            }
        }
    }
    wg_count_add(local, sm, counts + c);
}

// ---------------------------------------------------------------- the score: histogram pass
// A voxel with a label outside 0..4 or a map value above 100 is counted in `invalid` and in no bin.  Counters per wave in LDS; the cell
// nearly every voxel lands in -- background on both sides, map value 0: (TN, level 0) of all three regions -- is counted in registers.
struct UncHistLocal { unsigned tn0[UNC_REGIONS], bad; };

__device__ __forceinline__ void unc_hist_voxel(unsigned a, unsigned g, unsigned u0, unsigned u1, unsigned u2, unsigned* __restrict__ sw, UncHistLocal& l) {
    if (a > 4u || g > 4u || u0 > 100u || u1 > 100u || u2 > 100u) { ++l.bad; return; }
    const unsigned u[UNC_REGIONS] = {u0, u1, u2};
#pragma unroll
    for (int r = 0; r < UNC_REGIONS; ++r) {
        const unsigned cls = 3u - 2u * ((UNC_REGION_BITS[r] >> a) & 1u) - ((UNC_REGION_BITS[r] >> g) & 1u);     // TP 0, FP 1, FN 2, TN 3
        if (cls == 3u && u[r] == 0u) ++l.tn0[r];
        else atomicAdd(&sw[(r * UNC_LEVELS + u[r]) * UNC_CLASSES + cls], 1u);
    }
}

template <bool VEC>
__global__ __launch_bounds__(UNC_HIST_THREADS) void unc_histogram_kernel(const unsigned char* __restrict__ p, const unsigned char* __restrict__ g,
                                                                         const unsigned char* __restrict__ unc, size_t V,
                                                                         unsigned long long* __restrict__ hist, unsigned long long* __restrict__ invalid) {
    __shared__ unsigned s[UNC_HIST_WAVES][UNC_BINS + 1];               // [.][UNC_BINS]: the wave's invalid voxels
    for (int i = threadIdx.x; i < UNC_HIST_WAVES * (UNC_BINS + 1); i += UNC_HIST_THREADS) (&s[0][0])[i] = 0;
    __syncthreads();
    unsigned* sw = s[threadIdx.x >> 6];
    UncHistLocal l = {{0, 0, 0}, 0};
    const size_t stride = (size_t)gridDim.x * UNC_HIST_THREADS, first = (size_t)blockIdx.x * UNC_HIST_THREADS + threadIdx.x;
    if (VEC) {                                                         // V % 16 == 0 and 16-byte aligned bases: 16 voxels per lane and step
        const size_t V16 = V >> 4;
        for (size_t i = first; i < V16; i += stride) {
            const uint4 a = reinterpret_cast<const uint4*>(p)[i], b = reinterpret_cast<const uint4*>(g)[i];
            const uint4 u0 = reinterpret_cast<const uint4*>(unc)[i], u1 = reinterpret_cast<const uint4*>(unc + V)[i],
                        u2 = reinterpret_cast<const uint4*>(unc + 2 * V)[i];
            const unsigned aw[4] = {a.x, a.y, a.z, a.w}, bw[4] = {b.x, b.y, b.z, b.w};
            const unsigned w0[4] = {u0.x, u0.y, u0.z, u0.w}, w1[4] = {u1.x, u1.y, u1.z, u1.w}, w2[4] = {u2.x, u2.y, u2.z, u2.w};
#pragma unroll
            for (int d = 0; d < 4; ++d) {
                if ((aw[d] | bw[d] | w0[d] | w1[d] | w2[d]) == 0u) {   // four background voxels with zero maps
#pragma unroll
                    for (int r = 0; r < UNC_REGIONS; ++r) l.tn0[r] += 4u;
                    continue;
                }
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int sh = 8 * e;
                    unc_hist_voxel((aw[d] >> sh) & 0xffu, (bw[d] >> sh) & 0xffu, (w0[d] >> sh) & 0xffu, (w1[d] >> sh) & 0xffu, (w2[d] >> sh) & 0xffu, sw, l);
                }
            }
        }
    } else {
        for (size_t v = first; v < V; v += stride) unc_hist_voxel(p[v], g[v], unc[v], unc[V + v], unc[2 * V + v], sw, l);
    }
    // the register counters: wave sums, one LDS add per wave and cell
#pragma unroll
    for (int r = 0; r <= UNC_REGIONS; ++r) {
        unsigned t = r < UNC_REGIONS ? l.tn0[r] : l.bad;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) t += __shfl_xor(t, o);
        if ((threadIdx.x & 63) == 0 && t) atomicAdd(&sw[r < UNC_REGIONS ? (r * UNC_LEVELS) * UNC_CLASSES + 3 : UNC_BINS], t);
    }
    __syncthreads();
    for (int i = threadIdx.x; i <= UNC_BINS; i += UNC_HIST_THREADS) {
        unsigned long long t = 0;
#pragma unroll
        for (int w = 0; w < UNC_HIST_WAVES; ++w) t += s[w][i];
        if (t) atomicAdd(i < UNC_BINS ? hist + i : invalid, t);
    }
}

// ---------------------------------------------------------------- the score: curves and AUCs, one thread per region
// At threshold t the voxels with a map value above t are filtered out: the counts are the histogram's sums over the levels 0..t.
// Dice_t = 2TP / (2TP + FP + FN), 1 for an empty denominator; FTP_t = (TP_100 - TP_t) / TP_100, 0 for TP_100 = 0; FTN_t likewise.
// AUC = trapezoid rule over the thresholds / (t_last - t_first); with a single threshold it is the curve's value there.
__global__ void unc_score_kernel(const unsigned long long* __restrict__ hist, UncThresholds th, int T, double* __restrict__ out, double* __restrict__ acc) {
    const int r = threadIdx.x;
    if (r >= UNC_REGIONS) return;
    const unsigned long long* h = hist + (size_t)r * UNC_LEVELS * UNC_CLASSES;
    unsigned long long tp100 = 0, tn100 = 0;
    for (int u = 0; u < UNC_LEVELS; ++u) { tp100 += h[u * UNC_CLASSES + 0]; tn100 += h[u * UNC_CLASSES + 3]; }
    unsigned long long cum[UNC_CLASSES] = {0, 0, 0, 0};
    int level = 0;
    double prev[3] = {0.0, 0.0, 0.0}, auc[3] = {0.0, 0.0, 0.0};
    for (int i = 0; i < T; ++i) {
        for (; level <= th.t[i]; ++level) {
#pragma unroll
            for (int k = 0; k < UNC_CLASSES; ++k) cum[k] += h[level * UNC_CLASSES + k];
        }
        const unsigned long long den = 2 * cum[0] + cum[1] + cum[2];
        double cur[3];
        cur[0] = den ? (double)(2 * cum[0]) / (double)den : 1.0;
        cur[1] = tp100 ? (double)(tp100 - cum[0]) / (double)tp100 : 0.0;
        cur[2] = tn100 ? (double)(tn100 - cum[3]) / (double)tn100 : 0.0;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            if (i > 0) auc[k] += (double)(th.t[i] - th.t[i - 1]) * (prev[k] + cur[k]) / 2.0;
            prev[k] = cur[k];
        }
    }
    const int span = th.t[T - 1] - th.t[0];
#pragma unroll
    for (int k = 0; k < 3; ++k) auc[k] = span > 0 ? auc[k] / (double)span : prev[k];
    const double res[4] = {(auc[0] + (1.0 - auc[1]) + (1.0 - auc[2])) / 3.0, auc[0], auc[1], auc[2]};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        out[r * 4 + k] = res[k];
        if (acc) acc[r * 4 + k] += res[k];
    }
}

// full[c][D][H][W] = 0 except the box, which takes src[c][size].  VEC4 (W % 4 == 0, full 4-byte aligned): 4 voxels of a row per lane, one dword store.
template <bool VEC4>
__global__ __launch_bounds__(256) void paste_u8c_kernel(const unsigned char* __restrict__ src, unsigned char* __restrict__ full, int D, int H, int W, Box3 b) {
    const unsigned V = (unsigned)D * H * W, Vb = (unsigned)b.size[0] * b.size[1] * b.size[2];
    const int c = blockIdx.y;
    const unsigned char* s = src + (size_t)c * Vb;
    unsigned char* dst = full + (size_t)c * V;
    constexpr unsigned PER = VEC4 ? 4u : 1u;
    const unsigned n = V / PER;
    for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < n; i += gridDim.x * 256u) {
        const unsigned v = i * PER, r = v / (unsigned)W, zq = r / (unsigned)H;
        const int x0 = (int)(v - r * (unsigned)W) - b.lo[2], y = (int)(r - zq * (unsigned)H) - b.lo[1], z = (int)zq - b.lo[0];
        const bool line = z >= 0 && z < b.size[0] && y >= 0 && y < b.size[1];
        const unsigned char* srow = s + ((size_t)(line ? z : 0) * b.size[1] + (line ? y : 0)) * b.size[2];
        unsigned o = 0;
#pragma unroll
        for (unsigned j = 0; j < PER; ++j) {
            const int x = x0 + (int)j;
            if (line && x >= 0 && x < b.size[2]) o |= (unsigned)srow[x] << (8 * j);
        }
        if (VEC4) reinterpret_cast<unsigned*>(dst)[i] = o;
        else dst[v] = (unsigned char)o;
    }
}

int unc_accumulate_impl(const float* probs, int K, unsigned flips, float* acc, float* acc2, int first, int M, int measure, float* mean_out, unsigned char* mask,
                        unsigned long long* counts, unsigned char* unc, int C, int D, int H, int W, const int* lo, const int* size, hipStream_t s,
                        const char* who) {
    RU_REQUIRE(probs && lo && size && K >= 1 && K <= 8 && C >= 1 && C <= 65535, "%s: bad argument", who);
    RU_REQUIRE((size_t)D * H * W < (size_t)INT_MAX, "%s: volume too large for 32-bit voxel indices", who);
    Box3 b;
    int rc = make_box(b, lo, size, D, H, W, who);
    if (rc) return rc;
    const dim3 grid(grid1d(((size_t)size[0] * size[1] * size[2] + 3) / 4, 256 * 2, 2048), (unsigned)C), block(256);
    const double MK = (double)M * (double)K;
    if (M > 0) {
        hipLaunchKernelGGL((zero2_kernel<u64, u64>), dim3(cdiv(C, 256)), dim3(256), 0, s, counts, (size_t)C, (u64*)nullptr, (size_t)0);
        RU_CHECK_LAUNCH("zero2_kernel");
        if (first) hipLaunchKernelGGL((unc_accumulate_kernel<true, true>), grid, block, 0, s, probs, K, flips, acc, acc2, (float)M, MK, measure, mean_out, mask, counts, unc, C, D, H, W, b);
        else hipLaunchKernelGGL((unc_accumulate_kernel<false, true>), grid, block, 0, s, probs, K, flips, acc, acc2, (float)M, MK, measure, mean_out, mask, counts, unc, C, D, H, W, b);
    } else {
        if (first) hipLaunchKernelGGL((unc_accumulate_kernel<true, false>), grid, block, 0, s, probs, K, flips, acc, acc2, 1.f, MK, measure, mean_out, mask, counts, unc, C, D, H, W, b);
        else hipLaunchKernelGGL((unc_accumulate_kernel<false, false>), grid, block, 0, s, probs, K, flips, acc, acc2, 1.f, MK, measure, mean_out, mask, counts, unc, C, D, H, W, b);
    }
    RU_CHECK_LAUNCH("unc_accumulate_kernel");
    return RU_OK;
}

bool unc_measure_ok(int measure) { return measure == RU_UNC_STD || measure == RU_UNC_ENTROPY; }

}  // namespace
}  // namespace ru

using namespace ru;

extern "C" int ru_unc_accumulate(const float* probs, int K, unsigned flips, float* acc, float* acc2, int first, int C, int D, int H, int W, const int* lo,
                                 const int* size, ru_stream_t stream) {
    RU_REQUIRE(acc && acc2, "ru_unc_accumulate: null argument");
    return unc_accumulate_impl(probs, K, flips, acc, acc2, first, 0, RU_UNC_STD, nullptr, nullptr, nullptr, nullptr, C, D, H, W, lo, size, (hipStream_t)stream,
                               "ru_unc_accumulate");
}

extern "C" int ru_unc_accumulate_finalize(const float* probs, int K, unsigned flips, const float* acc, const float* acc2, int first, int M, int measure,
                                          float* mean_out, unsigned char* mask, unsigned long long* counts, unsigned char* unc, int C, int D, int H, int W,
                                          const int* lo, const int* size, ru_stream_t stream) {
    RU_REQUIRE(mask && counts && unc && M >= 1, "ru_unc_accumulate_finalize: bad argument");
    RU_REQUIRE(unc_measure_ok(measure), "ru_unc_accumulate_finalize: measure %d is neither RU_UNC_STD nor RU_UNC_ENTROPY", measure);
    RU_REQUIRE(first || (acc && (acc2 || measure == RU_UNC_ENTROPY)), "ru_unc_accumulate_finalize: the running sums are needed unless the only model is merged at once");
    return unc_accumulate_impl(probs, K, flips, const_cast<float*>(acc), const_cast<float*>(acc2), first, M, measure, mean_out, mask, counts, unc, C, D, H, W, lo, size,
                               (hipStream_t)stream, "ru_unc_accumulate_finalize");
}

extern "C" int ru_unc_finalize(const float* acc, const float* acc2, int M, int K, int measure, float* mean_out, unsigned char* mask, unsigned long long* counts,
                               unsigned char* unc, int C, size_t Vbox, ru_stream_t stream) {
    RU_REQUIRE(acc && mask && counts && unc && M >= 1 && K >= 1 && C >= 1 && C <= 65535 && Vbox > 0, "ru_unc_finalize: bad argument");
    RU_REQUIRE(unc_measure_ok(measure), "ru_unc_finalize: measure %d is neither RU_UNC_STD nor RU_UNC_ENTROPY", measure);
    RU_REQUIRE(acc2 || measure == RU_UNC_ENTROPY, "ru_unc_finalize: RU_UNC_STD needs the second-moment sum");
    RU_REQUIRE(Vbox < (size_t)INT_MAX, "ru_unc_finalize: volume too large for 32-bit voxel indices");
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL((zero2_kernel<u64, u64>), dim3(cdiv(C, 256)), dim3(256), 0, s, counts, (size_t)C, (u64*)nullptr, (size_t)0);
    RU_CHECK_LAUNCH("zero2_kernel");
    hipLaunchKernelGGL(unc_finalize_kernel, dim3(grid1d((Vbox + 3) / 4, 256 * 2, 2048), (unsigned)C), dim3(256), 0, s, acc, acc2, (float)M, (double)M * (double)K,
                       measure, mean_out, mask, counts, unc, (unsigned)Vbox);
    RU_CHECK_LAUNCH("unc_finalize_kernel");
    return RU_OK;
}

extern "C" int ru_unc_histogram(const unsigned char* pred, const unsigned char* target, const unsigned char* unc, int D, int H, int W, unsigned long long* hist,
                                unsigned long long* invalid, ru_stream_t stream) {
    RU_REQUIRE(pred && target && unc && hist && invalid && D > 0 && H > 0 && W > 0, "ru_unc_histogram: bad argument");
    const size_t V = (size_t)D * H * W;
    RU_REQUIRE(V < (1ull << 32), "ru_unc_histogram: volume too large for 32-bit counters per workgroup");
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL((zero2_kernel<u64, u64>), dim3(cdiv(UNC_BINS + 1, 256)), dim3(256), 0, s, hist, (size_t)UNC_BINS, invalid, (size_t)1);
    RU_CHECK_LAUNCH("zero2_kernel");
    const bool vec = V % 16 == 0 && (((uintptr_t)pred | (uintptr_t)target | (uintptr_t)unc) & 15) == 0;
    if (vec) hipLaunchKernelGGL(unc_histogram_kernel<true>, dim3(grid1d(V / 16, UNC_HIST_THREADS, UNC_HIST_MAX_BLOCKS)), dim3(UNC_HIST_THREADS), 0, s, pred, target,
                                unc, V, hist, invalid);
    else hipLaunchKernelGGL(unc_histogram_kernel<false>, dim3(grid1d(V, UNC_HIST_THREADS * 4, UNC_HIST_MAX_BLOCKS)), dim3(UNC_HIST_THREADS), 0, s, pred, target, unc,
                            V, hist, invalid);
    RU_CHECK_LAUNCH("unc_histogram_kernel");
    return RU_OK;
}

extern "C" int ru_unc_score(const unsigned long long* hist, const int* thresholds, int T, double* out, double* acc, ru_stream_t stream) {
    RU_REQUIRE(hist && thresholds && out && T >= 1 && T <= UNC_MAX_THRESHOLDS, "ru_unc_score: bad argument (1..%d thresholds)", UNC_MAX_THRESHOLDS);
    UncThresholds th = {};
    for (int i = 0; i < T; ++i) {
        RU_REQUIRE(thresholds[i] >= 0 && thresholds[i] <= 100 && (i == 0 || thresholds[i] > thresholds[i - 1]),
                   "ru_unc_score: the thresholds must rise strictly inside 0..100");
        th.t[i] = thresholds[i];
    }
    hipLaunchKernelGGL(unc_score_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, hist, th, T, out, acc);
    RU_CHECK_LAUNCH("unc_score_kernel");
    return RU_OK;
}

extern "C" int ru_paste_u8c(const unsigned char* src, unsigned char* full, int C, int D, int H, int W, const int* lo, const int* size, ru_stream_t stream) {
    RU_REQUIRE(src && full && lo && size && C >= 1 && C <= 65535, "ru_paste_u8c: bad argument");
    RU_REQUIRE((size_t)D * H * W < (size_t)INT_MAX, "ru_paste_u8c: volume too large for 32-bit voxel indices");
    Box3 b;
    int rc = make_box(b, lo, size, D, H, W, "ru_paste_u8c");
    if (rc) return rc;
    const size_t V = (size_t)D * H * W;
    if (W % 4 == 0 && ((uintptr_t)full & 3) == 0)
        hipLaunchKernelGGL(paste_u8c_kernel<true>, dim3(grid1d(V / 4, 256 * 2, 2048), (unsigned)C), dim3(256), 0, (hipStream_t)stream, src, full, D, H, W, b);
    else hipLaunchKernelGGL(paste_u8c_kernel<false>, dim3(grid1d(V, 256 * 4, 2048), (unsigned)C), dim3(256), 0, (hipStream_t)stream, src, full, D, H, W, b);
    RU_CHECK_LAUNCH("paste_u8c_kernel");
    return RU_OK;
}
