// uncertainty.hip -- the third BraTS 2019 task, quantification of uncertainty in segmentation, on the device: per case three uint8 maps
// (whole tumour, tumour core, enhancing tumour; 0 = certain .. 100 = uncertain) made from the M models x K flips an ensemble predicts
// anyway (ensemble.hip), and the challenge's score of such maps.
//
//   the maps                 : the merge family of ensemble.hip with its moment switch on -- merge_kernel<true, ..> adds the second-moment sum acc2
//                              in the SAME pass over the predictions (ru_unc_accumulate[_finalize]), finalize_kernel<true> works from stored sums
//                              (ru_unc_finalize); the arithmetic of the sums and of both measures is stated there.  paste_kernel puts the maps
//                              into the case's own frame (ru_paste_u8c).
//   unc_histogram_kernel     : one pass over (prediction labels, target labels, three maps) -> exact counts hist[region][map value][TP FP FN TN]
//   unc_score_kernel         : cumulative sums over the map value, the filtered Dice / FTP / FTN curves, their AUCs and the score, float64
#include "ru_common.h"
#include "pw_helpers.hpp"
#include "mask_bits.hpp"

namespace ru {
namespace {

constexpr int UNC_REGIONS = 3, UNC_LEVELS = 101, UNC_CLASSES = 4;
constexpr int UNC_BINS = UNC_REGIONS * UNC_LEVELS * UNC_CLASSES;
constexpr int UNC_HIST_THREADS = 256, UNC_HIST_WAVES = UNC_HIST_THREADS / 64;
constexpr int UNC_HIST_MAX_BLOCKS = 512;                                   // bounds the same-address atomics: <= 512 per bin
constexpr int UNC_MAX_THRESHOLDS = 101;
// labels of the three regions as bit sets over the label value: WT = {1,2,3,4}, TC = {1,3,4}, ET = {3,4} (mask_bits.hpp, brats_region)
constexpr unsigned UNC_REGION_BITS[UNC_REGIONS] = {0x1eu, 0x1au, 0x18u};

struct UncThresholds { int t[UNC_MAX_THRESHOLDS]; };

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

bool unc_measure_ok(int measure) { return measure == RU_UNC_STD || measure == RU_UNC_ENTROPY; }

}  // namespace
}  // namespace ru

using namespace ru;

extern "C" int ru_unc_accumulate(const float* probs, int K, unsigned flips, float* acc, float* acc2, int first, int C, int D, int H, int W, const int* lo,
                                 const int* size, ru_stream_t stream) {
    RU_REQUIRE(acc && acc2, "ru_unc_accumulate: null argument");
    return merge_launch("ru_unc_accumulate", true, probs, K, flips, acc, acc2, first, 0, RU_UNC_STD, nullptr, nullptr, nullptr, nullptr, C, D, H, W, lo, size,
                        (hipStream_t)stream);
}

extern "C" int ru_unc_accumulate_finalize(const float* probs, int K, unsigned flips, const float* acc, const float* acc2, int first, int M, int measure,
                                          float* mean_out, unsigned char* mask, unsigned long long* counts, unsigned char* unc, int C, int D, int H, int W,
                                          const int* lo, const int* size, ru_stream_t stream) {
    RU_REQUIRE(mask && counts && unc && M >= 1, "ru_unc_accumulate_finalize: bad argument");
    RU_REQUIRE(unc_measure_ok(measure), "ru_unc_accumulate_finalize: measure %d is neither RU_UNC_STD nor RU_UNC_ENTROPY", measure);
    RU_REQUIRE(first || (acc && (acc2 || measure == RU_UNC_ENTROPY)), "ru_unc_accumulate_finalize: the running sums are needed unless the only model is merged at once");
    return merge_launch("ru_unc_accumulate_finalize", true, probs, K, flips, const_cast<float*>(acc), const_cast<float*>(acc2), first, M, measure, mean_out, mask, counts,
                        unc, C, D, H, W, lo, size, (hipStream_t)stream);
}

extern "C" int ru_unc_finalize(const float* acc, const float* acc2, int M, int K, int measure, float* mean_out, unsigned char* mask, unsigned long long* counts,
                               unsigned char* unc, int C, size_t Vbox, ru_stream_t stream) {
    RU_REQUIRE(acc && mask && counts && unc && M >= 1 && K >= 1 && C >= 1 && C <= 65535 && Vbox > 0, "ru_unc_finalize: bad argument");
    RU_REQUIRE(unc_measure_ok(measure), "ru_unc_finalize: measure %d is neither RU_UNC_STD nor RU_UNC_ENTROPY", measure);
    RU_REQUIRE(acc2 || measure == RU_UNC_ENTROPY, "ru_unc_finalize: RU_UNC_STD needs the second-moment sum");
    return merge_finalize_launch("ru_unc_finalize", true, acc, acc2, M, K, measure, mean_out, mask, counts, unc, C, Vbox, (hipStream_t)stream);
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
    return paste_launch("ru_paste_u8c", src, full, C, D, H, W, lo, size, (hipStream_t)stream);
}
