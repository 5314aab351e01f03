// Label-overlap metrics on the device: the counterpart of the reference's `Dice1D`, `RMSE`, `DiceWT`, `Dice_ITK` (metrics.py:22-185) and of
// its offline scorer validate.py.  Every one of them is a count over the output volume, and every count they need is an entry of one
// per-sample confusion matrix conf[n][a][b] = #voxels with prediction label a and target label b:
//   ov_confusion_kernel  : one streaming pass, each input read once.  kind 0: label = argmax over C of float32 probabilities (torch's
//                          rules: first of equal maxima, NaN is the maximum, first NaN wins); kind 1: uint8 label volumes, 4 -> 3.
//                          Counts per wave with __ballot + __popcll per bin (compile-time L x L bins, wave-uniform counters), then
//                          one atomic per non-empty bin per workgroup and a bounded number of workgroups per sample: nearly every voxel
//                          lands in bin (0, 0), and per-voxel atomics on one line serialise (pointwise.hip, dice_counts_kernel).
//   ov_accumulate_kernel : Dice_ITK (ITK's union overlap -> mean overlap in float64), DiceWT (float32 ratio) and validate.py's per-case
//                          label Dice from the matrix, then the batch mean into the float64 accumulator.
//   ov_dice1d_kernel     : Dice1D from ru_dice_counts' {I, |P|+|G|}.
//   ov_rmse_kernel       : RMSE's sqrt(sum d^2 / count) from ru_crit_moments' RU_CRIT_M_D2 moment.
// The outputs are cleared by a kernel, not by hipMemsetAsync, so the calls capture into a hipGraph (mask_bits.hpp, zero2_kernel).
#include "ru_common.h"
#include "mask_bits.hpp"

namespace ru {
namespace {

constexpr int OV_THREADS = 512;                  // 8 waves
constexpr int OV_WAVES = OV_THREADS / 64;
constexpr int OV_TARGET_BLOCKS = 512;            // ~2 workgroups per CU over the whole batch
constexpr int OV_MAX_BLOCKS_PER_SAMPLE = 256;    // bounds the same-line atomics: <= 256 per bin and sample
constexpr int OV_LABEL_LABELS = 4;               // kind 1: labels 0..3 (4 -> 3)
constexpr unsigned OV_INVALID = 0xffu;

// torch.argmax over the channel axis: the first of equal maxima wins; a NaN is larger than everything, the first NaN wins
template <int L>
__device__ __forceinline__ int ov_argmax(const float (&x)[L]) {
    float best = x[0];
    int idx = 0;
#pragma unroll
    for (int c = 1; c < L; ++c) {
        const bool take = best == best && (x[c] > best || x[c] != x[c]);
        best = take ? x[c] : best;
        idx = take ? c : idx;
    }
    return idx;
}

// validate.py:70 / loader_helper.read_multimodal:30: 4 -> 3; anything else outside 0..3 is invalid
__device__ __forceinline__ unsigned ov_label(unsigned v) { return v < 4u ? v : (v == 4u ? 3u : OV_INVALID); }

// one bin index per lane -> the wave-uniform counters: one ballot per bin, 64 voxels per ballot
template <int NB>
__device__ __forceinline__ void ov_count(int bin, unsigned (&cnt)[NB]) {
#pragma unroll
    for (int k = 0; k < NB; ++k) cnt[k] += (unsigned)__popcll(__ballot(bin == k));
}

// the workgroup's counters -> one atomic per non-empty bin.  cnt[NB - 1] is the invalid counter for kind 1 (NB = L*L + 1).
template <int NB>
__device__ __forceinline__ void ov_publish(const unsigned (&cnt)[NB], unsigned long long* __restrict__ conf_n, unsigned long long* __restrict__ inv_n,
                                           int nbins) {
    __shared__ unsigned s[OV_WAVES][NB];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < NB; ++k) s[wave][k] = cnt[k];
    }
    __syncthreads();
    if ((int)threadIdx.x < NB) {
        unsigned long long t = 0;
#pragma unroll
        for (int w = 0; w < OV_WAVES; ++w) t += s[w][threadIdx.x];
        if (t) atomicAdd((int)threadIdx.x < nbins ? conf_n + threadIdx.x : inv_n, t);
    }
}

// kind 0: p, g = [N][L][V] float32.  grid (blocks per sample, N).  VEC4 (V % 4 == 0): 4 voxels per lane and step with float4 loads.
template <int L, bool VEC4>
__global__ __launch_bounds__(OV_THREADS) void ov_confusion_prob_kernel(const float* __restrict__ p, const float* __restrict__ g, size_t V,
                                                                       unsigned long long* __restrict__ conf) {
    constexpr int NB = L * L;
    const size_t n = blockIdx.y;
    const float* __restrict__ pn = p + n * L * V;
    const float* __restrict__ gn = g + n * L * V;
    unsigned cnt[NB];
#pragma unroll
    for (int k = 0; k < NB; ++k) cnt[k] = 0;
    const size_t stride = (size_t)gridDim.x * OV_THREADS;
    if (VEC4) {
        const size_t V4 = V >> 2;
        for (size_t v = (size_t)blockIdx.x * OV_THREADS + threadIdx.x; v < V4; v += stride) {
            float4 a[L], b[L];
#pragma unroll
            for (int c = 0; c < L; ++c) {
                a[c] = reinterpret_cast<const float4*>(pn + (size_t)c * V)[v];
                b[c] = reinterpret_cast<const float4*>(gn + (size_t)c * V)[v];
            }
            float xa[4][L], xb[4][L];
#pragma unroll
            for (int c = 0; c < L; ++c) {
                xa[0][c] = a[c].x; xa[1][c] = a[c].y; xa[2][c] = a[c].z; xa[3][c] = a[c].w;
                xb[0][c] = b[c].x; xb[1][c] = b[c].y; xb[2][c] = b[c].z; xb[3][c] = b[c].w;
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) ov_count<NB>(ov_argmax<L>(xa[u]) * L + ov_argmax<L>(xb[u]), cnt);
        }
    } else {
        for (size_t v = (size_t)blockIdx.x * OV_THREADS + threadIdx.x; v < V; v += stride) {
            float xa[L], xb[L];
#pragma unroll
            for (int c = 0; c < L; ++c) {
                xa[c] = pn[(size_t)c * V + v];
                xb[c] = gn[(size_t)c * V + v];
            }
            ov_count<NB>(ov_argmax<L>(xa) * L + ov_argmax<L>(xb), cnt);
        }
    }
    ov_publish<NB>(cnt, conf + n * NB, nullptr, NB);
}

// kind 1: p, g = [N][V] uint8 labels.  Bin 16 counts voxels where either label is invalid (they go into no other bin).
template <bool VEC4>
__global__ __launch_bounds__(OV_THREADS) void ov_confusion_label_kernel(const unsigned char* __restrict__ p, const unsigned char* __restrict__ g,
                                                                        size_t V, unsigned long long* __restrict__ conf,
                                                                        unsigned long long* __restrict__ invalid) {
    constexpr int L = OV_LABEL_LABELS, NB = L * L + 1;
    const size_t n = blockIdx.y;
    const unsigned char* __restrict__ pn = p + n * V;
    const unsigned char* __restrict__ gn = g + n * V;
    unsigned cnt[NB];
#pragma unroll
    for (int k = 0; k < NB; ++k) cnt[k] = 0;
    const size_t stride = (size_t)gridDim.x * OV_THREADS;
    auto bin = [](unsigned a, unsigned b) {
        a = ov_label(a);
        b = ov_label(b);
        return a == OV_INVALID || b == OV_INVALID ? L * L : (int)(a * L + b);
    };
    if (VEC4) {
        const size_t V4 = V >> 2;
        for (size_t v = (size_t)blockIdx.x * OV_THREADS + threadIdx.x; v < V4; v += stride) {
            const unsigned a = reinterpret_cast<const unsigned*>(pn)[v], b = reinterpret_cast<const unsigned*>(gn)[v];
#pragma unroll
            for (int u = 0; u < 4; ++u) ov_count<NB>(bin((a >> (8 * u)) & 0xffu, (b >> (8 * u)) & 0xffu), cnt);
        }
    } else {
        for (size_t v = (size_t)blockIdx.x * OV_THREADS + threadIdx.x; v < V; v += stride) ov_count<NB>(bin(pn[v], gn[v]), cnt);
    }
    ov_publish<NB>(cnt, conf + n * (L * L), invalid + n, L * L);
}

int ov_blocks(size_t V, int N, int per_block) {
    const size_t need = (V + per_block - 1) / per_block;
    int want = (OV_TARGET_BLOCKS + N - 1) / N;
    want = want < OV_MAX_BLOCKS_PER_SAMPLE ? want : OV_MAX_BLOCKS_PER_SAMPLE;
    return (int)(need < (size_t)want ? (need > 0 ? need : 1) : (size_t)want);
}

bool ov_aligned(const void* p, const void* g, size_t a) { return ((uintptr_t)p % a) == 0 && ((uintptr_t)g % a) == 0; }

template <int L>
void ov_launch_prob(const float* p, const float* g, size_t V, int N, unsigned long long* conf, hipStream_t s) {
    if (V % 4 == 0 && ov_aligned(p, g, 16)) {
        hipLaunchKernelGGL((ov_confusion_prob_kernel<L, true>), dim3(ov_blocks(V / 4, N, OV_THREADS), N), dim3(OV_THREADS), 0, s, p, g, V, conf);
    } else {
        hipLaunchKernelGGL((ov_confusion_prob_kernel<L, false>), dim3(ov_blocks(V, N, OV_THREADS), N), dim3(OV_THREADS), 0, s, p, g, V, conf);
    }
}

// ---------------------------------------------------------------- finalize: one thread per result column, samples in order
__device__ __forceinline__ unsigned long long ov_row(const unsigned long long* c, int L, int a) {
    unsigned long long t = 0;
    for (int b = 0; b < L; ++b) t += c[a * L + b];
    return t;
}
__device__ __forceinline__ unsigned long long ov_col(const unsigned long long* c, int L, int b) {
    unsigned long long t = 0;
    for (int a = 0; a < L; ++a) t += c[a * L + b];
    return t;
}

// mode ITK: column i-1 for label i = 1..nacc.  mode WT: one column.  mode VALIDATE: columns d1, d2, d3, dWT; acc is a running sum over
// the cases (validate.py:83-99), not a batch mean.
__global__ void ov_accumulate_kernel(const unsigned long long* __restrict__ conf, int N, int L, int mode, int nacc, double* __restrict__ acc,
                                     double* __restrict__ out) {
    const int j = threadIdx.x;
    if (j >= nacc) return;
    double sum = 0.0;
    for (int n = 0; n < N; ++n) {
        const unsigned long long* c = conf + (size_t)n * L * L;
        double r;
        if (mode == RU_OVERLAP_ITK) {
            const int i = j + 1;
            if (i >= L) {
                r = __builtin_nan("");                                    // label absent from both images: RU_OVERLAP_BOTH_EMPTY
            } else {
                const unsigned long long I = c[i * L + i], P = ov_row(c, L, i), G = ov_col(c, L, i);
                if (P + G == 0) {
                    r = __builtin_nan("");                                // RU_OVERLAP_BOTH_EMPTY
                } else {
                    const double J = (double)I / (double)(P + G - I);    // ITK's union overlap of the one non-zero label
                    r = 2.0 * J / (1.0 + J);                              // GetDiceCoefficient() = GetMeanOverlap()
                }
            }
        } else {
            unsigned long long I = 0, S = 0;
            if (mode == RU_OVERLAP_WT || j == 3) {                        // whole tumour: every label > 0
                for (int a = 1; a < L; ++a) {
                    for (int b = 1; b < L; ++b) I += c[a * L + b];
                    S += ov_row(c, L, a) + ov_col(c, L, a);
                }
            } else {
                const int i = j + 1;
                I = c[i * L + i];
                S = ov_row(c, L, i) + ov_col(c, L, i);
            }
            float f;
            if (mode == RU_OVERLAP_WT) {
                f = 2.f * (float)I / ((float)S + 1e-6f);                  // metrics.py:151: float32, both empty -> 0
            } else {
                f = 2.f * (float)I / (float)S;                            // validate.py:79-83 / 91-95: float32 sums, NaN -> 1
                if (f != f) f = 1.f;
            }
            r = (double)f;
        }
        if (out) out[(size_t)n * nacc + j] = r;
        sum += r;
    }
    acc[j] += mode == RU_OVERLAP_VALIDATE ? sum : sum / (double)N;
}

// metrics.py:41-50: r = 2*I / (S + 1e-6) in float32 per sample and channel c < classes, the batch mean and the accumulator in float64
__global__ void ov_dice1d_kernel(const unsigned long long* __restrict__ counts, double* __restrict__ acc, int N, int C, int classes) {
    const int c = threadIdx.x;
    if (c >= classes) return;
    double sum = 0.0;
    for (int n = 0; n < N; ++n) {
        const unsigned long long* q = counts + ((size_t)n * C + c) * 2;
        sum += (double)(2.f * (float)q[0] / ((float)q[1] + 1e-6f));
    }
    acc[c] += sum / (double)N;
}

__global__ void ov_rmse_kernel(const double* __restrict__ sums, double* __restrict__ acc) {
    if (threadIdx.x == 0) acc[0] += sqrt(sums[0] / sums[1]);
}

}  // namespace
}  // namespace ru

using namespace ru;

extern "C" int ru_label_confusion(const void* pred, const void* target, int kind, int N, int C, size_t V, unsigned long long* conf,
                                  unsigned long long* invalid, ru_stream_t stream) {
    RU_REQUIRE(pred && target && conf && N > 0 && N <= 65535 && V > 0 && V <= (1ull << 34), "ru_label_confusion: bad argument");
    RU_REQUIRE(kind == RU_CONF_PROB || kind == RU_CONF_LABEL, "ru_label_confusion: kind %d is neither RU_CONF_PROB nor RU_CONF_LABEL", kind);
    RU_REQUIRE(kind == RU_CONF_LABEL || (C >= 1 && C <= RU_OVERLAP_MAX_LABELS),
               "ru_label_confusion: C = %d channels, 1..%d (more: count on the host side)", C, RU_OVERLAP_MAX_LABELS);
    RU_REQUIRE(kind == RU_CONF_PROB || (C == 1 && invalid), "ru_label_confusion: label volumes have C = 1 and need the invalid counter");
    hipStream_t s = (hipStream_t)stream;
    const int L = kind == RU_CONF_PROB ? C : OV_LABEL_LABELS;
    const int nconf = N * L * L, ninv = invalid ? N : 0;
    hipLaunchKernelGGL((zero2_kernel<u64, u64>), dim3(cdiv(nconf + ninv, 256)), dim3(256), 0, s, conf, (size_t)nconf, invalid, (size_t)ninv);
    RU_CHECK_LAUNCH("zero2_kernel");
    if (kind == RU_CONF_LABEL) {
        const unsigned char* p = (const unsigned char*)pred;
        const unsigned char* g = (const unsigned char*)target;
        if (V % 4 == 0 && ov_aligned(p, g, 4)) {
            hipLaunchKernelGGL((ov_confusion_label_kernel<true>), dim3(ov_blocks(V / 4, N, OV_THREADS), N), dim3(OV_THREADS), 0, s, p, g, V, conf,
                               invalid);
        } else {
            hipLaunchKernelGGL((ov_confusion_label_kernel<false>), dim3(ov_blocks(V, N, OV_THREADS), N), dim3(OV_THREADS), 0, s, p, g, V, conf,
                               invalid);
        }
        RU_CHECK_LAUNCH("ov_confusion_label_kernel");
        return RU_OK;
    }
    const float* p = (const float*)pred;
    const float* g = (const float*)target;
    switch (C) {
        case 1: ov_launch_prob<1>(p, g, V, N, conf, s); break;
        case 2: ov_launch_prob<2>(p, g, V, N, conf, s); break;
        case 3: ov_launch_prob<3>(p, g, V, N, conf, s); break;
        case 4: ov_launch_prob<4>(p, g, V, N, conf, s); break;
        case 5: ov_launch_prob<5>(p, g, V, N, conf, s); break;
        case 6: ov_launch_prob<6>(p, g, V, N, conf, s); break;
        case 7: ov_launch_prob<7>(p, g, V, N, conf, s); break;
        default: ov_launch_prob<8>(p, g, V, N, conf, s); break;
    }
    RU_CHECK_LAUNCH("ov_confusion_prob_kernel");
    return RU_OK;
}

extern "C" int ru_overlap_accumulate(const unsigned long long* conf, int N, int L, int mode, int nacc, double* acc, double* out,
                                     ru_stream_t stream) {
    RU_REQUIRE(conf && acc && N > 0 && L >= 1 && L <= 1024, "ru_overlap_accumulate: bad argument");
    RU_REQUIRE(mode == RU_OVERLAP_ITK || mode == RU_OVERLAP_WT || mode == RU_OVERLAP_VALIDATE, "ru_overlap_accumulate: unknown mode %d", mode);
    RU_REQUIRE(mode != RU_OVERLAP_ITK || (nacc >= 1 && nacc <= 64), "ru_overlap_accumulate: ITK needs 1 <= nacc <= 64, got %d", nacc);
    RU_REQUIRE(mode != RU_OVERLAP_WT || nacc == 1, "ru_overlap_accumulate: WT has nacc = 1, got %d", nacc);
    RU_REQUIRE(mode != RU_OVERLAP_VALIDATE || (nacc == 4 && L == OV_LABEL_LABELS && out),
               "ru_overlap_accumulate: VALIDATE has nacc = 4, L = 4 and an output, got nacc %d, L %d", nacc, L);
    hipLaunchKernelGGL(ov_accumulate_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, conf, N, L, mode, nacc, acc, out);
    RU_CHECK_LAUNCH("ov_accumulate_kernel");
    return RU_OK;
}

extern "C" int ru_dice1d_accumulate(const unsigned long long* counts, double* acc, int N, int C, int classes, ru_stream_t stream) {
    RU_REQUIRE(counts && acc && N > 0 && classes >= 1 && classes <= C && classes <= 64, "ru_dice1d_accumulate: bad argument");
    hipLaunchKernelGGL(ov_dice1d_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, counts, acc, N, C, classes);
    RU_CHECK_LAUNCH("ov_dice1d_kernel");
    return RU_OK;
}

extern "C" int ru_rmse_accumulate(const double* sums, double* acc, ru_stream_t stream) {
    RU_REQUIRE(sums && acc, "ru_rmse_accumulate: bad argument");
    hipLaunchKernelGGL(ov_rmse_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, sums, acc);
    RU_CHECK_LAUNCH("ov_rmse_kernel");
    return RU_OK;
}
