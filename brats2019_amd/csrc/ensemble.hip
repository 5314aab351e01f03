// ensemble.hip -- the device side of the reference's ensemble step (README.md:1-5: an ensemble annotates the unlabeled cases the small
// network is distilled from; average_predicts.ipynb / emsemble_predicts.ipynb: `sum(data_files) / len(data_files)`, argmax, 3 -> 4), and
// the ONE kernel family every merge of un-flipped predictions is served from: test-time augmentation (ru_tta_merge[_box]), ensembles
// (ru_ens_*) and uncertainty maps (ru_unc_accumulate[_finalize], ru_unc_finalize), plus the paste into the case's own frame (ru_paste_*).
//
//   test.py:134-144 per model    un-flip, average the K flips, un-pad      -> merge_kernel<MOMENT, FIRST, FINAL>   (merge_launch)
//   notebooks: sum(...) / len    running float32 sum over the models, / M  -> merge_kernel + finalize_kernel<MOMENT> (merge_finalize_launch)
//   test.py:144                  mean > 0.5 per region, exact counts        -> merge_epilogue, called by both kernels
//   notebooks: argmax, 3 -> 4    class maps {0,1,2,4}                       -> ens_argmax_kernel      (ru_ens_argmax)
//   test.py:167-168              a box in the case's own frame              -> paste_kernel<PER> for bytes (paste_launch), paste_probs_kernel for floats
//
// The arithmetic is fixed (float32, one order, true divisions, no fma), so every result can be compared with numpy exactly:
//   mean      p_m = (((o0 + o1) + o2) + o3) / K;  S_1 = p_1, S_m = S_(m-1) + p_m in list order;  mean = S_M / (float)M
//   moment    q_m = ((o0*o0 + o1*o1) + o2*o2) + o3*o3, T_1 = q_1, T_m = T_(m-1) + q_m: float32, every product and sum rounded
//   std       e2 = (double)T_M / (double)(M*K), mu = (double)mean, var = max(e2 - mu*mu, 0), u = floor(min(200*sqrt(var), 100) + 0.5)
//   entropy   H = -(mu*log2(mu) + (1-mu)*log2(1-mu)), a term is 0 unless its argument lies inside (0, 1); u = floor(100*H + 0.5)
// TTA is the ensemble of one (FIRST, FINAL, M = 1: S / 1.0f is S), an ensemble is the uncertainty pass without the moment and the map
// (MOMENT off: acc2 and unc are neither read nor written, no product is formed).  Contraction is switched off where these are formed.
// All passes are HBM streams: 256-thread workgroups, 32-bit voxel indices, a lane takes 4 consecutive voxels of the box (16-byte loads
// and stores; the hardware takes them at dword alignment, which a box row at an odd offset needs), integer counts reduced per wave and per
// workgroup before ONE global atomic.
#include "ru_common.h"
#include "pw_helpers.hpp"
#include "mask_bits.hpp"

#include <limits.h>

namespace ru {
namespace {

typedef float f4u __attribute__((ext_vector_type(4), aligned(4)));         // 4 floats at dword alignment: one global_load/store_dwordx4

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

// t[0 .. n) = p[0 .. n), n <= 4: one 16-byte load for a full quad
__device__ __forceinline__ void load_quad(const float* __restrict__ p, unsigned n, float (&t)[4]) {
    if (n == 4u) {
        const f4u a = *reinterpret_cast<const f4u*>(p);
        t[0] = a.x; t[1] = a.y; t[2] = a.z; t[3] = a.w;
    } else {
        for (unsigned j = 0; j < n; ++j) t[j] = p[j];
    }
}
__device__ __forceinline__ void store_quad(float* __restrict__ p, unsigned n, const float (&t)[4]) {
    if (n == 4u) {
        f4u o;
        o.x = t[0]; o.y = t[1]; o.z = t[2]; o.w = t[3];
        *reinterpret_cast<f4u*>(p) = o;
    } else {
        for (unsigned j = 0; j < n; ++j) p[j] = t[j];
    }
}

// The finalize of the n <= 4 voxels at offset o of the outputs, from their sums (S, T): mean = S / M, mask = mean > 0.5, with MOMENT the
// map from (T, mean).  A vector store for a full quad, bytewise for a tail.  Returns the number of mask voxels set.
template <bool MOMENT>
__device__ __forceinline__ unsigned merge_epilogue(const float (&S)[4], const float (&T)[4], unsigned n, float M, double MK, int measure,
                                                   float* __restrict__ mean_out, unsigned char* __restrict__ mask, unsigned char* __restrict__ unc, size_t o) {
#pragma clang fp contract(off)
    float m[4];
    unsigned on[4], u[4], local = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        m[j] = S[j] / M;
        on[j] = m[j] > 0.5f ? 1u : 0u;
        if (MOMENT) u[j] = (unsigned)j < n ? unc_value(measure, T[j], m[j], MK) : 0u;
        local += (unsigned)j < n ? on[j] : 0u;
    }
    if (mean_out) store_quad(mean_out + o, n, m);
    if (n == 4u) {
        unc_store_u8x4(mask + o, on);
        if (MOMENT) unc_store_u8x4(unc + o, u);
    } else {
        for (unsigned j = 0; j < n; ++j) {
            mask[o + j] = (unsigned char)on[j];
            if (MOMENT) unc[o + j] = (unsigned char)u[j];
        }
    }
    return local;
}

// One streaming pass per model; a lane takes the box voxels v .. v+3 of channel blockIdx.y.  S = FIRST ? p_m : acc + p_m and, with MOMENT,
// T = FIRST ? q_m : acc2 + q_m.  !FINAL: acc = S, acc2 = T.  FINAL (the last model of the list): mean_out / mask / counts / unc from (S, T)
// by merge_epilogue -- the values finalize_kernel would produce from the stored sums; acc, acc2 are not written, and with the entropy
// measure acc2 is not read either.
template <bool MOMENT, bool FIRST, bool FINAL>
__global__ __launch_bounds__(256) void merge_kernel(const float* __restrict__ p, int K, unsigned flips, float* __restrict__ acc, float* __restrict__ acc2,
                                                    float M, double MK, int measure, float* __restrict__ mean_out, unsigned char* __restrict__ mask,
                                                    unsigned long long* __restrict__ counts, unsigned char* __restrict__ unc, int C, int D, int H, int W,
                                                    Box3 b) {
#pragma clang fp contract(off)
    __shared__ unsigned sm[4];
    const unsigned sx = (unsigned)b.size[2], sy = (unsigned)b.size[1];
    const unsigned Vb = (unsigned)b.size[0] * sy * sx, n4 = (Vb + 3u) >> 2;
    const int c = blockIdx.y;
    const size_t HW = (size_t)H * W, DHW = (size_t)D * HW, cb = (size_t)c * Vb;
    const bool moment = MOMENT && (!FINAL || measure == RU_UNC_STD);
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
                    const f4u a = *reinterpret_cast<const f4u*>(line + (W - 1 - x - 3));
                    t[0] = a.w; t[1] = a.z; t[2] = a.y; t[3] = a.x;
                } else {
                    const f4u a = *reinterpret_cast<const f4u*>(line + x);
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
                s[j] = k == 0 ? t[j] : s[j] + t[j];
                if (MOMENT) {
                    const float tt = t[j] * t[j];
                    q[j] = k == 0 ? tt : q[j] + tt;
                }
            }
        }
        float S[4], T[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            S[j] = s[j] / (float)K;
            if (MOMENT) T[j] = q[j];
        }
        if (!FIRST) {
            float a[4] = {0.f, 0.f, 0.f, 0.f};
            load_quad(acc + cb + v, n, a);
#pragma unroll
            for (int j = 0; j < 4; ++j) S[j] = a[j] + S[j];
            if (moment) {
                load_quad(acc2 + cb + v, n, a);
#pragma unroll
                for (int j = 0; j < 4; ++j) T[j] = a[j] + T[j];
            }
        }
        if (!FINAL) {
            store_quad(acc + cb + v, n, S);
            if (MOMENT) store_quad(acc2 + cb + v, n, T);
        } else {
            local += merge_epilogue<MOMENT>(S, T, n, M, MK, measure, mean_out, mask, unc, cb + v);
        }
    }
    if (FINAL) wg_count_add(local, sm, counts + c);
}

// stored sums -> mean = S_M / (float)M, mask, counts and, with MOMENT, the map; acc2 may be null with the entropy measure
template <bool MOMENT>
__global__ __launch_bounds__(256) void finalize_kernel(const float* __restrict__ acc, const float* __restrict__ acc2, float M, double MK, int measure,
                                                       float* __restrict__ mean_out, unsigned char* __restrict__ mask,
                                                       unsigned long long* __restrict__ counts, unsigned char* __restrict__ unc, unsigned Vb) {
    __shared__ unsigned sm[4];
    const int c = blockIdx.y;
    const size_t cb = (size_t)c * Vb;
    const unsigned n4 = (Vb + 3u) >> 2;
    unsigned local = 0;
    for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < n4; i += gridDim.x * 256u) {
        const unsigned v = i << 2, n = Vb - v < 4u ? Vb - v : 4u;
        float S[4] = {0.f, 0.f, 0.f, 0.f}, T[4] = {0.f, 0.f, 0.f, 0.f};
        load_quad(acc + cb + v, n, S);
        if (MOMENT && measure == RU_UNC_STD) load_quad(acc2 + cb + v, n, T);
        local += merge_epilogue<MOMENT>(S, T, n, M, MK, measure, mean_out, mask, unc, cb + v);
    }
    wg_count_add(local, sm, counts + c);
}

// labels[v] = argmax_c (acc[c][v] / M), first maximum wins and a NaN counts as a maximum (np.argmax); class 3 is written as 4
__global__ __launch_bounds__(256) void ens_argmax_kernel(const float* __restrict__ acc, float M, unsigned char* __restrict__ labels, int C, size_t V) {
    for (size_t v = (size_t)blockIdx.x * 256 + threadIdx.x; v < V; v += (size_t)gridDim.x * 256) {
        float best = acc[v] / M;
        int arg = 0;
        for (int c = 1; c < C; ++c) {
            const float m = acc[(size_t)c * V + v] / M;
            if (m > best || (m != m && best == best)) { best = m; arg = c; }
        }
        labels[v] = (unsigned char)(arg == 3 ? 4 : arg);
    }
}

// full[c][D][H][W] = 0 except the box, which takes mean[c][size].  The float paste keeps a kernel and a launch of its own: as the float instantiation
// of a paste template over the element type it was 0.4 - 1.3 us slower back to back than this one at each of the three grid caps in use (profiles/merge_family_time.txt).
__global__ __launch_bounds__(256) void paste_probs_kernel(const float* __restrict__ mean, float* __restrict__ full, int D, int H, int W, Box3 b) {
    const unsigned V = (unsigned)D * H * W, Vb = (unsigned)b.size[0] * b.size[1] * b.size[2];
    const int c = blockIdx.y;
    const float* src = mean + (size_t)c * Vb;
    float* dst = full + (size_t)c * V;
    for (unsigned v = blockIdx.x * 256u + threadIdx.x; v < V; v += gridDim.x * 256u) {
        const unsigned r = v / (unsigned)W;
        const int x = (int)(v - r * (unsigned)W) - b.lo[2];
        const unsigned zq = r / (unsigned)H;
        const int y = (int)(r - zq * (unsigned)H) - b.lo[1], z = (int)zq - b.lo[0];
        float o = 0.f;
        if (z >= 0 && z < b.size[0] && y >= 0 && y < b.size[1] && x >= 0 && x < b.size[2]) o = src[((size_t)z * b.size[1] + y) * b.size[2] + x];
        dst[v] = o;
    }
}

// full[c][D][H][W] = 0 except the box, which takes src[c][size], bytes; a lane writes PER consecutive voxels of a row.  PER = 4 (W % 4 == 0 and full
// 4-byte aligned) is one dword store, PER = 1 one byte.
template <unsigned PER>
__global__ __launch_bounds__(256) void paste_kernel(const unsigned char* __restrict__ src, unsigned char* __restrict__ full, int D, int H, int W, Box3 b) {
    const unsigned V = (unsigned)D * H * W, Vb = (unsigned)b.size[0] * b.size[1] * b.size[2];
    const int c = blockIdx.y;
    const unsigned char* s = src + (size_t)c * Vb;
    unsigned char* dst = full + (size_t)c * V;
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
        if (PER == 4) reinterpret_cast<unsigned*>(dst)[i] = o;
        else dst[v] = (unsigned char)o;
    }
}

typedef unsigned long long ull;

// counts[0 .. C) = 0 by a kernel node, not a hipMemsetAsync, so that the finalizing entries capture into a hipGraph (mask_bits.hpp)
int zero_counts(ull* counts, int C, hipStream_t s) {
    hipLaunchKernelGGL((zero2_kernel<u64, u64>), dim3(cdiv(C, 256)), dim3(256), 0, s, counts, (size_t)C, (u64*)nullptr, (size_t)0);
    RU_CHECK_LAUNCH("zero2_kernel");
    return RU_OK;
}

// The one grid rule of the family.  A pass that only streams takes 2 quads per lane (at most 2048 workgroups per channel).  A pass that counts ends
// every workgroup in an atomic on its channel's count, and those same-address atomics, not the bytes, bound it: it takes 8 quads per lane (at most
// 512 workgroups).  The three rules tried, entry by entry: profiles/merge_family_time.txt.
dim3 quad_grid(size_t voxels, int C, bool counts) {
    const int quads = counts ? 8 : 2;
    return dim3(grid1d((voxels + 3) / 4, 256 * quads, 4096 / quads), (unsigned)C);
}

template <bool MOMENT>
auto merge_instance(bool first, bool final) {
    return first ? (final ? merge_kernel<MOMENT, true, true> : merge_kernel<MOMENT, true, false>)
                 : (final ? merge_kernel<MOMENT, false, true> : merge_kernel<MOMENT, false, false>);
}

}  // namespace

int merge_launch(const char* who, bool moment, const float* probs, int K, unsigned flips, float* acc, float* acc2, int first, int M, int measure, float* mean_out,
                 unsigned char* mask, ull* counts, unsigned char* unc, int C, int D, int H, int W, const int* lo, const int* size, hipStream_t s) {
    RU_REQUIRE(probs && lo && size && K >= 1 && K <= 8 && C >= 1 && C <= 65535, "%s: bad argument", who);
    RU_REQUIRE(acc || (first && M > 0), "%s: the running sum is needed unless the only model is merged at once", who);
    RU_REQUIRE((size_t)D * H * W < (size_t)INT_MAX, "%s: volume too large for 32-bit voxel indices", who);
    Box3 b;
    int rc = make_box(b, lo, size, D, H, W, who);
    if (rc) return rc;
    if (M > 0 && (rc = zero_counts(counts, C, s))) return rc;
    hipLaunchKernelGGL(moment ? merge_instance<true>(first, M > 0) : merge_instance<false>(first, M > 0), quad_grid((size_t)size[0] * size[1] * size[2], C, M > 0), dim3(256),
                       0, s, probs, K, flips, acc, acc2, M > 0 ? (float)M : 1.f, (double)M * (double)K, measure, mean_out, mask, counts, unc, C, D, H, W, b);
    RU_CHECK_LAUNCH("merge_kernel");
    return RU_OK;
}

int merge_finalize_launch(const char* who, bool moment, const float* acc, const float* acc2, int M, int K, int measure, float* mean_out, unsigned char* mask,
                          ull* counts, unsigned char* unc, int C, size_t Vbox, hipStream_t s) {
    RU_REQUIRE(Vbox < (size_t)INT_MAX, "%s: volume too large for 32-bit voxel indices", who);
    int rc = zero_counts(counts, C, s);
    if (rc) return rc;
    hipLaunchKernelGGL(moment ? finalize_kernel<true> : finalize_kernel<false>, quad_grid(Vbox, C, true), dim3(256), 0, s, acc, acc2, (float)M, (double)M * (double)K, measure,
                       mean_out, mask, counts, unc, (unsigned)Vbox);
    RU_CHECK_LAUNCH("finalize_kernel");
    return RU_OK;
}

int paste_launch(const char* who, const unsigned char* src, unsigned char* full, int C, int D, int H, int W, const int* lo, const int* size, hipStream_t s) {
    RU_REQUIRE((size_t)D * H * W < (size_t)INT_MAX, "%s: volume too large for 32-bit voxel indices", who);
    Box3 b;
    int rc = make_box(b, lo, size, D, H, W, who);
    if (rc) return rc;
    const size_t V = (size_t)D * H * W;
    if (W % 4 == 0 && ((uintptr_t)full & 3) == 0) hipLaunchKernelGGL(paste_kernel<4>, dim3(grid1d(V / 4, 256 * 2, 2048), (unsigned)C), dim3(256), 0, s, src, full, D, H, W, b);
    else hipLaunchKernelGGL(paste_kernel<1>, dim3(grid1d(V, 256 * 4, 2048), (unsigned)C), dim3(256), 0, s, src, full, D, H, W, b);
    RU_CHECK_LAUNCH("paste_kernel");
    return RU_OK;
}

}  // namespace ru

using namespace ru;

extern "C" int ru_ens_accumulate(const float* probs, int K, unsigned flips, float* acc, int first, int C, int D, int H, int W, const int* lo, const int* size,
                                 ru_stream_t stream) {
    RU_REQUIRE(acc, "ru_ens_accumulate: null argument");
    return merge_launch("ru_ens_accumulate", false, probs, K, flips, acc, nullptr, first, 0, 0, nullptr, nullptr, nullptr, nullptr, C, D, H, W, lo, size,
                        (hipStream_t)stream);
}

extern "C" int ru_ens_accumulate_finalize(const float* probs, int K, unsigned flips, const float* acc, int first, int M, float* mean_out, unsigned char* mask,
                                          unsigned long long* counts, int C, int D, int H, int W, const int* lo, const int* size, ru_stream_t stream) {
    RU_REQUIRE(mask && counts && M >= 1, "ru_ens_accumulate_finalize: bad argument");
    return merge_launch("ru_ens_accumulate_finalize", false, probs, K, flips, const_cast<float*>(acc), nullptr, first, M, 0, mean_out, mask, counts, nullptr, C, D, H, W,
                        lo, size, (hipStream_t)stream);
}

extern "C" int ru_ens_finalize(const float* acc, int M, float* mean_out, unsigned char* mask, unsigned long long* counts, int C, size_t Vbox, ru_stream_t stream) {
    RU_REQUIRE(acc && mask && counts && M >= 1 && C >= 1 && C <= 65535 && Vbox > 0, "ru_ens_finalize: bad argument");
    return merge_finalize_launch("ru_ens_finalize", false, acc, nullptr, M, 1, 0, mean_out, mask, counts, nullptr, C, Vbox, (hipStream_t)stream);
}

extern "C" int ru_ens_argmax(const float* acc, int M, unsigned char* labels, int C, size_t V, ru_stream_t stream) {
    RU_REQUIRE(acc && labels && M >= 1 && C >= 1 && V > 0, "ru_ens_argmax: bad argument");
    hipLaunchKernelGGL(ens_argmax_kernel, dim3(grid1d(V, 256 * 4, 2048)), dim3(256), 0, (hipStream_t)stream, acc, (float)M, labels, C, V);
    RU_CHECK_LAUNCH("ens_argmax_kernel");
    return RU_OK;
}

extern "C" int ru_paste_probs(const float* mean, float* full, int C, int D, int H, int W, const int* lo, const int* size, ru_stream_t stream) {
    RU_REQUIRE(mean && full && lo && size && C >= 1 && C <= 65535, "ru_paste_probs: bad argument");
    RU_REQUIRE((size_t)D * H * W < (size_t)INT_MAX, "ru_paste_probs: volume too large for 32-bit voxel indices");
    Box3 b;
    int rc = make_box(b, lo, size, D, H, W, "ru_paste_probs");
    if (rc) return rc;
    hipLaunchKernelGGL(paste_probs_kernel, dim3(grid1d((size_t)D * H * W, 256 * 4, 1024), (unsigned)C), dim3(256), 0, (hipStream_t)stream, mean, full, D, H, W, b);
    RU_CHECK_LAUNCH("paste_probs_kernel");
    return RU_OK;
}
