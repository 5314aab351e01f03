// ensemble.hip -- the device side of the reference's ensemble step (README.md:1-5: an ensemble annotates the unlabeled cases the small
// network is distilled from; average_predicts.ipynb / emsemble_predicts.ipynb: `sum(data_files) / len(data_files)`, argmax, 3 -> 4).
//
//   test.py:134-144 per model    un-flip, average the K flips, un-pad      -> ens_accumulate_kernel  (ru_ens_accumulate[_finalize])
//   notebooks: sum(...) / len    running float32 sum over the models, / M  -> ens_accumulate_kernel + ens_finalize_kernel (ru_ens_finalize)
//   test.py:144                  mean > 0.5 per region, exact counts        -> ens_finalize_kernel / the fused last accumulate
//   notebooks: argmax, 3 -> 4    class maps {0,1,2,4}                       -> ens_argmax_kernel      (ru_ens_argmax)
//   test.py:167-168 for floats   the mean in the case's own frame           -> paste_probs_kernel     (ru_paste_probs)
//
// The arithmetic is fixed (float32, one order, true divisions), so every result can be compared bit for bit with numpy:
//   p_m = (((o0 + o1) + o2) + o3) / K as tta_merge_box_kernel;  S_1 = p_1, S_m = S_(m-1) + p_m in list order;  mean = S_M / (float)M.
// All of it is pure HBM traffic: one coalesced dword per lane and copy (x-flipped rows are read backwards, still one 256-byte segment per
// wave), 32-bit index arithmetic, integer counts reduced per wave and per workgroup before ONE global atomic.
#include "ru_common.h"
#include "pw_helpers.hpp"
#include "mask_bits.hpp"

#include <limits.h>

namespace ru {

// One streaming pass per model.  S = FIRST ? p_m : acc + p_m.  !FINAL: acc = S.  FINAL (the last model of the list): mean = S / M goes
// straight to mean_out / mask / counts and acc is not written -- the same values ens_finalize_kernel would produce from the stored S.
template <bool FIRST, bool FINAL>
__global__ __launch_bounds__(256) void ens_accumulate_kernel(const float* __restrict__ p, int K, unsigned flips, float* __restrict__ acc, float M,
                                                             float* __restrict__ mean_out, unsigned char* __restrict__ mask,
                                                             unsigned long long* __restrict__ counts, int C, int D, int H, int W, Box3 b) {
    __shared__ unsigned sm[4];
    const unsigned Vb = (unsigned)b.size[0] * b.size[1] * b.size[2];
    const int c = blockIdx.y;
    const size_t HW = (size_t)H * W, DHW = (size_t)D * HW;
    float* a = acc + (size_t)c * Vb;
    unsigned local = 0;
    for (unsigned v = blockIdx.x * 256u + threadIdx.x; v < Vb; v += gridDim.x * 256u) {
        const unsigned r = v / (unsigned)b.size[2];
        const int x = (int)(v - r * (unsigned)b.size[2]) + b.lo[2];
        const unsigned zq = r / (unsigned)b.size[1];
        const int y = (int)(r - zq * (unsigned)b.size[1]) + b.lo[1], z = (int)zq + b.lo[0];
        float s = 0.f;
        for (int k = 0; k < K; ++k) {
            const unsigned f = (flips >> (3 * k)) & 7u;
            const int zz = (f & 1u) ? D - 1 - z : z, yy = (f & 2u) ? H - 1 - y : y, xx = (f & 4u) ? W - 1 - x : x;
            const float t = p[((size_t)k * C + c) * DHW + (size_t)zz * HW + (size_t)yy * W + xx];
            s = k == 0 ? t : s + t;
        }
        float S = s / (float)K;
        if (!FIRST) S = a[v] + S;
        if (!FINAL) a[v] = S;
        else {
            const float m = S / M;
            if (mean_out) mean_out[(size_t)c * Vb + v] = m;
            const bool on = m > 0.5f;
            mask[(size_t)c * Vb + v] = on ? 1 : 0;
            local += on ? 1u : 0u;
        }
    }
    if (FINAL) wg_count_add(local, sm, counts + c);
}

// mean = S_M / (float)M, mask = mean > 0.5, counts: acc is contiguous, so a lane takes 4 voxels (16-byte load, 16-byte + 4-byte stores) when
// the channel pitch allows it
template <bool VEC>
__global__ __launch_bounds__(256) void ens_finalize_kernel(const float* __restrict__ acc, float M, float* __restrict__ mean_out, unsigned char* __restrict__ mask,
                                                           unsigned long long* __restrict__ counts, unsigned Vb) {
    __shared__ unsigned sm[4];
    const int c = blockIdx.y;
    const size_t base = (size_t)c * Vb;
    unsigned local = 0;
    if (VEC) {
        const float4* a4 = reinterpret_cast<const float4*>(acc + base);
        float4* m4 = mean_out ? reinterpret_cast<float4*>(mean_out + base) : nullptr;
        uchar4* k4 = reinterpret_cast<uchar4*>(mask + base);
        const unsigned n4 = Vb >> 2;
        for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < n4; i += gridDim.x * 256u) {
            const float4 s = a4[i];
            const float4 m = make_float4(s.x / M, s.y / M, s.z / M, s.w / M);
            if (m4) m4[i] = m;
            const uchar4 k = make_uchar4(m.x > 0.5f ? 1 : 0, m.y > 0.5f ? 1 : 0, m.z > 0.5f ? 1 : 0, m.w > 0.5f ? 1 : 0);
            k4[i] = k;
            local += (unsigned)k.x + k.y + k.z + k.w;
        }
    } else {
        for (unsigned v = blockIdx.x * 256u + threadIdx.x; v < Vb; v += gridDim.x * 256u) {
            const float m = acc[base + v] / M;
            if (mean_out) mean_out[base + v] = m;
            const bool on = m > 0.5f;
            mask[base + v] = on ? 1 : 0;
            local += on ? 1u : 0u;
        }
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

// full[c][D][H][W] = 0 except the box, which takes mean[c][size]
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

static int ens_accumulate_impl(const float* probs, int K, unsigned flips, float* acc, int first, int M, float* mean_out, unsigned char* mask,
                               unsigned long long* counts, int C, int D, int H, int W, const int* lo, const int* size, hipStream_t s, const char* who) {
    RU_REQUIRE(probs && lo && size && K >= 1 && K <= 8 && C >= 1 && C <= 65535, "%s: bad argument", who);
    RU_REQUIRE(acc || (first && M > 0), "%s: the running sum is needed unless the only model is merged at once", who);
    RU_REQUIRE((size_t)D * H * W < (size_t)INT_MAX, "%s: volume too large for 32-bit voxel indices", who);
    Box3 b;
    int rc = make_box(b, lo, size, D, H, W, who);
    if (rc) return rc;
    const dim3 grid(grid1d((size_t)size[0] * size[1] * size[2], 256 * 4, 1024), (unsigned)C), block(256);
    if (M > 0) {
        hipError_t e = hipMemsetAsync(counts, 0, sizeof(unsigned long long) * C, s);
        if (e != hipSuccess) return hip_fail(e, "hipMemsetAsync(counts)");
        if (first) hipLaunchKernelGGL((ens_accumulate_kernel<true, true>), grid, block, 0, s, probs, K, flips, acc, (float)M, mean_out, mask, counts, C, D, H, W, b);
        else hipLaunchKernelGGL((ens_accumulate_kernel<false, true>), grid, block, 0, s, probs, K, flips, acc, (float)M, mean_out, mask, counts, C, D, H, W, b);
    } else {
        if (first) hipLaunchKernelGGL((ens_accumulate_kernel<true, false>), grid, block, 0, s, probs, K, flips, acc, 1.f, mean_out, mask, counts, C, D, H, W, b);
        else hipLaunchKernelGGL((ens_accumulate_kernel<false, false>), grid, block, 0, s, probs, K, flips, acc, 1.f, mean_out, mask, counts, C, D, H, W, b);
    }
    RU_CHECK_LAUNCH("ens_accumulate_kernel");
    return RU_OK;
}

}  // namespace ru

using namespace ru;

extern "C" int ru_ens_accumulate(const float* probs, int K, unsigned flips, float* acc, int first, int C, int D, int H, int W, const int* lo, const int* size,
                                 ru_stream_t stream) {
    RU_REQUIRE(acc, "ru_ens_accumulate: null argument");
    return ens_accumulate_impl(probs, K, flips, acc, first, 0, nullptr, nullptr, nullptr, C, D, H, W, lo, size, (hipStream_t)stream, "ru_ens_accumulate");
}

extern "C" int ru_ens_accumulate_finalize(const float* probs, int K, unsigned flips, const float* acc, int first, int M, float* mean_out, unsigned char* mask,
                                          unsigned long long* counts, int C, int D, int H, int W, const int* lo, const int* size, ru_stream_t stream) {
    RU_REQUIRE(mask && counts && M >= 1, "ru_ens_accumulate_finalize: bad argument");
    return ens_accumulate_impl(probs, K, flips, const_cast<float*>(acc), first, M, mean_out, mask, counts, C, D, H, W, lo, size, (hipStream_t)stream,
                               "ru_ens_accumulate_finalize");
}

extern "C" int ru_ens_finalize(const float* acc, int M, float* mean_out, unsigned char* mask, unsigned long long* counts, int C, size_t Vbox, ru_stream_t stream) {
    RU_REQUIRE(acc && mask && counts && M >= 1 && C >= 1 && C <= 65535 && Vbox > 0, "ru_ens_finalize: bad argument");
    RU_REQUIRE(Vbox < (size_t)INT_MAX, "ru_ens_finalize: volume too large for 32-bit voxel indices");
    hipStream_t s = (hipStream_t)stream;
    hipError_t e = hipMemsetAsync(counts, 0, sizeof(unsigned long long) * C, s);
    if (e != hipSuccess) return hip_fail(e, "hipMemsetAsync(counts)");
    const bool vec = (Vbox & 3) == 0 && ((uintptr_t)acc & 15) == 0 && ((uintptr_t)mean_out & 15) == 0 && ((uintptr_t)mask & 3) == 0;
    if (vec) hipLaunchKernelGGL(ens_finalize_kernel<true>, dim3(grid1d(Vbox / 4, 256 * 2, 1024), (unsigned)C), dim3(256), 0, s, acc, (float)M, mean_out, mask, counts,
                                (unsigned)Vbox);
    else hipLaunchKernelGGL(ens_finalize_kernel<false>, dim3(grid1d(Vbox, 256 * 4, 1024), (unsigned)C), dim3(256), 0, s, acc, (float)M, mean_out, mask, counts,
                            (unsigned)Vbox);
    RU_CHECK_LAUNCH("ens_finalize_kernel");
    return RU_OK;
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
