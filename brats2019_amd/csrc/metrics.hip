// Hausdorff distance of binary masks on the device: the counterpart of the reference's `Hausdorff_ITK` / `Hausdorff_ITKWT`
// (metrics.py:188-271, SimpleITK's HausdorffDistanceImageFilter at unit spacing on the (D, H, W) axes).
//
// HD(P, G) = max(directed(P, G), directed(G, P)), directed(A, B) = max over a in A of min over b in B of |a - b| (voxel centres).
// Per (sample n, channel k) two exact squared Euclidean distance transforms run in integer arithmetic (edt_exact.hpp), to G and to P:
//   pass W  (hd_pass_w_kernel): thresholds both masks on the fly, counts their voxels and hands each row's ballots to edt_row_pass;
//   pass H  (edt_line_kernel<false>): in place;
//   pass D  (edt_line_kernel<true, HdMax>): writes no distance map, it takes the max of d^2 over the voxels of the OTHER mask (P for the
//           transform to G, G for the one to P).
// hd_accumulate_kernel then applies the reference's bookkeeping (empty masks, the i-1 quirk), the float64 sqrt and the batch mean.
#include "ru_common.h"
#include "edt_exact.hpp"

namespace ru {
namespace {

// mask of sample n, channel k at voxel v.  mode 0: x > 0.5 (metrics.py:205-206).  mode 1: argmax over the channels > 0 (metrics.py:245-246);
// torch's argmax takes the first of equal maxima, so this is max(x[1:]) > x[0]
__device__ __forceinline__ bool hd_mask(const float* __restrict__ x, int mode, int C, size_t V, int n, int k, size_t v) {
    if (mode == 0) return x[((size_t)n * C + k) * V + v] > 0.5f;
    const float* b = x + (size_t)n * C * V + v;
    const float x0 = b[0];
    bool any = false;
    for (int c = 1; c < C; ++c) any |= b[(size_t)c * V] > x0;
    return any;
}

// grid (D, N*K), 256 threads: wave q takes the rows h = q, q + 4, ... of plane d.  f = [N*K][2][V]: transform 0 = to G, 1 = to P.
// out[nk*4 + 2] / [nk*4 + 3] += #P / #G.
__global__ __launch_bounds__(256) void hd_pass_w_kernel(const float* __restrict__ p, const float* __restrict__ g, int mode, int C, int K,
                                                        int D, int H, int W, unsigned* __restrict__ f, unsigned long long* __restrict__ out) {
    const int d = blockIdx.x, nk = blockIdx.y, n = nk / K, k = nk % K;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const size_t V = (size_t)D * H * W;
    unsigned* __restrict__ fg = f + ((size_t)nk * 2) * V;
    unsigned* __restrict__ fp = fg + V;
    unsigned long long cp = 0, cg = 0;
    for (int h = wave; h < H; h += 4) {
        const size_t row = ((size_t)d * H + h) * W;
        u64 mp[MAX_WORDS], mg[MAX_WORDS];
#pragma unroll
        for (int c = 0; c < MAX_WORDS; ++c) {
            const int w = c * 64 + lane;
            const bool in = w < W;
            mp[c] = __ballot(in && hd_mask(p, mode, C, V, n, k, row + w));
            mg[c] = __ballot(in && hd_mask(g, mode, C, V, n, k, row + w));
            cp += __popcll(mp[c]);
            cg += __popcll(mg[c]);
        }
        edt_row_pass(mg, W, fg + row);
        edt_row_pass(mp, W, fp + row);
    }
    if (lane == 0) {
        if (cp) atomicAdd(out + (size_t)nk * 4 + 2, cp);
        if (cg) atomicAdd(out + (size_t)nk * 4 + 3, cg);
    }
}

// the D pass's query: the transform to G (t = 0) is sampled on P and vice versa; out[nk*4 + t] = max of d^2, one atomicMax per wave
struct HdMax {
    const float *p, *g, *smp;
    int mode, C, K, n, k;
    unsigned long long* out;
    unsigned best;
    __device__ void begin(const MaskGeom&, int nk, int t) {
        smp = t == 0 ? p : g;
        n = nk / K;
        k = nk % K;
        out += (size_t)nk * 4 + t;
        best = 0;
    }
    __device__ bool query(const MaskGeom& s, int d, int h, int w) const { return hd_mask(smp, mode, C, s.V, n, k, ((size_t)d * s.H + h) * s.W + w); }
    __device__ void consume(unsigned sq) { best = max(best, sq); }
    __device__ void finish() {
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) best = max(best, (unsigned)__shfl_xor((int)best, m));
        if ((threadIdx.x & 63) == 0 && best) atomicMax(out, (unsigned long long)best);
    }
};

// metrics.py:208-228 (mode 0) / 248-263 (mode 1) from the squared maxima and counts, then metrics.py:230 / 265: acc += the batch mean.
// One thread per result column, samples in order (numpy's axis-0 sum is sequential; its 1-D pairwise sum is too below 8 samples).
__global__ void hd_accumulate_kernel(const unsigned long long* __restrict__ sq, double* __restrict__ acc, int N, int K, int nacc, int mode) {
    const int i = threadIdx.x;
    if (i >= nacc) return;
    double sum = 0.0;
    for (int n = 0; n < N; ++n) {
        const unsigned long long* q = sq + ((size_t)n * K + i) * 4;
        const bool empty_i = q[2] == 0 && q[3] == 0;
        const bool empty_next = mode == 0 && i + 1 < nacc && q[4 + 2] == 0 && q[4 + 3] == 0;
        double r;
        if (empty_next) {
            // The reference writes result[n, i-1] = 0 when BOTH masks of channel i are empty (metrics.py:215-217), an index slip that zeroes
            // the value already stored for the channel before.  For i = 0 it writes the last column, which step classes-2 then overwrites.
            // Kept: the project's metric is the reference's number.  So column i ends 0 when channel i+1 is empty on both sides ...
            r = 0.0;
        } else if (mode == 0 && empty_i) {
            r = 0.0;                                      // ... and when channel i itself is (never written, or zeroed by step 0 if i is last)
        } else if (q[2] == 0 || q[3] == 0) {
            r = 1e6;                                      // ITK raises on an empty image; the reference stores 1e+6 (metrics.py:220-226)
        } else {
            r = sqrt((double)(q[0] > q[1] ? q[0] : q[1]));
        }
        sum += r;
    }
    acc[i] += sum / (double)N;
}

size_t hd_workspace_bytes(int N, int C, int D, int H, int W, int mode) {
    if (N <= 0 || C <= 0 || D <= 0 || H <= 0 || W <= 0 || (mode != 0 && mode != 1)) return 0;
    const size_t K = mode == 0 ? (size_t)C : 1;
    return (size_t)N * K * 2 * ((size_t)D * H * W) * sizeof(unsigned);
}

}  // namespace
}  // namespace ru

using namespace ru;

extern "C" size_t ru_hausdorff_workspace_bytes(int N, int C, int D, int H, int W, int mode) { return hd_workspace_bytes(N, C, D, H, W, mode); }

extern "C" int ru_hausdorff_sq(const float* p, const float* g, int N, int C, int D, int H, int W, int mode, unsigned long long* out,
                               void* ws, size_t ws_bytes, ru_stream_t stream) {
    RU_REQUIRE(p && g && out && N > 0 && C > 0 && (mode == 0 || mode == 1), "ru_hausdorff_sq: bad argument");
    RU_REQUIRE(D > 0 && H > 0 && W > 0 && D <= MAX_EXTENT && H <= MAX_EXTENT && W <= MAX_EXTENT,
               "ru_hausdorff_sq: extents %d x %d x %d: every axis must be in [1, %d]", D, H, W, MAX_EXTENT);
    const int K = mode == 0 ? C : 1;
    RU_REQUIRE((long long)N * K * 2 <= 65535, "ru_hausdorff_sq: N * channels too large");
    RU_REQUIRE(ws && ws_bytes >= hd_workspace_bytes(N, C, D, H, W, mode), "ru_hausdorff_sq: workspace too small");
    hipStream_t s = (hipStream_t)stream;
    unsigned* f = (unsigned*)ws;
    hipLaunchKernelGGL((zero2_kernel<u64, u64>), dim3(cdiv(4 * N * K, 256)), dim3(256), 0, s, out, (size_t)4 * N * K, (u64*)nullptr, (size_t)0);
    RU_CHECK_LAUNCH("zero2_kernel");
    hipLaunchKernelGGL(hd_pass_w_kernel, dim3(D, N * K), dim3(256), 0, s, p, g, mode, C, K, D, H, W, f, out);
    RU_CHECK_LAUNCH("hd_pass_w_kernel");
    const HdMax q = {p, g, nullptr, mode, C, K, 0, 0, out, 0u};
    return edt_line_passes(f, mask_geom(D, H, W), N * K, q, s);
}

extern "C" int ru_hausdorff_accumulate(const unsigned long long* sq, double* acc, int N, int K, int nacc, int mode, ru_stream_t stream) {
    RU_REQUIRE(sq && acc && N > 0 && K > 0 && nacc > 0 && nacc <= K && nacc <= 64 && (mode == 0 || (mode == 1 && K == 1)),
               "ru_hausdorff_accumulate: bad argument");
    hipLaunchKernelGGL(hd_accumulate_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, sq, acc, N, K, nacc, mode);
    RU_CHECK_LAUNCH("hd_accumulate_kernel");
    return RU_OK;
}
