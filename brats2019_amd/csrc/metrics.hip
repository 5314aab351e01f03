// Hausdorff distance of binary masks on the device: the counterpart of the reference's `Hausdorff_ITK` / `Hausdorff_ITKWT`
// (metrics.py:188-271, SimpleITK's HausdorffDistanceImageFilter at unit spacing on the (D, H, W) axes).
//
// HD(P, G) = max(directed(P, G), directed(G, P)), directed(A, B) = max over a in A of min over b in B of |a - b| (voxel centres).
// Per (sample n, channel k) two exact squared Euclidean distance transforms run in integer arithmetic, separable over the axes:
//   pass W  (hd_pass_w_kernel):    thresholds both masks on the fly, counts their voxels and writes the 1-D squared distance to the
//                                  nearest site of each row, for the transform to G and the one to P;
//   pass H  (hd_pass_line_kernel<false>): f(i) = min_j f(j) + (i - j)^2 over the H line, in place;
//   pass D  (hd_pass_line_kernel<true>):  the same over the D line, fused with the reduction: it writes no distance map, it takes the
//                                  max of d^2 over the voxels of the OTHER mask (P for the transform to G, G for the one to P).
// The H / D passes stage a tile of 32 neighbouring W columns over the whole line in LDS (coalesced 128-B row segments, at most
// 32 x 512 x 4 B = 64 KiB) and take the minimum by brute force over the line.  Squared distances stay exact integers: the largest is
// 3 * 511^2 < 2^20, and the "no site" sentinel 2^30 plus any (i - j)^2 stays below 2^31.
// hd_accumulate_kernel then applies the reference's bookkeeping (empty masks, the i-1 quirk), the float64 sqrt and the batch mean.
#include "ru_common.h"

namespace ru {
namespace {

constexpr int HD_MAX_EXTENT = 512;       // every axis; the W pass holds a row in 8 ballots of 64
constexpr unsigned HD_INF = 1u << 30;    // "no site"
constexpr int HD_TW = 32;                // W columns per tile of the line passes
constexpr int HD_LINE_THREADS = 256;     // 32 columns x 8 line positions

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

__device__ __forceinline__ unsigned hd_row_sq(unsigned long long m, unsigned long long below, int w, int c, int lane, int prev, int next) {
    // nearest site at or left of w: in this chunk (bits <= lane) or the last site of an earlier chunk; at or right of w likewise
    const int left = below ? c * 64 + 63 - __clzll((long long)below) : prev;
    const unsigned long long above = m >> lane;
    const int right = above ? w + __ffsll((long long)above) - 1 : next;
    const int best = min(w - left, right - w);
    return best < HD_MAX_EXTENT ? (unsigned)(best * best) : HD_INF;
}

// out = 0 as a kernel node rather than a hipMemsetAsync: captured into a hipGraph, the memset was seen to leave these slots uncleared on replay
__global__ void hd_zero_kernel(unsigned long long* __restrict__ out, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = 0;
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
    const unsigned long long upto = lane == 63 ? ~0ull : (2ull << lane) - 1;
    unsigned long long cp = 0, cg = 0;
    for (int h = wave; h < H; h += 4) {
        const size_t row = ((size_t)d * H + h) * W;
        unsigned long long mp[8], mg[8];
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const int w = c * 64 + lane;
            const bool in = w < W;
            mp[c] = __ballot(in && hd_mask(p, mode, C, V, n, k, row + w));
            mg[c] = __ballot(in && hd_mask(g, mode, C, V, n, k, row + w));
            cp += __popcll(mp[c]);
            cg += __popcll(mg[c]);
        }
        // first site after each chunk (wave-uniform), then a forward sweep with the last site before it
        int nextp[8], nextg[8];
        int np_ = 1 << 20, ng_ = 1 << 20;
#pragma unroll
        for (int c = 7; c >= 0; --c) {
            nextp[c] = np_;
            nextg[c] = ng_;
            if (mp[c]) np_ = c * 64 + __ffsll((long long)mp[c]) - 1;
            if (mg[c]) ng_ = c * 64 + __ffsll((long long)mg[c]) - 1;
        }
        int prevp = -(1 << 20), prevg = -(1 << 20);
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            if (c * 64 >= W) break;
            const int w = c * 64 + lane;
            if (w < W) {
                fg[row + w] = hd_row_sq(mg[c], mg[c] & upto, w, c, lane, prevg, nextg[c]);
                fp[row + w] = hd_row_sq(mp[c], mp[c] & upto, w, c, lane, prevp, nextp[c]);
            }
            if (mp[c]) prevp = c * 64 + 63 - __clzll((long long)mp[c]);
            if (mg[c]) prevg = c * 64 + 63 - __clzll((long long)mg[c]);
        }
    }
    if (lane == 0) {
        if (cp) atomicAdd(out + (size_t)nk * 4 + 2, cp);
        if (cg) atomicAdd(out + (size_t)nk * 4 + 3, cg);
    }
}

// grid (cdiv(W, 32), lines, N*K*2), 256 threads, dynamic LDS L x 32 x 4 B.  FINAL = false: the H pass (lines = D planes, L = H, in place).
// FINAL = true: the D pass (lines = H rows, L = D): max of d^2 over the sample mask's voxels -> out[nk*4 + t], one atomicMax per wave.
template <bool FINAL>
__global__ __launch_bounds__(HD_LINE_THREADS) void hd_pass_line_kernel(unsigned* __restrict__ f, const float* __restrict__ p, const float* __restrict__ g,
                                                                       int mode, int C, int K, int D, int H, int W, unsigned long long* __restrict__ out) {
    extern __shared__ unsigned s[];
    const int x = threadIdx.x % HD_TW, r = threadIdx.x / HD_TW;
    constexpr int R = HD_LINE_THREADS / HD_TW;
    const int w = blockIdx.x * HD_TW + x, a = blockIdx.y, t = blockIdx.z & 1, nk = blockIdx.z >> 1;
    const size_t V = (size_t)D * H * W;
    const int L = FINAL ? D : H;
    const size_t stride = FINAL ? (size_t)H * W : (size_t)W;
    const size_t off = FINAL ? (size_t)a * W + w : (size_t)a * H * W + w;          // voxel index of line element 0
    unsigned* __restrict__ fl = f + ((size_t)nk * 2 + t) * V;
    const bool col = w < W;
    for (int i = r; i < L; i += R) s[i * HD_TW + x] = col ? fl[off + i * stride] : HD_INF;
    __syncthreads();
    const float* __restrict__ smp = t == 0 ? p : g;                                 // transform to G is sampled on P and vice versa
    const int n = nk / K, k = nk % K;
    unsigned best = 0;
    for (int i0 = r; i0 < L; i0 += 4 * R) {
        bool on[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int i = i0 + u * R;
            on[u] = col && i < L;
            if (FINAL && on[u]) on[u] = hd_mask(smp, mode, C, V, n, k, off + i * stride);
        }
        if (FINAL && !__any(on[0] || on[1] || on[2] || on[3])) continue;           // no voxel of the sample mask here: nothing to reduce
        unsigned acc[4] = {HD_INF, HD_INF, HD_INF, HD_INF};
        for (int j = 0; j < L; ++j) {
            const unsigned fj = s[j * HD_TW + x];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int dd = i0 + u * R - j;
                acc[u] = min(acc[u], fj + (unsigned)__mul24(dd, dd));
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (!on[u]) continue;
            if (FINAL) best = max(best, acc[u]);
            else fl[off + (size_t)(i0 + u * R) * stride] = acc[u];                // the block owns its lines: in place after the barrier
        }
    }
    if (FINAL) {
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) best = max(best, (unsigned)__shfl_xor((int)best, m));
        if ((threadIdx.x & 63) == 0 && best) atomicMax(out + (size_t)nk * 4 + t, (unsigned long long)best);
    }
}

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
    RU_REQUIRE(D > 0 && H > 0 && W > 0 && D <= HD_MAX_EXTENT && H <= HD_MAX_EXTENT && W <= HD_MAX_EXTENT,
               "ru_hausdorff_sq: extents %d x %d x %d: every axis must be in [1, %d]", D, H, W, HD_MAX_EXTENT);
    const int K = mode == 0 ? C : 1;
    RU_REQUIRE((long long)N * K * 2 <= 65535, "ru_hausdorff_sq: N * channels too large");
    RU_REQUIRE(ws && ws_bytes >= hd_workspace_bytes(N, C, D, H, W, mode), "ru_hausdorff_sq: workspace too small");
    hipStream_t s = (hipStream_t)stream;
    unsigned* f = (unsigned*)ws;
    hipLaunchKernelGGL(hd_zero_kernel, dim3(cdiv(4 * N * K, 256)), dim3(256), 0, s, out, 4 * N * K);
    RU_CHECK_LAUNCH("hd_zero_kernel");
    hipLaunchKernelGGL(hd_pass_w_kernel, dim3(D, N * K), dim3(256), 0, s, p, g, mode, C, K, D, H, W, f, out);
    RU_CHECK_LAUNCH("hd_pass_w_kernel");
    hipLaunchKernelGGL(hd_pass_line_kernel<false>, dim3(cdiv(W, HD_TW), D, N * K * 2), dim3(HD_LINE_THREADS), (size_t)H * HD_TW * sizeof(unsigned), s,
                       f, p, g, mode, C, K, D, H, W, out);
    RU_CHECK_LAUNCH("hd_pass_line_kernel<H>");
    hipLaunchKernelGGL(hd_pass_line_kernel<true>, dim3(cdiv(W, HD_TW), H, N * K * 2), dim3(HD_LINE_THREADS), (size_t)D * HD_TW * sizeof(unsigned), s,
                       f, p, g, mode, C, K, D, H, W, out);
    RU_CHECK_LAUNCH("hd_pass_line_kernel<D>");
    return RU_OK;
}

extern "C" int ru_hausdorff_accumulate(const unsigned long long* sq, double* acc, int N, int K, int nacc, int mode, ru_stream_t stream) {
    RU_REQUIRE(sq && acc && N > 0 && K > 0 && nacc > 0 && nacc <= K && nacc <= 64 && (mode == 0 || (mode == 1 && K == 1)),
               "ru_hausdorff_accumulate: bad argument");
    hipLaunchKernelGGL(hd_accumulate_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, sq, acc, N, K, nacc, mode);
    RU_CHECK_LAUNCH("hd_accumulate_kernel");
    return RU_OK;
}
