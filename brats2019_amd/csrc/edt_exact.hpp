// Exact squared Euclidean distance transform of a [D][H][W] grid in integer arithmetic, separable over the axes (metrics.hip: the
// Hausdorff distance; surface.hip: HD95).  f holds one uint32 per voxel:
//   W pass  edt_row_pass, a device function: a wave writes the squared distance to the nearest site of its row from the row's site bits;
//   H pass  edt_line_kernel<false>: f(i) = min_j f(j) + (i - j)^2 over every H line, in place;
//   D pass  edt_line_kernel<true, Q>: the same minimum over every D line, but no distance map is written: the value at each QUERY voxel
//           goes to the functor Q, which says what a query voxel is and what becomes of its value (a maximum, a histogram).
// Squared distances stay exact integers: every axis is at most MAX_EXTENT = 512, so the largest is 3 * 511^2 < 2^20, and the "no site"
// sentinel 2^30 plus any (i - j)^2 stays below 2^31.
#pragma once
#include "mask_bits.hpp"

namespace ru {
namespace {

constexpr unsigned EDT_INF = 1u << 30;        // "no site"
constexpr int EDT_TW = 32;                    // W columns per tile of the line passes
constexpr int EDT_LINE_THREADS = 256;         // 32 columns x 8 line positions

__device__ __forceinline__ int edt_first_bit(u64 m) { return __ffsll((long long)m) - 1; }
__device__ __forceinline__ int edt_last_bit(u64 m) { return 63 - __clzll((long long)m); }

// One wave, one row: m[c] = the sites among the voxels 64 c .. 64 c + 63 (wave-uniform, bits >= W zero); frow[w] = the squared distance
// from w to the nearest site of the row, EDT_INF if the row has none.  Lane l takes the voxels l, 64 + l, ...
__device__ __forceinline__ void edt_row_pass(const u64 (&m)[MAX_WORDS], int W, unsigned* __restrict__ frow) {
    const int lane = threadIdx.x & 63;
    const u64 upto = lane == 63 ? ~0ull : (2ull << lane) - 1;
    // first site after each word, then a forward sweep with the last site before it
    int next[MAX_WORDS];
    int nx = 1 << 20;
#pragma unroll
    for (int c = MAX_WORDS - 1; c >= 0; --c) {
        next[c] = nx;
        if (m[c]) nx = c * 64 + edt_first_bit(m[c]);
    }
    int prev = -(1 << 20);
#pragma unroll
    for (int c = 0; c < MAX_WORDS; ++c) {
        if (c * 64 >= W) break;
        const int w = c * 64 + lane;
        if (w < W) {
            // nearest site at or left of w: in this word (bits <= lane) or the last site of an earlier word; at or right of w likewise
            const u64 below = m[c] & upto, above = m[c] >> lane;
            const int left = below ? c * 64 + edt_last_bit(below) : prev;
            const int right = above ? w + edt_first_bit(above) : next[c];
            const int best = min(w - left, right - w);
            frow[w] = best < MAX_EXTENT ? (unsigned)(best * best) : EDT_INF;
        }
        if (m[c]) prev = c * 64 + edt_last_bit(m[c]);
    }
}

// the H pass has no query: it rewrites the line
struct EdtInPlace {};

// grid (cdiv(W, 32), lines, items * 2), 256 threads, dynamic LDS L x 32 x 4 B; f = [items][2][V].  FINAL = false: the H pass (lines = D
// planes, L = H).  FINAL = true: the D pass (lines = H rows, L = D).  The block stages a tile of 32 neighbouring W columns over the whole
// line in LDS (coalesced 128-B row segments, at most 32 x 512 x 4 B = 64 KiB) and takes the minimum by brute force, 8 x 4 line positions
// per step.  Q (FINAL only), a copy per thread:
//   void begin(const MaskGeom&, int item, int t)       once; t = blockIdx.z & 1 is the transform, item = blockIdx.z >> 1
//   bool query(const MaskGeom&, int d, int h, int w)   is this voxel a query voxel?
//   void consume(unsigned sq)                          its squared distance
//   void finish()                                      once, reached by every thread of the block
template <bool FINAL, class Q>
__global__ __launch_bounds__(EDT_LINE_THREADS) void edt_line_kernel(unsigned* __restrict__ f, MaskGeom s, Q q) {
    extern __shared__ unsigned edt_lds[];
    const int x = threadIdx.x % EDT_TW, r = threadIdx.x / EDT_TW;
    constexpr int R = EDT_LINE_THREADS / EDT_TW;
    const int w = blockIdx.x * EDT_TW + x, a = blockIdx.y, t = blockIdx.z & 1, item = blockIdx.z >> 1;
    const int L = FINAL ? s.D : s.H;
    const size_t stride = FINAL ? (size_t)s.H * s.W : (size_t)s.W;
    const size_t off = FINAL ? (size_t)a * s.W + w : (size_t)a * s.H * s.W + w;       // voxel index of line element 0
    unsigned* __restrict__ fl = f + ((size_t)item * 2 + t) * s.V;
    const bool col = w < s.W;
    for (int i = r; i < L; i += R) edt_lds[i * EDT_TW + x] = col ? fl[off + i * stride] : EDT_INF;
    __syncthreads();
    if constexpr (FINAL) q.begin(s, item, t);
    for (int i0 = r; i0 < L; i0 += 4 * R) {
        bool on[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int i = i0 + u * R;
            on[u] = col && i < L;
            if constexpr (FINAL) {
                if (on[u]) on[u] = q.query(s, i, a, w);
            }
        }
        if (FINAL && !__any(on[0] || on[1] || on[2] || on[3])) continue;             // no query voxel here: nothing to reduce
        unsigned acc[4] = {EDT_INF, EDT_INF, EDT_INF, EDT_INF};
        for (int j = 0; j < L; ++j) {
            const unsigned fj = edt_lds[j * EDT_TW + x];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int dd = i0 + u * R - j;
                acc[u] = min(acc[u], fj + (unsigned)__mul24(dd, dd));
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (!on[u]) continue;
            if constexpr (FINAL) q.consume(acc[u]);
            else fl[off + (size_t)(i0 + u * R) * stride] = acc[u];                    // the block owns its lines: in place after the barrier
        }
    }
    if constexpr (FINAL) q.finish();
}

// both line passes of `items` pairs of transforms, on stream st
template <class Q>
inline int edt_line_passes(unsigned* f, const MaskGeom& s, int items, const Q& q, hipStream_t st) {
    hipLaunchKernelGGL((edt_line_kernel<false, EdtInPlace>), dim3(cdiv(s.W, EDT_TW), s.D, items * 2), dim3(EDT_LINE_THREADS),
                       (size_t)s.H * EDT_TW * sizeof(unsigned), st, f, s, EdtInPlace());
    RU_CHECK_LAUNCH("edt_line_kernel<H>");
    hipLaunchKernelGGL((edt_line_kernel<true, Q>), dim3(cdiv(s.W, EDT_TW), s.H, items * 2), dim3(EDT_LINE_THREADS),
                       (size_t)s.D * EDT_TW * sizeof(unsigned), st, f, s, q);
    RU_CHECK_LAUNCH("edt_line_kernel<D>");
    return RU_OK;
}

}  // namespace
}  // namespace ru
