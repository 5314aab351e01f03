// Bit-packed binary masks and the small reductions every device scorer needs (surface.hip, lesion.hip, metrics.hip; the zero and count
// helpers also serve overlap.hip, uncertainty.hip and ensemble.hip).  A mask of a [D][H][W] volume is D * H rows of WW = cdiv(W, 64)
// 64-bit words, bit x & 63 of word x >> 6 for voxel x; bits >= W of a row are ZERO (the surface and dilation shifts rely on it).
// Everything here has internal linkage: each translation unit that includes the header gets its own copy of the kernels it launches.
#pragma once
#include "ru_common.h"

namespace ru {
namespace {

typedef unsigned long long u64;

constexpr int MAX_EXTENT = 512;               // every axis of a scored volume: a row is at most 8 words, a squared distance < 2^20
constexpr int MAX_WORDS = MAX_EXTENT / 64;

struct MaskGeom {
    int D, H, W, WW;
    size_t V, words;                          // voxels of a volume, words of a bit plane
};

__host__ __device__ inline MaskGeom mask_geom(int D, int H, int W) {
    MaskGeom g;
    g.D = D;
    g.H = H;
    g.W = W;
    g.WW = (W + 63) / 64;
    g.V = (size_t)D * H * W;
    g.words = (size_t)D * H * g.WW;
    return g;
}

// kind RU_SURFACE_PROB: float32 [N][C][V], one mask per channel (x > 0.5).  RU_SURFACE_LABEL: uint8 [N][V], the three BraTS regions.
inline bool mask_shape_ok(int kind, int N, int C, int D, int H, int W) {
    return (kind == RU_SURFACE_PROB || (kind == RU_SURFACE_LABEL && C == 1)) && N > 0 && C > 0 && D >= 1 && H >= 1 && W >= 1 &&
           D <= MAX_EXTENT && H <= MAX_EXTENT && W <= MAX_EXTENT;
}

inline int mask_regions(int kind, int C) { return kind == RU_SURFACE_LABEL ? RU_SURFACE_REGIONS : C; }

// region k of a BraTS label: WT = {1, 2, 3, 4}, TC = {1, 3, 4}, ET = {3, 4} (the model's channel order); values above 4 are in none.
// (A shift into a per-region bit set computes the same and is what uncertainty.hip's histogram does with compile-time regions; with
// the run-time k of the pack kernels it made the uint8 pack 30 % slower, 111 -> 144 us on a 240 x 240 x 155 case.)
__device__ __forceinline__ bool brats_region(unsigned v, int k) {
    if (k == 0) return v >= 1u && v <= 4u;
    if (k == 1) return v == 1u || v == 3u || v == 4u;
    return v == 3u || v == 4u;
}

__device__ __forceinline__ bool mask_bit(const u64* __restrict__ plane, int WW, size_t row, int x) {
    return (plane[row * WW + (x >> 6)] >> (x & 63)) & 1ull;
}

// Block (d, nk) of a grid (D, N*K) with 256 threads packs plane d of the masks P (plane 0) and G (plane 1) of (n, k) = nk into
// bits[nk][4][words]: wave q takes the rows h = q, q + 4, ..., one ballot per word.  c = the wave's {|P|, |G|, |P & G|} (COUNTS only)
// and its invalid label voxels (KIND 1; a label above 4), the same in every lane.
template <int KIND, bool COUNTS>
__device__ __forceinline__ void mask_pack_rows(const void* __restrict__ pv, const void* __restrict__ gv, int C, int K, const MaskGeom& s,
                                               u64* __restrict__ bits, u64 (&c)[4]) {
    const int d = blockIdx.x, nk = blockIdx.y, n = nk / K, k = nk % K;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    u64* __restrict__ bp = bits + (size_t)nk * 4 * s.words;
    u64* __restrict__ bg = bp + s.words;
    const size_t base = KIND == 0 ? ((size_t)n * C + k) * s.V : (size_t)n * s.V;
    c[0] = c[1] = c[2] = c[3] = 0;
    for (int h = wave; h < s.H; h += 4) {
        const size_t row = (size_t)d * s.H + h;
        for (int w0 = 0; w0 < s.WW; ++w0) {                     // (whole waves: the ballots need every lane)
            const int w = w0 * 64 + lane;
            bool pm = false, gm = false, bad = false;
            if (w < s.W) {
                const size_t v = base + row * s.W + w;
                if (KIND == 0) {
                    pm = static_cast<const float*>(pv)[v] > 0.5f;
                    gm = static_cast<const float*>(gv)[v] > 0.5f;
                } else {
                    const unsigned a = static_cast<const unsigned char*>(pv)[v], b = static_cast<const unsigned char*>(gv)[v];
                    pm = brats_region(a, k);
                    gm = brats_region(b, k);
                    bad = a > 4u || b > 4u;
                }
            }
            const u64 mp = __ballot(pm), mg = __ballot(gm);
            if (COUNTS) {
                c[0] += __popcll(mp);
                c[1] += __popcll(mg);
                c[2] += __popcll(mp & mg);
            }
            if (KIND == 1) c[3] += __popcll(__ballot(bad));
            if (lane == 0) {
                bp[row * s.WW + w0] = mp;
                bg[row * s.WW + w0] = mg;
            }
        }
    }
}

// a[0 .. na) = 0 and b[0 .. nb) = 0 (b may be null with nb = 0).  A kernel node rather than a hipMemsetAsync: captured into a hipGraph,
// the memset was seen to leave such slots uncleared on replay.
template <typename A, typename B>
__global__ void zero2_kernel(A* __restrict__ a, size_t na, B* __restrict__ b, size_t nb) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < na + nb; i += stride) {
        if (i < na) a[i] = 0;
        else b[i - na] = 0;
    }
}

// *dst += the sum of `local` over a 256-thread workgroup: wave shuffle, four partials through LDS (sm[4]), one atomic
__device__ __forceinline__ void wg_count_add(unsigned local, unsigned* sm, u64* dst) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) local += __shfl_xor(local, o);
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = local;
    __syncthreads();
    if (threadIdx.x == 0) {
        const u64 n = (u64)sm[0] + sm[1] + sm[2] + sm[3];
        if (n) atomicAdd(dst, n);
    }
}

// acc[i] += mean over the N samples of values[n][i][column], rows of WIDTH values, i < nacc <= blockDim.x; samples summed in order
template <int WIDTH>
__global__ void column_mean_kernel(const double* __restrict__ values, double* __restrict__ acc, int N, int K, int nacc, int column) {
    const int i = threadIdx.x;
    if (i >= nacc) return;
    double sum = 0.0;
    for (int n = 0; n < N; ++n) sum += values[((size_t)n * K + i) * WIDTH + column];
    acc[i] += sum / (double)N;
}

}  // namespace
}  // namespace ru
