// elastic.hip -- elastic deformation of a training patch, the augmentation the reference's reader defines and leaves switched off
// (dataloader.py:24-48 `elastic_transform`; the call sites :177 / :180 are commented out, the draws at :166-168 are still made).
//
//   random_state.rand(*shape) * 2 - 1, three fields        a counter-based generator              -> elastic_noise_kernel   (ru_elastic_noise)
//   gaussian_filter(noise, sigma, mode="constant", cval=0) three separable float64 passes          -> elastic_weights_kernel, gauss_outer_kernel (axes 0, 1),
//     * alpha, * alpha, * (alpha / 2.5)                    in scipy's axis order 0, 1, 2              gauss_row_kernel (axis 2, scaled)     (ru_elastic_field)
//   map_coordinates(image, (x + dx, y + dy, z + dz),       order 1 on the image channels, order 0 on -> elastic_warp_kernel    (ru_elastic_warp)
//     order, mode='reflect'), then :184-204                the target channels, flips, transpose, gain, bias
//
// The field is float64 from the noise to the source coordinate, like scipy: a float32 filter misses the reference's displacements by 1e-6
// voxels, which moves order-0 picks next to a half-integer.  scipy's kernel: radius = int(4 * sigma + 0.5), w[x] = exp(-0.5 / sigma^2 * x^2) /
// sum, out[i] = sum_j w[i - j] in[j] over the j inside the volume.  The radius may exceed the extent (sigma 30 -> 120 taps each side of a
// 128-voxel axis), so a pass is a banded matrix product along its axis: every thread keeps a tile of outputs in registers and walks the
// inputs that reach it, reading the weights from a zero-padded copy in LDS (the padding stands in for the |i - j| > radius test).
#include "ru_common.h"
#include "pw_helpers.hpp"

#include <limits.h>
#include <math.h>

namespace ru {

constexpr int EL_MAX_RADIUS = 256;
constexpr int EL_WPAD = 128;                                   // zeros on each side of the 2 r + 1 weights: covers the widest output tile (128 along W)
constexpr int EL_WLEN = 2 * EL_MAX_RADIUS + 1 + 2 * EL_WPAD;   // 769 doubles
constexpr int EL_MAX_ROW = 512;                                // W extent the row pass stages in LDS
constexpr int EL_TI = 16;                                      // outputs per thread along the axis of an outer pass

// ---------------------------------------------------------------------------------------------------------------- noise
// splitmix64's finalizer (Steele, Lea, Flood 2014; public domain reference code by S. Vigna), applied twice: once to derive a stream key from
// (seed, field), once to the key advanced by the voxel's counter.  The value depends on (seed, field, linear voxel index) only.
__host__ __device__ __forceinline__ unsigned long long el_mix64(unsigned long long z) {
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
__global__ __launch_bounds__(256) void elastic_noise_kernel(double* __restrict__ out, unsigned long long k0, unsigned long long k1, unsigned long long k2,
                                                            unsigned V) {
    const unsigned long long key = blockIdx.y == 0 ? k0 : (blockIdx.y == 1 ? k1 : k2);
    double* o = out + (size_t)blockIdx.y * V;
    for (unsigned v = blockIdx.x * 256u + threadIdx.x; v < V; v += gridDim.x * 256u) {
        const unsigned long long z = el_mix64(key + ((unsigned long long)v + 1ull) * 0x9E3779B97F4A7C15ull);
        o[v] = (double)(z >> 11) * (2.0 / 9007199254740992.0) - 1.0;           // 53 bits -> [0, 2) - 1: every value is exact, the largest is 1 - 2^-52
    }
}

// ---------------------------------------------------------------------------------------------------------------- weights
// wpad[EL_WPAD + r + d] = exp(-0.5 / sigma^2 * d^2) / sum for |d| <= r, zero elsewhere.  One workgroup; the sum runs in index order.
__global__ __launch_bounds__(256) void elastic_weights_kernel(double* __restrict__ wpad, double sigma, int r) {
    __shared__ double e[2 * EL_MAX_RADIUS + 1];
    __shared__ double total;
    const int n = 2 * r + 1;
    const double q = -0.5 / (sigma * sigma);
    for (int i = threadIdx.x; i < n; i += 256) {
        const double d = (double)(i - r);
        e[i] = exp(q * (d * d));
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = 0.0;
        for (int i = 0; i < n; ++i) s += e[i];
        total = s;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < EL_WLEN; i += 256) {
        const int d = i - EL_WPAD;
        wpad[i] = (d >= 0 && d < n) ? e[d] / total : 0.0;
    }
}

// ---------------------------------------------------------------------------------------------------------------- axes 0 and 1
// in / out [outer][n][inner], filtered along n; inner is contiguous (a multiple of the W rows), so a wave reads and writes 512 contiguous
// bytes per step.  Workgroup = 64 columns x 4 tiles of EL_TI outputs; grid = (inner / 64, n / 64, outer).
__global__ __launch_bounds__(256) void gauss_outer_kernel(const double* __restrict__ in, double* __restrict__ out, const double* __restrict__ wpad, int r, int n,
                                                          unsigned inner) {
    __shared__ double sw[EL_WLEN];
    for (int i = threadIdx.x; i < EL_WLEN; i += 256) sw[i] = wpad[i];
    __syncthreads();
    const unsigned c = blockIdx.x * 64u + (threadIdx.x & 63u);
    const int i0 = ((int)blockIdx.y * 4 + (int)(threadIdx.x >> 6)) * EL_TI;
    if (c >= inner || i0 >= n) return;
    const size_t base = (size_t)blockIdx.z * (size_t)n * inner + c;
    double acc[EL_TI];
#pragma unroll
    for (int t = 0; t < EL_TI; ++t) acc[t] = 0.0;
    const int jlo = max(0, i0 - r), jhi = min(n - 1, i0 + EL_TI - 1 + r);
    const int wb = EL_WPAD + r - i0;                           // sw[wb + j - t] = weight of input j for output i0 + t; j - i0 - t in [-(r + TI - 1), r + TI - 1]
    for (int j = jlo; j <= jhi; ++j) {
        const double x = in[base + (size_t)j * inner];
#pragma unroll
        for (int t = 0; t < EL_TI; ++t) acc[t] = fma(sw[wb + j - t], x, acc[t]);
    }
#pragma unroll
    for (int t = 0; t < EL_TI; ++t)
        if (i0 + t < n) out[base + (size_t)(i0 + t) * inner] = acc[t];
}

// ---------------------------------------------------------------------------------------------------------------- axis 2
// One W row per wave, staged in LDS; lane l owns outputs l and l + 64 of each 128-wide tile.  The row value is a broadcast read, the weights
// are 64 consecutive doubles per read.  `scale` per field: alpha, alpha, alpha / 2.5 (one multiplication after the filter, as the reference).
__global__ __launch_bounds__(256) void gauss_row_kernel(const double* __restrict__ in, double* __restrict__ out, const double* __restrict__ wpad, int r, int n,
                                                        unsigned rows, unsigned rows_per_field, double s0, double s1, double s2) {
    __shared__ double sw[EL_WLEN];
    __shared__ double srow[4][EL_MAX_ROW];
    for (int i = threadIdx.x; i < EL_WLEN; i += 256) sw[i] = wpad[i];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const unsigned row = blockIdx.x * 4u + (unsigned)wave;
    const bool live = row < rows;
    if (live)
        for (int k = lane; k < n; k += 64) srow[wave][k] = in[(size_t)row * n + k];
    __syncthreads();
    if (!live) return;
    const unsigned f = row / rows_per_field;
    const double scale = f == 0 ? s0 : (f == 1 ? s1 : s2);
    const double* x = srow[wave];
    for (int kb = 0; kb < n; kb += 128) {
        const int ka = kb + lane, kc = ka + 64;
        const int jlo = max(0, kb - r), jhi = min(n - 1, kb + 127 + r);
        const int wb = EL_WPAD + r - ka;                       // sw[wb + j] = weight of input j for output ka: j - ka in [-(r + 63), r + 127], and
        double a = 0.0, b = 0.0;                               // sw[wb - 64 + j] for output kc: j - kc in [-(r + 127), r + 63] -- both inside the padding
        for (int j = jlo; j <= jhi; ++j) {
            const double v = x[j];
            a = fma(sw[wb + j], v, a);
            b = fma(sw[wb - 64 + j], v, b);
        }
        if (ka < n) out[(size_t)row * n + ka] = a * scale;
        if (kc < n) out[(size_t)row * n + kc] = b * scale;
    }
}

// ---------------------------------------------------------------------------------------------------------------- warp
struct ElasticWarpArgs {
    const float* data;           // [C][P0][P1][P2]
    const float* target;         // [T][P0][P1][P2]
    const double* disp;          // [3][P0][P1][P2]
    float* data_out;             // [C][Q0][Q1][P2]
    float* target_out;           // [T][Q0][Q1][P2]
    int C, T, P[3], flags;
    float gain[RU_AUG_MAXC], bias[RU_AUG_MAXC];
};
__device__ __forceinline__ int el_reflect(int i, int n) {      // half-sample symmetric extension (d c b a | a b c d | d c b a), periodic in 2 n
    int m = i % (2 * n);
    if (m < 0) m += 2 * n;
    return m < n ? m : 2 * n - 1 - m;
}
// One thread per OUTPUT voxel (after flips and transpose, so the stores are contiguous); the displacement is read at the voxel it came from.
// Every index goes through el_reflect, so no coordinate -- not even a NaN in `disp` -- reaches outside the patch.
__global__ __launch_bounds__(256) void elastic_warp_kernel(const ElasticWarpArgs a) {
    const int P0 = a.P[0], P1 = a.P[1], P2 = a.P[2];
    const bool tr = (a.flags & 8) != 0;
    const int Q1 = tr ? P0 : P1;
    const unsigned V = (unsigned)P0 * P1 * P2;
    for (unsigned o = blockIdx.x * 256u + threadIdx.x; o < V; o += gridDim.x * 256u) {
        const int k = (int)(o % (unsigned)P2);
        const unsigned rr = o / (unsigned)P2;
        const int j = (int)(rr % (unsigned)Q1), i = (int)(rr / (unsigned)Q1);
        const int pa = tr ? j : i, pb = tr ? i : j;            // indices before the transpose
        const int p[3] = {(a.flags & 1) ? P0 - 1 - pa : pa, (a.flags & 2) ? P1 - 1 - pb : pb, (a.flags & 4) ? P2 - 1 - k : k};
        const unsigned v = ((unsigned)p[0] * P1 + p[1]) * P2 + p[2];
        unsigned off[3][2], near[3];
        float wgt[3][2];
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) {
            double c = (double)p[ax] + a.disp[(size_t)ax * V + v];
            if (!(fabs(c) < 1.0e9)) c = 0.0;                   // NaN / overflow: keep the integer conversions defined
            const double f = floor(c);
            const int i0 = (int)f;
            const float t = (float)(c - f);
            const unsigned stride = ax == 0 ? (unsigned)P1 * P2 : (ax == 1 ? (unsigned)P2 : 1u);
            off[ax][0] = (unsigned)el_reflect(i0, a.P[ax]) * stride;
            off[ax][1] = (unsigned)el_reflect(i0 + 1, a.P[ax]) * stride;
            near[ax] = (unsigned)el_reflect((int)floor(c + 0.5), a.P[ax]) * stride;
            wgt[ax][0] = 1.f - t;
            wgt[ax][1] = t;
        }
        float acc[RU_AUG_MAXC];
#pragma unroll
        for (int c = 0; c < RU_AUG_MAXC; ++c) acc[c] = 0.f;
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int qa = q >> 2, qb = (q >> 1) & 1, qc = q & 1;
            const float w = wgt[0][qa] * wgt[1][qb] * wgt[2][qc];
            const unsigned s = off[0][qa] + off[1][qb] + off[2][qc];
#pragma unroll
            for (int c = 0; c < RU_AUG_MAXC; ++c)
                if (c < a.C) acc[c] += w * a.data[(size_t)c * V + s];
        }
#pragma unroll
        for (int c = 0; c < RU_AUG_MAXC; ++c)
            if (c < a.C) a.data_out[(size_t)c * V + o] = acc[c] * a.gain[c] + a.bias[c];
        const unsigned s0 = near[0] + near[1] + near[2];
        for (int c = 0; c < a.T; ++c) a.target_out[(size_t)c * V + o] = a.target[(size_t)c * V + s0];
    }
}

static int elastic_shape_ok(int P0, int P1, int P2, const char* who) {
    RU_REQUIRE(P0 > 0 && P1 > 0 && P2 > 0, "%s: the patch extents must be positive", who);
    RU_REQUIRE((size_t)P0 * P1 * P2 * 3 < (size_t)INT_MAX, "%s: patch too large for 32-bit voxel indices", who);
    return RU_OK;
}

}  // namespace ru

using namespace ru;

// workspace of ru_elastic_field: the padded weights + one [3][P0][P1][P2] float64 intermediate
extern "C" size_t ru_elastic_workspace_bytes(int P0, int P1, int P2) {
    if (P0 <= 0 || P1 <= 0 || P2 <= 0) return 0;
    return 256 + align_up(EL_WLEN * sizeof(double), 256) + align_up((size_t)3 * P0 * P1 * P2 * sizeof(double), 256);
}

extern "C" int ru_elastic_noise(unsigned long long seed, int P0, int P1, int P2, double* noise_out, ru_stream_t stream) {
    RU_REQUIRE(noise_out, "ru_elastic_noise: null argument");
    if (int rc = elastic_shape_ok(P0, P1, P2, "ru_elastic_noise")) return rc;
    const unsigned V = (unsigned)P0 * P1 * P2;
    unsigned long long key[3];
    for (int f = 0; f < 3; ++f) key[f] = el_mix64(seed + (unsigned long long)(f + 1) * 0x9E3779B97F4A7C15ull);
    hipLaunchKernelGGL(elastic_noise_kernel, dim3(grid1d(V, 256 * 4, 4096), 3), dim3(256), 0, (hipStream_t)stream, noise_out, key[0], key[1], key[2], V);
    RU_CHECK_LAUNCH("elastic_noise_kernel");
    return RU_OK;
}

extern "C" int ru_elastic_field(const double* noise, double sigma, double alpha, int P0, int P1, int P2, double* disp_out, void* ws, size_t ws_bytes,
                                ru_stream_t stream) {
    RU_REQUIRE(noise && disp_out && noise != disp_out, "ru_elastic_field: null argument, or noise and disp_out are the same buffer");
    if (int rc = elastic_shape_ok(P0, P1, P2, "ru_elastic_field")) return rc;
    RU_REQUIRE(sigma > 0.0 && sigma < 1.0e6 && alpha == alpha, "ru_elastic_field: sigma must be positive and finite (got %g), alpha a number", sigma);
    const int r = (int)(4.0 * sigma + 0.5);                    // scipy: lw = int(truncate * sd + 0.5), truncate = 4
    RU_REQUIRE(r <= EL_MAX_RADIUS, "ru_elastic_field: radius int(4 sigma + 0.5) = %d exceeds %d", r, EL_MAX_RADIUS);
    RU_REQUIRE(P2 <= EL_MAX_ROW, "ru_elastic_field: W extent %d exceeds %d", P2, EL_MAX_ROW);
    RU_REQUIRE(3 * (size_t)P0 <= 65535, "ru_elastic_field: D extent %d exceeds %d", P0, 65535 / 3);      // axis 1 runs (field, D) as grid.z
    RU_REQUIRE(ws && ws_bytes >= ru_elastic_workspace_bytes(P0, P1, P2), "ru_elastic_field: workspace too small");
    char* base = (char*)align_up((size_t)ws, 256);
    double* wpad = (double*)base;
    double* tmp = (double*)(base + align_up(EL_WLEN * sizeof(double), 256));
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(elastic_weights_kernel, dim3(1), dim3(256), 0, s, wpad, sigma, r);
    RU_CHECK_LAUNCH("elastic_weights_kernel");
    const unsigned in0 = (unsigned)P1 * P2, in1 = (unsigned)P2;
    hipLaunchKernelGGL(gauss_outer_kernel, dim3(cdiv((int)in0, 64), cdiv(P0, 4 * EL_TI), 3), dim3(256), 0, s, noise, disp_out, wpad, r, P0, in0);
    RU_CHECK_LAUNCH("gauss_outer_kernel");
    hipLaunchKernelGGL(gauss_outer_kernel, dim3(cdiv((int)in1, 64), cdiv(P1, 4 * EL_TI), 3 * P0), dim3(256), 0, s, disp_out, tmp, wpad, r, P1, in1);
    RU_CHECK_LAUNCH("gauss_outer_kernel");
    const unsigned rows = 3u * P0 * P1;
    hipLaunchKernelGGL(gauss_row_kernel, dim3((rows + 3) / 4), dim3(256), 0, s, tmp, disp_out, wpad, r, P2, rows, rows / 3, alpha, alpha, alpha / 2.5);
    RU_CHECK_LAUNCH("gauss_row_kernel");
    return RU_OK;
}

extern "C" int ru_elastic_warp(const float* data_in, int C, const float* target_in, int T, const double* disp, int P0, int P1, int P2, int flags,
                               const float* gain, const float* bias, float* data_out, float* target_out, ru_stream_t stream) {
    RU_REQUIRE(disp && C >= 0 && C <= RU_AUG_MAXC && T >= 0 && T <= RU_AUG_MAXC && C + T > 0, "ru_elastic_warp: 0..%d image and target channels, at least one", RU_AUG_MAXC);
    RU_REQUIRE((C == 0 || (data_in && data_out && gain && bias)) && (T == 0 || (target_in && target_out)), "ru_elastic_warp: null argument");
    RU_REQUIRE(data_in != data_out || C == 0, "ru_elastic_warp: the warp cannot run in place");
    RU_REQUIRE(target_in != target_out || T == 0, "ru_elastic_warp: the warp cannot run in place");
    RU_REQUIRE((flags & ~15) == 0, "ru_elastic_warp: flags are bits 0..3");
    if (int rc = elastic_shape_ok(P0, P1, P2, "ru_elastic_warp")) return rc;
    ElasticWarpArgs a{};
    a.data = data_in; a.target = target_in; a.disp = disp; a.data_out = data_out; a.target_out = target_out;
    a.C = C; a.T = T; a.P[0] = P0; a.P[1] = P1; a.P[2] = P2; a.flags = flags;
    for (int c = 0; c < C; ++c) { a.gain[c] = gain[c]; a.bias[c] = bias[c]; }
    hipLaunchKernelGGL(elastic_warp_kernel, dim3(grid1d((size_t)P0 * P1 * P2, 256, 8192)), dim3(256), 0, (hipStream_t)stream, a);
    RU_CHECK_LAUNCH("elastic_warp_kernel");
    return RU_OK;
}
