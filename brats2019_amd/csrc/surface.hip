// BraTS challenge metrics on the device: per (sample n, region k) the Dice, sensitivity, specificity and 95th-percentile surface
// Hausdorff distance (HD95) of two binary masks P (prediction) and G (target), distances in voxels between voxel centres at unit spacing.
//
//   surface  dA = { v in A : one of v's 6 face neighbours is not in A or lies outside the grid }
//   S        = { d(v, dG) : v in dP } + { d(v, dP) : v in dG }, a multiset of |dP| + |dG| exact integer squared distances
//   HD95     = numpy.percentile(sqrt(S), 95), numpy's default `linear` method reproduced operation by operation
//
// Per call, for every (n, k):
//   zero2_kernel          : clears the counts and the histograms (mask_bits.hpp).
//   sf_pack_kernel<KIND>  : the masks as bit rows, and |P|, |G|, |P & G| (and the invalid label voxels) by popcount (mask_bits.hpp,
//                           mask_pack_rows).  KIND 0: float32 [N][C][V], mask = x > 0.5 per channel.  KIND 1: uint8 label volumes
//                           [N][V], regions WT / TC / ET (3 counts as 4).
//   sf_surface_w_kernel   : one wave per row: lane c derives word c of both surfaces bit-parallel, m & ~(m & left & right & the four
//                           neighbour rows), zeros outside the grid; then the W pass of two exact squared distance transforms (to dG and
//                           to dP) from those words (edt_exact.hpp, edt_row_pass).
//   edt_line_kernel       : the H pass in place; the D pass (<true, SfHist>) writes no distance map: at every voxel of the QUERY surface
//                           (dP for the transform to dG, dG for the one to dP) it adds one count to the (n, k) histogram of squared
//                           distances, (D-1)^2 + (H-1)^2 + (W-1)^2 + 1 bins.
//   sf_select_kernel      : one workgroup per (n, k): a prefix scan over the histogram finds the order statistics s_(i), s_(j), then
//                           the empty rules and numpy's lerp; writes {Dice, sensitivity, specificity, HD95} in float64.
//   sf_tolerance_kernel   : (ru_surface_distances and the packed sibling only) one workgroup per (n, k) rereads the histogram: the counts
//                           of the distances within each of T <= RU_SURFACE_MAX_TOL tolerances (64-bit integers), sum h_b sqrt(b) in
//                           float64 (per-thread partials in bin order, then a fixed LDS tree) and the largest non-empty bin; writes
//                           {NSD_0..NSD_T-1, ASSD, HD}.  The tolerances are integer bin limits passed by value: nothing is uploaded.
// column_mean_kernel (a call of its own) adds the batch mean of one of the four columns to a float64 device accumulator.
#include "ru_common.h"
#include "surface_packed.hpp"
#include "edt_exact.hpp"

namespace ru {
namespace {

constexpr int SF_SELECT_THREADS = 1024;
constexpr double SF_Q = 0.95;             // numpy: 95 / 100 in float64

// word c of row (d, h) of the surface of the mask in `b`: the voxels with a face neighbour outside the mask or the grid
__device__ __forceinline__ u64 sf_surface_word(const u64* __restrict__ b, int d, int h, int c, int D, int H, int WW) {
    const size_t base = ((size_t)d * H + h) * WW;
    const u64 m = b[base + c];
    if (!m) return 0;
    const u64 prev = c > 0 ? b[base + c - 1] : 0, next = c + 1 < WW ? b[base + c + 1] : 0;
    u64 in = m & ((m << 1) | (prev >> 63)) & ((m >> 1) | (next << 63));      // W - 1 and W + 1; bits >= W of a row are zero
    in &= h > 0 ? b[base - WW + c] : 0;
    in &= h + 1 < H ? b[base + WW + c] : 0;
    in &= d > 0 ? b[base - (size_t)H * WW + c] : 0;
    in &= d + 1 < D ? b[base + (size_t)H * WW + c] : 0;
    return m & ~in;
}

// grid (D, N*K), 256 threads.  counts[nk*6 + 0..2, 5] += |P|, |G|, |P & G|, invalid
template <int KIND>
__global__ __launch_bounds__(256) void sf_pack_kernel(const void* __restrict__ pv, const void* __restrict__ gv, int C, int K, MaskGeom s,
                                                      u64* __restrict__ bits, u64* __restrict__ counts) {
    u64 c[4];
    mask_pack_rows<KIND, true>(pv, gv, C, K, s, bits, c);
    if ((threadIdx.x & 63) == 0) {
        u64* q = counts + (size_t)blockIdx.y * RU_SURFACE_COUNTS;
        if (c[0]) atomicAdd(q + 0, c[0]);
        if (c[1]) atomicAdd(q + 1, c[1]);
        if (c[2]) atomicAdd(q + 2, c[2]);
        if (c[3]) atomicAdd(q + RU_SURFACE_C_INVALID, c[3]);
    }
}

// grid (D, N*K), 256 threads, one wave per row.  f = [N*K][2][V]: transform 0 = to dG, 1 = to dP.  counts[nk*6 + 3 / 4] += |dP| / |dG|.
__global__ __launch_bounds__(256) void sf_surface_w_kernel(MaskGeom s, u64* __restrict__ bits, unsigned* __restrict__ f, u64* __restrict__ counts) {
    const int d = blockIdx.x, nk = blockIdx.y;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const u64* __restrict__ bp = bits + (size_t)nk * 4 * s.words;
    const u64* __restrict__ bg = bp + s.words;
    u64* __restrict__ sp = bits + ((size_t)nk * 4 + 2) * s.words;
    u64* __restrict__ sg = sp + s.words;
    unsigned* __restrict__ fg = f + (size_t)nk * 2 * s.V;
    unsigned* __restrict__ fp = fg + s.V;
    unsigned csp = 0, csg = 0;
    for (int h = wave; h < s.H; h += 4) {
        const size_t row = (size_t)d * s.H + h;
        u64 wp = 0, wg = 0;
        if (lane < s.WW) {
            wp = sf_surface_word(bp, d, h, lane, s.D, s.H, s.WW);
            wg = sf_surface_word(bg, d, h, lane, s.D, s.H, s.WW);
            sp[row * s.WW + lane] = wp;
            sg[row * s.WW + lane] = wg;
            csp += __popcll(wp);
            csg += __popcll(wg);
        }
        u64 mp[MAX_WORDS], mg[MAX_WORDS];
#pragma unroll
        for (int c = 0; c < MAX_WORDS; ++c) {
            mp[c] = c < s.WW ? __shfl(wp, c) : 0;
            mg[c] = c < s.WW ? __shfl(wg, c) : 0;
        }
        edt_row_pass(mg, s.W, fg + row * s.W);
        edt_row_pass(mp, s.W, fp + row * s.W);
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        csp += __shfl_xor(csp, m);
        csg += __shfl_xor(csg, m);
    }
    if (lane == 0) {
        u64* q = counts + (size_t)nk * RU_SURFACE_COUNTS;
        if (csp) atomicAdd(q + 3, (u64)csp);
        if (csg) atomicAdd(q + 4, (u64)csg);
    }
}

// the D pass's query: the transform to dG (t = 0) is sampled on dP (plane 2), the one to dP on dG (plane 3); one histogram count per voxel
struct SfHist {
    const u64* plane;
    unsigned* hist;
    size_t bins;
    __device__ void begin(const MaskGeom& s, int nk, int t) {
        plane += ((size_t)nk * 4 + 2 + t) * s.words;
        hist += (size_t)nk * bins;
    }
    __device__ bool query(const MaskGeom& s, int d, int h, int w) const { return mask_bit(plane, s.WW, (size_t)d * s.H + h, w); }
    __device__ void consume(unsigned sq) {
        if (sq < bins) atomicAdd(hist + sq, 1u);                                      // >= bins only without sites: the empty rules decide
    }
    __device__ void finish() {}
};

// numpy's _lerp: a + (b - a) * t, or b - (b - a) * (1 - t) where t >= 0.5; two roundings each, no fused multiply-add
__device__ __forceinline__ double sf_lerp(double a, double b, double t) {
#pragma clang fp contract(off)
    const double diff = b - a;
    return t >= 0.5 ? b - diff * (1.0 - t) : a + diff * t;
}

// grid (N*K), SF_SELECT_THREADS threads.  out[nk*4 + RU_SURFACE_DICE / _SENS / _SPEC / _HD95].
__global__ __launch_bounds__(SF_SELECT_THREADS) void sf_select_kernel(const unsigned* __restrict__ hist, size_t V, size_t bins, const u64* __restrict__ counts,
                                                                      double empty_value, double* __restrict__ out) {
    __shared__ u64 scan[SF_SELECT_THREADS];
    __shared__ unsigned pick[2];
    const int nk = blockIdx.x, tid = threadIdx.x;
    const u64* cn = counts + (size_t)nk * RU_SURFACE_COUNTS;
    const u64 P = cn[0], G = cn[1], TP = cn[2], n = cn[3] + cn[4];
    double hd;
    if (P == 0 && G == 0) {
        hd = 0.0;
    } else if (P == 0 || G == 0) {
        hd = empty_value;
    } else {                                                                          // both surfaces non-empty: n >= 2
        const double x = (double)(n - 1) * SF_Q;
        const u64 i = (u64)floor(x), j = i + 1 < n ? i + 1 : n - 1;
        const unsigned* __restrict__ hn = hist + (size_t)nk * bins;
        const size_t chunk = (bins + SF_SELECT_THREADS - 1) / SF_SELECT_THREADS;
        const size_t lo = min(bins, (size_t)tid * chunk), hi = min(bins, lo + chunk);
        u64 sum = 0;
        for (size_t b = lo; b < hi; ++b) sum += hn[b];
        scan[tid] = sum;
        __syncthreads();
        for (int o = 1; o < SF_SELECT_THREADS; o <<= 1) {                             // inclusive scan of the chunk sums
            const u64 v = tid >= o ? scan[tid - o] : 0;
            __syncthreads();
            scan[tid] += v;
            __syncthreads();
        }
        const u64 incl = scan[tid], excl = incl - sum;
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const u64 rank = e ? j : i;                                               // s_(rank) = the first bin whose running count exceeds rank
            if (excl <= rank && rank < incl) {
                u64 run = excl;
                for (size_t b = lo; b < hi; ++b) {
                    run += hn[b];
                    if (run > rank) {
                        pick[e] = (unsigned)b;
                        break;
                    }
                }
            }
        }
        __syncthreads();
        hd = sf_lerp(sqrt((double)pick[0]), sqrt((double)pick[1]), x - (double)i);
    }
    if (tid != 0) return;
    double* o = out + (size_t)nk * 4;
    o[RU_SURFACE_DICE] = P + G == 0 ? 1.0 : (double)(2 * TP) / (double)(P + G);
    o[RU_SURFACE_SENS] = G == 0 ? 1.0 : (double)TP / (double)G;
    o[RU_SURFACE_SPEC] = V == G ? 1.0 : (double)((V - G) - (P - TP)) / (double)(V - G);
    o[RU_SURFACE_HD95] = hd;
}

// the tolerances of one call, by value: bin b counts for tolerance t when b <= tb[t]
struct SfTol {
    unsigned tb[RU_SURFACE_MAX_TOL];
    int T;
    double* out;                                                                      // [NK][T + 2], or NULL: no extras
};

// grid (N*K), SF_SELECT_THREADS threads.  ex[nk*(T+2) + 0..T-1] = NSD_t, [T] = ASSD, [T+1] = HD.
__global__ __launch_bounds__(SF_SELECT_THREADS) void sf_tolerance_kernel(const unsigned* __restrict__ hist, size_t bins, const u64* __restrict__ counts,
                                                                         double empty_value, SfTol tol) {
#pragma clang fp contract(off)
    __shared__ double tree[SF_SELECT_THREADS];
    __shared__ u64 wsum[SF_SELECT_THREADS / 64][RU_SURFACE_MAX_TOL];
    __shared__ unsigned wmax[SF_SELECT_THREADS / 64];
    const int nk = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const u64* cn = counts + (size_t)nk * RU_SURFACE_COUNTS;
    const u64 P = cn[0], G = cn[1], n = cn[3] + cn[4];
    double* o = tol.out + (size_t)nk * (tol.T + 2);
    if (P == 0 || G == 0) {                                                           // (uniform over the workgroup)
        if (tid == 0) {
            const bool both = P == 0 && G == 0;
            for (int t = 0; t < tol.T; ++t) o[t] = both ? 1.0 : 0.0;
            o[tol.T] = o[tol.T + 1] = both ? 0.0 : empty_value;
        }
        return;
    }
    const unsigned* __restrict__ hn = hist + (size_t)nk * bins;
    const size_t chunk = (bins + SF_SELECT_THREADS - 1) / SF_SELECT_THREADS;
    const size_t lo = min(bins, (size_t)tid * chunk), hi = min(bins, lo + chunk);
    u64 c[RU_SURFACE_MAX_TOL];
#pragma unroll
    for (int t = 0; t < RU_SURFACE_MAX_TOL; ++t) c[t] = 0;
    double a = 0.0;
    unsigned top = 0;
    for (size_t b = lo; b < hi; ++b) {
        const unsigned h = hn[b];
        if (!h) continue;
        top = (unsigned)b;
#pragma unroll
        for (int t = 0; t < RU_SURFACE_MAX_TOL; ++t) c[t] += (t < tol.T && b <= (size_t)tol.tb[t]) ? h : 0u;
        a += (double)h * sqrt((double)b);                                             // three roundings: sqrt, product, sum
    }
    // integers: wave shuffles, then the 16 wave sums; order is free, the sums are exact
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
#pragma unroll
        for (int t = 0; t < RU_SURFACE_MAX_TOL; ++t) c[t] += __shfl_xor(c[t], m);
        top = max(top, (unsigned)__shfl_xor((int)top, m));
    }
    if (lane == 0) {
#pragma unroll
        for (int t = 0; t < RU_SURFACE_MAX_TOL; ++t) wsum[wave][t] = c[t];
        wmax[wave] = top;
    }
    // float64: the fixed tree, thread i adds thread i + o
    tree[tid] = a;
    __syncthreads();
    for (int s = SF_SELECT_THREADS / 2; s >= 1; s >>= 1) {
        if (tid < s) tree[tid] += tree[tid + s];
        __syncthreads();
    }
    if (tid != 0) return;
    for (int t = 0; t < tol.T; ++t) {
        u64 ct = 0;
        for (int w = 0; w < SF_SELECT_THREADS / 64; ++w) ct += wsum[w][t];
        o[t] = (double)ct / (double)n;
    }
    unsigned m = 0;
    for (int w = 0; w < SF_SELECT_THREADS / 64; ++w) m = max(m, wmax[w]);
    o[tol.T] = tree[0] / (double)n;
    o[tol.T + 1] = sqrt((double)m);
}

// the tolerances of a call, checked: T in [0, RU_SURFACE_MAX_TOL], host limits, a destination
bool sf_tol_make(const unsigned* tol_bins, int T, double* extras, SfTol* tol) {
    if (T < 0 || T > RU_SURFACE_MAX_TOL || (T > 0 && !tol_bins) || !extras) return false;
    for (int t = 0; t < RU_SURFACE_MAX_TOL; ++t) tol->tb[t] = t < T ? tol_bins[t] : 0u;
    tol->T = T;
    tol->out = extras;
    return true;
}

// workspace slices of NK pairs of masks: per pair 4 bit planes (P, G, dP, dG) of `words` each, 2 distance maps of V, one histogram of `bins`
struct SfWs {
    u64* bits;
    unsigned *f, *hist;
    size_t bins, bytes;
};

SfWs sf_layout(void* ws, size_t NK, int D, int H, int W) {
    const MaskGeom s = mask_geom(D, H, W);
    SfWs w;
    w.bits = (u64*)ws;
    w.f = (unsigned*)(w.bits + NK * 4 * s.words);
    w.hist = w.f + NK * 2 * s.V;
    w.bins = (size_t)(D - 1) * (D - 1) + (size_t)(H - 1) * (H - 1) + (size_t)(W - 1) * (W - 1) + 1;
    w.bytes = NK * (4 * s.words * sizeof(u64) + 2 * s.V * sizeof(unsigned) + w.bins * sizeof(unsigned));
    return w;
}

size_t sf_workspace_bytes(int kind, int N, int C, int D, int H, int W) {
    if (!mask_shape_ok(kind, N, C, D, H, W)) return 0;
    return sf_layout(nullptr, (size_t)N * mask_regions(kind, C), D, H, W).bytes;
}

// clears the first `ncounts` counts and the histograms, then (pack, if any, and) the passes on NK pairs of packed masks
template <class Pack>
int sf_run(int D, int H, int W, int NK, void* ws, u64* counts, size_t ncounts, double empty_value, double* values, const SfTol& tol, hipStream_t st,
           Pack pack) {
    const MaskGeom s = mask_geom(D, H, W);
    const SfWs w = sf_layout(ws, (size_t)NK, D, H, W);
    const size_t nhist = (size_t)NK * w.bins;
    hipLaunchKernelGGL((zero2_kernel<u64, unsigned>), dim3((unsigned)std::min<size_t>(1024, (ncounts + nhist + 255) / 256)), dim3(256), 0, st, counts,
                       ncounts, w.hist, nhist);
    RU_CHECK_LAUNCH("zero2_kernel");
    const int rc = pack(s, w.bits);
    if (rc) return rc;
    hipLaunchKernelGGL(sf_surface_w_kernel, dim3(D, NK), dim3(256), 0, st, s, w.bits, w.f, counts);
    RU_CHECK_LAUNCH("sf_surface_w_kernel");
    const SfHist q = {w.bits, w.hist, w.bins};
    const int rl = edt_line_passes(w.f, s, NK, q, st);
    if (rl) return rl;
    hipLaunchKernelGGL(sf_select_kernel, dim3(NK), dim3(SF_SELECT_THREADS), 0, st, w.hist, s.V, w.bins, counts, empty_value, values);
    RU_CHECK_LAUNCH("sf_select_kernel");
    if (tol.out) {
        hipLaunchKernelGGL(sf_tolerance_kernel, dim3(NK), dim3(SF_SELECT_THREADS), 0, st, w.hist, w.bins, counts, empty_value, tol);
        RU_CHECK_LAUNCH("sf_tolerance_kernel");
    }
    return RU_OK;
}

const SfTol SF_NO_TOL = {{0, 0, 0, 0, 0, 0, 0, 0}, 0, nullptr};

// acc[i] += the batch mean of column `column` of rows of `ncols` (column_mean_kernel's sum, for a row stride known at run time)
__global__ void sf_extras_mean_kernel(const double* __restrict__ values, double* __restrict__ acc, int N, int K, int nacc, int ncols, int column) {
    const int i = threadIdx.x;
    if (i >= nacc) return;
    double sum = 0.0;
    for (int n = 0; n < N; ++n) sum += values[((size_t)n * K + i) * ncols + column];
    acc[i] += sum / (double)N;
}

}  // namespace

size_t sf_packed_workspace_bytes(int items, int D, int H, int W) { return sf_workspace_bytes(RU_SURFACE_PROB, 1, items, D, H, W); }

unsigned long long* sf_packed_bits(void* ws) { return (u64*)ws; }

int sf_packed_run(int items, int D, int H, int W, void* ws, unsigned long long* counts, double empty_value, double* values, hipStream_t st) {
    RU_REQUIRE(ws && counts && values && items > 0 && (long long)items * 2 <= 65535 && mask_shape_ok(RU_SURFACE_PROB, 1, items, D, H, W),
               "sf_packed_run: bad argument");
    return sf_run(D, H, W, items, ws, counts, 0, empty_value, values, SF_NO_TOL, st, [](const MaskGeom&, u64*) { return RU_OK; });
}

int sf_packed_run_extras(int items, int D, int H, int W, void* ws, unsigned long long* counts, double empty_value, double* values,
                         const unsigned* tol_bins, int T, double* extras, hipStream_t st) {
    RU_REQUIRE(ws && counts && values && items > 0 && (long long)items * 2 <= 65535 && mask_shape_ok(RU_SURFACE_PROB, 1, items, D, H, W),
               "sf_packed_run_extras: bad argument");
    SfTol tol;
    RU_REQUIRE(sf_tol_make(tol_bins, T, extras, &tol), "sf_packed_run_extras: bad tolerances (T = %d)", T);
    return sf_run(D, H, W, items, ws, counts, 0, empty_value, values, tol, st, [](const MaskGeom&, u64*) { return RU_OK; });
}

}  // namespace ru

using namespace ru;

extern "C" size_t ru_surface_workspace_bytes(int kind, int N, int C, int D, int H, int W) { return sf_workspace_bytes(kind, N, C, D, H, W); }

namespace {

int sf_entry(const char* who, const void* pred, const void* target, int kind, int N, int C, int D, int H, int W, double empty_value, double* values,
             unsigned long long* counts, const SfTol& tol, void* ws, size_t ws_bytes, ru_stream_t stream) {
    RU_REQUIRE(pred && target && values && counts && N > 0 && C > 0, "%s: bad argument", who);
    RU_REQUIRE(kind == RU_SURFACE_PROB || (kind == RU_SURFACE_LABEL && C == 1), "%s: bad kind %d (C = %d)", who, kind, C);
    RU_REQUIRE(D >= 1 && H >= 1 && W >= 1 && D <= MAX_EXTENT && H <= MAX_EXTENT && W <= MAX_EXTENT,
               "%s: extents %d x %d x %d: every axis must be in [1, %d]", who, D, H, W, MAX_EXTENT);
    const int K = mask_regions(kind, C), NK = N * K;
    RU_REQUIRE((long long)N * K * 2 <= 65535, "%s: N * regions = %lld: the grid needs 2 * N * regions <= 65535", who, (long long)N * K);
    RU_REQUIRE(ws && ws_bytes >= sf_workspace_bytes(kind, N, C, D, H, W), "%s: workspace too small", who);
    hipStream_t st = (hipStream_t)stream;
    return sf_run(D, H, W, NK, ws, counts, (size_t)NK * RU_SURFACE_COUNTS, empty_value, values, tol, st, [&](const MaskGeom& s, u64* bits) {
        if (kind == RU_SURFACE_PROB)
            hipLaunchKernelGGL(sf_pack_kernel<0>, dim3(D, NK), dim3(256), 0, st, pred, target, C, K, s, bits, counts);
        else
            hipLaunchKernelGGL(sf_pack_kernel<1>, dim3(D, NK), dim3(256), 0, st, pred, target, C, K, s, bits, counts);
        RU_CHECK_LAUNCH("sf_pack_kernel");
        return RU_OK;
    });
}

}  // namespace

extern "C" int ru_surface_metrics(const void* pred, const void* target, int kind, int N, int C, int D, int H, int W, double empty_value,
                                  double* values, unsigned long long* counts, void* ws, size_t ws_bytes, ru_stream_t stream) {
    return sf_entry("ru_surface_metrics", pred, target, kind, N, C, D, H, W, empty_value, values, counts, SF_NO_TOL, ws, ws_bytes, stream);
}

extern "C" int ru_surface_distances(const void* pred, const void* target, int kind, int N, int C, int D, int H, int W, double empty_value,
                                    const unsigned* tol_bins, int T, double* values, unsigned long long* counts, double* extras, void* ws,
                                    size_t ws_bytes, ru_stream_t stream) {
    SfTol tol;
    RU_REQUIRE(sf_tol_make(tol_bins, T, extras, &tol), "ru_surface_distances: T = %d tolerances: needs 0 <= T <= %d, their bin limits and `extras`", T,
               RU_SURFACE_MAX_TOL);
    return sf_entry("ru_surface_distances", pred, target, kind, N, C, D, H, W, empty_value, values, counts, tol, ws, ws_bytes, stream);
}

extern "C" int ru_surface_extras_accumulate(const double* extras, double* acc, int N, int K, int nacc, int ncols, int column, ru_stream_t stream) {
    RU_REQUIRE(extras && acc && N > 0 && K > 0 && nacc > 0 && nacc <= K && nacc <= 64 && ncols >= 1 && column >= 0 && column < ncols,
               "ru_surface_extras_accumulate: bad argument");
    hipLaunchKernelGGL(sf_extras_mean_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, extras, acc, N, K, nacc, ncols, column);
    RU_CHECK_LAUNCH("sf_extras_mean_kernel");
    return RU_OK;
}

extern "C" int ru_surface_accumulate(const double* values, double* acc, int N, int K, int nacc, int column, ru_stream_t stream) {
    RU_REQUIRE(values && acc && N > 0 && K > 0 && nacc > 0 && nacc <= K && nacc <= 64 && column >= 0 && column < 4,
               "ru_surface_accumulate: bad argument");
    hipLaunchKernelGGL(column_mean_kernel<4>, dim3(1), dim3(64), 0, (hipStream_t)stream, values, acc, N, K, nacc, column);
    RU_CHECK_LAUNCH("column_mean_kernel");
    return RU_OK;
}
