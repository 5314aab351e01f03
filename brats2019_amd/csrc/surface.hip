// BraTS challenge metrics on the device: per (sample n, region k) the Dice, sensitivity, specificity and 95th-percentile surface
// Hausdorff distance (HD95) of two binary masks P (prediction) and G (target), distances in voxels between voxel centres at unit spacing.
//
//   surface  dA = { v in A : one of v's 6 face neighbours is not in A or lies outside the grid }
//   S        = { d(v, dG) : v in dP } + { d(v, dP) : v in dG }, a multiset of |dP| + |dG| exact integer squared distances
//   HD95     = numpy.percentile(sqrt(S), 95), numpy's default `linear` method reproduced operation by operation
//
// Per call, for every (n, k):
//   sf_zero_kernel        : clears the counts and the histograms (a kernel node, not a hipMemsetAsync: metrics.hip, hd_zero_kernel).
//   sf_pack_kernel<KIND>  : one wave per row: the masks as bit rows (one 64-bit word per 64 voxels along W, bits >= W zero) from wave
//                           ballots, and |P|, |G|, |P & G| (and the invalid label voxels) by popcount.  KIND 0: float32 [N][C][V],
//                           mask = x > 0.5 per channel.  KIND 1: uint8 label volumes [N][V], regions WT / TC / ET (3 counts as 4).
//   sf_surface_w_kernel   : one wave per row: lane c derives word c of both surfaces bit-parallel, m & ~(m & left & right & the four
//                           neighbour rows), zeros outside the grid; then the W pass of two exact squared distance transforms (to dG and
//                           to dP) from those words, as metrics.hip's hd_pass_w_kernel does from its ballots.
//   sf_pass_line_kernel   : metrics.hip's brute-force line minimum over 32-column tiles staged in LDS.  H pass in place; the D pass
//                           writes no distance map: at every voxel of the QUERY surface (dP for the transform to dG, dG for the one to
//                           dP) it adds one count to the (n, k) histogram of squared distances, (D-1)^2 + (H-1)^2 + (W-1)^2 + 1 bins.
//   sf_select_kernel      : one workgroup per (n, k): a prefix scan over the histogram finds the order statistics s_(i), s_(j), then
//                           the empty rules and numpy's lerp; writes {Dice, sensitivity, specificity, HD95} in float64.
// sf_accumulate_kernel (a call of its own) adds the batch mean of one of the four columns to a float64 device accumulator.
// Squared distances stay exact integers: the largest is 3 * 511^2 < 2^20; the "no site" sentinel 2^30 plus any (i - j)^2 stays below 2^31.
#include "ru_common.h"
#include "surface_packed.hpp"

namespace ru {
namespace {

constexpr int SF_MAX_EXTENT = 512;        // every axis; a row is at most 8 words
constexpr int SF_MAX_WORDS = SF_MAX_EXTENT / 64;
constexpr unsigned SF_INF = 1u << 30;     // "no site"
constexpr int SF_TW = 32;                 // W columns per tile of the line passes
constexpr int SF_LINE_THREADS = 256;      // 32 columns x 8 line positions
constexpr int SF_SELECT_THREADS = 1024;
constexpr double SF_Q = 0.95;             // numpy: 95 / 100 in float64

typedef unsigned long long u64;

// workspace slices of one (n, k): 4 bit planes (P, G, dP, dG) of `words` each, 2 distance maps of V, one histogram of `bins`
struct SfGeom {
    int D, H, W, WW;
    size_t V, words, bins;
};

__host__ __device__ inline SfGeom sf_geom(int D, int H, int W) {
    SfGeom g;
    g.D = D;
    g.H = H;
    g.W = W;
    g.WW = (W + 63) / 64;
    g.V = (size_t)D * H * W;
    g.words = (size_t)D * H * g.WW;
    g.bins = (size_t)(D - 1) * (D - 1) + (size_t)(H - 1) * (H - 1) + (size_t)(W - 1) * (W - 1) + 1;
    return g;
}

// region k of a BraTS label: WT = {1, 2, 3, 4}, TC = {1, 3, 4}, ET = {3, 4} (the model's channel order); values above 4 are in none
__device__ __forceinline__ bool sf_region(unsigned v, int k) {
    if (k == 0) return v >= 1u && v <= 4u;
    if (k == 1) return v == 1u || v == 3u || v == 4u;
    return v == 3u || v == 4u;
}

__device__ __forceinline__ unsigned sf_row_sq(u64 m, u64 below, int w, int c, int lane, int prev, int next) {
    // nearest site at or left of w: in this word (bits <= lane) or the last site of an earlier word; at or right of w likewise
    const int left = below ? c * 64 + 63 - __clzll((long long)below) : prev;
    const u64 above = m >> lane;
    const int right = above ? w + __ffsll((long long)above) - 1 : next;
    const int best = min(w - left, right - w);
    return best < SF_MAX_EXTENT ? (unsigned)(best * best) : SF_INF;
}

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

__global__ void sf_zero_kernel(u64* __restrict__ counts, size_t ncounts, unsigned* __restrict__ hist, size_t nhist) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < ncounts + nhist; i += stride) {
        if (i < ncounts) counts[i] = 0;
        else hist[i - ncounts] = 0;
    }
}

// grid (D, N*K), 256 threads: wave q takes the rows h = q, q + 4, ... of plane d.  counts[nk*6 + 0..2, 5] += |P|, |G|, |P & G|, invalid
template <int KIND>
__global__ __launch_bounds__(256) void sf_pack_kernel(const void* __restrict__ pv, const void* __restrict__ gv, int C, int K, SfGeom s,
                                                      u64* __restrict__ bits, u64* __restrict__ counts) {
    const int d = blockIdx.x, nk = blockIdx.y, n = nk / K, k = nk % K;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    u64* __restrict__ bp = bits + (size_t)nk * 4 * s.words;
    u64* __restrict__ bg = bp + s.words;
    const size_t base = KIND == 0 ? ((size_t)n * C + k) * s.V : (size_t)n * s.V;
    u64 cp = 0, cg = 0, ct = 0, ci = 0;
    for (int h = wave; h < s.H; h += 4) {
        const size_t row = (size_t)d * s.H + h;
        for (int c = 0; c < s.WW; ++c) {
            const int w = c * 64 + lane;
            bool pm = false, gm = false, bad = false;
            if (w < s.W) {
                const size_t v = base + row * s.W + w;
                if (KIND == 0) {
                    pm = static_cast<const float*>(pv)[v] > 0.5f;
                    gm = static_cast<const float*>(gv)[v] > 0.5f;
                } else {
                    const unsigned a = static_cast<const unsigned char*>(pv)[v], b = static_cast<const unsigned char*>(gv)[v];
                    pm = sf_region(a, k);
                    gm = sf_region(b, k);
                    bad = a > 4u || b > 4u;
                }
            }
            const u64 mp = __ballot(pm), mg = __ballot(gm);
            cp += __popcll(mp);
            cg += __popcll(mg);
            ct += __popcll(mp & mg);
            if (KIND == 1) ci += __popcll(__ballot(bad));
            if (lane == 0) {
                bp[row * s.WW + c] = mp;
                bg[row * s.WW + c] = mg;
            }
        }
    }
    if (lane == 0) {
        u64* q = counts + (size_t)nk * RU_SURFACE_COUNTS;
        if (cp) atomicAdd(q + 0, cp);
        if (cg) atomicAdd(q + 1, cg);
        if (ct) atomicAdd(q + 2, ct);
        if (ci) atomicAdd(q + 5, ci);
    }
}

// grid (D, N*K), 256 threads, one wave per row.  f = [N*K][2][V]: transform 0 = to dG, 1 = to dP.  counts[nk*6 + 3 / 4] += |dP| / |dG|.
__global__ __launch_bounds__(256) void sf_surface_w_kernel(SfGeom s, u64* __restrict__ bits, unsigned* __restrict__ f, u64* __restrict__ counts) {
    const int d = blockIdx.x, nk = blockIdx.y;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const u64* __restrict__ bp = bits + (size_t)nk * 4 * s.words;
    const u64* __restrict__ bg = bp + s.words;
    u64* __restrict__ sp = bits + ((size_t)nk * 4 + 2) * s.words;
    u64* __restrict__ sg = sp + s.words;
    unsigned* __restrict__ fg = f + (size_t)nk * 2 * s.V;
    unsigned* __restrict__ fp = fg + s.V;
    const u64 upto = lane == 63 ? ~0ull : (2ull << lane) - 1;
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
        u64 mp[SF_MAX_WORDS], mg[SF_MAX_WORDS];
#pragma unroll
        for (int c = 0; c < SF_MAX_WORDS; ++c) {
            mp[c] = c < s.WW ? __shfl(wp, c) : 0;
            mg[c] = c < s.WW ? __shfl(wg, c) : 0;
        }
        // first site after each word (wave-uniform), then a forward sweep with the last site before it
        int nextp[SF_MAX_WORDS], nextg[SF_MAX_WORDS];
        int np_ = 1 << 20, ng_ = 1 << 20;
#pragma unroll
        for (int c = SF_MAX_WORDS - 1; c >= 0; --c) {
            nextp[c] = np_;
            nextg[c] = ng_;
            if (mp[c]) np_ = c * 64 + __ffsll((long long)mp[c]) - 1;
            if (mg[c]) ng_ = c * 64 + __ffsll((long long)mg[c]) - 1;
        }
        int prevp = -(1 << 20), prevg = -(1 << 20);
#pragma unroll
        for (int c = 0; c < SF_MAX_WORDS; ++c) {
            if (c >= s.WW) break;
            const int w = c * 64 + lane;
            if (w < s.W) {
                fg[row * s.W + w] = sf_row_sq(mg[c], mg[c] & upto, w, c, lane, prevg, nextg[c]);
                fp[row * s.W + w] = sf_row_sq(mp[c], mp[c] & upto, w, c, lane, prevp, nextp[c]);
            }
            if (mp[c]) prevp = c * 64 + 63 - __clzll((long long)mp[c]);
            if (mg[c]) prevg = c * 64 + 63 - __clzll((long long)mg[c]);
        }
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

// grid (cdiv(W, 32), lines, N*K*2), 256 threads, dynamic LDS L x 32 x 4 B.  FINAL = false: the H pass (lines = D planes, L = H, in place).
// FINAL = true: the D pass (lines = H rows, L = D): one histogram count per voxel of the query surface.
template <bool FINAL>
__global__ __launch_bounds__(SF_LINE_THREADS) void sf_pass_line_kernel(unsigned* __restrict__ f, SfGeom s, const u64* __restrict__ bits,
                                                                       unsigned* __restrict__ hist) {
    extern __shared__ unsigned lds[];
    const int x = threadIdx.x % SF_TW, r = threadIdx.x / SF_TW;
    constexpr int R = SF_LINE_THREADS / SF_TW;
    const int w = blockIdx.x * SF_TW + x, a = blockIdx.y, t = blockIdx.z & 1, nk = blockIdx.z >> 1;
    const int L = FINAL ? s.D : s.H;
    const size_t stride = FINAL ? (size_t)s.H * s.W : (size_t)s.W;
    const size_t off = FINAL ? (size_t)a * s.W + w : (size_t)a * s.H * s.W + w;       // voxel index of line element 0
    unsigned* __restrict__ fl = f + ((size_t)nk * 2 + t) * s.V;
    const bool col = w < s.W;
    for (int i = r; i < L; i += R) lds[i * SF_TW + x] = col ? fl[off + i * stride] : SF_INF;
    __syncthreads();
    // the transform to dG (t = 0) is sampled on dP (plane 2), the one to dP on dG (plane 3)
    const u64* __restrict__ q = bits + ((size_t)nk * 4 + 2 + t) * s.words;
    unsigned* __restrict__ hn = hist + (size_t)nk * s.bins;
    for (int i0 = r; i0 < L; i0 += 4 * R) {
        bool on[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int i = i0 + u * R;
            on[u] = col && i < L;
            if (FINAL && on[u]) on[u] = (q[((size_t)i * s.H + a) * s.WW + (w >> 6)] >> (w & 63)) & 1ull;
        }
        if (FINAL && !__any(on[0] || on[1] || on[2] || on[3])) continue;             // no query voxel here
        unsigned acc[4] = {SF_INF, SF_INF, SF_INF, SF_INF};
        for (int j = 0; j < L; ++j) {
            const unsigned fj = lds[j * SF_TW + x];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int dd = i0 + u * R - j;
                acc[u] = min(acc[u], fj + (unsigned)__mul24(dd, dd));
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (!on[u]) continue;
            if (FINAL) {
                if (acc[u] < s.bins) atomicAdd(hn + acc[u], 1u);                     // >= bins only without sites: the empty rules decide
            } else {
                fl[off + (size_t)(i0 + u * R) * stride] = acc[u];                   // the block owns its lines: in place after the barrier
            }
        }
    }
}

// numpy's _lerp: a + (b - a) * t, or b - (b - a) * (1 - t) where t >= 0.5; two roundings each, no fused multiply-add
__device__ __forceinline__ double sf_lerp(double a, double b, double t) {
#pragma clang fp contract(off)
    const double diff = b - a;
    return t >= 0.5 ? b - diff * (1.0 - t) : a + diff * t;
}

// grid (N*K), SF_SELECT_THREADS threads.  out[nk*4 + RU_SURFACE_DICE / _SENS / _SPEC / _HD95].
__global__ __launch_bounds__(SF_SELECT_THREADS) void sf_select_kernel(const unsigned* __restrict__ hist, SfGeom s, const u64* __restrict__ counts,
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
        const unsigned* __restrict__ hn = hist + (size_t)nk * s.bins;
        const size_t chunk = (s.bins + SF_SELECT_THREADS - 1) / SF_SELECT_THREADS;
        const size_t lo = min(s.bins, (size_t)tid * chunk), hi = min(s.bins, lo + chunk);
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
    const u64 V = s.V;
    double* o = out + (size_t)nk * 4;
    o[RU_SURFACE_DICE] = P + G == 0 ? 1.0 : (double)(2 * TP) / (double)(P + G);
    o[RU_SURFACE_SENS] = G == 0 ? 1.0 : (double)TP / (double)G;
    o[RU_SURFACE_SPEC] = V == G ? 1.0 : (double)((V - G) - (P - TP)) / (double)(V - G);
    o[RU_SURFACE_HD95] = hd;
}

// acc[i] += mean over the N samples of values[n][i][column], i < nacc; samples summed in order
__global__ void sf_accumulate_kernel(const double* __restrict__ values, double* __restrict__ acc, int N, int K, int nacc, int column) {
    const int i = threadIdx.x;
    if (i >= nacc) return;
    double sum = 0.0;
    for (int n = 0; n < N; ++n) sum += values[((size_t)n * K + i) * 4 + column];
    acc[i] += sum / (double)N;
}

bool sf_shape_ok(int kind, int N, int C, int D, int H, int W) {
    return (kind == RU_SURFACE_PROB || (kind == RU_SURFACE_LABEL && C == 1)) && N > 0 && C > 0 && D >= 1 && H >= 1 && W >= 1 &&
           D <= SF_MAX_EXTENT && H <= SF_MAX_EXTENT && W <= SF_MAX_EXTENT;
}

int sf_regions(int kind, int C) { return kind == RU_SURFACE_LABEL ? RU_SURFACE_REGIONS : C; }

size_t sf_workspace_bytes(int kind, int N, int C, int D, int H, int W) {
    if (!sf_shape_ok(kind, N, C, D, H, W)) return 0;
    const SfGeom s = sf_geom(D, H, W);
    const size_t nk = (size_t)N * sf_regions(kind, C);
    return nk * (4 * s.words * sizeof(u64) + 2 * s.V * sizeof(unsigned) + s.bins * sizeof(unsigned));
}

// the passes after the masks are packed and the counts and histograms cleared
int sf_passes(const SfGeom& s, int NK, u64* bits, unsigned* f, unsigned* hist, u64* counts, double empty_value, double* values, hipStream_t st) {
    hipLaunchKernelGGL(sf_surface_w_kernel, dim3(s.D, NK), dim3(256), 0, st, s, bits, f, counts);
    RU_CHECK_LAUNCH("sf_surface_w_kernel");
    hipLaunchKernelGGL(sf_pass_line_kernel<false>, dim3(cdiv(s.W, SF_TW), s.D, NK * 2), dim3(SF_LINE_THREADS), (size_t)s.H * SF_TW * sizeof(unsigned), st,
                       f, s, bits, hist);
    RU_CHECK_LAUNCH("sf_pass_line_kernel<H>");
    hipLaunchKernelGGL(sf_pass_line_kernel<true>, dim3(cdiv(s.W, SF_TW), s.H, NK * 2), dim3(SF_LINE_THREADS), (size_t)s.D * SF_TW * sizeof(unsigned), st,
                       f, s, bits, hist);
    RU_CHECK_LAUNCH("sf_pass_line_kernel<D>");
    hipLaunchKernelGGL(sf_select_kernel, dim3(NK), dim3(SF_SELECT_THREADS), 0, st, hist, s, counts, empty_value, values);
    RU_CHECK_LAUNCH("sf_select_kernel");
    return RU_OK;
}

}  // namespace

size_t sf_packed_workspace_bytes(int items, int D, int H, int W) { return sf_workspace_bytes(RU_SURFACE_PROB, 1, items, D, H, W); }

unsigned long long* sf_packed_bits(void* ws) { return (u64*)ws; }

int sf_packed_run(int items, int D, int H, int W, void* ws, unsigned long long* counts, double empty_value, double* values, hipStream_t st) {
    RU_REQUIRE(ws && counts && values && items > 0 && (long long)items * 2 <= 65535 && sf_shape_ok(RU_SURFACE_PROB, 1, items, D, H, W),
               "sf_packed_run: bad argument");
    const SfGeom s = sf_geom(D, H, W);
    u64* bits = (u64*)ws;
    unsigned* f = (unsigned*)(bits + (size_t)items * 4 * s.words);
    unsigned* hist = f + (size_t)items * 2 * s.V;
    const size_t nhist = (size_t)items * s.bins;
    hipLaunchKernelGGL(sf_zero_kernel, dim3((unsigned)std::min<size_t>(1024, (nhist + 255) / 256)), dim3(256), 0, st, counts, (size_t)0, hist, nhist);
    RU_CHECK_LAUNCH("sf_zero_kernel");
    return sf_passes(s, items, bits, f, hist, counts, empty_value, values, st);
}

}  // namespace ru

using namespace ru;

extern "C" size_t ru_surface_workspace_bytes(int kind, int N, int C, int D, int H, int W) { return sf_workspace_bytes(kind, N, C, D, H, W); }

extern "C" int ru_surface_metrics(const void* pred, const void* target, int kind, int N, int C, int D, int H, int W, double empty_value,
                                  double* values, unsigned long long* counts, void* ws, size_t ws_bytes, ru_stream_t stream) {
    RU_REQUIRE(pred && target && values && counts && N > 0 && C > 0, "ru_surface_metrics: bad argument");
    RU_REQUIRE(kind == RU_SURFACE_PROB || (kind == RU_SURFACE_LABEL && C == 1), "ru_surface_metrics: bad kind %d (C = %d)", kind, C);
    RU_REQUIRE(D >= 1 && H >= 1 && W >= 1 && D <= SF_MAX_EXTENT && H <= SF_MAX_EXTENT && W <= SF_MAX_EXTENT,
               "ru_surface_metrics: extents %d x %d x %d: every axis must be in [1, %d]", D, H, W, SF_MAX_EXTENT);
    const int K = sf_regions(kind, C);
    RU_REQUIRE((long long)N * K * 2 <= 65535, "ru_surface_metrics: N * regions = %lld: the grid needs 2 * N * regions <= 65535", (long long)N * K);
    RU_REQUIRE(ws && ws_bytes >= sf_workspace_bytes(kind, N, C, D, H, W), "ru_surface_metrics: workspace too small");
    hipStream_t st = (hipStream_t)stream;
    const SfGeom s = sf_geom(D, H, W);
    const int NK = N * K;
    u64* bits = (u64*)ws;
    unsigned* f = (unsigned*)(bits + (size_t)NK * 4 * s.words);
    unsigned* hist = f + (size_t)NK * 2 * s.V;
    const size_t ncounts = (size_t)NK * RU_SURFACE_COUNTS, nhist = (size_t)NK * s.bins;
    hipLaunchKernelGGL(sf_zero_kernel, dim3((unsigned)std::min<size_t>(1024, (ncounts + nhist + 255) / 256)), dim3(256), 0, st, counts, ncounts,
                       hist, nhist);
    RU_CHECK_LAUNCH("sf_zero_kernel");
    if (kind == RU_SURFACE_PROB)
        hipLaunchKernelGGL(sf_pack_kernel<0>, dim3(D, NK), dim3(256), 0, st, pred, target, C, K, s, bits, counts);
    else
        hipLaunchKernelGGL(sf_pack_kernel<1>, dim3(D, NK), dim3(256), 0, st, pred, target, C, K, s, bits, counts);
    RU_CHECK_LAUNCH("sf_pack_kernel");
    return sf_passes(s, NK, bits, f, hist, counts, empty_value, values, st);
}

extern "C" int ru_surface_accumulate(const double* values, double* acc, int N, int K, int nacc, int column, ru_stream_t stream) {
    RU_REQUIRE(values && acc && N > 0 && K > 0 && nacc > 0 && nacc <= K && nacc <= 64 && column >= 0 && column < 4,
               "ru_surface_accumulate: bad argument");
    hipLaunchKernelGGL(sf_accumulate_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, values, acc, N, K, nacc, column);
    RU_CHECK_LAUNCH("sf_accumulate_kernel");
    return RU_OK;
}
