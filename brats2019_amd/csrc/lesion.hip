// Lesion-wise Dice and HD95 on the device (the BraTS ranking since 2023; include/resunet_hip.h states the definition).  Per (sample n,
// region k), P and G are bit-packed along x (mask_bits.hpp): one 64-bit word per 64 voxels, bits >= W of a row zero.
//
//   ls_clear_kernel      : clears the outputs, the per-lesion counters and the pair table.
//   ls_pack_kernel<KIND> : the masks P and G, and the invalid label voxels (mask_bits.hpp, mask_pack_rows).
//   ls_dilate_kernel     : (mask_dilate.hpp, shared with lesion_loss.hip) one thread per word, one launch per iteration, ping-pong
//                          between two planes: the rows (dz, dy) = (0, 0) and the four face rows contribute themselves and their x +- 1
//                          shifts (carries cross word boundaries), the four diagonal rows themselves only -- the 18-neighbour
//                          structure.  Z = Dil(G).
//   cc_*_kernel<LsPlanes>: the union-find labelling of cc_unionfind.hpp (init, compress, merge, compress) from bit planes, for Z and P of
//                          every (n, k) in one launch.  Roots are smallest indices.
//   ls_count_kernel      : the roots of Z are appended to a list; |Q_j| at every root of P (cc_count_members).
//   ls_rank_kernel       : sorts the list: lesion i = the component of Z with the i-th smallest root, scipy.ndimage.label's order.
//   ls_pair_kernel       : one wave per row: vol_i and tp_i by popcount, and every run start of P & Z inserts its pair (root of P,
//                          lesion) into an open-addressing table.  Distinct pairs <= components of P & Z <= ceil(D/2) ceil(H/2)
//                          ceil(W/2); the table has at least twice as many slots, so it never fills.  The table's CONTENT is a set: it
//                          does not depend on the order of insertion.
//   ls_table_kernel      : every pair adds |Q_j| to |M_i| and marks Q_j as matched.
//   ls_fp_kernel         : counts the roots of P that no pair marked.
//   ls_item_kernel       : one chunk of lesions: (M_i, L_i) as bit planes of the whole grid, handed to surface.hip's packed entry
//                          (surface_packed.hpp), which writes Dice_i and HD95_i.
//   ls_summary_kernel    : one thread per (n, k): the float64 sums in ascending lesion order, the counts, the optional table.
//   ls_summary_ex_kernel : (ru_lesion_distances only) the same loop over the per-lesion {NSD_t, ASSD, HD} that the packed entry's extras
//                          sibling wrote: LesionNSD_t and LesionASSD, the optional per-lesion table of extras.
// Integer atomics only.  The one host synchronisation reads the lesion counts back: the chunk loop needs them.
#include "ru_common.h"
#include "pw_helpers.hpp"
#include "cc_unionfind.hpp"
#include "surface_packed.hpp"
#include "mask_bits.hpp"
#include "mask_dilate.hpp"

#include <limits.h>

namespace ru {
namespace {

constexpr int LS_MAX_LESIONS = 1 << 16;
constexpr u64 LS_FREE = ~0ull;                      // an unused table slot
constexpr unsigned LS_MATCHED = 0x80000000u;        // high bit of |Q_j|: some lesion matched the component

// slots of the pair table of one (n, k): a power of two >= 2 * ceil(D/2) * ceil(H/2) * ceil(W/2)
unsigned ls_slots(int D, int H, int W) {
    const size_t need = 2 * (size_t)((D + 1) / 2) * ((H + 1) / 2) * ((W + 1) / 2);
    unsigned s = 64;
    while (s < need) s <<= 1;
    return s;
}

// workspace slices; planes per (n, k): 0 = P, 1 = G, 2 and 3 = the dilation's ping-pong
struct LsWs {
    int *nles, *nfp, *pz, *pp, *cnt, *roots, *sorted;
    unsigned *vol, *msz, *tp;
    u64 *bits, *tab, *icounts;
    double *vals, *ex;
    void* sf;
    size_t bytes;
};

LsWs ls_layout(char* base, size_t NK, const MaskGeom& g, unsigned slots, size_t max_lesions, size_t ex_cols = 0) {
    LsWs w;
    size_t off = 0;
    auto take = [&](size_t bytes) { char* p = base + off; off += align_up(bytes, 256); return p; };
    w.bits = (u64*)take(NK * 4 * g.words * sizeof(u64));
    w.tab = (u64*)take(NK * slots * sizeof(u64));
    w.vals = (double*)take(NK * max_lesions * 4 * sizeof(double));
    w.icounts = (u64*)take((size_t)RU_LESION_CHUNK * RU_SURFACE_COUNTS * sizeof(u64));
    w.pz = (int*)take(NK * g.V * sizeof(int));
    w.pp = (int*)take(NK * g.V * sizeof(int));
    w.cnt = (int*)take(NK * g.V * sizeof(int));
    w.roots = (int*)take(NK * max_lesions * sizeof(int));
    w.sorted = (int*)take(NK * max_lesions * sizeof(int));
    w.vol = (unsigned*)take(NK * max_lesions * sizeof(unsigned));
    w.msz = (unsigned*)take(NK * max_lesions * sizeof(unsigned));
    w.tp = (unsigned*)take(NK * max_lesions * sizeof(unsigned));
    w.nles = (int*)take(NK * sizeof(int));
    w.nfp = (int*)take(NK * sizeof(int));
    w.sf = (void*)take(sf_packed_workspace_bytes(RU_LESION_CHUNK, g.D, g.H, g.W));
    w.ex = (double*)take(NK * max_lesions * ex_cols * sizeof(double));        // ru_lesion_distances only: the per-lesion extras, last
    w.bytes = off;
    return w;
}

bool ls_shape_ok(int kind, int N, int C, int D, int H, int W, int max_lesions) {
    return mask_shape_ok(kind, N, C, D, H, W) && max_lesions >= 1 && max_lesions <= LS_MAX_LESIONS;
}

__global__ void ls_clear_kernel(LsWs w, size_t NK, size_t max_lesions, unsigned slots, double* __restrict__ summary, u64* __restrict__ counts) {
    const size_t stride = (size_t)gridDim.x * blockDim.x, nl = NK * max_lesions, nt = NK * slots;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < nt || i < nl; i += stride) {
        if (i < nt) w.tab[i] = LS_FREE;
        if (i < nl) w.vol[i] = w.msz[i] = w.tp[i] = 0u;
        if (i < NK) w.nles[i] = w.nfp[i] = 0;
        if (i < NK * 2) summary[i] = 0.0;
        if (i < NK * RU_LESION_COUNTS) counts[i] = 0;
    }
}

// grid (D, N*K), 256 threads.  counts[nk*6 + 5] += invalid voxels
template <int KIND>
__global__ __launch_bounds__(256) void ls_pack_kernel(const void* __restrict__ pv, const void* __restrict__ gv, int C, int K, MaskGeom s,
                                                      u64* __restrict__ bits, u64* __restrict__ counts) {
    u64 c[4];
    mask_pack_rows<KIND, false>(pv, gv, C, K, s, bits, c);
    if ((threadIdx.x & 63) == 0 && c[3]) atomicAdd(counts + (size_t)blockIdx.y * RU_LESION_COUNTS + RU_LESION_C_INVALID, c[3]);
}

// the labelling's foreground: block (., nk, z) labels plane `zplane` (Z) of (n, k) = nk for z = 0, plane 0 (P) for z = 1
struct LsPlanes {
    const u64* plane;
    size_t words;
    int WW, zplane;
    __device__ void select(int nk, int z) { plane += ((size_t)nk * 4 + (z ? 0 : zplane)) * words; }
    __device__ bool operator()(size_t row, int x) const { return mask_bit(plane, WW, row, x); }
};

// grid (blocks, N*K): the roots of Z join the list; cnt[root of P] += members
__global__ __launch_bounds__(256) void ls_count_kernel(size_t V, const int* __restrict__ pz, const int* __restrict__ pp, int* __restrict__ cnt,
                                                       int* __restrict__ roots, int* __restrict__ nles, int max_lesions) {
    const int nk = blockIdx.y;
    const int* __restrict__ zparent = pz + (size_t)nk * V;
    for (size_t v = (size_t)blockIdx.x * 256 + threadIdx.x; v < V; v += (size_t)gridDim.x * 256) {
        if (zparent[v] != (int)v) continue;
        const int at = atomicAdd(nles + nk, 1);
        if (at < max_lesions) roots[(size_t)nk * max_lesions + at] = (int)v;
    }
    cc_count_members(pp + (size_t)nk * V, cnt + (size_t)nk * V, V);
}

// grid (N*K), 256 threads: sorted[rank] = root, the rank by counting the smaller roots (the roots are distinct)
__global__ __launch_bounds__(256) void ls_rank_kernel(const int* __restrict__ roots, int* __restrict__ sorted, const int* __restrict__ nles, int max_lesions) {
    const int nk = blockIdx.x, n = min(nles[nk], max_lesions);
    const int* __restrict__ r = roots + (size_t)nk * max_lesions;
    for (int i = threadIdx.x; i < n; i += 256) {
        const int mine = r[i];
        int rank = 0;
        for (int k = 0; k < n; ++k) rank += r[k] < mine ? 1 : 0;
        sorted[(size_t)nk * max_lesions + rank] = mine;
    }
}

// the lesion whose component of Z has this root; -1 if the list was cut at max_lesions (the call then returns the error)
__device__ __forceinline__ int ls_lesion_of(const int* __restrict__ sorted, int n, int root) {
    int lo = 0, hi = n - 1;
    while (lo <= hi) {
        const int mid = (lo + hi) >> 1, r = sorted[mid];
        if (r == root) return mid;
        if (r < root) lo = mid + 1;
        else hi = mid - 1;
    }
    return -1;
}

__device__ __forceinline__ unsigned ls_hash(u64 key, unsigned slots) {
    key *= 0x9E3779B97F4A7C15ull;
    return (unsigned)(key >> 32) & (slots - 1);
}
__device__ __forceinline__ void ls_insert(u64* __restrict__ tab, unsigned slots, u64 key) {
    unsigned at = ls_hash(key, slots);
    for (;;) {                                                  // the table has free slots left whatever the masks are: terminates
        const u64 old = atomicCAS(tab + at, LS_FREE, key);
        if (old == LS_FREE || old == key) return;
        at = (at + 1) & (slots - 1);
    }
}
__device__ __forceinline__ bool ls_contains(const u64* __restrict__ tab, unsigned slots, u64 key) {
    unsigned at = ls_hash(key, slots);
    for (;;) {
        const u64 cur = tab[at];
        if (cur == key) return true;
        if (cur == LS_FREE) return false;
        at = (at + 1) & (slots - 1);
    }
}
__device__ __forceinline__ u64 ls_key(int proot, int lesion) { return ((u64)(unsigned)proot << 32) | (u64)(unsigned)lesion; }

// grid (D, N*K), 256 threads, one wave per row.  vol[i] += |G & Z_i|, tp[i] += |P & G & Z_i|; pairs from the run starts of P & Z
__global__ __launch_bounds__(256) void ls_pair_kernel(MaskGeom s, unsigned slots, const u64* __restrict__ bits, int zplane, const int* __restrict__ pz, const int* __restrict__ pp,
                                                      const int* __restrict__ sorted, const int* __restrict__ nles, int max_lesions,
                                                      unsigned* __restrict__ vol, unsigned* __restrict__ tp, u64* __restrict__ tab) {
    const int d = blockIdx.x, nk = blockIdx.y;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const u64* __restrict__ bp = bits + (size_t)nk * 4 * s.words;
    const u64* __restrict__ bg = bp + s.words;
    const u64* __restrict__ bz = bits + ((size_t)nk * 4 + zplane) * s.words;
    const int* __restrict__ zparent = pz + (size_t)nk * s.V;
    const int* __restrict__ parent = pp + (size_t)nk * s.V;
    const int* __restrict__ srt = sorted + (size_t)nk * max_lesions;
    const int n = min(nles[nk], max_lesions);
    unsigned* __restrict__ voln = vol + (size_t)nk * max_lesions;
    unsigned* __restrict__ tpn = tp + (size_t)nk * max_lesions;
    u64* __restrict__ tabn = tab + (size_t)nk * slots;
    for (int h = wave; h < s.H; h += 4) {
        const size_t row = (size_t)d * s.H + h;
        u64 carry = 0;                                          // bit 63 of P & Z of the previous word
        for (int c = 0; c < s.WW; ++c) {
            const u64 gw = bg[row * s.WW + c], pw = bp[row * s.WW + c], pzw = pw & bz[row * s.WW + c];
            const u64 start = pzw & ~((pzw << 1) | carry);
            carry = pzw >> 63;
            if (!(gw | pzw)) continue;                          // (wave-uniform)
            const int v = (int)(row * s.W + c * 64 + lane);
            int les = -1;
            if (((gw | pzw) >> lane) & 1ull) les = ls_lesion_of(srt, n, cc_find(zparent, v));
            u64 todo = __ballot(les >= 0);
            while (todo) {
                const int leader = __builtin_ctzll(todo);
                const int l = __shfl(les, leader);
                const u64 same = __ballot(les == l) & todo;
                if (lane == leader) {
                    const unsigned nv = (unsigned)__popcll(same & gw), nt = (unsigned)__popcll(same & gw & pw);
                    if (nv) atomicAdd(voln + l, nv);
                    if (nt) atomicAdd(tpn + l, nt);
                }
                todo &= ~same;
            }
            if (les >= 0 && ((start >> lane) & 1ull)) ls_insert(tabn, slots, ls_key(cc_find(parent, v), les));
        }
    }
}

// grid (blocks, N*K): every pair (j, i): |M_i| += |Q_j|, Q_j is matched
__global__ __launch_bounds__(256) void ls_table_kernel(size_t V, unsigned slots, const u64* __restrict__ tab, int* __restrict__ cnt, unsigned* __restrict__ msz, int max_lesions) {
    const int nk = blockIdx.y;
    unsigned* __restrict__ count = (unsigned*)(cnt + (size_t)nk * V);
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < slots; i += (size_t)gridDim.x * 256) {
        const u64 key = tab[(size_t)nk * slots + i];
        if (key == LS_FREE) continue;
        const unsigned j = (unsigned)(key >> 32), les = (unsigned)key;
        const unsigned size = __hip_atomic_load(count + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & ~LS_MATCHED;
        atomicAdd(msz + (size_t)nk * max_lesions + les, size);
        atomicOr(count + j, LS_MATCHED);
    }
}

// grid (blocks, N*K): nfp += roots of P without the mark
__global__ __launch_bounds__(256) void ls_fp_kernel(MaskGeom s, const int* __restrict__ pp, const int* __restrict__ cnt, int* __restrict__ nfp) {
    const int nk = blockIdx.y;
    const int* __restrict__ parent = pp + (size_t)nk * s.V;
    const unsigned* __restrict__ count = (const unsigned*)(cnt + (size_t)nk * s.V);
    int local = 0;
    for (size_t v = (size_t)blockIdx.x * 256 + threadIdx.x; v < s.V; v += (size_t)gridDim.x * 256)
        local += (parent[v] == (int)v && !(count[v] & LS_MATCHED)) ? 1 : 0;
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) local += __shfl_xor(local, m);
    if ((threadIdx.x & 63) == 0 && local) atomicAdd(nfp + nk, local);
}

// grid (D, items), 256 threads, one wave per row: item t is lesion i0 + t of (n, k) = nk.  Plane 0 of the item = M_i, plane 1 = L_i.
__global__ __launch_bounds__(256) void ls_item_kernel(MaskGeom s, unsigned slots, const u64* __restrict__ bits, const int* __restrict__ pz, const int* __restrict__ pp,
                                                      const int* __restrict__ sorted, const u64* __restrict__ tab, const unsigned* __restrict__ vol,
                                                      const unsigned* __restrict__ msz, const unsigned* __restrict__ tp, int max_lesions, int nk, int i0,
                                                      u64* __restrict__ ibits, u64* __restrict__ icounts) {
    const int d = blockIdx.x, t = blockIdx.y, i = i0 + t;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const u64* __restrict__ bp = bits + (size_t)nk * 4 * s.words;
    const u64* __restrict__ bg = bp + s.words;
    const int* __restrict__ zparent = pz + (size_t)nk * s.V;
    const int* __restrict__ parent = pp + (size_t)nk * s.V;
    const u64* __restrict__ tabn = tab + (size_t)nk * slots;
    const int root = sorted[(size_t)nk * max_lesions + i];
    u64* __restrict__ im = ibits + (size_t)t * 4 * s.words;
    u64* __restrict__ il = im + s.words;
    for (int h = wave; h < s.H; h += 4) {
        const size_t row = (size_t)d * s.H + h;
        for (int c = 0; c < s.WW; ++c) {
            const u64 gw = bg[row * s.WW + c], pw = bp[row * s.WW + c];
            const int v = (int)(row * s.W + c * 64 + lane);
            bool inl = false, inm = false;
            if ((gw >> lane) & 1ull) inl = cc_find(zparent, v) == root;
            if ((pw >> lane) & 1ull) inm = ls_contains(tabn, slots, ls_key(cc_find(parent, v), i));
            const u64 ml = __ballot(inl), mm = __ballot(inm);
            if (lane == 0) {
                im[row * s.WW + c] = mm;
                il[row * s.WW + c] = ml;
            }
        }
    }
    if (d == 0 && threadIdx.x == 0) {
        u64* q = icounts + (size_t)t * RU_SURFACE_COUNTS;
        const size_t at = (size_t)nk * max_lesions + i;
        q[0] = msz[at];
        q[1] = vol[at];
        q[2] = tp[at];
        q[3] = q[4] = q[5] = 0;
    }
}

// grid cdiv(N*K, 64): vals [N*K][max_lesions][4] = surface.hip's {Dice, ., ., HD95} per lesion
__global__ void ls_summary_kernel(int NK, int max_lesions, const int* __restrict__ nles, const int* __restrict__ nfp, const unsigned* __restrict__ vol,
                                  const unsigned* __restrict__ msz, const unsigned* __restrict__ tp, const double* __restrict__ vals,
                                  long long min_volume, double empty_value, double* __restrict__ summary, u64* __restrict__ counts,
                                  double* __restrict__ table) {
#pragma clang fp contract(off)
    const int nk = blockIdx.x * blockDim.x + threadIdx.x;
    if (nk >= NK) return;
    const int n = nles[nk], fp = nfp[nk];
    u64 kept = 0, hit = 0;
    double sd = 0.0, sh = 0.0;
    for (int i = 0; i < n; ++i) {
        const size_t at = (size_t)nk * max_lesions + i;
        const double dice = vals[at * 4 + RU_SURFACE_DICE], hd = vals[at * 4 + RU_SURFACE_HD95];
        if (table) {
            double* r = table + at * RU_LESION_COLUMNS;
            r[0] = (double)vol[at];
            r[1] = (double)msz[at];
            r[2] = (double)tp[at];
            r[3] = dice;
            r[4] = hd;
        }
        if ((long long)vol[at] <= min_volume) continue;
        ++kept;
        hit += msz[at] ? 1 : 0;
        sd += dice;
        sh += hd;
    }
    const u64 den = kept + (u64)fp;
    summary[nk * 2 + 0] = den ? sd / (double)den : 1.0;
    summary[nk * 2 + 1] = den ? (sh + (double)fp * empty_value) / (double)den : 0.0;
    u64* q = counts + (size_t)nk * RU_LESION_COUNTS;
    q[0] = (u64)n;
    q[1] = kept;
    q[2] = hit;
    q[3] = kept - hit;
    q[4] = (u64)fp;
}

// grid cdiv(N*K, 64): ex [N*K][max_lesions][T + 2] = surface.hip's {NSD_0..NSD_T-1, ASSD, HD} per lesion; ls_summary_kernel's loop and
// its kept rule, the sums in the same ascending order
__global__ void ls_summary_ex_kernel(int NK, int max_lesions, int T, const int* __restrict__ nles, const int* __restrict__ nfp, const unsigned* __restrict__ vol,
                                     const double* __restrict__ ex, long long min_volume, double empty_value, double* __restrict__ summary_ex,
                                     double* __restrict__ table_ex) {
#pragma clang fp contract(off)
    const int nk = blockIdx.x * blockDim.x + threadIdx.x;
    if (nk >= NK) return;
    const int n = nles[nk], fp = nfp[nk], cols = T + 2;
    u64 kept = 0;
    double sum[RU_SURFACE_MAX_TOL + 1];
    for (int t = 0; t <= T; ++t) sum[t] = 0.0;
    for (int i = 0; i < n; ++i) {
        const size_t at = (size_t)nk * max_lesions + i;
        const double* e = ex + at * cols;
        if (table_ex)
            for (int t = 0; t < cols; ++t) table_ex[at * cols + t] = e[t];
        if ((long long)vol[at] <= min_volume) continue;
        ++kept;
        for (int t = 0; t <= T; ++t) sum[t] += e[t];
    }
    const u64 den = kept + (u64)fp;
    double* o = summary_ex + (size_t)nk * (T + 1);
    for (int t = 0; t < T; ++t) o[t] = den ? sum[t] / (double)den : 1.0;
    o[T] = den ? (sum[T] + (double)fp * empty_value) / (double)den : 0.0;
}

// the extras of one ru_lesion_distances call; T < 0: none (ru_lesion_metrics)
struct LsEx {
    const unsigned* tol_bins;
    int T;
    double *summary_ex, *table_ex;
};

}  // namespace
}  // namespace ru

using namespace ru;

extern "C" size_t ru_lesion_workspace_bytes(int kind, int N, int C, int D, int H, int W, int max_lesions) {
    if (!ls_shape_ok(kind, N, C, D, H, W, max_lesions) || (size_t)D * H * W >= (size_t)INT_MAX) return 0;
    return ls_layout(nullptr, (size_t)N * mask_regions(kind, C), mask_geom(D, H, W), ls_slots(D, H, W), (size_t)max_lesions).bytes;
}

namespace {

int ls_entry(const char* who, const void* pred, const void* target, int kind, int N, int C, int D, int H, int W, int dilation, long long min_volume,
             double empty_value, double* summary, unsigned long long* counts, double* table, const LsEx& ex, int max_lesions, void* ws,
             size_t ws_bytes, ru_stream_t stream) {
    RU_REQUIRE(pred && target && summary && counts && N > 0 && C > 0, "%s: bad argument", who);
    RU_REQUIRE(kind == RU_SURFACE_PROB || (kind == RU_SURFACE_LABEL && C == 1), "%s: bad kind %d (C = %d)", who, kind, C);
    RU_REQUIRE(D >= 1 && H >= 1 && W >= 1 && D <= MAX_EXTENT && H <= MAX_EXTENT && W <= MAX_EXTENT,
               "%s: extents %d x %d x %d: every axis must be in [1, %d]", who, D, H, W, MAX_EXTENT);
    RU_REQUIRE((size_t)D * H * W < (size_t)INT_MAX, "%s: volume too large for 32-bit voxel indices", who);
    RU_REQUIRE(dilation >= 0 && dilation <= MAX_EXTENT && min_volume >= 0, "%s: dilation %d, min_volume %lld: both must be >= 0", who, dilation, min_volume);
    RU_REQUIRE(max_lesions >= 1 && max_lesions <= LS_MAX_LESIONS, "%s: max_lesions %d: must be in [1, %d]", who, max_lesions, LS_MAX_LESIONS);
    const int K = mask_regions(kind, C);
    RU_REQUIRE((long long)N * K <= 65535, "%s: N * regions = %lld: the grid needs N * regions <= 65535", who, (long long)N * K);
    const size_t ex_cols = ex.T >= 0 ? (size_t)ex.T + 2 : 0;
    const size_t need = ls_layout(nullptr, (size_t)N * K, mask_geom(D, H, W), ls_slots(D, H, W), (size_t)max_lesions, ex_cols).bytes;
    RU_REQUIRE(ws && ws_bytes >= need, "%s: workspace too small", who);
    hipStream_t st = (hipStream_t)stream;
    const MaskGeom s = mask_geom(D, H, W);
    const unsigned slots = ls_slots(D, H, W);
    const int NK = N * K;
    const LsWs w = ls_layout((char*)ws, (size_t)NK, s, slots, (size_t)max_lesions, ex_cols);
    const size_t nclear = std::max((size_t)NK * slots, (size_t)NK * max_lesions);
    hipLaunchKernelGGL(ls_clear_kernel, dim3(grid1d(nclear, 256, 4096)), dim3(256), 0, st, w, (size_t)NK, (size_t)max_lesions, slots, summary, counts);
    RU_CHECK_LAUNCH("ls_clear_kernel");
    if (kind == RU_SURFACE_PROB)
        hipLaunchKernelGGL(ls_pack_kernel<0>, dim3(D, NK), dim3(256), 0, st, pred, target, C, K, s, w.bits, counts);
    else
        hipLaunchKernelGGL(ls_pack_kernel<1>, dim3(D, NK), dim3(256), 0, st, pred, target, C, K, s, w.bits, counts);
    RU_CHECK_LAUNCH("ls_pack_kernel");
    int zplane = 1;                                              // dilation 0: Z = G
    const unsigned gw = grid1d(s.words, 256, 4096), gv = grid1d(s.V, 256 * 4, 4096);
    for (int it = 0; it < dilation; ++it) {
        const int dst = zplane == 2 ? 3 : 2;
        hipLaunchKernelGGL(ls_dilate_kernel, dim3(gw, NK), dim3(256), 0, st, s, w.bits, zplane, dst);
        RU_CHECK_LAUNCH("ls_dilate_kernel");
        zplane = dst;
    }
    const LsPlanes planes = {w.bits, s.words, s.WW, zplane};
    const int rl = cc_label(planes, w.pz, (size_t)(w.pp - w.pz), w.cnt, D, H, W, dim3(gv, NK, 2), st);       // z = 0: Z into pz, z = 1: P into pp
    if (rl) return rl;
    hipLaunchKernelGGL(ls_count_kernel, dim3(gv, NK), dim3(256), 0, st, s.V, w.pz, w.pp, w.cnt, w.roots, w.nles, max_lesions);
    RU_CHECK_LAUNCH("ls_count_kernel");
    hipLaunchKernelGGL(ls_rank_kernel, dim3(NK), dim3(256), 0, st, w.roots, w.sorted, w.nles, max_lesions);
    RU_CHECK_LAUNCH("ls_rank_kernel");
    hipLaunchKernelGGL(ls_pair_kernel, dim3(D, NK), dim3(256), 0, st, s, slots, w.bits, zplane, w.pz, w.pp, w.sorted, w.nles, max_lesions, w.vol, w.tp, w.tab);
    RU_CHECK_LAUNCH("ls_pair_kernel");
    hipLaunchKernelGGL(ls_table_kernel, dim3(grid1d(slots, 256, 4096), NK), dim3(256), 0, st, s.V, slots, w.tab, w.cnt, w.msz, max_lesions);
    RU_CHECK_LAUNCH("ls_table_kernel");
    hipLaunchKernelGGL(ls_fp_kernel, dim3(gv, NK), dim3(256), 0, st, s, w.pp, w.cnt, w.nfp);
    RU_CHECK_LAUNCH("ls_fp_kernel");
    // the lesion counts come back to the host: they size the chunk loop, and more lesions than max_lesions is an error
    std::vector<int> nles(NK);
    hipError_t e = hipMemcpyAsync(nles.data(), w.nles, sizeof(int) * NK, hipMemcpyDeviceToHost, st);
    if (e != hipSuccess) return hip_fail(e, "hipMemcpyAsync(lesion counts)");
    e = hipStreamSynchronize(st);
    if (e != hipSuccess) return hip_fail(e, "hipStreamSynchronize(lesion counts)");
    for (int nk = 0; nk < NK; ++nk)
        RU_REQUIRE(nles[nk] <= max_lesions, "%s: %d ground-truth lesions in sample %d, region %d: more than max_lesions = %d", who, nles[nk], nk / K,
                   nk % K, max_lesions);
    for (int nk = 0; nk < NK; ++nk)
        for (int i0 = 0; i0 < nles[nk]; i0 += RU_LESION_CHUNK) {
            const int items = std::min(RU_LESION_CHUNK, nles[nk] - i0);
            hipLaunchKernelGGL(ls_item_kernel, dim3(D, items), dim3(256), 0, st, s, slots, w.bits, w.pz, w.pp, w.sorted, w.tab, w.vol, w.msz, w.tp, max_lesions, nk,
                               i0, sf_packed_bits(w.sf), w.icounts);
            RU_CHECK_LAUNCH("ls_item_kernel");
            const size_t at = (size_t)nk * max_lesions + i0;
            const int rc = ex.T >= 0 ? sf_packed_run_extras(items, D, H, W, w.sf, w.icounts, empty_value, w.vals + at * 4, ex.tol_bins, ex.T,
                                                            w.ex + at * ex_cols, st)
                                     : sf_packed_run(items, D, H, W, w.sf, w.icounts, empty_value, w.vals + at * 4, st);
            if (rc) return rc;
        }
    hipLaunchKernelGGL(ls_summary_kernel, dim3(cdiv(NK, 64)), dim3(64), 0, st, NK, max_lesions, w.nles, w.nfp, w.vol, w.msz, w.tp, w.vals, min_volume,
                       empty_value, summary, counts, table);
    RU_CHECK_LAUNCH("ls_summary_kernel");
    if (ex.T >= 0) {
        hipLaunchKernelGGL(ls_summary_ex_kernel, dim3(cdiv(NK, 64)), dim3(64), 0, st, NK, max_lesions, ex.T, w.nles, w.nfp, w.vol, w.ex, min_volume,
                           empty_value, ex.summary_ex, ex.table_ex);
        RU_CHECK_LAUNCH("ls_summary_ex_kernel");
    }
    return RU_OK;
}

}  // namespace

extern "C" int ru_lesion_metrics(const void* pred, const void* target, int kind, int N, int C, int D, int H, int W, int dilation, long long min_volume,
                                 double empty_value, double* summary, unsigned long long* counts, double* table, int max_lesions, void* ws,
                                 size_t ws_bytes, ru_stream_t stream) {
    const LsEx none = {nullptr, -1, nullptr, nullptr};
    return ls_entry("ru_lesion_metrics", pred, target, kind, N, C, D, H, W, dilation, min_volume, empty_value, summary, counts, table, none,
                    max_lesions, ws, ws_bytes, stream);
}

extern "C" size_t ru_lesion_distances_workspace_bytes(int kind, int N, int C, int D, int H, int W, int max_lesions, int T) {
    if (!ls_shape_ok(kind, N, C, D, H, W, max_lesions) || (size_t)D * H * W >= (size_t)INT_MAX || T < 0 || T > RU_SURFACE_MAX_TOL) return 0;
    return ls_layout(nullptr, (size_t)N * mask_regions(kind, C), mask_geom(D, H, W), ls_slots(D, H, W), (size_t)max_lesions, (size_t)T + 2).bytes;
}

extern "C" int ru_lesion_distances(const void* pred, const void* target, int kind, int N, int C, int D, int H, int W, int dilation, long long min_volume,
                                   double empty_value, const unsigned* tol_bins, int T, double* summary, unsigned long long* counts, double* table,
                                   double* summary_ex, double* table_ex, int max_lesions, void* ws, size_t ws_bytes, ru_stream_t stream) {
    RU_REQUIRE(T >= 0 && T <= RU_SURFACE_MAX_TOL && (T == 0 || tol_bins) && summary_ex,
               "ru_lesion_distances: T = %d tolerances: needs 0 <= T <= %d, their bin limits and `summary_ex`", T, RU_SURFACE_MAX_TOL);
    const LsEx ex = {tol_bins, T, summary_ex, table_ex};
    return ls_entry("ru_lesion_distances", pred, target, kind, N, C, D, H, W, dilation, min_volume, empty_value, summary, counts, table, ex,
                    max_lesions, ws, ws_bytes, stream);
}

extern "C" int ru_lesion_accumulate(const double* summary, double* acc, int N, int K, int nacc, int column, ru_stream_t stream) {
    RU_REQUIRE(summary && acc && N > 0 && K > 0 && nacc > 0 && nacc <= K && nacc <= 64 && column >= 0 && column < 2, "ru_lesion_accumulate: bad argument");
    hipLaunchKernelGGL(column_mean_kernel<2>, dim3(1), dim3(64), 0, (hipStream_t)stream, summary, acc, N, K, nacc, column);
    RU_CHECK_LAUNCH("column_mean_kernel");
    return RU_OK;
}
