// resident.hip -- the training set resident in HBM: packed case storage (ru_case_probe / ru_case_pack / ru_case_unpack) and the gather that cuts
// N training patches from N packed cases in one launch (ru_augment_batch_packed).
//
// Storage.  BraTS intensities are non-negative integers and most of a volume is exact zero around the brain.  A case is stored as the bounding
// box of everything that is not +0.0f / label 0 (by BIT PATTERN, so -0.0f and NaN are inside), the image as uint16 where every value survives
// float -> uint16 -> float bit for bit and as float32 otherwise, label uint8, soft float32.  Everything outside the box is +0.0f / label 0 bit for
// bit and everything inside is stored exactly, so unpack(pack(x)) == x byte for byte for ANY input, and a gather that reads +0.0f / 0 outside
// the box computes what the same gather computes on the unpacked case.
//
// Gather.  One workgroup-uniform sample index (blockIdx.y) picks a sample's descriptor out of the kernel arguments -- no host-to-device copy, no
// allocation, no workspace, no atomics, no synchronisation -- and the workgroup runs zoom_voxel or affine_voxel (augment_voxel.hpp), the same
// text ru_augment_patch and ru_augment_patch_affine instantiate on the whole-volume source, on a box source of float or unsigned short.  blockIdx.x
// is a 4 x 4 x 16 tile of the output (the brick mapping of rotate.hip) for affine samples and 256 consecutive output voxels for zoom samples and for
// affine samples that ask for the row mapping; the bytes do not depend on the mapping.  A launch whose samples all share kind, target and mode
// runs an instantiation of the kernel that holds that one body (the registers of the standalone gathers: 53-73 VGPRs); a launch that mixes them
// runs the instantiation with all eight bodies behind workgroup-uniform branches (86 VGPRs).  In the affine pass the uint16 source fetches the two W
// corners of a voxel with one 4-byte load where they are adjacent (augment_voxel.hpp), which halves the image loads of a rotated gather.
#include "ru_common.h"
#include "pw_helpers.hpp"
#include "augment_voxel.hpp"

#include <limits.h>
#include <math.h>

namespace ru {

// ------------------------------------------------------------------ probe
// out[0..2] = box lo, out[3..5] = box size, out[6] = 1 if every image value is an exact uint16 (outside the box every value is +0.0f, which
// is one, so "inside the box" and "anywhere" are the same statement), out[7] = 0.  Integer min / max atomics only: two calls give the same bytes.
struct ProbeState { int lo[3], hi[3], inexact, pad; };

__global__ void case_probe_init_kernel(ProbeState* st) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        for (int a = 0; a < 3; ++a) { st->lo[a] = INT_MAX; st->hi[a] = -1; }
        st->inexact = 0;
        st->pad = 0;
    }
}

__device__ __forceinline__ int wave_min_i(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const int u = __shfl_xor(v, o); v = u < v ? u : v; }
    return v;
}
__device__ __forceinline__ int wave_max_i(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const int u = __shfl_xor(v, o); v = u > v ? u : v; }
    return v;
}

__global__ __launch_bounds__(256) void case_probe_kernel(const float* __restrict__ image, const unsigned char* __restrict__ label,
                                                         const float* __restrict__ soft, int C, int D, int H, int W, ProbeState* st) {
    const size_t V = (size_t)D * H * W;
    int lo[3] = {INT_MAX, INT_MAX, INT_MAX}, hi[3] = {-1, -1, -1}, inexact = 0;
    for (size_t v = (size_t)blockIdx.x * 256 + threadIdx.x; v < V; v += (size_t)gridDim.x * 256) {
        unsigned any = label ? (unsigned)label[v] : 0u;
        for (int c = 0; c < C; ++c) {
            const float x = image[(size_t)c * V + v];
            const unsigned b = __builtin_bit_cast(unsigned, x);
            any |= b;
            // exact uint16 by bit pattern: a value in [0, 65535] whose integer part converts back to the same bits (-0.0f, NaN, fractions do not)
            const bool ok = x >= 0.f && x <= 65535.f && __builtin_bit_cast(unsigned, (float)(unsigned short)(unsigned)x) == b;
            inexact |= ok ? 0 : 1;
        }
        if (soft)
            for (int k = 0; k < 3; ++k) any |= __builtin_bit_cast(unsigned, soft[(size_t)k * V + v]);
        if (any) {
            const int p[3] = {(int)(v / ((size_t)H * W)), (int)((v / W) % H), (int)(v % W)};
#pragma unroll
            for (int a = 0; a < 3; ++a) { lo[a] = p[a] < lo[a] ? p[a] : lo[a]; hi[a] = p[a] > hi[a] ? p[a] : hi[a]; }
        }
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) { lo[a] = wave_min_i(lo[a]); hi[a] = wave_max_i(hi[a]); }
    inexact = wave_max_i(inexact);
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            if (hi[a] >= 0) { atomicMin(&st->lo[a], lo[a]); atomicMax(&st->hi[a], hi[a]); }
        }
        if (inexact) atomicMax(&st->inexact, 1);
    }
}

__global__ void case_probe_final_kernel(ProbeState* st) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    int* out = (int*)st;
    const bool empty = st->hi[0] < 0;                              // an all-zero case: lo = (0,0,0), size = (1,1,1)
    const int inexact = st->inexact;
    for (int a = 0; a < 3; ++a) {
        const int l = empty ? 0 : st->lo[a], h = empty ? 0 : st->hi[a];
        out[a] = l;
        out[3 + a] = h - l + 1;
    }
    out[6] = inexact ? 0 : 1;
    out[7] = 0;
}

// ------------------------------------------------------------------ pack / unpack
struct PackArgs {
    const float* image; const unsigned char* label; const float* soft;          // full arrays (pack: in, unpack: out)
    void* pimage; unsigned char* plabel; float* psoft;                           // packed arrays (pack: out, unpack: in)
    int C, D, H, W;
    Box3 b;
};

template <class T>
__global__ __launch_bounds__(256) void case_pack_kernel(const PackArgs a) {
    const size_t V = (size_t)a.D * a.H * a.W, bV = (size_t)a.b.size[0] * a.b.size[1] * a.b.size[2];
    T* pimg = (T*)a.pimage;
    for (size_t o = (size_t)blockIdx.x * 256 + threadIdx.x; o < bV; o += (size_t)gridDim.x * 256) {
        const int k = (int)(o % a.b.size[2]);
        const size_t r = o / a.b.size[2];
        const int j = (int)(r % a.b.size[1]), i = (int)(r / a.b.size[1]);
        const size_t v = ((size_t)(i + a.b.lo[0]) * a.H + (j + a.b.lo[1])) * a.W + (k + a.b.lo[2]);
        for (int c = 0; c < a.C; ++c) {
            const float x = a.image[(size_t)c * V + v];
            pimg[(size_t)c * bV + o] = sizeof(T) == 2 ? (T)(unsigned)x : (T)x;
        }
        a.plabel[o] = a.label[v];
        if (a.soft)
            for (int c = 0; c < 3; ++c) a.psoft[(size_t)c * bV + o] = a.soft[(size_t)c * V + v];
    }
}

template <class T>
__global__ __launch_bounds__(256) void case_unpack_kernel(const PackArgs a, float* image_out, unsigned char* label_out, float* soft_out) {
    const size_t V = (size_t)a.D * a.H * a.W, bV = (size_t)a.b.size[0] * a.b.size[1] * a.b.size[2];
    const T* pimg = (const T*)a.pimage;
    for (size_t v = (size_t)blockIdx.x * 256 + threadIdx.x; v < V; v += (size_t)gridDim.x * 256) {
        const int k = (int)(v % a.W) - a.b.lo[2];
        const size_t r = v / a.W;
        const int j = (int)(r % a.H) - a.b.lo[1], i = (int)(r / a.H) - a.b.lo[0];
        const bool in = i >= 0 && i < a.b.size[0] && j >= 0 && j < a.b.size[1] && k >= 0 && k < a.b.size[2];
        const size_t o = in ? ((size_t)i * a.b.size[1] + j) * a.b.size[2] + k : 0;
        for (int c = 0; c < a.C; ++c) image_out[(size_t)c * V + v] = in ? (float)pimg[(size_t)c * bV + o] : 0.f;
        label_out[v] = in ? a.plabel[o] : (unsigned char)0;
        if (soft_out)
            for (int c = 0; c < 3; ++c) soft_out[(size_t)c * V + v] = in ? a.psoft[(size_t)c * bV + o] : 0.f;
    }
}

// ------------------------------------------------------------------ the packed gather
// one sample of a launch: a case descriptor and a patch descriptor flattened into the field names zoom_voxel / affine_voxel read
struct PackedSample {
    const void* image;           // packed [C][b0][b1][b2] unsigned short (RU_PACK_U16) or float (RU_PACK_F32)
    const unsigned char* label;  // packed [b0][b1][b2]
    const float* soft;           // packed [3][b0][b1][b2] or null
    int kind, mode, mapping, C, flags;
    int dims[3], blo[3], bsize[3];
    int lo[3], P[3];             // crop (zoom) and patch extents
    double scale[3];             // zoom
    double m[9], off[3];         // affine
    float mean[RU_AUG_MAXC], istd[RU_AUG_MAXC], gain[RU_AUG_MAXC], bias[RU_AUG_MAXC];
};
struct PackedBatch {
    PackedSample s[RU_AUG_BATCH_MAX];
    float* data;                 // [n][C][Q0][Q1][P2]
    float* target;               // [n][3][Q0][Q1][P2]
    AffineTiles tiles;
};
static_assert(sizeof(PackedBatch) <= 4096 - 64, "the kernel argument block must stay under HIP's 4 KB limit");

template <bool SOFT, class Src>
__device__ __forceinline__ void packed_sample(const PackedSample& a, const Src& S, int mode, const AffineTiles& tiles, float* data, float* target) {
    const bool tr = (a.flags & 8) != 0;
    const int Q0 = tr ? a.P[1] : a.P[0], Q1 = tr ? a.P[0] : a.P[1], P2 = a.P[2];
    const size_t total = (size_t)Q0 * Q1 * P2;
    if (mode == RU_AUG_AFFINE && a.mapping != RU_AFFINE_MAP_ROW) {
        int i, j, k;
        if (brick_voxel(tiles, blockIdx.x, threadIdx.x, Q0, Q1, P2, i, j, k))
            affine_voxel<SOFT>(a, S, a.dims, data, target, i, j, k, ((size_t)i * Q1 + j) * P2 + k, total);
        return;
    }
    for (size_t o = (size_t)blockIdx.x * 256 + threadIdx.x; o < total; o += (size_t)gridDim.x * 256) {
        const int k = (int)(o % P2);
        const size_t r = o / P2;
        if (mode == RU_AUG_AFFINE) affine_voxel<SOFT>(a, S, a.dims, data, target, (int)(r / Q1), (int)(r % Q1), k, o, total);
        else zoom_voxel<SOFT>(a, S, data, target, (int)(r / Q1), (int)(r % Q1), k, o, total);
    }
}

// SPEC < 0: the launch mixes samples, and kind, soft and mode are read from the sample (workgroup-uniform branches over all eight bodies).
// SPEC >= 0: every sample of the launch has kind = SPEC & 1, soft = (SPEC >> 1) & 1, mode = (SPEC >> 2) & 1, and the kernel holds that one body
// only -- the registers of the standalone gather instead of the union's.  The bodies are the same instantiations either way.
constexpr int packed_spec(int kind, bool soft, int mode) { return (kind == RU_PACK_U16 ? 1 : 0) | (soft ? 2 : 0) | (mode == RU_AUG_AFFINE ? 4 : 0); }
static_assert(RU_PACK_U16 == 1 && RU_PACK_F32 == 0 && RU_AUG_AFFINE == 1 && RU_AUG_ZOOM == 0, "packed_spec's bits are the header's values");
template <int SPEC>
__global__ __launch_bounds__(256) void augment_batch_packed_kernel(const PackedBatch b) {
    const unsigned n = blockIdx.y;                                 // workgroup-uniform: every branch below is
    // b.s[n] with a run-time n would make the compiler copy the whole by-value argument to scratch first.  The explicit arguments start at offset 0
    // of the kernel argument segment (the code object's .args metadata), so the sample is addressed there and read with scalar loads.
    static_assert(offsetof(PackedBatch, s) == 0, "the samples lead the argument block");
    const PackedSample& a = ((const PackedSample*)__builtin_amdgcn_kernarg_segment_ptr())[n];
    const size_t total = (size_t)a.P[0] * a.P[1] * a.P[2];
    float* data = b.data + (size_t)n * a.C * total;
    float* target = b.target + (size_t)n * 3 * total;
    const int kind = SPEC < 0 ? a.kind : (SPEC & 1), mode = SPEC < 0 ? a.mode : ((SPEC >> 2) & 1);
    const bool soft = SPEC < 0 ? a.soft != nullptr : ((SPEC >> 1) & 1) != 0;
    if (kind == RU_PACK_U16) {
        const SrcBox<unsigned short> S(a.image, a.label, a.soft, a.blo, a.bsize);
        if (soft) packed_sample<true>(a, S, mode, b.tiles, data, target);
        else packed_sample<false>(a, S, mode, b.tiles, data, target);
    } else {
        const SrcBox<float> S(a.image, a.label, a.soft, a.blo, a.bsize);
        if (soft) packed_sample<true>(a, S, mode, b.tiles, data, target);
        else packed_sample<false>(a, S, mode, b.tiles, data, target);
    }
}

template <int SPEC>
static void packed_launch(const PackedBatch& b, dim3 grid, hipStream_t s) {
    hipLaunchKernelGGL(augment_batch_packed_kernel<SPEC>, grid, dim3(256), 0, s, b);
}

static int pack_args(PackArgs& a, const char* who, int kind, int C, int D, int H, int W, const int* box_lo, const int* box_size) {
    RU_REQUIRE(C >= 1 && C <= RU_AUG_MAXC, "%s: 1..%d channels (got %d)", who, RU_AUG_MAXC, C);
    RU_REQUIRE(D > 0 && H > 0 && W > 0, "%s: the volume extents must be positive", who);
    RU_REQUIRE(kind == RU_PACK_F32 || kind == RU_PACK_U16, "%s: unknown kind %d", who, kind);
    RU_REQUIRE(box_lo && box_size, "%s: null argument", who);
    a.C = C; a.D = D; a.H = H; a.W = W;
    return make_box(a.b, box_lo, box_size, D, H, W, who);
}

}  // namespace ru

using namespace ru;

extern "C" int ru_case_probe(const float* image, const unsigned char* label, const float* soft, int C, int D, int H, int W, int* out8, ru_stream_t stream) {
    RU_REQUIRE(image && label && out8, "ru_case_probe: null argument");
    RU_REQUIRE(C >= 1 && C <= RU_AUG_MAXC, "ru_case_probe: 1..%d channels (got %d)", RU_AUG_MAXC, C);
    RU_REQUIRE(D > 0 && H > 0 && W > 0, "ru_case_probe: the volume extents must be positive");
    hipStream_t s = (hipStream_t)stream;
    ProbeState* st = (ProbeState*)out8;
    static_assert(sizeof(ProbeState) == 8 * sizeof(int), "ru_case_probe writes 8 ints");
    hipLaunchKernelGGL(case_probe_init_kernel, dim3(1), dim3(64), 0, s, st);
    RU_CHECK_LAUNCH("case_probe_init_kernel");
    hipLaunchKernelGGL(case_probe_kernel, dim3(grid1d((size_t)D * H * W, 256 * 4, 2048)), dim3(256), 0, s, image, label, soft, C, D, H, W, st);
    RU_CHECK_LAUNCH("case_probe_kernel");
    hipLaunchKernelGGL(case_probe_final_kernel, dim3(1), dim3(64), 0, s, st);
    RU_CHECK_LAUNCH("case_probe_final_kernel");
    return RU_OK;
}

extern "C" int ru_case_pack(const float* image, const unsigned char* label, const float* soft, int C, int D, int H, int W, const int* box_lo,
                            const int* box_size, int kind, void* image_out, unsigned char* label_out, float* soft_out, ru_stream_t stream) {
    RU_REQUIRE(image && label && image_out && label_out && (soft == nullptr) == (soft_out == nullptr), "ru_case_pack: null argument");
    PackArgs a{};
    const int rc = pack_args(a, "ru_case_pack", kind, C, D, H, W, box_lo, box_size);
    if (rc) return rc;
    a.image = image; a.label = label; a.soft = soft; a.pimage = image_out; a.plabel = label_out; a.psoft = soft_out;
    const size_t bV = (size_t)box_size[0] * box_size[1] * box_size[2];
    if (kind == RU_PACK_U16) hipLaunchKernelGGL(case_pack_kernel<unsigned short>, dim3(grid1d(bV, 256, 4096)), dim3(256), 0, (hipStream_t)stream, a);
    else hipLaunchKernelGGL(case_pack_kernel<float>, dim3(grid1d(bV, 256, 4096)), dim3(256), 0, (hipStream_t)stream, a);
    RU_CHECK_LAUNCH("case_pack_kernel");
    return RU_OK;
}

extern "C" int ru_case_unpack(const void* image, const unsigned char* label, const float* soft, int kind, int C, int D, int H, int W, const int* box_lo,
                              const int* box_size, float* image_out, unsigned char* label_out, float* soft_out, ru_stream_t stream) {
    RU_REQUIRE(image && label && image_out && label_out && (soft == nullptr) == (soft_out == nullptr), "ru_case_unpack: null argument");
    PackArgs a{};
    const int rc = pack_args(a, "ru_case_unpack", kind, C, D, H, W, box_lo, box_size);
    if (rc) return rc;
    a.pimage = const_cast<void*>(image); a.plabel = const_cast<unsigned char*>(label); a.psoft = const_cast<float*>(soft);
    const unsigned g = grid1d((size_t)D * H * W, 256, 4096);
    if (kind == RU_PACK_U16) hipLaunchKernelGGL(case_unpack_kernel<unsigned short>, dim3(g), dim3(256), 0, (hipStream_t)stream, a, image_out, label_out, soft_out);
    else hipLaunchKernelGGL(case_unpack_kernel<float>, dim3(g), dim3(256), 0, (hipStream_t)stream, a, image_out, label_out, soft_out);
    RU_CHECK_LAUNCH("case_unpack_kernel");
    return RU_OK;
}

extern "C" int ru_augment_batch_packed(const ru_case_desc* cases, const ru_patch_desc* patches, int N, const int* patch, float* data_out,
                                       float* target_out, ru_stream_t stream) {
    RU_REQUIRE(cases && patches && patch && data_out && target_out, "ru_augment_batch_packed: null argument");
    RU_REQUIRE(N >= 1, "ru_augment_batch_packed: at least one sample (got %d)", N);
    RU_REQUIRE(patch[0] > 0 && patch[1] > 0 && patch[2] > 0, "ru_augment_batch_packed: the patch extents must be positive");
    RU_REQUIRE((size_t)patch[0] * patch[1] * patch[2] < (size_t)INT_MAX, "ru_augment_batch_packed: patch too large for 32-bit voxel indices");
    const size_t total = (size_t)patch[0] * patch[1] * patch[2];
    const int C = cases[0].C;
    // every check of every sample before the first launch
    for (int n = 0; n < N; ++n) {
        const ru_case_desc& c = cases[n];
        const ru_patch_desc& p = patches[n];
        RU_REQUIRE(c.image && c.label, "ru_augment_batch_packed: sample %d: null case pointer", n);
        RU_REQUIRE(c.kind == RU_PACK_F32 || c.kind == RU_PACK_U16, "ru_augment_batch_packed: sample %d: unknown kind %d", n, c.kind);
        RU_REQUIRE(c.C >= 1 && c.C <= RU_AUG_MAXC, "ru_augment_batch_packed: sample %d: 1..%d channels (got %d)", n, RU_AUG_MAXC, c.C);
        RU_REQUIRE(c.C == C, "ru_augment_batch_packed: sample %d has %d channels, sample 0 has %d", n, c.C, C);
        Box3 box;
        RU_REQUIRE(c.dims[0] > 0 && c.dims[1] > 0 && c.dims[2] > 0, "ru_augment_batch_packed: sample %d: the volume extents must be positive", n);
        if (make_box(box, c.box_lo, c.box_size, c.dims[0], c.dims[1], c.dims[2], "ru_augment_batch_packed")) return RU_EINVAL;
        RU_REQUIRE((p.flags & ~15) == 0, "ru_augment_batch_packed: sample %d: flags are bits 0..3", n);
        RU_REQUIRE(!(p.flags & 8) || N == 1 || patch[0] == patch[1],
                   "ru_augment_batch_packed: sample %d is transposed: a batch needs P0 == P1 (got %d x %d)", n, patch[0], patch[1]);
        if (p.mode == RU_AUG_ZOOM) {
            for (int i = 0; i < 3; ++i) {
                RU_REQUIRE(p.crop_lo[i] >= 0 && p.crop_lo[i] + patch[i] <= c.dims[i], "ru_augment_batch_packed: sample %d: the crop must lie inside the volume", n);
                RU_REQUIRE(p.scale[i] > 0.0, "ru_augment_batch_packed: sample %d: scale must be positive", n);
                RU_REQUIRE(isfinite(p.scale[i]), "ru_augment_batch_packed: sample %d: scale[%d] is not finite", n, i);
                RU_REQUIRE(p.scale[i] * (double)(patch[i] - 1) < 1073741824.0,
                           "ru_augment_batch_packed: sample %d: scale[%d] * (patch[%d] - 1) = %g reaches 2^30", n, i, i, p.scale[i] * (double)(patch[i] - 1));
            }
        } else {
            RU_REQUIRE(p.mode == RU_AUG_AFFINE, "ru_augment_batch_packed: sample %d: unknown mode %d", n, p.mode);
            RU_REQUIRE(p.mapping == RU_AFFINE_MAP_DEFAULT || p.mapping == RU_AFFINE_MAP_ROW || p.mapping == RU_AFFINE_MAP_BRICK,
                       "ru_augment_batch_packed: sample %d: unknown thread mapping %d", n, p.mapping);
            for (int i = 0; i < 9; ++i) RU_REQUIRE(isfinite(p.matrix[i]), "ru_augment_batch_packed: sample %d: matrix[%d] is not finite", n, i);
            for (int i = 0; i < 3; ++i) RU_REQUIRE(isfinite(p.offset[i]), "ru_augment_batch_packed: sample %d: offset[%d] is not finite", n, i);
            const double* m = p.matrix;
            const double det = m[0] * (m[4] * m[8] - m[5] * m[7]) - m[1] * (m[3] * m[8] - m[5] * m[6]) + m[2] * (m[3] * m[7] - m[4] * m[6]);
            RU_REQUIRE(fabs(det) >= 1e-6, "ru_augment_batch_packed: sample %d: |det(matrix)| = %g is below 1e-6 (a collapsed patch)", n, fabs(det));
        }
    }
    // the tile grid of the brick mapping covers the output; with a transposed sample P0 == P1 (or N == 1), so one grid serves every sample
    const bool tr = N == 1 && (patches[0].flags & 8) != 0;
    AffineTiles tiles;
    tiles.n0 = ((unsigned)(tr ? patch[1] : patch[0]) + AF_TILE_I - 1u) / AF_TILE_I;
    tiles.n1 = ((unsigned)(tr ? patch[0] : patch[1]) + AF_TILE_J - 1u) / AF_TILE_J;
    tiles.n2 = ((unsigned)patch[2] + AF_TILE_K - 1u) / AF_TILE_K;
    const size_t nblk = (size_t)tiles.n0 * tiles.n1 * tiles.n2;   // every tile holds a voxel, so nblk <= total < 2^31; and nblk * 256 >= total
    for (int n0 = 0; n0 < N; n0 += RU_AUG_BATCH_MAX) {
        const int cnt = N - n0 < RU_AUG_BATCH_MAX ? N - n0 : RU_AUG_BATCH_MAX;
        PackedBatch b{};
        int spec = -2;                                             // -2: no sample yet, -1: mixed
        b.data = data_out + (size_t)n0 * C * total;
        b.target = target_out + (size_t)n0 * 3 * total;
        b.tiles = tiles;
        for (int n = 0; n < cnt; ++n) {
            const ru_case_desc& c = cases[n0 + n];
            const ru_patch_desc& p = patches[n0 + n];
            PackedSample& a = b.s[n];
            a.image = c.image; a.label = c.label; a.soft = c.soft; a.kind = c.kind; a.mode = p.mode; a.mapping = p.mapping; a.C = c.C; a.flags = p.flags;
            for (int i = 0; i < 3; ++i) {
                a.dims[i] = c.dims[i]; a.blo[i] = c.box_lo[i]; a.bsize[i] = c.box_size[i];
                a.lo[i] = p.crop_lo[i]; a.P[i] = patch[i]; a.scale[i] = p.scale[i]; a.off[i] = p.offset[i];
            }
            for (int i = 0; i < 9; ++i) a.m[i] = p.matrix[i];
            for (int ch = 0; ch < c.C; ++ch) { a.mean[ch] = c.mean[ch]; a.istd[ch] = c.inv_std[ch]; a.gain[ch] = p.gain[ch]; a.bias[ch] = p.bias[ch]; }
            const int sp = packed_spec(c.kind, c.soft != nullptr, p.mode);
            spec = spec == -2 || spec == sp ? sp : -1;
        }
        // a launch of zoom samples only takes ru_augment_patch's grid; the tile grid covers the output for every other mix
        const bool zoom_only = spec >= 0 && !(spec & 4);
        const dim3 grid(zoom_only ? grid1d(total, 256, 4096) : (unsigned)nblk, (unsigned)cnt);
        hipStream_t s = (hipStream_t)stream;
        switch (spec) {
            case 0: packed_launch<0>(b, grid, s); break;
            case 1: packed_launch<1>(b, grid, s); break;
            case 2: packed_launch<2>(b, grid, s); break;
            case 3: packed_launch<3>(b, grid, s); break;
            case 4: packed_launch<4>(b, grid, s); break;
            case 5: packed_launch<5>(b, grid, s); break;
            case 6: packed_launch<6>(b, grid, s); break;
            case 7: packed_launch<7>(b, grid, s); break;
            default: packed_launch<-1>(b, grid, s); break;
        }
        RU_CHECK_LAUNCH("augment_batch_packed_kernel");
    }
    return RU_OK;
}
