// augment_voxel.hpp -- the per-voxel function of the training gathers, ONE copy for every entry point that produces a patch:
//   ru_augment_patch / ru_augment_patch_soft (pointwise.hip)   zoom_voxel   on SrcVolume
//   ru_augment_patch_affine (rotate.hip)                       affine_voxel on SrcVolume
//   ru_augment_batch_packed (resident.hip)                     both, on SrcBox<float> and SrcBox<unsigned short>
// Under -ffp-contract a second copy of these expressions need not round the same way, so the packed gathers instantiate THIS text with another
// source functor instead of restating it.  Nor need a second INSTANTIATION: which multiply the compiler fuses into an add depends on where it
// finds the two after inlining, hoisting and merging (in a kernel that holds several instantiations the zoom pass's scale * index was found
// apart from its subtraction and left unfused, and 128^3 patches then differed in a few voxels).  So contraction is OFF in these functions and
// every fused multiply-add the standalone kernels have always executed is written out: fma(scale, index, -floor) for the zoom weight,
// fmaf(w, value, acc) per corner, fmaf(z, gain, bias) in the tail.  What they compute does not depend on the optimiser any more.
//
// A source functor answers two questions: per axis, where a source index lies in its storage and whether it is stored at all (`tap`), and what is
// stored there (`image`, `label`, `soft`).  A corner that is not stored contributes raw intensity +0.0f, label 0, soft +0.0f: for SrcVolume that is
// the fill outside the volume, for SrcBox also the case's own zeros around its non-zero box.
//
// `Args` is any struct with the fields the bodies name: C, flags, P[3], mean / istd / gain / bias [RU_AUG_MAXC], and lo[3] + scale[3] (zoom) or
// m[9] + off[3] (affine).  data / target are passed on their own so that a batch can point them at a sample's slice.
#pragma once
#include "ru_common.h"

#include <math.h>

namespace ru {

struct AxisTap {
    size_t off;                  // offset of the index along this axis, in elements of one channel; harmless (0) where `in` is false
    bool in;                     // the index is stored
};

// the whole case [C][D][H][W] float32, label [D][H][W], soft [3][D][H][W] or null
struct SrcVolume {
    const float* img;
    const unsigned char* lab;
    const float* sft;
    int dims[3];
    size_t HW, DHW;
    __device__ __forceinline__ SrcVolume(const float* image, const unsigned char* label, const float* soft, int D, int H, int W)
        : img(image), lab(label), sft(soft), dims{D, H, W}, HW((size_t)H * W), DHW((size_t)D * H * W) {}
    // CHECK = false: the caller guarantees an index inside the volume (the zoom pass reflects into its crop)
    template <bool CHECK>
    __device__ __forceinline__ AxisTap tap(int ax, int idx) const {
        const size_t stride = ax == 0 ? HW : (ax == 1 ? (size_t)dims[2] : 1);
        AxisTap t;
        t.in = !CHECK || (idx >= 0 && idx < dims[ax]);
        t.off = t.in ? (size_t)idx * stride : 0;
        return t;
    }
    __device__ __forceinline__ float image(int c, size_t v) const { return img[(size_t)c * DHW + v]; }
    __device__ __forceinline__ int label(size_t v) const { return lab[v]; }
    __device__ __forceinline__ float soft(int k, size_t v) const { return sft[(size_t)k * DHW + v]; }
    static constexpr bool PAIRED = false;                          // see SrcBox<unsigned short>
    __device__ __forceinline__ bool adjacent(const AxisTap (&)[2]) const { return false; }
    __device__ __forceinline__ void image_pair(int, size_t, float&, float&) const {}
    __device__ __forceinline__ void label_pair(size_t, int&, int&) const {}
};

// a packed case (resident.hip): the non-zero box [lo, lo + size) of the volume, image [C][b0][b1][b2] of T = float or unsigned short (every
// value an exact integer 0..65535), label [b0][b1][b2], soft [3][b0][b1][b2] or null.  The box lies inside the volume, so its test per axis
// covers the volume's: an index inside the volume but outside the box reads as +0.0f / label 0, which is what the unpacked case holds there.
template <class T>
struct SrcBox {
    const T* img;
    const unsigned char* lab;
    const float* sft;
    int lo[3], size[3];
    size_t bHW, bDHW;
    __device__ __forceinline__ SrcBox(const void* image, const unsigned char* label, const float* soft, const int* box_lo, const int* box_size)
        : img((const T*)image), lab(label), sft(soft), lo{box_lo[0], box_lo[1], box_lo[2]}, size{box_size[0], box_size[1], box_size[2]},
          bHW((size_t)box_size[1] * box_size[2]), bDHW((size_t)box_size[0] * box_size[1] * box_size[2]) {}
    template <bool CHECK>
    __device__ __forceinline__ AxisTap tap(int ax, int idx) const {
        const size_t stride = ax == 0 ? bHW : (ax == 1 ? (size_t)size[2] : 1);
        const int r = idx - lo[ax];
        AxisTap t;
        t.in = r >= 0 && r < size[ax];
        t.off = t.in ? (size_t)r * stride : 0;
        return t;
    }
    __device__ __forceinline__ float image(int c, size_t v) const { return (float)img[(size_t)c * bDHW + v]; }
    __device__ __forceinline__ int label(size_t v) const { return lab[v]; }
    __device__ __forceinline__ float soft(int k, size_t v) const { return sft[(size_t)k * bDHW + v]; }
    // PAIRED (2-byte values only): where the two corners of a voxel along W are both stored and next to each other -- everywhere except at the
    // box's W faces -- one 4-byte load fetches both values of a channel and one 2-byte load both labels (gather_store decides who uses it).
    // The loads need not be aligned; the values, and so every operation on them, are those of the single loads.
    static constexpr bool PAIRED = sizeof(T) == 2;
    __device__ __forceinline__ bool adjacent(const AxisTap (&w)[2]) const { return w[0].in && w[1].in && w[1].off == w[0].off + 1; }
    __device__ __forceinline__ void image_pair(int c, size_t v, float& x0, float& x1) const {
        unsigned u;
        __builtin_memcpy(&u, (const unsigned short*)img + (size_t)c * bDHW + v, 4);
        x0 = (float)(u & 0xffffu);
        x1 = (float)(u >> 16);
    }
    __device__ __forceinline__ void label_pair(size_t v, int& l0, int& l1) const {
        unsigned short u;
        __builtin_memcpy(&u, lab + v, 2);
        l0 = u & 0xff;
        l1 = u >> 8;
    }
};

// the eight corners, z-score, gain / bias and the WT / TC / ET targets of one output voxel, linear index o of `total`.  PAIRS: the source fetches
// the two W corners of a (D, H) corner pair together (Src::adjacent holds for this voxel); the values and the order of the operations do not change.
template <bool SOFT, bool PAIRS, class Args, class Src>
__device__ __forceinline__ void gather_corners(const Args& a, const Src& S, const AxisTap (&tp)[3][2], const float (&wgt)[3][2], float* data, float* target,
                                               size_t o, size_t total) {
#pragma clang fp contract(off)
    float acc[RU_AUG_MAXC], nxt[RU_AUG_MAXC];
    int lnxt = 0;
#pragma unroll
    for (int c = 0; c < RU_AUG_MAXC; ++c) acc[c] = 0.f;
    float cw1 = 0.f, cw2 = 0.f, cw3 = 0.f;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const int qa = q >> 2, qb = (q >> 1) & 1, qc = q & 1;
        const float w = wgt[0][qa] * wgt[1][qb] * wgt[2][qc];
        const size_t v = tp[0][qa].off + tp[1][qb].off + tp[2][qc].off;
        const bool inside = tp[0][qa].in && tp[1][qb].in && tp[2][qc].in;
#pragma unroll
        for (int c = 0; c < RU_AUG_MAXC; ++c)
            if (c < a.C) {
                float x;
                if (!PAIRS) {
                    x = inside ? S.image(c, v) : 0.f;
                } else if (qc == 0) {
                    x = nxt[c] = 0.f;
                    if (inside) S.image_pair(c, v, x, nxt[c]);
                } else {
                    x = nxt[c];
                }
                acc[c] = __builtin_fmaf(w, x, acc[c]);
            }
        if (SOFT) {                                                // cw1..3 hold WT, TC, ET
            cw1 = __builtin_fmaf(w, inside ? S.soft(0, v) : 0.f, cw1);
            cw2 = __builtin_fmaf(w, inside ? S.soft(1, v) : 0.f, cw2);
            cw3 = __builtin_fmaf(w, inside ? S.soft(2, v) : 0.f, cw3);
        } else {
            int l;
            if (!PAIRS) {
                l = inside ? S.label(v) : 0;
            } else if (qc == 0) {
                l = lnxt = 0;
                if (inside) S.label_pair(v, l, lnxt);
            } else {
                l = lnxt;
            }
            cw1 += l == 1 ? w : 0.f;
            cw2 += l == 2 ? w : 0.f;
            cw3 += l == 3 ? w : 0.f;
        }
    }
#pragma unroll
    for (int c = 0; c < RU_AUG_MAXC; ++c)
        if (c < a.C) data[(size_t)c * total + o] = __builtin_fmaf((acc[c] - a.mean[c]) * a.istd[c], a.gain[c], a.bias[c]);
    if (SOFT) {
        target[o] = cw1;
        target[total + o] = cw2;
        target[2 * total + o] = cw3;
    } else {
        target[o] = (cw1 + cw2) + cw3;                             // WT = 1 + 2 + 3
        target[total + o] = cw1 + cw3;                             // TC = 1 + 3
        target[2 * total + o] = cw3;                               // ET = 3
    }
}

// MAY_PAIR: the caller's choice.  MI355X, 128^3 patch, uint16 case: pairing takes the affine pass at 30 degrees from 119 to 76 us (its scattered
// loads are what it waits for) and is even at 0 degrees, but costs the zoom pass 10 us (73 -> 83 us): its lanes read consecutive 2-byte values,
// which coalesce as they are, and half of the overlapping 4-byte loads are misaligned.  So affine_voxel pairs and zoom_voxel does not.
template <bool SOFT, bool MAY_PAIR, class Args, class Src>
__device__ __forceinline__ void gather_store(const Args& a, const Src& S, const AxisTap (&tp)[3][2], const float (&wgt)[3][2], float* data, float* target,
                                             size_t o, size_t total) {
    if constexpr (MAY_PAIR && Src::PAIRED) {
        if (S.adjacent(tp[2])) {
            gather_corners<SOFT, true>(a, S, tp, wgt, data, target, o, total);
            return;
        }
    }
    gather_corners<SOFT, false>(a, S, tp, wgt, data, target, o, total);
}

__device__ __forceinline__ int reflect_idx(int i, int n) {
    int m = i % (2 * n);
    if (m < 0) m += 2 * n;
    return m < n ? m : 2 * n - 1 - m;
}

// zoom pass (dataloader.py:147-205): output voxel (i, j, k) of the final layout [Q0][Q1][P2]; linear interpolation on the half-sample-symmetric
// extension of the CROP [a.lo, a.lo + a.P), source coordinate = scale * output index
template <bool SOFT, class Args, class Src>
__device__ __forceinline__ void zoom_voxel(const Args& a, const Src& S, float* data, float* target, int i, int j, int k, size_t o, size_t total) {
#pragma clang fp contract(off)
    const bool tr = (a.flags & 8) != 0;
    const int pa = tr ? j : i, pb = tr ? i : j;                    // indices before the transpose
    const int p[3] = {(a.flags & 1) ? a.P[0] - 1 - pa : pa, (a.flags & 2) ? a.P[1] - 1 - pb : pb, (a.flags & 4) ? a.P[2] - 1 - k : k};
    AxisTap tp[3][2];
    float wgt[3][2];
#pragma unroll
    for (int ax = 0; ax < 3; ++ax) {
        const double x = (double)p[ax] * a.scale[ax];
        const double f = floor(x);
        const int i0 = (int)f;
        const float t = (float)__builtin_fma((double)p[ax], a.scale[ax], -f);      // the exact product minus its floor, rounded once
        tp[ax][0] = S.template tap<false>(ax, reflect_idx(i0, a.P[ax]) + a.lo[ax]);
        tp[ax][1] = S.template tap<false>(ax, reflect_idx(i0 + 1, a.P[ax]) + a.lo[ax]);
        wgt[ax][0] = 1.f - t;
        wgt[ax][1] = t;
    }
    gather_store<SOFT, false>(a, S, tp, wgt, data, target, o, total);
}

// source coordinate of one axis of the affine pass; the roundings are the host restatement's (no fused multiply-add)
__device__ __forceinline__ double affine_coord(const double* m, double off, double q0, double q1, double q2, int n) {
#pragma clang fp contract(off)
    double s = ((m[0] * q0 + m[1] * q1) + m[2] * q2) + off;
    if (!(s >= -2.0)) s = -2.0;                                    // NaN too
    if (s > (double)n) s = (double)n;
    return s;
}

// affine pass (rotate.hip): output voxel (i, j, k) of the final layout [Q0][Q1][P2], gathered from the whole volume of extents dims[3]
template <bool SOFT, class Args, class Src>
__device__ __forceinline__ void affine_voxel(const Args& a, const Src& S, const int (&dims)[3], float* data, float* target, int i, int j, int k, size_t o,
                                             size_t total) {
#pragma clang fp contract(off)
    const bool tr = (a.flags & 8) != 0;
    const int pa = tr ? j : i, pb = tr ? i : j;                    // indices before the transpose
    const int p[3] = {(a.flags & 1) ? a.P[0] - 1 - pa : pa, (a.flags & 2) ? a.P[1] - 1 - pb : pb, (a.flags & 4) ? a.P[2] - 1 - k : k};
    AxisTap tp[3][2];
    float wgt[3][2];
#pragma unroll
    for (int ax = 0; ax < 3; ++ax) {
        const double x = affine_coord(a.m + 3 * ax, a.off[ax], (double)p[0], (double)p[1], (double)p[2], dims[ax]);
        const double f = floor(x);
        const int i0 = (int)f;                                     // -2 .. dims[ax]
        const float t = (float)(x - f);
        tp[ax][0] = S.template tap<true>(ax, i0);                  // a corner that is not stored is never loaded
        tp[ax][1] = S.template tap<true>(ax, i0 + 1);
        wgt[ax][0] = 1.f - t;
        wgt[ax][1] = t;
    }
    gather_store<SOFT, true>(a, S, tp, wgt, data, target, o, total);
}

// thread mappings of rotate.hip: a wave's brick is AF_BI x AF_BJ x AF_BK = 64 output voxels (D x H x W of the output layout); a workgroup's 4 waves
// sit 2 x 2 along H and W
constexpr unsigned AF_BI = 4, AF_BJ = 2, AF_BK = 8, AF_WJ = 2, AF_WK = 2;
constexpr unsigned AF_TILE_I = AF_BI, AF_TILE_J = AF_BJ * AF_WJ, AF_TILE_K = AF_BK * AF_WK;       // 4 x 4 x 16 per workgroup
static_assert(AF_BI * AF_BJ * AF_BK == 64 && AF_WJ * AF_WK == 4, "one brick per wavefront, four wavefronts per workgroup");
struct AffineTiles { unsigned n0, n1, n2; };                       // tiles per output axis; n0 * n1 * n2 workgroups
// output voxel of thread `tid` in tile `tile`; false where the brick is clipped at a far face
__device__ __forceinline__ bool brick_voxel(const AffineTiles& tiles, unsigned tile, unsigned tid, int Q0, int Q1, int P2, int& i, int& j, int& k) {
    const unsigned t2 = tile % tiles.n2, r = tile / tiles.n2;
    const unsigned t1 = r % tiles.n1, t0 = r / tiles.n1;
    const unsigned lane = tid & 63u, wave = tid >> 6;
    i = (int)(t0 * AF_TILE_I + lane / (AF_BK * AF_BJ));
    j = (int)(t1 * AF_TILE_J + (wave / AF_WK) * AF_BJ + (lane / AF_BK) % AF_BJ);
    k = (int)(t2 * AF_TILE_K + (wave % AF_WK) * AF_BK + lane % AF_BK);
    return i < Q0 && j < Q1 && k < P2;
}

}  // namespace ru
