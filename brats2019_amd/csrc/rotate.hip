// rotate.hip -- rotation augmentation: one affine resampling pass from the resident case to a training patch (ru_augment_patch_affine).
//
// The reference cannot rotate cheaply: its reader crops first and resamples the crop with mode='reflect', so a rotated patch would show mirrored
// tissue in its corners.  Here the whole case is in HBM, so the patch is gathered from the real volume around the crop and a fill value is needed
// only where the patch leaves the VOLUME:
//
//   scipy.ndimage.affine_transform(volume, matrix, offset, output_shape=patch, order=1, mode='grid-constant', cval=0)
//
// per image channel, per one-hot label class (or per soft channel), followed by the tail of augment_patch_kernel (pointwise.hip), expression for
// expression: ((acc - mean) * istd) * gain + bias, WT / TC / ET sums, flips, D <-> H transpose.  For output index q (before flips and transpose)
// the source coordinate is s = matrix q + offset in float64, each product and sum rounded on its own in the order
// ((m0 q0 + m1 q1) + m2 q2) + offset; f = floor(s), t = (float)(s - f); the eight corners f + {0,1}^3 are weighted by products of 1 - t and t; a
// corner outside the volume contributes raw intensity 0 (it z-scores to what real background gets), label 0, soft 0.  A coordinate that is not a
// number, below -2 or above the extent is moved to -2 / the extent: both of its corners are outside either way, and the integer conversion stays defined.
//
// Thread mapping, chosen at launch (`mapping`):
//   RU_AFFINE_MAP_ROW    256 consecutive output voxels along W per workgroup, as augment_patch_kernel: contiguous stores, but under a rotation a
//                        wave's 64 voxels lie on a slanted line and the 8 corners of every lane fall into 128-byte lines of their own.
//   RU_AFFINE_MAP_BRICK  a wave owns a compact 4 x 2 x 8 (D x H x W) brick of output voxels and the 4 waves of a workgroup sit 2 x 2 along H and W
//                        (a 4 x 4 x 16 tile): the wave's source footprint is a small rotated box whose lines are shared between lanes, and a
//                        brick row is 32 contiguous bytes of every output channel.  Bricks are clipped at the patch's far faces.
//   RU_AFFINE_MAP_DEFAULT = BRICK: the faster one on a rotated patch.  MI355X, 4 x 240 x 240 x 155 case, 128^3 patch, back to back
//   (tools/rotate_time.py, profiles/rotate_time.txt): at 15 / 30 degrees on all axes the row mapping costs about 3.0x / 3.9x the zoom pass, the
//   brick mapping about 1.75x / 1.9x; at 0 degrees both are within 10 % of the zoom pass.  Brick shapes tried in the same
//   setting, at 0 / 15 / 30 degrees: 4 x 4 x 4 per wave, waves along W: 99 / 147 / 155 us; 2 x 4 x 8, waves along W: 67 / 143 / 182 us;
//   2 x 2 x 16: 65 / 173 / 191 us; 4 x 2 x 8 with waves 2 x 2 (this one): 75 / 125 / 139 us; the row mapping: 80 / 218 / 289 us.  Sending
//   consecutive tiles to one XCD (blockIdx remapped by blockIdx % 8) made 30 degrees 2x slower on every shape and is not done.
// Both mappings run the same per-voxel function, so they give the same bytes.  No atomics, no workspace, no synchronisation: the call only enqueues.
#include "ru_common.h"
#include "pw_helpers.hpp"
#include "augment_voxel.hpp"

#include <limits.h>
#include <math.h>

namespace ru {

struct AffineArgs {
    const float* image;          // [C][D][H][W] raw modalities
    const unsigned char* label;  // [D][H][W] values 0..3
    const float* soft;           // [3][D][H][W] or null
    float* data;                 // [C][Q0][Q1][P2]
    float* target;               // [3][Q0][Q1][P2]
    int C, D, H, W;
    int P[3];
    double m[9], off[3];
    int flags;                   // bit 0-2: flip D, H, W; bit 3: transpose D <-> H
    float mean[RU_AUG_MAXC], istd[RU_AUG_MAXC], gain[RU_AUG_MAXC], bias[RU_AUG_MAXC];
};

// The per-voxel function is affine_voxel (augment_voxel.hpp), shared with the packed gather of resident.hip; so are the brick constants.
template <bool SOFT>
__global__ __launch_bounds__(256) void affine_row_kernel(const AffineArgs a) {
    const bool tr = (a.flags & 8) != 0;
    const int Q0 = tr ? a.P[1] : a.P[0], Q1 = tr ? a.P[0] : a.P[1], P2 = a.P[2];
    const size_t total = (size_t)Q0 * Q1 * P2;
    const SrcVolume S(a.image, a.label, a.soft, a.D, a.H, a.W);
    for (size_t o = (size_t)blockIdx.x * 256 + threadIdx.x; o < total; o += (size_t)gridDim.x * 256) {
        const int k = (int)(o % P2);
        const size_t r = o / P2;
        affine_voxel<SOFT>(a, S, S.dims, a.data, a.target, (int)(r / Q1), (int)(r % Q1), k, o, total);
    }
}

template <bool SOFT>
__global__ __launch_bounds__(256) void affine_brick_kernel(const AffineArgs a, const AffineTiles tiles) {
    const bool tr = (a.flags & 8) != 0;
    const int Q0 = tr ? a.P[1] : a.P[0], Q1 = tr ? a.P[0] : a.P[1], P2 = a.P[2];
    const size_t total = (size_t)Q0 * Q1 * P2;
    const SrcVolume S(a.image, a.label, a.soft, a.D, a.H, a.W);
    int i, j, k;
    if (brick_voxel(tiles, blockIdx.x, threadIdx.x, Q0, Q1, P2, i, j, k))      // bricks are clipped at the far faces
        affine_voxel<SOFT>(a, S, S.dims, a.data, a.target, i, j, k, ((size_t)i * Q1 + j) * P2 + k, total);
}

}  // namespace ru

using namespace ru;

extern "C" int ru_augment_patch_affine(const float* image, const unsigned char* label, const float* soft, const float* mean, const float* inv_std,
                                       int C, int D, int H, int W, const int* patch, const double* matrix, const double* offset, int flags,
                                       const float* gain, const float* bias, int mapping, float* data_out, float* target_out, ru_stream_t stream) {
    RU_REQUIRE(image && (label || soft) && mean && inv_std && patch && matrix && offset && gain && bias && data_out && target_out,
               "ru_augment_patch_affine: null argument");
    RU_REQUIRE(C >= 1 && C <= RU_AUG_MAXC, "ru_augment_patch_affine: 1..%d channels (got %d)", RU_AUG_MAXC, C);
    RU_REQUIRE(D > 0 && H > 0 && W > 0, "ru_augment_patch_affine: the volume extents must be positive");
    RU_REQUIRE(patch[0] > 0 && patch[1] > 0 && patch[2] > 0, "ru_augment_patch_affine: the patch extents must be positive");
    RU_REQUIRE((size_t)patch[0] * patch[1] * patch[2] < (size_t)INT_MAX, "ru_augment_patch_affine: patch too large for 32-bit voxel indices");
    RU_REQUIRE((flags & ~15) == 0, "ru_augment_patch_affine: flags are bits 0..3");
    RU_REQUIRE(mapping == RU_AFFINE_MAP_DEFAULT || mapping == RU_AFFINE_MAP_ROW || mapping == RU_AFFINE_MAP_BRICK,
               "ru_augment_patch_affine: unknown thread mapping %d", mapping);
    for (int i = 0; i < 9; ++i) RU_REQUIRE(isfinite(matrix[i]), "ru_augment_patch_affine: matrix[%d] is not finite", i);
    for (int i = 0; i < 3; ++i) RU_REQUIRE(isfinite(offset[i]), "ru_augment_patch_affine: offset[%d] is not finite", i);
    const double* m = matrix;
    const double det = m[0] * (m[4] * m[8] - m[5] * m[7]) - m[1] * (m[3] * m[8] - m[5] * m[6]) + m[2] * (m[3] * m[7] - m[4] * m[6]);
    RU_REQUIRE(fabs(det) >= 1e-6, "ru_augment_patch_affine: |det(matrix)| = %g is below 1e-6 (a collapsed patch)", fabs(det));      // false for NaN as well
    AffineArgs a{};
    a.image = image; a.label = label; a.soft = soft; a.data = data_out; a.target = target_out; a.C = C; a.D = D; a.H = H; a.W = W; a.flags = flags;
    for (int i = 0; i < 3; ++i) { a.P[i] = patch[i]; a.off[i] = offset[i]; }
    for (int i = 0; i < 9; ++i) a.m[i] = matrix[i];
    for (int c = 0; c < C; ++c) { a.mean[c] = mean[c]; a.istd[c] = inv_std[c]; a.gain[c] = gain[c]; a.bias[c] = bias[c]; }
    const size_t total = (size_t)patch[0] * patch[1] * patch[2];
    hipStream_t s = (hipStream_t)stream;
    if (mapping == RU_AFFINE_MAP_ROW) {
        if (soft) hipLaunchKernelGGL(affine_row_kernel<true>, dim3(grid1d(total, 256, 4096)), dim3(256), 0, s, a);
        else hipLaunchKernelGGL(affine_row_kernel<false>, dim3(grid1d(total, 256, 4096)), dim3(256), 0, s, a);
        RU_CHECK_LAUNCH("affine_row_kernel");
        return RU_OK;
    }
    const bool tr = (flags & 8) != 0;
    AffineTiles t;
    t.n0 = ((unsigned)(tr ? patch[1] : patch[0]) + AF_TILE_I - 1u) / AF_TILE_I;
    t.n1 = ((unsigned)(tr ? patch[0] : patch[1]) + AF_TILE_J - 1u) / AF_TILE_J;
    t.n2 = ((unsigned)patch[2] + AF_TILE_K - 1u) / AF_TILE_K;
    const size_t nblk = (size_t)t.n0 * t.n1 * t.n2;                // every tile holds a voxel, so nblk <= total < 2^31
    if (soft) hipLaunchKernelGGL(affine_brick_kernel<true>, dim3((unsigned)nblk), dim3(256), 0, s, a, t);
    else hipLaunchKernelGGL(affine_brick_kernel<false>, dim3((unsigned)nblk), dim3(256), 0, s, a, t);
    RU_CHECK_LAUNCH("affine_brick_kernel");
    return RU_OK;
}
