// Binary dilation of bit-packed masks (mask_bits.hpp) by the 18-neighbour structure -- the voxel, its 6 face and its 12 edge neighbours,
// scipy.ndimage.generate_binary_structure(3, 2) -- shared by lesion.hip (ru_lesion_metrics) and lesion_loss.hip (ru_lesion_loss_forward), so
// that the loss groups the target into the lesions the scorer groups it into.  Planes are laid out bits[nk][4][words]; outside the grid is
// background.  Everything here has internal linkage: each translation unit that includes the header gets its own copy of the kernel.
#pragma once
#include "ru_common.h"
#include "mask_bits.hpp"

namespace ru {
namespace {

__device__ __forceinline__ u64 ls_word(const u64* __restrict__ b, const MaskGeom& s, int d, int h, int c) {
    return (d < 0 || d >= s.D || h < 0 || h >= s.H || c < 0 || c >= s.WW) ? 0ull : b[((size_t)d * s.H + h) * s.WW + c];
}
// word c of row (d, h) or-ed with its shifts by one voxel along x, the carries taken from the neighbouring words
__device__ __forceinline__ u64 ls_row3(const u64* __restrict__ b, const MaskGeom& s, int d, int h, int c) {
    if (d < 0 || d >= s.D || h < 0 || h >= s.H) return 0ull;
    const u64 m = ls_word(b, s, d, h, c), prev = ls_word(b, s, d, h, c - 1), next = ls_word(b, s, d, h, c + 1);
    return m | (m << 1) | (prev >> 63) | (m >> 1) | (next << 63);
}

// grid (blocks, N*K): one iteration, plane `src` -> plane `dst` of every (n, k).  One thread per word: the rows (dz, dy) = (0, 0) and the
// four face rows contribute themselves and their x +- 1 shifts (carries cross word boundaries), the four diagonal rows themselves only.
__global__ __launch_bounds__(256) void ls_dilate_kernel(MaskGeom s, u64* __restrict__ bits, int src, int dst) {
    const int nk = blockIdx.y;
    const u64* __restrict__ a = bits + ((size_t)nk * 4 + src) * s.words;
    u64* __restrict__ o = bits + ((size_t)nk * 4 + dst) * s.words;
    const u64 last = (s.W & 63) ? (1ull << (s.W & 63)) - 1 : ~0ull;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < s.words; i += (size_t)gridDim.x * 256) {
        const int c = (int)(i % s.WW);
        const size_t r = i / s.WW;
        const int h = (int)(r % s.H), d = (int)(r / s.H);
        u64 m = ls_row3(a, s, d, h, c) | ls_row3(a, s, d - 1, h, c) | ls_row3(a, s, d + 1, h, c) | ls_row3(a, s, d, h - 1, c) | ls_row3(a, s, d, h + 1, c);
        m |= ls_word(a, s, d - 1, h - 1, c) | ls_word(a, s, d - 1, h + 1, c) | ls_word(a, s, d + 1, h - 1, c) | ls_word(a, s, d + 1, h + 1, c);
        o[i] = c == s.WW - 1 ? m & last : m;
    }
}

}  // namespace
}  // namespace ru
