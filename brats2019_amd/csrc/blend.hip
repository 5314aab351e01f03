// blend.hip -- overlap-and-blend sliding-window inference: the predictions of overlapping tiles are summed with a window that falls off
// towards the tile's edge and divided by the summed window (nnU-Net's / MONAI's sliding window; the reference has only the centre paste
// of loader_helper.py:82-97, ru_tile_scatter).
//
//   blend_kernel<false>  : ru_blend_accumulate, S += w * p over the tiles [t0, t0 + T) of one forward
//   blend_kernel<true>   : ru_blend_finalize, out = S / Wn with Wn recomputed from the geometry (no second volume in HBM)
//
// The arithmetic is fixed so that a result can be compared with numpy exactly ("Blended sliding window"):
//   geometry  per axis a strictly rising list of tile starts; the tiles are their Cartesian product, tile index = (iz*ny + iy)*nx + ix
//   weight    w = fl32(fl32(gz[z] * gy[y]) * gx[x]) from the three float32 window profiles
//   sums      over the tiles that cover a voxel IN RISING TILE INDEX:  S <- fl32(S + fl32(w*p)),  Wn <- fl32(Wn + w), both from 0
//   result    fl32(S / Wn), a true division
// Contraction is switched off where these are formed.  Both kernels are GATHERS over the volume: a lane owns the four voxels x0 .. x0+3
// (x0 % 4 == 0) of one volume row and walks the tiles that cover them in index order, so overlapping tiles of one launch cannot race, no
// atomics are needed and the result depends neither on the launch geometry nor on how the tiles are split into launches.  The first
// touch of a voxel is decided from the geometry -- its smallest covering tile index is (first iz, first iy, first ix) -- and starts from
// 0 instead of reading acc: no memset, and no read of acc for the voxels a launch is the first to reach.
// HBM streams: 256-thread workgroups, 16-byte accesses (tile rows are 16-byte aligned, tw % 4 == 0: a quad at (x0 - start) % 4 == 0 lies
// wholly inside the tile; volume rows start at any dword, which the hardware takes), dword accesses for a tile whose start is not a
// multiple of 4.  Start lists and profiles are staged in LDS once per workgroup.
#include "ru_common.h"
#include "pw_helpers.hpp"

#include <limits.h>

namespace ru {
namespace {

typedef float blend_f4 __attribute__((ext_vector_type(4), aligned(4)));    // 4 floats at dword alignment: one global_load/store_dwordx4

constexpr int BLEND_MAX_STARTS = 128;          // tile starts per axis (the lists travel by value: 1.5 KB of kernel arguments)
constexpr size_t BLEND_MAX_LDS = 48 * 1024;

struct BlendGeom { int n[3], t[3], s[3][BLEND_MAX_STARTS]; };

// the tiles [lo, hi] of a strictly rising start list whose extent [s, s + t) meets [c0, c1]; the lists cover the volume, so lo <= hi
__device__ __forceinline__ void blend_cover(const int* __restrict__ s, int n, int t, int c0, int c1, int& lo, int& hi) {
    int a = 0, b = n - 1;                      // first tile that ends behind c0: s[i] + t > c0 is monotone in i
    while (a < b) {
        const int m = (a + b) >> 1;
        if (s[m] + t > c0) b = m; else a = m + 1;
    }
    lo = a;
    hi = a;
    while (hi + 1 < n && s[hi + 1] <= c1) ++hi;
}

// FINAL = false: acc[n][c][voxel] (+)= sum over the launch's tiles; FINAL = true: out = acc / Wn over all tiles (tiles, t0, T unused).
// blockIdx.y = n * C + c; blockIdx.x strides over the quads of the box b, whose x origin is rounded down to a multiple of 4.
template <bool FINAL>
__global__ __launch_bounds__(256) void blend_kernel(const float* __restrict__ tiles, const float* acc, float* out, const float* __restrict__ prof,
                                                    const BlendGeom g, int N, int C, int D, int H, int W, int t0, int T, Box3 b) {
#pragma clang fp contract(off)
    extern __shared__ int blend_lds[];
    const int nz = g.n[0], ny = g.n[1], nx = g.n[2], td = g.t[0], th = g.t[1], tw = g.t[2];
    int* sz = blend_lds;
    int* sy = sz + nz;
    int* sx = sy + ny;
    float* pz = reinterpret_cast<float*>(sx + nx);
    float* py = pz + td;
    float* px = py + th;
    for (int i = threadIdx.x; i < nz + ny + nx; i += 256) blend_lds[i] = i < nz ? g.s[0][i] : i < nz + ny ? g.s[1][i - nz] : g.s[2][i - nz - ny];
    for (int i = threadIdx.x; i < td + th + tw; i += 256) pz[i] = prof[i];
    __syncthreads();

    const int nc = blockIdx.y;                                         // n * C + c
    const size_t HW = (size_t)H * W, tile_vox = (size_t)td * th * tw;
    const float* ain = acc + (size_t)nc * D * HW;
    float* dst = out + (size_t)nc * D * HW;
    const int xq0 = b.lo[2] & ~3;
    const unsigned nq = (unsigned)(b.lo[2] + b.size[2] - xq0 + 3) >> 2, sby = (unsigned)b.size[1];
    const unsigned total = (unsigned)b.size[0] * sby * nq;
    for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < total; i += gridDim.x * 256u) {
        const unsigned r = i / nq, zq = r / sby;
        const int x0 = xq0 + (int)((i - r * nq) << 2), y = b.lo[1] + (int)(r - zq * sby), z = b.lo[0] + (int)zq;
        const int xe = x0 + 3 < W ? x0 + 3 : W - 1;
        const bool whole = x0 + 3 < W;                                 // the four voxels exist: 16-byte access to the volume row
        int zlo, zhi, ylo, yhi, xlo, xhi;
        blend_cover(sz, nz, td, z, z, zlo, zhi);
        blend_cover(sy, ny, th, y, y, ylo, yhi);
        blend_cover(sx, nx, tw, x0, xe, xlo, xhi);
        const size_t row = (size_t)z * HW + (size_t)y * W + x0;
        float S[4] = {0.f, 0.f, 0.f, 0.f};
        bool touched[4] = {false, false, false, false};
        if (!FINAL) {
            // a voxel some earlier launch reached (its smallest covering tile index lies before t0) continues from acc
            const int tfirst = (zlo * ny + ylo) * nx;
            bool prior[4] = {false, false, false, false};
            for (int ix = xhi; ix >= xlo; --ix) {
                const int lx = x0 - sx[ix];
#pragma unroll
                for (int j = 0; j < 4; ++j) if ((unsigned)(lx + j) < (unsigned)tw) prior[j] = tfirst + ix < t0;
            }
            if (prior[0] || prior[1] || prior[2] || prior[3]) {
                if (whole) {
                    const blend_f4 a = *reinterpret_cast<const blend_f4*>(ain + row);
                    S[0] = prior[0] ? a.x : 0.f; S[1] = prior[1] ? a.y : 0.f; S[2] = prior[2] ? a.z : 0.f; S[3] = prior[3] ? a.w : 0.f;
                } else {
                    for (int j = 0; x0 + j < W; ++j) if (prior[j]) S[j] = ain[row + j];
                }
            }
        }
        for (int iz = zlo; iz <= zhi; ++iz) {
            const int lz = z - sz[iz];
            const float wz = pz[lz];
            for (int iy = ylo; iy <= yhi; ++iy) {
                const int ly = y - sy[iy];
                const float wzy = wz * py[ly];
                for (int ix = xlo; ix <= xhi; ++ix) {
                    const int t = (iz * ny + iy) * nx + ix - t0;
                    if (!FINAL && (unsigned)t >= (unsigned)T) continue;
                    const int lx = x0 - sx[ix];
                    const bool quad = (lx & 3) == 0 && (unsigned)lx < (unsigned)tw && whole;
                    if (FINAL) {
#pragma unroll
                        for (int j = 0; j < 4; ++j) if ((unsigned)(lx + j) < (unsigned)tw) S[j] = S[j] + wzy * px[lx + j];
                    } else {
                        const float* src = tiles + ((size_t)t * N * C + nc) * tile_vox + ((size_t)lz * th + ly) * tw;
                        if (quad) {
                            const float4 p = *reinterpret_cast<const float4*>(src + lx);
                            const float pj[4] = {p.x, p.y, p.z, p.w};
#pragma unroll
                            for (int j = 0; j < 4; ++j) {
                                const float w = wzy * px[lx + j];
                                S[j] = S[j] + w * pj[j];
                                touched[j] = true;
                            }
                        } else {
#pragma unroll
                            for (int j = 0; j < 4; ++j) {
                                if ((unsigned)(lx + j) < (unsigned)tw && x0 + j < W) {
                                    const float w = wzy * px[lx + j];
                                    S[j] = S[j] + w * src[lx + j];
                                    touched[j] = true;
                                }
                            }
                        }
                    }
                }
            }
        }
        if (FINAL) {
            if (whole) {
                const blend_f4 a = *reinterpret_cast<const blend_f4*>(ain + row);
                blend_f4 o;
                o.x = a.x / S[0]; o.y = a.y / S[1]; o.z = a.z / S[2]; o.w = a.w / S[3];
                *reinterpret_cast<blend_f4*>(dst + row) = o;
            } else {
                for (int j = 0; x0 + j < W; ++j) dst[row + j] = ain[row + j] / S[j];
            }
        } else if (touched[0] && touched[1] && touched[2] && touched[3]) {
            blend_f4 o;
            o.x = S[0]; o.y = S[1]; o.z = S[2]; o.w = S[3];
            *reinterpret_cast<blend_f4*>(dst + row) = o;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) if (touched[j]) dst[row + j] = S[j];
        }
    }
}

// checks shared by the two entries; fills g and the LDS bytes of a launch
int blend_geometry(BlendGeom& g, size_t& lds, const int* const* starts, const int* counts, const int* tile, int D, int H, int W, const char* who) {
    const int dims[3] = {D, H, W};
    for (int a = 0; a < 3; ++a) {
        RU_REQUIRE(dims[a] > 0 && tile[a] > 0, "%s: volume and tile extents must be positive", who);
        RU_REQUIRE(starts[a] && counts[a] >= 1 && counts[a] <= BLEND_MAX_STARTS, "%s: 1 to %d tile starts per axis", who, BLEND_MAX_STARTS);
        g.n[a] = counts[a];
        g.t[a] = tile[a];
        for (int i = 0; i < counts[a]; ++i) {
            const int s = starts[a][i];
            RU_REQUIRE(i == 0 ? s == 0 : s > starts[a][i - 1], "%s: the tile starts of an axis begin at 0 and are strictly increasing", who);
            RU_REQUIRE(i == 0 || s <= starts[a][i - 1] + tile[a], "%s: the tiles leave a gap in the volume", who);
            RU_REQUIRE(s < dims[a], "%s: a tile starts behind the volume's end", who);
            g.s[a][i] = s;
        }
        RU_REQUIRE(starts[a][counts[a] - 1] + tile[a] >= dims[a], "%s: the tiles do not reach the volume's end", who);
    }
    RU_REQUIRE((tile[2] & 3) == 0, "%s: the tile width must be a multiple of 4", who);
    RU_REQUIRE((size_t)D * H * W < (size_t)INT_MAX && (size_t)tile[0] * tile[1] * tile[2] < (size_t)INT_MAX, "%s: volume too large for 32-bit voxel indices", who);
    RU_REQUIRE((size_t)counts[0] * counts[1] * counts[2] < (size_t)INT_MAX / 2, "%s: too many tiles", who);
    lds = ((size_t)counts[0] + counts[1] + counts[2] + tile[0] + tile[1] + tile[2]) * 4;
    RU_REQUIRE(lds <= BLEND_MAX_LDS, "%s: start lists and profiles exceed %zu bytes of LDS", who, BLEND_MAX_LDS);
    return RU_OK;
}

}  // namespace
}  // namespace ru

using namespace ru;

extern "C" int ru_blend_accumulate(const float* tiles, float* acc, const float* profiles, int N, int C, int D, int H, int W, int td, int th, int tw,
                                   const int* starts_z, int nz, const int* starts_y, int ny, const int* starts_x, int nx, int t0, int T, ru_stream_t stream) {
    RU_REQUIRE(tiles && acc && profiles, "ru_blend_accumulate: null argument");
    RU_REQUIRE(N > 0 && C > 0 && (size_t)N * C <= 65535, "ru_blend_accumulate: N and C must be positive, N * C at most 65535");
    BlendGeom g;
    size_t lds;
    const int* starts[3] = {starts_z, starts_y, starts_x};
    const int counts[3] = {nz, ny, nx}, tile[3] = {td, th, tw}, dims[3] = {D, H, W};
    int rc = blend_geometry(g, lds, starts, counts, tile, D, H, W, "ru_blend_accumulate");
    if (rc) return rc;
    RU_REQUIRE(t0 >= 0 && T >= 1 && (long long)t0 + T <= (long long)nz * ny * nx, "ru_blend_accumulate: the tile range [%d, %d + %d) lies outside the %d tiles", t0, t0, T,
               nz * ny * nx);
    // bounding box of the launch's tiles, clipped to the volume
    int ilo[3] = {INT_MAX, INT_MAX, INT_MAX}, ihi[3] = {-1, -1, -1};
    for (int t = t0; t < t0 + T; ++t) {
        const int idx[3] = {t / (ny * nx), (t / nx) % ny, t % nx};
        for (int a = 0; a < 3; ++a) { ilo[a] = idx[a] < ilo[a] ? idx[a] : ilo[a]; ihi[a] = idx[a] > ihi[a] ? idx[a] : ihi[a]; }
    }
    Box3 b;
    for (int a = 0; a < 3; ++a) {
        const int end = g.s[a][ihi[a]] + tile[a];
        b.lo[a] = g.s[a][ilo[a]];
        b.size[a] = (end < dims[a] ? end : dims[a]) - b.lo[a];
    }
    const size_t quads = (size_t)b.size[0] * b.size[1] * ((size_t)(b.lo[2] + b.size[2] - (b.lo[2] & ~3) + 3) / 4);
    hipLaunchKernelGGL(blend_kernel<false>, dim3(grid1d(quads, 256, 2048), (unsigned)(N * C)), dim3(256), lds, (hipStream_t)stream, tiles, acc, acc, profiles, g, N, C, D,
                       H, W, t0, T, b);
    RU_CHECK_LAUNCH("blend_kernel");
    return RU_OK;
}

extern "C" int ru_blend_finalize(const float* acc, float* out, const float* profiles, int N, int C, int D, int H, int W, int td, int th, int tw, const int* starts_z,
                                 int nz, const int* starts_y, int ny, const int* starts_x, int nx, ru_stream_t stream) {
    RU_REQUIRE(acc && out && profiles, "ru_blend_finalize: null argument");
    RU_REQUIRE(N > 0 && C > 0 && (size_t)N * C <= 65535, "ru_blend_finalize: N and C must be positive, N * C at most 65535");
    BlendGeom g;
    size_t lds;
    const int* starts[3] = {starts_z, starts_y, starts_x};
    const int counts[3] = {nz, ny, nx}, tile[3] = {td, th, tw};
    int rc = blend_geometry(g, lds, starts, counts, tile, D, H, W, "ru_blend_finalize");
    if (rc) return rc;
    Box3 b = {{0, 0, 0}, {D, H, W}};
    const size_t quads = (size_t)D * H * (((size_t)W + 3) / 4);
    hipLaunchKernelGGL(blend_kernel<true>, dim3(grid1d(quads, 256, 2048), (unsigned)(N * C)), dim3(256), lds, (hipStream_t)stream, (const float*)nullptr, acc, out,
                       profiles, g, N, C, D, H, W, 0, 0, b);
    RU_CHECK_LAUNCH("blend_kernel");
    return RU_OK;
}
