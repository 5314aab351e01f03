// The surface -> distance transform -> histogram -> order statistic sequence of surface.hip on pairs of masks that are already
// bit-packed (lesion.hip: one pair (M_i, L_i) per ground-truth lesion).  Item t owns four bit planes of D * H * cdiv(W, 64) 64-bit
// words at sf_packed_bits(ws) + t * 4 * words: the caller writes plane 0 (P) and plane 1 (G), bits >= W of a row zero; planes 2 and
// 3 take the surfaces.  counts [items][RU_SURFACE_COUNTS]: the caller sets {|P|, |G|, TP, 0, 0, 0}; values [items][4] as
// ru_surface_metrics writes them.  2 * items <= 65535 (the launch grids).
#pragma once
#include "ru_common.h"

namespace ru {

size_t sf_packed_workspace_bytes(int items, int D, int H, int W);
unsigned long long* sf_packed_bits(void* ws);
int sf_packed_run(int items, int D, int H, int W, void* ws, unsigned long long* counts, double empty_value, double* values, hipStream_t st);
// the same passes and the same `values`, then ru_surface_distances' finalize: extras [items][T + 2] = {NSD_0..NSD_T-1, ASSD, HD} for the
// T <= RU_SURFACE_MAX_TOL host bin limits `tol_bins` (passed on by value: no upload).  Same workspace.
int sf_packed_run_extras(int items, int D, int H, int W, void* ws, unsigned long long* counts, double empty_value, double* values,
                         const unsigned* tol_bins, int T, double* extras, hipStream_t st);

}  // namespace ru
