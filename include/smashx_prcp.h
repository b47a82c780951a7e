/* smashx_prcp.h -- C ABI of libsmashx, precipitation indices of the forcing: what the reference's Model.prcp_indices() derives from the
 * rain and the flow distances (smash/core/prcp_indices.py:111-124), computed on the forcing a plan already holds in HBM.
 * Part of the ABI of smashx.h, which includes this file after smashx_forcing.h: include either.  Conventions, error codes and
 * smashx_last_error() as in smashx.h; no struct and no constant is declared here, so SMASHX_ABI_VERSION and the struct-size guard
 * (smashx_abi_sizes) do not change with it.  The Python mirror is PRCP_PROTOTYPES in smash_amd/_lib.py
 * (tests/test_prcp_indices_cpu.py compares the two as tests/test_abi_header_cpu.py compares smashx.h with PROTOTYPES).
 */
#ifndef SMASHX_PRCP_H
#define SMASHX_PRCP_H

#include "smashx.h"

#ifdef __cplusplus
extern "C" {
#endif

/* mw_forcing_statistic::compute_prcp_indices (mw_forcing_statistic.f90:77-220) on the plan's resident rain.
 * flwdst: (nrow, ncol) column-major, mesh%flwdst, read over the whole grid.  prcp_indices: (4, ng, nt) column-major, (std, d1, d2, vg)
 * per gauge and step, INOUT: a step whose rain sum over the gauge's upstream cells is not > 0 keeps its four entries as passed.
 * Bit for bit the reference: sequential fp32 sums in column-major cell order, IEEE divisions and square root.  As there, the first
 * point of the width function reads the rain of the cell (gauge_row, gauge_row) -- the column is indexed with the gauge's row
 * (mw_forcing_statistic.f90:181) -- and the ten distance bins are taken over the whole grid, not over the catchment.
 * SMASHX_E_STATE without complete forcing; SMASHX_E_ARG for a NULL argument; SMASHX_E_UNSUPPORTED for a tiled plan, for a catchment of
 * fewer than 2 cells (the reference's quantile reads two) and for any cell the reference would read whose forcing the plan does not
 * hold: an inactive cell inside a catchment or a distance bin, a (gauge_row, gauge_row) cell that is inactive or outside the grid.
 * ng == 0: SMASHX_OK, nothing written. */
int smashx_prcp_indices(smashx_plan* plan, const float* flwdst, float* prcp_indices);

#ifdef __cplusplus
}
#endif
#endif /* SMASHX_PRCP_H */
