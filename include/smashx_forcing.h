/* smashx_forcing.h -- C ABI of libsmashx, statistics of the forcing: what the reference's Model.__init__ derives from the forcing for
 * the signatures and the event segmentation (smash/core/_build_model.py:212-231), computed on the forcing a plan already holds in HBM.
 * Part of the ABI of smashx.h, which includes this file: include either.  Conventions, error codes and smashx_last_error() as in
 * smashx.h; no struct and no constant is declared here, so SMASHX_ABI_VERSION and the struct-size guard (smashx_abi_sizes) do not
 * change with it.  The Python mirror is FORCING_PROTOTYPES in smash_amd/_lib.py (tests/test_mean_forcing_cpu.py compares the two as
 * tests/test_abi_header_cpu.py compares smashx.h with PROTOTYPES).
 */
#ifndef SMASHX_FORCING_H
#define SMASHX_FORCING_H

#include "smashx.h"

#ifdef __cplusplus
extern "C" {
#endif

/* mw_forcing_statistic::compute_mean_forcing (mw_forcing_statistic.f90:18-75) on the plan's resident forcing.
 * mean_prcp / mean_pet: (ng, nt) column-major like qsim, fully overwritten; either may be NULL (that field is then not read).
 * Per gauge and step: the fp32 sum, in column-major cell order, of the values >= 0 over the gauge's upstream cells (mw_mask.f90:11-54),
 * divided by their count; a step without such a value gives NaN (0 / 0), as in the reference.
 * SMASHX_E_STATE without complete forcing; SMASHX_E_ARG for a NULL plan or two NULL outputs; SMASHX_E_UNSUPPORTED for a tiled plan
 * (a sequential sum does not split across parts) and for a gauge whose upstream cells include an inactive one (the plan holds no
 * forcing there).  ng == 0: SMASHX_OK, nothing written. */
int smashx_mean_forcing(smashx_plan* plan, float* mean_prcp, float* mean_pet);

#ifdef __cplusplus
}
#endif
#endif /* SMASHX_FORCING_H */
