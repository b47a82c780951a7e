/* smashx_setup.h -- C ABI of libsmashx, model set-up: what the reference's Model.__init__ derives from the forcing before the first
 * forward run (smash/core/_build_model.py:233-257), computed on the forcing a plan already holds in HBM.  Part of the ABI of
 * smashx.h, which includes this file: include either.  Conventions, error codes and smashx_last_error() as in smashx.h; no struct is
 * declared here, so SMASHX_ABI_VERSION and the struct-size guard (smashx_abi_sizes) do not change with it.  The Python mirror is
 * SETUP_PROTOTYPES in smash_amd/_lib.py (tests/test_interception_cpu.py compares the two as tests/test_abi_header_cpu.py compares
 * smashx.h with PROTOTYPES).
 */
#ifndef SMASHX_SETUP_H
#define SMASHX_SETUP_H

#include "smashx.h"

#ifdef __cplusplus
extern "C" {
#endif

/* mw_interception_store::adjust_interception_store (mw_interception_store.f90:19-160) on the plan's resident forcing.
 * day_index[nt]: 1-based day number of every step, non-decreasing, steps of +0/+1 (what _build_model.py:238-248 builds).
 * ci (nrow,ncol) column-major, inout: active cells the plan owns are overwritten, every other element keeps its value.
 * SMASHX_E_STATE without complete forcing; SMASHX_E_ARG for NULL pointers or a day_index that is not of that form or does not end at
 * nday; SMASHX_E_UNSUPPORTED for a structure without an interception store (gr-a, gr-d, vic-a).  A tiled plan fills its own cells. */
int smashx_adjust_interception(smashx_plan* plan, int nday, const int* day_index, float* ci);

#ifdef __cplusplus
}
#endif
#endif /* SMASHX_SETUP_H */
