/* smashx_signature.h -- C ABI of libsmashx, inputs of the signature-based criteria of the cost: SMASHX_CRC, SMASHX_CFP2 / 10 / 50 / 90,
 * SMASHX_EPF, SMASHX_ELT, SMASHX_ERC in smashx_options.jobs_fun (mwd_cost.f90:125-129 -> signature, :772-970; their adjoint and tangent
 * SIGNATURE_B / SIGNATURE_D, forward_db.f90:4501-4926).
 * Part of the ABI of smashx.h, which includes this file after smashx_prcp.h: include either.  Conventions, error codes and
 * smashx_last_error() as in smashx.h; no struct and no constant is declared here, so SMASHX_ABI_VERSION and the struct-size guard
 * (smashx_abi_sizes) do not change with it.  The Python mirror is SIGNATURE_PROTOTYPES in smash_amd/_lib.py
 * (tests/test_signature_cost_cpu.py compares the two as tests/test_abi_header_cpu.py compares smashx.h with PROTOTYPES).
 */
#ifndef SMASHX_SIGNATURE_H
#define SMASHX_SIGNATURE_H

#include "smashx.h"

#ifdef __cplusplus
extern "C" {
#endif

/* What compute_jobs hands to signature beside the discharges (mwd_cost.f90:82, 127-129):
 *   mean_prcp   (ng, nt) column-major, input_data%mean_prcp as smashx_mean_forcing writes it;
 *   mask_event  (ng, nt) column-major int, setup%optimize%mask_event: 0 outside events, 1..n inside (the reference's Python event
 *               segmentation fills it; the segmentation is a caller's business).  May be NULL when no E* criterion will be asked for.
 * Both are copied; call again after either changed, then smashx_set_options again (a sweep in between returns SMASHX_E_STATE, as it
 * does when qobs changed under signature criteria): the options decide the refusals below and build the criteria's tables.
 * SMASHX_E_ARG: NULL plan or mean_prcp, a mask entry outside 0..nt.  SMASHX_E_UNSUPPORTED: a tiled plan.  ng == 0: SMASHX_OK.
 *
 * smashx_set_options then refuses with SMASHX_E_UNSUPPORTED where the reference would read a num / den it never assigned -- which
 * depends on qobs, mean_prcp and mask_event only, never on the simulated discharge -- for a gauge with wgauge != 0 and any qobs >= 0
 * from optimize_start_step on:
 *   SMASHX_CRC   when the sum of mean_prcp over the steps with qobs >= 0 and mean_prcp >= 0 is not > 0 (the -99 prefill is such a case);
 *   SMASHX_ERC   when that holds for an event and no earlier event of the gauge assigned the ratio;
 * and likewise a signature criterion without these inputs, an E* criterion without mask_event, a tiled plan.  smashx_multiple_run
 * refuses options that hold a signature criterion.  The hyper sweeps are smashx_forward / _b / _d behind host maps and take the
 * criteria as those do.  At most 8 criteria at once, as before. */
int smashx_set_signature_inputs(smashx_plan* plan, const float* mean_prcp, const int* mask_event);

/* compute_jobs, COMPUTE_JOBS_B and COMPUTE_JOBS_D (mwd_cost.f90:37-156, forward_db.f90:2463-2715) on a discharge the CALLER prescribes
 * instead of the one a sweep left, with the plan's qobs, options and signature inputs: the cost kernels alone, which is how
 * tests/test_gpu_signature_cost.py feeds them hand-made series.  qsim (ng, nt) column-major; *jobs = the criteria's cost; qsim_b, when
 * not NULL, (ng, nt) = output_b%qsim for the seed jobs_b; qsim_d, when not NULL, (ng, nt) the direction and *jobs_d its tangent.
 * The gauge discharges and the cost the last sweep left on the device are put aside and put back, so a later smashx_download returns
 * what it would have returned; the sweep's timing marks (smashx_get_timing) are reset.
 * SMASHX_E_ARG: NULL plan / qsim / jobs, qsim_d without jobs_d, two gauges on one cell.  SMASHX_E_STATE: qobs not set, or as a sweep.
 * SMASHX_E_UNSUPPORTED: a tiled plan. */
int smashx_jobs_of_qsim(smashx_plan* plan, const float* qsim, float jobs_b, float* jobs, float* qsim_b, const float* qsim_d, float* jobs_d);

#ifdef __cplusplus
}
#endif
#endif /* SMASHX_SIGNATURE_H */
