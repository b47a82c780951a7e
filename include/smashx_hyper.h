/* smashx_hyper.h -- C ABI of libsmashx, the hyper-linear / hyper-polynomial maps of the regionalisation ON THE DEVICE: the control
 * vector of mw_optimize::optimize_hyper_lbfgsb (mw_optimize.f90:779-958) is at most 24 x (1 + 2 nd) coefficients, so an evaluation
 * sends the two hyper matrices up and brings the two gradient matrices back -- no plane crosses PCIe.  The host maps of smashx.h
 * ("hyper mappings", sx_hyper.cpp) stay as they are; these calls compute the same numbers bit for bit: the same fp32 operations in the
 * same order, expf / powf / logf as glibc evaluates them (sx_libm.h) in either build, the adjoint's sums sequential over the active
 * cells with the column index outer and the row index inner (kernels: smash_amd/csrc/sx_hypermap.h).
 * Part of the ABI of smashx.h, which includes this file after smashx_signature.h: include either.  Conventions, error codes and
 * smashx_last_error() as in smashx.h; no struct and no constant is declared here, so SMASHX_ABI_VERSION and the struct-size guard
 * (smashx_abi_sizes) do not change with it.  The Python mirror is HYPER_DEVICE_PROTOTYPES in smash_amd/_lib.py
 * (tests/test_hyper_device_cpu.py compares the two as tests/test_abi_header_cpu.py compares smashx.h with PROTOTYPES).
 *
 * One evaluation of base_hyper_forward_b:   smashx_hyper_upload -> smashx_sweep(adjoint = 1) -> smashx_hyper_gradient,
 * with smashx_hyper_set_descriptors and smashx_set_options once before.  Refusals are argument checks that leave every buffer
 * untouched:
 *   SMASHX_E_ARG          NULL plan or matrix; mapping other than SMASHX_HYPER_LINEAR / _POLYNOMIAL; nd < 0
 *   SMASHX_E_STATE        no descriptors set; no options set; smashx_hyper_gradient without an adjoint sweep behind a smashx_hyper_upload;
 *                         smashx_hyper_fields before a smashx_hyper_upload
 *   SMASHX_E_UNSUPPORTED  a tiled plan (tile rectangle or owner_mask, of one part too: an ordered whole-grid sum does not split across
 *                         parts); denormalize_forward; a regulariser (njr > 0: hyper_compute_cost knows neither)
 */
#ifndef SMASHX_HYPER_H
#define SMASHX_HYPER_H

#include "smashx.h"

#ifdef __cplusplus
extern "C" {
#endif

/* input_data%descriptor (nrow, ncol, nd) column-major, gathered to plan-cell order and kept in HBM with the mapping (setup%optimize%
 * mapping) until replaced.  Sending the contents the plan already holds costs a comparison on the host and no transfer.  nd = 0 is
 * legal (every field is a constant; descriptor is not read); descriptor = NULL with nd > 0 drops what the plan holds. */
int smashx_hyper_set_descriptors(smashx_plan* plan, int mapping, int nd, const float* descriptor);

/* hyper_parameters_to_parameters + hyper_states_to_states on the device, in place of smashx_upload in front of smashx_sweep: every
 * field the structure reads is mapped from its column of hyper_parameters (nhyper, 16) / hyper_states (nhyper, 8) -- column-major,
 * nhyper = 1 + nd (linear) or 1 + 2 nd (polynomial), bounds from smashx_set_options -- into its cell vectors and its plane. */
int smashx_hyper_upload(smashx_plan* plan, const float* hyper_parameters, const float* hyper_states);

/* HYPER_PARAMETERS_TO_PARAMETERS_B + HYPER_STATES_TO_STATES_B after an adjoint sweep: hyper_parameters_b (nhyper, 16) and
 * hyper_states_b (nhyper, 8) are overwritten with the gradient of the cost w.r.t. the coefficients (times the sweep's cost_b); the
 * columns of fields the structure does not read are zero. */
int smashx_hyper_gradient(smashx_plan* plan, float* hyper_parameters_b, float* hyper_states_b);

/* The mapped fields of the last smashx_hyper_upload back on the host: all 16 / 8 of them, also those the structure does not read.
 * Planes are (nrow, ncol) column-major; the active cells are written, every other cell is left as the caller had it; a NULL plane (or
 * structure) is skipped. */
int smashx_hyper_fields(smashx_plan* plan, smashx_parameters* params, smashx_states* states);

/* the last smashx_hyper_upload / smashx_hyper_gradient of the plan: info = {nd, nhyper, chains of the adjoint, cells per span},
 * device_ms = {the map kernel, the adjoint's kernels over all spans} between HIP events on the plan's stream */
int smashx_hyper_info(const smashx_plan* plan, int info[4], float device_ms[2]);

#ifdef __cplusplus
}
#endif
#endif /* SMASHX_HYPER_H */
