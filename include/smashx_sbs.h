/* smashx_sbs.h -- C ABI of libsmashx, the uniform ("step by step") calibration: the optimiser of mw_optimize::optimize_sbs
 * (smash/solver/optimize/mw_optimize.f90:53-294) in ask / tell form, and the cost of a batch of spatially uniform candidates on a
 * catchment-resident kernel.  Part of the ABI of smashx.h, which includes this file after smashx_ann.h: include either.  Conventions,
 * error codes and smashx_last_error() as in smashx.h; no struct with a layout and no constant is declared here, so SMASHX_ABI_VERSION
 * and the struct-size guard (smashx_abi_sizes) do not change with it.  The Python mirror is SBS_PROTOTYPES in smash_amd/_lib.py
 * (tests/test_sbs_cpu.py compares the two as tests/test_abi_header_cpu.py compares smashx.h with PROTOTYPES).
 */
#ifndef SMASHX_SBS_H
#define SMASHX_SBS_H

#include "smashx.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- the optimiser (smash_amd/csrc/sx_sbs.cpp: host C++, no GPU): the loop of optimize_sbs restated statement by statement in fp32
 * with glibc's float functions, turned inside out so that the candidates of one stage leave as one batch.  A batch is legal because
 * every candidate of an iteration is built from the current point alone; telling the costs in order with the strict `<` is the
 * reference's sequential choice (first wins on ties, a NaN never wins).
 * n: size of the control vector; lower / upper / x0: n values each (the bounds pick the transformation per component: asinh when
 * lower < 0, logit when 0 <= lower and upper <= 1, log otherwise); cost0: the cost at x0 (the reference's first forward, nfg = 1);
 * maxiter: the reference's setup%optimize%maxiter (the loop runs maxiter * n iterations at the most).
 * Protocol: loop { ask(opt, y, &m); m == 0: finished; evaluate the m columns of y; tell(opt, cost) }.  y: room for (n, 2 n) floats,
 * column-major, untransformed values: column c is the whole control vector of candidate c.  A stage is the up to 2 n coordinate
 * candidates of an iteration or, once iter > 4 n, the one line-search candidate that follows them.  Skipped candidates are neither
 * asked nor counted.  After m == 0 the caller evaluates the model at smashx_sbs_x once more, as the reference does when it stops by
 * one of its two rules (not when maxiter * n == 0: the loop never runs then).
 * SMASHX_E_ARG: a NULL argument, n < 1, maxiter < 0, lower > upper; SMASHX_E_STATE: tell without a batch asked, ask with one open. */
typedef struct smashx_sbs smashx_sbs;
int smashx_sbs_create(int n, const float* lower, const float* upper, const float* x0, float cost0, int maxiter, smashx_sbs** out);
int smashx_sbs_ask(smashx_sbs* opt, float* y /* (n, m) column-major */, int* m);
int smashx_sbs_tell(smashx_sbs* opt, const float* cost /* (m) */);
int smashx_sbs_x(const smashx_sbs* opt, float* x /* (n): the current point, untransformed */);
float smashx_sbs_gx(const smashx_sbs* opt);          /* the cost at the current point */
float smashx_sbs_ddx(const smashx_sbs* opt);         /* the step in the transformed space */
int smashx_sbs_iter(const smashx_sbs* opt);          /* iterations of the reference's loop completed (its iterate lines print iter / n) */
int smashx_sbs_nfg(const smashx_sbs* opt);           /* evaluations counted as the reference counts them: cost0 and every told cost */
const char* smashx_sbs_message(const smashx_sbs* opt);   /* "" while running, then the reference's CONVERGENCE / STOP line */
int smashx_sbs_destroy(smashx_sbs* opt);

/* ---- the cost of nsamples spatially uniform candidates, one workgroup per candidate (smash_amd/csrc/sx_resident.h): the contract of
 * smashx_multiple_run without res_qsim -- same arguments, same checks, same refusals (denormalize_forward, wjreg with a regulariser,
 * a tiled plan, signature criteria), the plan's own device state untouched, res_cost bit for bit what nsamples calls of
 * smashx_forward return as cost.  The whole catchment of a candidate is resident in one workgroup, one thread per active cell, and
 * one launch marches the whole period; the discharge handed downstream stays in LDS.
 * SMASHX_E_UNSUPPORTED in addition: more than 1024 active cells (one cell per thread), delay lines that do not fit the LDS a workgroup
 * may claim; res_cost is untouched by any refusal. */
int smashx_uniform_costs(smashx_plan* plan, const smashx_parameters* params, const smashx_states* states, int nfields,
                         const int* ind_parameters_states, const float* sample /* (nfields, nsamples) column-major */, int nsamples,
                         float* res_cost /* (nsamples) */);
/* the last smashx_uniform_costs of the plan: info = {active cells, levels of the forest, threads per workgroup, LDS bytes per
 * workgroup (delay lines + the exact-libm build's tables)}; device_ms = time between the first and the last operation of the call on
 * the plan's stream (HIP events) */
int smashx_uniform_costs_info(const smashx_plan* plan, int info[4], float* device_ms);

#ifdef __cplusplus
}
#endif
#endif /* SMASHX_SBS_H */
