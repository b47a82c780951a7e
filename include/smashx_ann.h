/* smashx_ann.h -- C ABI of libsmashx, the ANN regionalisation (Model.ann_optimize; smash/core/net.py, core/simulation/_ann_optimize.py)
 * ON THE DEVICE: the trainable state of the descriptor -> field network is a few thousand weights, so an epoch sends the packed
 * weights up and brings their gradient back -- no plane crosses PCIe.  The network is evaluated per active cell straight into the
 * sweep's cell vectors, the back-propagation and the weight-gradient sums run on the device after an adjoint sweep.  Arithmetic
 * contract (smash_amd/csrc/sx_ann.h): fp32 descriptors in, fp64 inside, fp32 fields out rounded once; no contracted product, one exp
 * shared by host and device, the weight-gradient sums in a stated order over the active cells in column-major position.  The
 * smashx_ann_host_* calls are that same network on the host (sx_annhost.h, no GPU needed) and give the same bits.
 * Part of the ABI of smashx.h, which includes this file after smashx_hyper.h: include either.  Conventions, error codes and
 * smashx_last_error() as in smashx.h; no struct is declared here, so SMASHX_ABI_VERSION and the struct-size guard (smashx_abi_sizes)
 * do not change with it.  The Python mirror is ANN_PROTOTYPES in smash_amd/_lib.py (tests/test_ann_cpu.py compares the two).
 *
 * A graph is nlayers layers, kind[l] one of the enum below, width[l] the OUTPUT width of layer l (an element-wise layer repeats its
 * input's width); the first layer is dense, the last width is ncv.  Packed weights: per dense layer W (fin, fout) row-major, then b
 * (fout), in layer order.  lower / upper (ncv) belong to the scale layer (NULL without one).
 *
 * One epoch:   smashx_upload (background fields) -> smashx_ann_upload -> smashx_sweep(adjoint = 1) -> smashx_ann_gradient,
 * with smashx_ann_set_descriptors, smashx_ann_set_net and smashx_set_options once before.  Refusals leave every buffer untouched:
 *   SMASHX_E_ARG          NULL arguments; a kind outside the enum; a field outside 0 .. 23 or named twice; nd < 1; a first layer that
 *                         is not dense; an element-wise width that differs from its input's; a last width that is not ncv
 *   SMASHX_E_STATE        no descriptors; no net; nd of the net and of the descriptors differ; no smashx_upload;
 *                         smashx_ann_gradient without an adjoint sweep behind a smashx_ann_upload; smashx_ann_gradient /
 *                         smashx_ann_fields after new descriptors or a new net
 *   SMASHX_E_UNSUPPORTED  a tiled plan (tile rectangle or owner_mask: whole-grid sums); softplus, softmax, dropout; on the device more
 *                         than 4 dense layers, a dense width > 64, ncv > 24, nd + the sum of the dense widths + the widest > 312;
 *                         a regulariser (njr > 0, from smashx_ann_upload / _gradient / _fields: the jreg term reads the planes of
 *                         smashx_upload, not the mapped ones)
 * denormalize_forward is not refused and has no effect here: the network's outputs are stored as the physical values the sweep reads.
 */
#ifndef SMASHX_ANN_H
#define SMASHX_ANN_H

#include "smashx.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { SMASHX_ANN_DENSE = 1, SMASHX_ANN_RELU = 2, SMASHX_ANN_LEAKY_RELU = 3, SMASHX_ANN_ELU = 4, SMASHX_ANN_SELU = 5,
       SMASHX_ANN_SIGMOID = 6, SMASHX_ANN_TANH = 7, SMASHX_ANN_SCALE = 8,
       /* known and refused */
       SMASHX_ANN_SOFTPLUS = 9, SMASHX_ANN_SOFTMAX = 10, SMASHX_ANN_DROPOUT = 11 };

/* The descriptors as the network reads them -- normalised by the caller --, (nrow, ncol, nd) column-major, gathered to plan-cell order
 * and kept in HBM until replaced; separate from the descriptors of smashx_hyper_set_descriptors.  Sending the contents the plan
 * already holds costs a comparison on the host and no transfer. */
int smashx_ann_set_descriptors(smashx_plan* plan, int nd, const float* descriptor);

/* The graph.  field[j] is the field (0 .. 15 = SMASHX_P_*, 16 .. 23 = SMASHX_GNP + SMASHX_S_*) output j is stored to, in the caller's
 * control-vector order; a field the structure does not read is legal (mapped, zero gradient).  Behind smashx_ann_set_descriptors, whose
 * nd is the net's input width (SMASHX_E_STATE before). */
int smashx_ann_set_net(smashx_plan* plan, int nlayers, const int* kind, const int* width, int ncv, const int* field,
                       const double* lower, const double* upper);

/* The network at every active cell, behind an ordinary smashx_upload of the background fields: the control fields' cell vectors and
 * planes are overwritten with its outputs, every other field stays. */
int smashx_ann_upload(smashx_plan* plan, const double* weights);

/* After an adjoint sweep: weights_b, packed like weights, is overwritten with the gradient of the cost (times the sweep's cost_b). */
int smashx_ann_gradient(smashx_plan* plan, double* weights_b);

/* The mapped control fields of the last smashx_ann_upload back on the host: planes are (nrow, ncol) column-major, the active cells
 * of the control fields are written, everything else is left as the caller had it; a NULL plane (or structure) is skipped. */
int smashx_ann_fields(smashx_plan* plan, smashx_parameters* params, smashx_states* states);

/* the last smashx_ann_upload / smashx_ann_gradient of the plan: info = {nd, packed weights, cells per span, LDS bytes per workgroup},
 * device_ms = {the map kernel, the adjoint's kernels over all spans} between HIP events on the plan's stream */
int smashx_ann_info(const smashx_plan* plan, int info[4], float device_ms[2]);

/* ---- the same network on the host (no plan, no GPU): the reference path of the tests and of ann_optimize(device_map = False) ---------- */
/* number of packed weights of the graph, or an error code (< 0) */
int smashx_ann_host_nweights(int nd, int nlayers, const int* kind, const int* width, int ncv);
/* y (n, ncv) row-major <- the network at the n rows of x (n, nd) row-major */
int smashx_ann_host_forward(int nd, int nlayers, const int* kind, const int* width, int ncv, const double* lower, const double* upper,
                            const double* weights, long n, const float* x, float* y);
/* weights_b <- the gradient given loss_grad (n, ncv) row-major, the rows in the order of the sums (sx_ann.h) */
int smashx_ann_host_gradient(int nd, int nlayers, const int* kind, const int* width, int ncv, const double* lower, const double* upper,
                             const double* weights, long n, const float* x, const float* loss_grad, double* weights_b);
/* y[i], dy[i] <- an activation (SMASHX_ANN_RELU .. SMASHX_ANN_TANH) and its derivative at x[i]; dy may be NULL */
int smashx_ann_host_activation(int kind, long n, const double* x, double* y, double* dy);
/* y[i] <- the contract's exp at x[i] */
int smashx_ann_host_exp(long n, const double* x, double* y);

#ifdef __cplusplus
}
#endif
#endif /* SMASHX_ANN_H */
