"""smash_amd -- MI355X-native forward + adjoint solver for smash's distributed rainfall-runoff path.

The package is a thin host-side mirror of the reference's ``mw_forward`` boundary over libsmashx
(HIP kernels behind the C ABI of include/smashx.h).  Importing it does not need a GPU; calling the
solver does, and fails loudly without one.
"""
from .solver import (Solver, adjust_interception_store, check_adjust_interception, check_mean_forcing, check_prcp_indices, compute_mean_forcing, compute_multiple_run, compute_prcp_indices, day_index, forward, forward_b, forward_d, gradient_test, hyper_forward, hyper_forward_b, hyper_forward_d,  # noqa: F401
                     check_ann_control_vector, check_ann_descriptors, check_ann_weights, check_hyper_descriptors, check_hyper_matrices, check_signature_inputs, invalidate_forcing, multiple_run, prcp_indices, scalar_product_test, signature_refusal, uniform_costs)
from .types import (Hyper_ParametersDT, Hyper_StatesDT, Input_DataDT, MeshDT, Optimize_SetupDT, OutputDT,  # noqa: F401
                    ParametersDT, SetupDT, StatesDT)
from ._lib import SmashxError  # noqa: F401
from .net import Net  # noqa: F401
from .optimize import ann_optimize, optimize_hyper_lbfgsb, optimize_lbfgsb, optimize_sbs  # noqa: F401
