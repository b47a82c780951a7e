"""ctypes view of include/smashx.h, declared once: the header's constants, one class per struct (STRUCTS), one prototype per function
(PROTOTYPES; SETUP_PROTOTYPES for include/smashx_setup.h, FORCING_PROTOTYPES for include/smashx_forcing.h, PRCP_PROTOTYPES for include/smashx_prcp.h, SIGNATURE_PROTOTYPES for include/smashx_signature.h HYPER_DEVICE_PROTOTYPES for include/smashx_hyper.h, ANN_PROTOTYPES for include/smashx_ann.h and SBS_PROTOTYPES for include/smashx_sbs.h, which smashx.h includes).  tests/test_abi_header_cpu.py compares all three with the header's text; adding an entry point is one line in
PROTOTYPES.  Loading fails loudly when libsmashx.so is missing: there is no Python / CPU implementation of the solver behind this
module."""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# SMASHX_EXACT_LIBM=1 selects the exact-libm build (glibc's float functions restated, IEEE divisions: csrc/sx_libm.h) -- the
# slower library that reproduces the reference bit for bit; SMASHX_LIB overrides the path for A/B experiments.
EXACT = os.environ.get("SMASHX_EXACT_LIBM", "0") not in ("", "0")
LIB_PATH = os.environ.get("SMASHX_LIB", os.path.join(_HERE, "libsmashx_exact.so" if EXACT else "libsmashx.so"))

# ---- the header's numeric constants, each stated once; tests/test_abi_header_cpu.py compares every one with include/smashx.h ----
ABI_VERSION = 9
GNP, GNS = 16, 8
E_OK, E_ARG, E_UNSUPPORTED, E_HIP, E_NODEVICE, E_MESH, E_STATE = 0, -1, -2, -3, -4, -5, -6
STRUCTURES = {"gr-a": 1, "gr-b": 2, "gr-c": 3, "gr-d": 4, "vic-a": 5}                       # SMASHX_GR_A ...
JOBS_FUN = {"nse": 1, "kge": 2, "kge2": 3, "se": 4, "rmse": 5, "logarithmic": 6,              # SMASHX_NSE ...
            "Crc": 7, "Cfp2": 8, "Cfp10": 9, "Cfp50": 10, "Cfp90": 11, "Epf": 12, "Elt": 13, "Erc": 14}   # SMASHX_CRC ... (the signatures)
SIGNATURE_FUN = ("Crc", "Cfp2", "Cfp10", "Cfp50", "Cfp90", "Epf", "Elt", "Erc")                 # read mean_prcp (and, E*, mask_event)
JREG_FUN = {"prior": 1, "smoothing": 2, "hard_smoothing": 3}                                  # SMASHX_PRIOR ...
HYPER = {"hyper-linear": 1, "hyper-polynomial": 2}                                            # SMASHX_HYPER_LINEAR ...
LBFGSB_START, LBFGSB_FG, LBFGSB_NEW_X, LBFGSB_CONVERGED, LBFGSB_ABNORMAL = range(5)
COMM_ID_BYTES = 128
# SMASHX_FN_*: the ids of smashx_selftest_eval
FN = {k: i for i, k in enumerate("TANH TANH_BRANCHY EXPM1 EXP LOG POW POWB POW_M4 POW_M4_M5 POW_M025 POW_M025_M125 POW_3P5 POW_3P5_2P5 "
                                 "DIV DIV4 FDIV DIV_FAST".split())}
FN_COUNT = len(FN)

HALO_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int)
REDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_float), C.c_int)


class Config(C.Structure):
    _fields_ = [("structure", C.c_int), ("nrow", C.c_int), ("ncol", C.c_int), ("nt", C.c_int), ("ng", C.c_int),
                ("dt", C.c_float), ("dx", C.c_float), ("chunk_steps", C.c_int), ("pipe_steps", C.c_int), ("group_size", C.c_int),
                ("device", C.c_int), ("tile", C.c_int * 4)]


class Mesh(C.Structure):
    _fields_ = [("flwdir", C.c_void_p), ("flwacc", C.c_void_p), ("active_cell", C.c_void_p), ("path", C.c_void_p),
                ("gauge_pos", C.c_void_p), ("area", C.c_void_p), ("owner_mask", C.c_void_p)]


class Options(C.Structure):
    _fields_ = [("denormalize_forward", C.c_int), ("optimize_start_step", C.c_int), ("njf", C.c_int),
                ("jobs_fun", C.c_int * 8), ("wjobs_fun", C.c_float * 8), ("njr", C.c_int), ("jreg_fun", C.c_int * 4),
                ("wjreg_fun", C.c_float * 4), ("wjreg", C.c_float), ("optim_parameters", C.c_int * GNP),
                ("optim_states", C.c_int * GNS), ("lb_parameters", C.c_float * GNP), ("ub_parameters", C.c_float * GNP),
                ("lb_states", C.c_float * GNS), ("ub_states", C.c_float * GNS), ("wgauge", C.c_void_p)]


class ForcingLayout(C.Structure):
    _fields_ = [("compact", C.c_int), ("prcp_factor", C.c_float), ("pet_ratio", C.c_float * 24), ("pet_hour0", C.c_int)]


class HyperMap(C.Structure):
    _fields_ = [("mapping", C.c_int), ("nrow", C.c_int), ("ncol", C.c_int), ("nd", C.c_int), ("nfields", C.c_int),
                ("descriptor", C.c_void_p), ("lb", C.c_void_p), ("ub", C.c_void_p)]


class Parameters(C.Structure):
    _fields_ = [("f", C.c_void_p * GNP)]


class States(C.Structure):
    _fields_ = [("f", C.c_void_p * GNS)]


class Costs(C.Structure):
    _fields_ = [("cost", C.c_float), ("cost_jobs", C.c_float), ("cost_jreg", C.c_float)]


class Timing(C.Structure):
    _fields_ = [("sweep_ms", C.c_float), ("vert_fwd_ms", C.c_float), ("route_fwd_ms", C.c_float), ("cost_ms", C.c_float),
                ("route_adj_ms", C.c_float), ("vert_adj_ms", C.c_float), ("vert_fwd_launches", C.c_int),
                ("route_fwd_launches", C.c_int), ("route_adj_launches", C.c_int), ("vert_adj_launches", C.c_int),
                ("n_chunks", C.c_int), ("chunk_steps", C.c_int), ("pipe_steps", C.c_int), ("n_rounds", C.c_int), ("n_groups", C.c_int),
                ("device_bytes", C.c_double), ("cellsteps", C.c_double * 4),
                ("route_fwd_chained_ms", C.c_float), ("route_adj_chained_ms", C.c_float),
                ("route_fwd_chained_launches", C.c_int), ("route_adj_chained_launches", C.c_int), ("max_stage", C.c_int),
                ("n_chained_groups", C.c_int), ("chain_staged", C.c_int)]


# the ctypes class of every struct the header defines, by its C name
STRUCTS = {"smashx_config": Config, "smashx_mesh": Mesh, "smashx_options": Options, "smashx_forcing_layout": ForcingLayout,
           "smashx_hyper_map": HyperMap, "smashx_parameters": Parameters, "smashx_states": States, "smashx_costs": Costs,
           "smashx_timing": Timing}

# ---- every function of include/smashx.h: name -> (restype, argtypes), in the header's order.  Scalars as the header has them; ptr for
# data pointers and opaque handles (it takes None, an address as int, byref(...), a ctypes array, a POINTER(...) or c_void_p instance);
# struct parameters typed, so that byref() of another struct is refused.  tests/test_abi_header_cpu.py reads the header and compares.
_int, _long, _llong, _uint, _float, _double, _str, ptr = C.c_int, C.c_long, C.c_longlong, C.c_uint, C.c_float, C.c_double, C.c_char_p, C.c_void_p
_out = C.POINTER(ptr)                            # smashx_plan** / smashx_lbfgsb** / void**: where a new handle is stored
_cfg, _mesh, _opt, _lay, _map = (C.POINTER(t) for t in (Config, Mesh, Options, ForcingLayout, HyperMap))
_par, _sta, _cst, _tim = (C.POINTER(t) for t in (Parameters, States, Costs, Timing))
PROTOTYPES = {
    "smashx_last_error": (_str, []),
    "smashx_device_count": (_int, []),
    "smashx_abi_sizes": (_int, [ptr]),
    "smashx_plan_create": (_int, [_cfg, _mesh, _out]),
    "smashx_plan_destroy": (_int, [ptr]),
    "smashx_plan_ncells": (_int, [ptr]),
    "smashx_plan_cell_order": (_int, [ptr, ptr, ptr]),
    "smashx_set_forcing": (_int, [ptr, ptr, ptr, _int]),
    "smashx_set_forcing_device_block": (_int, [ptr, _int, _int, ptr, ptr]),
    "smashx_set_forcing_layout": (_int, [ptr, _lay]),
    "smashx_forcing_info": (_int, [ptr, ptr, ptr]),
    "smashx_set_qobs": (_int, [ptr, ptr]),
    "smashx_set_options": (_int, [ptr, _opt]),
    "smashx_forward": (_int, [ptr, _par, _par, _sta, _sta, ptr, _cst, _sta]),
    "smashx_forward_b": (_int, [ptr, _par, _par, _sta, _sta, _float, ptr, _cst, _par, _sta]),
    "smashx_multiple_run": (_int, [ptr, _par, _sta, _int, ptr, ptr, _int, ptr, ptr]),
    "smashx_multiple_run_info": (_int, [ptr, ptr, ptr]),
    "smashx_upload": (_int, [ptr, _par, _par, _sta, _sta]),
    "smashx_sweep": (_int, [ptr, _int, _float]),
    "smashx_download": (_int, [ptr, _int, _par, _sta, ptr, _cst, _sta, _par, _sta]),
    "smashx_get_timing": (_int, [ptr, _tim]),
    "smashx_control_size": (_int, [ptr]),
    "smashx_control_set": (_int, [ptr, ptr]),
    "smashx_control_get": (_int, [ptr, ptr]),
    "smashx_control_gradient": (_int, [ptr, ptr]),
    "smashx_set_domain_outputs": (_int, [ptr, ptr, ptr, _int]),
    "smashx_forward_d": (_int, [ptr, _par, _par, _par, _sta, _sta, _sta, ptr, ptr, _cst, ptr]),
    "smashx_tangent_terms": (_int, [ptr, ptr, ptr]),
    "smashx_tile_probe": (_int, [_cfg, _mesh, ptr, ptr, ptr, ptr, ptr, _int]),
    "smashx_halo_counts": (_int, [ptr, ptr, ptr]),
    "smashx_halo_edges": (_int, [ptr, ptr, ptr, ptr, ptr]),
    "smashx_plan_chunking": (_int, [ptr, ptr, ptr]),
    "smashx_plan_hbm": (_int, [ptr, ptr]),
    "smashx_set_halo": (_int, [ptr, ptr, ptr, HALO_FN, ptr]),
    "smashx_set_median_slots": (_int, [ptr, _int, ptr, REDUCE_FN, ptr]),
    "smashx_comm_unique_id": (_int, [ptr]),
    "smashx_comm_create": (_int, [ptr, _int, _int, _int, _out]),
    "smashx_comm_destroy": (_int, [ptr]),
    "smashx_comm_allreduce_sum": (_int, [ptr, ptr, _int]),
    "smashx_comm_info": (_int, [ptr, ptr, ptr]),
    "smashx_set_exchange": (_int, [ptr, ptr, ptr, ptr]),
    "smashx_hyper_nhyper": (_int, [_map]),
    "smashx_hyper_map_forward": (_int, [_map, ptr, ptr]),
    "smashx_hyper_map_d": (_int, [_map, ptr, ptr, ptr, ptr]),
    "smashx_hyper_map_b": (_int, [_map, ptr, ptr, ptr]),
    "smashx_debug_group_times": (_int, [ptr, ptr, ptr]),
    "smashx_selftest_math": (_int, [_int, _llong, _uint, _float, _float, ptr]),
    "smashx_selftest_paths": (_int, [_int, _llong, _uint, ptr]),
    "smashx_selftest_eval": (_int, [_int, _int, ptr, ptr, _llong, ptr, ptr]),
    "smashx_lbfgsb_create": (_int, [_long, _int, ptr, ptr, _double, _double, _out]),
    "smashx_lbfgsb_step": (_int, [ptr, ptr, _double, ptr, ptr]),
    "smashx_lbfgsb_iterations": (_long, [ptr]),
    "smashx_lbfgsb_evaluations": (_long, [ptr]),
    "smashx_lbfgsb_projected_gradient": (_double, [ptr]),
    "smashx_lbfgsb_message": (_str, [ptr]),
    "smashx_lbfgsb_destroy": (_int, [ptr]),
}
SYMBOLS = list(PROTOTYPES)
# ---- every function of include/smashx_setup.h (the model set-up part of the ABI, which smashx.h includes), the same way;
# tests/test_interception_cpu.py reads that header and compares
SETUP_PROTOTYPES = {
    "smashx_adjust_interception": (_int, [ptr, _int, ptr, ptr]),
}
SETUP_SYMBOLS = list(SETUP_PROTOTYPES)
# ---- every function of include/smashx_forcing.h (statistics of the resident forcing, which smashx.h includes as well), the same way;
# tests/test_mean_forcing_cpu.py reads that header and compares
FORCING_PROTOTYPES = {
    "smashx_mean_forcing": (_int, [ptr, ptr, ptr]),
}
FORCING_SYMBOLS = list(FORCING_PROTOTYPES)
# ---- every function of include/smashx_prcp.h (precipitation indices of the resident forcing, which smashx.h includes as well), the same
# way; tests/test_prcp_indices_cpu.py reads that header and compares
PRCP_PROTOTYPES = {
    "smashx_prcp_indices": (_int, [ptr, ptr, ptr]),
}
PRCP_SYMBOLS = list(PRCP_PROTOTYPES)
# ---- every function of include/smashx_signature.h (inputs of the signature-based criteria, which smashx.h includes as well), the same
# way; tests/test_signature_cost_cpu.py reads that header and compares
SIGNATURE_PROTOTYPES = {
    "smashx_set_signature_inputs": (_int, [ptr, ptr, ptr]),
    "smashx_jobs_of_qsim": (_int, [ptr, ptr, _float, ptr, ptr, ptr, ptr]),
}
SIGNATURE_SYMBOLS = list(SIGNATURE_PROTOTYPES)
# ---- every function of include/smashx_hyper.h (the hyper maps on the device, which smashx.h includes as well), the same way;
# tests/test_hyper_device_cpu.py reads that header and compares
HYPER_DEVICE_PROTOTYPES = {
    "smashx_hyper_set_descriptors": (_int, [ptr, _int, _int, ptr]),
    "smashx_hyper_upload": (_int, [ptr, ptr, ptr]),
    "smashx_hyper_gradient": (_int, [ptr, ptr, ptr]),
    "smashx_hyper_fields": (_int, [ptr, _par, _sta]),
    "smashx_hyper_info": (_int, [ptr, ptr, ptr]),
}
HYPER_DEVICE_SYMBOLS = list(HYPER_DEVICE_PROTOTYPES)
# ---- every function of include/smashx_ann.h (the ANN regionalisation on the device and the same network on the host, which smashx.h
# includes as well), the same way; tests/test_ann_cpu.py reads that header and compares.  ANN_LAYER: the header's enum.
ANN_LAYER = {"dense": 1, "relu": 2, "leaky_relu": 3, "elu": 4, "selu": 5, "sigmoid": 6, "tanh": 7, "scale": 8,       # SMASHX_ANN_DENSE ...
             "softplus": 9, "softmax": 10, "dropout": 11}
_graph = [_int, _int, ptr, ptr, _int]             # nd, nlayers, kind, width, ncv
ANN_PROTOTYPES = {
    "smashx_ann_set_descriptors": (_int, [ptr, _int, ptr]),
    "smashx_ann_set_net": (_int, [ptr, _int, ptr, ptr, _int, ptr, ptr, ptr]),
    "smashx_ann_upload": (_int, [ptr, ptr]),
    "smashx_ann_gradient": (_int, [ptr, ptr]),
    "smashx_ann_fields": (_int, [ptr, _par, _sta]),
    "smashx_ann_info": (_int, [ptr, ptr, ptr]),
    "smashx_ann_host_nweights": (_int, _graph),
    "smashx_ann_host_forward": (_int, _graph + [ptr, ptr, ptr, _long, ptr, ptr]),
    "smashx_ann_host_gradient": (_int, _graph + [ptr, ptr, ptr, _long, ptr, ptr, ptr]),
    "smashx_ann_host_activation": (_int, [_int, _long, ptr, ptr, ptr]),
    "smashx_ann_host_exp": (_int, [_long, ptr, ptr]),
}
ANN_SYMBOLS = list(ANN_PROTOTYPES)
# ---- every function of include/smashx_sbs.h (the optimiser of optimize_sbs in ask / tell form and the cost of a batch of uniform
# candidates on the catchment-resident kernel, which smashx.h includes as well), the same way; tests/test_sbs_cpu.py reads that header
# and compares
SBS_PROTOTYPES = {
    "smashx_sbs_create": (_int, [_int, ptr, ptr, ptr, _float, _int, _out]),
    "smashx_sbs_ask": (_int, [ptr, ptr, ptr]),
    "smashx_sbs_tell": (_int, [ptr, ptr]),
    "smashx_sbs_x": (_int, [ptr, ptr]),
    "smashx_sbs_gx": (_float, [ptr]),
    "smashx_sbs_ddx": (_float, [ptr]),
    "smashx_sbs_iter": (_int, [ptr]),
    "smashx_sbs_nfg": (_int, [ptr]),
    "smashx_sbs_message": (_str, [ptr]),
    "smashx_sbs_destroy": (_int, [ptr]),
    "smashx_uniform_costs": (_int, [ptr, _par, _sta, _int, ptr, ptr, _int, ptr]),
    "smashx_uniform_costs_info": (_int, [ptr, ptr, ptr]),
}
SBS_SYMBOLS = list(SBS_PROTOTYPES)


class SmashxError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"libsmashx error {code}: {msg}")
        self.code = code


_lib = None


def lib():
    """The C-ABI library.  Raises if the HIP extension has not been built (python -c 'import
    __graft_entry__ as g; g.build()')."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(f"{LIB_PATH} is missing: build the HIP library first (__graft_entry__.build()); "
                              "smash_amd has no CPU fallback")
        L = C.CDLL(LIB_PATH)
        for name, (restype, argtypes) in list(PROTOTYPES.items()) + list(SETUP_PROTOTYPES.items()) + list(FORCING_PROTOTYPES.items()) + list(PRCP_PROTOTYPES.items()) + list(SIGNATURE_PROTOTYPES.items()) + list(HYPER_DEVICE_PROTOTYPES.items()) + list(ANN_PROTOTYPES.items()) + list(SBS_PROTOTYPES.items()):
            fn = getattr(L, name)
            fn.restype, fn.argtypes = restype, argtypes
        # the structs above mirror include/smashx.h by hand: refuse a library built from another layout (a stale .so would have
        # smashx_get_timing write past the end of Timing)
        sizes = (C.c_int * 7)()
        L.smashx_abi_sizes(sizes)
        mine = [C.sizeof(t) for t in (Config, Mesh, Options, Parameters, States, Costs, Timing)]
        if list(sizes) != mine:
            raise ImportError(f"{LIB_PATH} was built from another include/smashx.h (struct sizes {list(sizes)}, this module expects {mine}): "
                              "rebuild it (__graft_entry__.build())")
        _lib = L
    return _lib


def check(rc):
    if rc != 0:
        raise SmashxError(rc, lib().smashx_last_error().decode())
