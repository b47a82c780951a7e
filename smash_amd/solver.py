"""Host-side mirror of the reference's wrapped boundary for the hot path:

    forward    smash/solver/forward/mw_forward.f90:18-39   -> base_forward   (forward.f90:1-80)
    forward_b  smash/solver/forward/mw_forward.f90:41-68   -> base_forward_b (forward_db.f90:10648-10936)

Same names, argument order and in/out behaviour as the f90wrap functions the reference's Python calls
(smash/core/model.py:490, smash/core/net.py:1044): parameters / states are modified in place
(denormalised on return when setup.optimize.denormalize_forward), results land in ``output`` and in the
``*_b`` objects, and -- like the reference -- nothing is raised for a cost that is NaN.  Differences a
caller can see: unsupported options raise SmashxError instead of being silently ignored, and only the
fields the structure uses are touched.

All arithmetic happens in libsmashx (HIP, gfx950) behind the C ABI of include/smashx.h.
"""
from __future__ import annotations

import ctypes as C

import zlib

import numpy as np

from . import _lib
from ._lib import HYPER, JOBS_FUN, JREG_FUN, SIGNATURE_FUN, STRUCTURES
from .synth import PARAM_DEFAULTS, PARAM_NAMES, STATE_NAMES


# hourly share of the daily PET in the reference's reader (smash/core/_constant.py:47-75)
RATIO_PET_HOURLY = np.array([0, 0, 0, 0, 0, 0, 0, 0.035, 0.062, 0.079, 0.097, 0.11, 0.117, 0.117, 0.11, 0.097, 0.079, 0.062, 0.035,
                             0, 0, 0, 0, 0], dtype=np.float32)


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def make_config(setup, mesh, chunk_steps=0, pipe_steps=0, group_size=0, device=-1, tile=None):
    cfg = _lib.Config()
    cfg.structure, cfg.nrow, cfg.ncol = STRUCTURES[setup.structure], mesh.nrow, mesh.ncol
    cfg.nt, cfg.ng, cfg.dt, cfg.dx = setup.ntime_step, mesh.ng, setup.dt, mesh.dx
    cfg.chunk_steps, cfg.pipe_steps, cfg.group_size, cfg.device = chunk_steps, pipe_steps, group_size, device
    for i in range(4):
        cfg.tile[i] = int(tile[i]) if tile is not None else 0
    return cfg


def _f32(a):
    return np.asfortranarray(a, dtype=np.float32)


def _i32(a):
    return np.asfortranarray(a, dtype=np.int32)


def _pack(obj, names, struct_cls, only=None, rebind=True):
    """The fields `names` of obj (all, or those in `only`) as a smashx_parameters / smashx_states struct of pointers to Fortran-ordered
    float32 planes, plus the arrays that must outlive the call.  A field that needs a converted copy is rebound on obj so that the
    library's writes reach the caller; rebind=False is for read-only fields (never touches obj)."""
    s = struct_cls()
    keep = []
    for i, k in enumerate(names):
        a = getattr(obj, k, None) if obj is not None and (only is None or k in only) else None
        if a is None:
            s.f[i] = None
            continue
        if not (isinstance(a, np.ndarray) and a.dtype == np.float32 and a.flags.f_contiguous):
            a = np.asfortranarray(a, dtype=np.float32)
            if rebind:
                setattr(obj, k, a)
        keep.append(a)
        s.f[i] = a.ctypes.data
    return s, keep


def _pack_const(obj, names, struct_cls):
    """_pack for read-only fields (tools/ensemble_bench.py and the ensemble tests call it by this name)"""
    return _pack(obj, names, struct_cls, rebind=False)


def _store_costs(output, qs, costs):
    """cost terms and discharge of a finished call into output (may be None); returns the cost"""
    if output is not None:
        if qs is not None:
            output.qsim = qs
        output.cost, output.cost_jobs, output.cost_jreg = float(costs.cost), float(costs.cost_jobs), float(costs.cost_jreg)
    return float(costs.cost)


class Comm:
    """One RCCL communicator per process (= per GPU) for the native exchange of boundary series (include/smashx.h
    "native exchange").  Rank 0 draws the id (Comm.unique_id()); the launcher hands it to every rank."""

    @staticmethod
    def unique_id() -> bytes:
        buf = (C.c_ubyte * _lib.COMM_ID_BYTES)()
        _lib.check(_lib.lib().smashx_comm_unique_id(buf))
        return bytes(buf)

    def __init__(self, uid: bytes, rank: int, nranks: int, device: int = -1):
        buf = (C.c_ubyte * _lib.COMM_ID_BYTES).from_buffer_copy(uid)
        self.handle = C.c_void_p()
        self.rank, self.nranks = rank, nranks
        _lib.check(_lib.lib().smashx_comm_create(buf, int(rank), int(nranks), int(device), C.byref(self.handle)))

    def allreduce_sum(self, values):
        v = np.ascontiguousarray(values, np.float64).copy()
        _lib.check(_lib.lib().smashx_comm_allreduce_sum(self.handle, _ptr(v), v.size))
        return v

    def info(self):
        """{nranks, version}: what the communicator itself reports (ncclCommCount, ncclGetVersion)."""
        n, v = C.c_int(0), C.c_int(0)
        _lib.check(_lib.lib().smashx_comm_info(self.handle, C.byref(n), C.byref(v)))
        return {"nranks": n.value, "version": v.value}

    def close(self):
        if getattr(self, "handle", None):
            _lib.lib().smashx_comm_destroy(self.handle)
            self.handle = None


class Solver:
    """A libsmashx plan: routing schedule + HBM-resident forcing for one (setup, mesh, input_data)."""

    def __init__(self, setup, mesh, *, chunk_steps: int = 0, pipe_steps: int = 0, group_size: int = 0, device: int = -1,
                 tile=None, owner_mask=None):
        """tile = (row0, row1, col0, col1): this plan only owns that rectangle of the grid (multi-GPU, see
        smash_amd.tiles); owner_mask (nrow, ncol), 1 = owned, does the same for an arbitrary partition (sub-catchments);
        mesh and field arrays stay global-sized."""
        L = _lib.lib()
        self.nrow, self.ncol, self.nt, self.ng = mesh.nrow, mesh.ncol, setup.ntime_step, mesh.ng
        self.structure = setup.structure
        if setup.structure not in STRUCTURES:
            raise _lib.SmashxError(_lib.E_UNSUPPORTED, f"structure {setup.structure!r} is not on the hot path yet")
        cfg = make_config(setup, mesh, chunk_steps, pipe_steps, group_size, device, tile)
        self._keep = [_i32(mesh.flwdir), _i32(mesh.flwacc), _i32(mesh.active_cell), _i32(mesh.path),
                      _i32(np.asarray(mesh.gauge_pos).reshape(-1, 2)), np.ascontiguousarray(mesh.area, np.float32)]
        m = _lib.Mesh(*[_ptr(a) for a in self._keep])
        if owner_mask is not None:
            self._keep.append(_i32(owner_mask))
            m.owner_mask = self._keep[-1].ctypes.data
        self._h = C.c_void_p()
        _lib.check(L.smashx_plan_create(C.byref(cfg), C.byref(m), C.byref(self._h)))
        self.ncells = L.smashx_plan_ncells(self._h)
        self._sig = self.signature(setup, mesh)

    @staticmethod
    def signature(setup, mesh):
        """Everything a cached plan was built from: sizes, dt, dx and the contents of the mesh arrays."""
        # (checksums of the arrays in their own memory order: no transposed copy of a Fortran-ordered 2048^2 plane per call)
        def crc(a):
            a = np.asarray(a)
            if not (a.flags.c_contiguous or a.flags.f_contiguous):
                a = np.ascontiguousarray(a)
            return (a.shape, a.dtype.str, bool(a.flags.f_contiguous and not a.flags.c_contiguous), zlib.crc32(memoryview(a.ravel(order="K")).cast("B")))
        h = hash(tuple(crc(getattr(mesh, k)) for k in ("flwdir", "flwacc", "active_cell", "gauge_pos", "area")))
        return (setup.structure, setup.ntime_step, float(setup.dt), mesh.nrow, mesh.ncol, mesh.ng, float(mesh.dx), bool(setup.sparse_storage), h)

    FULL_HASH_ELEMENTS = 1 << 24        # fields up to 64 MB are hashed whole

    @staticmethod
    def forcing_fingerprint(prcp, pet):
        """Hash of the forcing arrays, recomputed on every call: values written in place, or new arrays that happen to land at the
        old address, must not be served the forcing already resident in HBM.  Fields up to FULL_HASH_ELEMENTS values are hashed
        whole; larger ones by a strided sample of ~65 k values per field (hashing 70 GB per call would cost more than the sweep), so
        an in-place edit of a small window of a LARGE field can go unnoticed: after such an edit call invalidate_forcing(input_data)
        (or Solver.set_forcing again) -- the reference has no such cache because it has no device copy."""
        out = []
        for a in (prcp, pet):
            a = np.asarray(a)
            flat = a.reshape(-1, order="A") if (a.flags.f_contiguous or a.flags.c_contiguous) else a.ravel()
            step = 1 if flat.size <= Solver.FULL_HASH_ELEMENTS else max(1, flat.size // 65536)
            out.append((a.shape, flat[::step].tobytes()))
        return hash(tuple(out))

    def close(self):
        if getattr(self, "_h", None):
            _lib.lib().smashx_plan_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- residency ---------------------------------------------------------------------------
    def cell_order(self):
        rows = np.zeros(self.ncells, np.int32)
        cols = np.zeros(self.ncells, np.int32)
        _lib.check(_lib.lib().smashx_plan_cell_order(self._h, _ptr(rows), _ptr(cols)))
        return rows, cols

    def set_forcing(self, prcp, pet, sparse=False):
        p, e = _f32(prcp), _f32(pet)
        self._fp = Solver.forcing_fingerprint(prcp, pet)
        _lib.check(_lib.lib().smashx_set_forcing(self._h, _ptr(p), _ptr(e), bool(sparse)))

    def set_forcing_device_block(self, t0, t1, d_prcp_ptr, d_pet_ptr):
        self._forcing_external = True
        _lib.check(_lib.lib().smashx_set_forcing_device_block(self._h, int(t0), int(t1), d_prcp_ptr, d_pet_ptr))

    def set_forcing_layout(self, compact=True, prcp_factor=0.1, pet_ratio=None, pet_hour0=1):
        """Lossless compact residency of the forcing (include/smashx.h smashx_set_forcing_layout): uint16 rain counts x
        prcp_factor + daily PET x pet_ratio[(t + pet_hour0) % 24], verified bit for bit when the forcing is set.
        pet_ratio defaults to the reference's RATIO_PET_HOURLY (smash/core/_constant.py:47-75); pet_hour0 = 1 is a run that
        starts at midnight (the first step is start_time + dt)."""
        lay = _lib.ForcingLayout()
        lay.compact, lay.prcp_factor, lay.pet_hour0 = int(bool(compact)), float(np.float32(prcp_factor)), int(pet_hour0)
        r = RATIO_PET_HOURLY if pet_ratio is None else np.asarray(pet_ratio, np.float32)
        for h in range(24):
            lay.pet_ratio[h] = float(r[h])
        _lib.check(_lib.lib().smashx_set_forcing_layout(self._h, C.byref(lay)))

    def forcing_info(self):
        c, b = C.c_int(0), C.c_double(0.0)
        _lib.check(_lib.lib().smashx_forcing_info(self._h, C.byref(c), C.byref(b)))
        return {"layout": "compact: uint16 rain counts + daily PET x hourly ratio (lossless, verified bit for bit)" if c.value
                else "fp32 rows", "resident_bytes_per_cellstep": round(b.value, 4)}

    def set_qobs(self, qobs):
        q = _f32(qobs)
        _lib.check(_lib.lib().smashx_set_qobs(self._h, _ptr(q)))

    # -- signature-based criteria ------------------------------------------------------------------
    def set_signature_inputs(self, mean_prcp, mask_event=None):
        """What the signature criteria read beside the discharges (include/smashx_signature.h): mean_prcp (ng, nt) float32 and
        mask_event (ng, nt) int32, Fortran order; mask_event = None when no E* criterion will be asked for.  Call before set_options."""
        mp, mk = check_signature_inputs(self.ng, self.nt, mean_prcp, mask_event)
        _lib.check(_lib.lib().smashx_set_signature_inputs(self._h, _ptr(mp), _ptr(mk)))

    def jobs_of_qsim(self, qsim, jobs_b=None, qsim_d=None):
        """The cost kernels on a prescribed discharge (smashx_jobs_of_qsim): qsim (ng, nt) float32 Fortran order.  Returns
        (jobs, qsim_b or None, jobs_d or None): qsim_b = output_b%qsim for the seed jobs_b, jobs_d the tangent along qsim_d."""
        def bad(msg):
            return _lib.SmashxError(_lib.E_ARG, "jobs_of_qsim: " + msg)
        for name, a in (("qsim", qsim), ("qsim_d", qsim_d)):
            if a is not None and (not isinstance(a, np.ndarray) or a.shape != (self.ng, self.nt) or a.dtype != np.float32 or not a.flags.f_contiguous):
                raise bad(f"{name} must be a Fortran-ordered float32 array of shape ({self.ng}, {self.nt})")
        if qsim is None:
            raise bad("qsim is None")
        qb = np.zeros((self.ng, self.nt), np.float32, order="F") if jobs_b is not None else None
        jobs, jobs_d = C.c_float(0.0), C.c_float(0.0)
        _lib.check(_lib.lib().smashx_jobs_of_qsim(self._h, _ptr(qsim), float(jobs_b or 0.0), C.byref(jobs), _ptr(qb), _ptr(qsim_d),
                                                  C.byref(jobs_d) if qsim_d is not None else None))
        return np.float32(jobs.value), qb, (np.float32(jobs_d.value) if qsim_d is not None else None)

    # -- tiles ---------------------------------------------------------------------------------
    def halo_counts(self):
        a, b = C.c_int(0), C.c_int(0)
        _lib.check(_lib.lib().smashx_halo_counts(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def halo_edges(self):
        no, ni = self.halo_counts()
        arr = [np.zeros(max(n, 1), np.int32) for n in (no, no, ni, ni)]
        _lib.check(_lib.lib().smashx_halo_edges(self._h, *[_ptr(a) for a in arr]))
        return arr[0][:no], arr[1][:no], arr[2][:ni], arr[3][:ni]

    def chunking(self):
        a, b = C.c_int(0), C.c_int(0)
        _lib.check(_lib.lib().smashx_plan_chunking(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def hbm(self):
        """{free_at_plan, total, held} in bytes (smashx_plan_hbm): free HBM when the storage-chunk length was chosen, the device's
        total, what the plan holds now."""
        v = (C.c_double * 3)()
        _lib.check(_lib.lib().smashx_plan_hbm(self._h, v))
        return {"free_at_plan": v[0], "total": v[1], "held": v[2]}

    def set_domain_outputs(self, qsim_domain=None, net_prcp_domain=None, sparse=False):
        """Host arrays the following forward sweeps fill (OutputDT%qsim_domain / net_prcp_domain or sparse_ forms)."""
        for a in (qsim_domain, net_prcp_domain):
            if a is not None and not (a.dtype == np.float32 and a.flags.f_contiguous):
                raise _lib.SmashxError(_lib.E_ARG, "domain outputs must be Fortran-ordered float32 arrays")
        self._dom_keep = (qsim_domain, net_prcp_domain)
        _lib.check(_lib.lib().smashx_set_domain_outputs(self._h, _ptr(qsim_domain), _ptr(net_prcp_domain), bool(sparse)))

    def tangent_terms(self):
        """(jobs_d, jreg_d) of the last forward_d on this plan (include/smashx.h smashx_tangent_terms): over a decomposition the
        parts' jobs_d add up and jreg_d -- the whole grid's on every part -- enters once."""
        a, b = C.c_float(0.0), C.c_float(0.0)
        _lib.check(_lib.lib().smashx_tangent_terms(self._h, C.byref(a), C.byref(b)))
        return float(a.value), float(b.value)

    def group_times(self):
        """Diagnostics (SMASHX_TRACE_GROUPS=1): (ticks[2][groups][2] at 100 MHz, round_of_group[groups])."""
        ng = self.timing()["n_groups"]
        out = np.zeros((2, ng, 2), np.int64)
        rnd = np.zeros(ng, np.int32)
        _lib.check(_lib.lib().smashx_debug_group_times(self._h, _ptr(out), _ptr(rnd)))
        return out, rnd

    def set_halo(self, out_ptr, in_ptr, fn):
        """fn(phase, t0, nsteps) -> 0; out_ptr / in_ptr: device addresses of the message buffers."""
        def tramp(user, phase, t0, nsteps):
            try:
                return int(fn(phase, t0, nsteps) or 0)
            except Exception:  # pragma: no cover
                import traceback
                traceback.print_exc()
                return 1
        self._halo_cb = _lib.HALO_FN(tramp)
        _lib.check(_lib.lib().smashx_set_halo(self._h, out_ptr, in_ptr, self._halo_cb, None))

    def set_median_slots(self, nslots, slot_of_gauge, reduce_fn=None):
        """The median over the negative-weight gauges of a decomposition (include/smashx.h "cost terms that span the tiles";
        tiles.median_slots builds the arguments).  reduce_fn(values: float32 array, in place) sums the slot values over the tiles;
        not needed with the native exchange (set_exchange), which all-reduces them on the routing stream.  Call before set_options."""
        sl = np.ascontiguousarray(slot_of_gauge, np.int32) if self.ng else np.full(1, -1, np.int32)
        cb = _lib.REDUCE_FN()               # a NULL function pointer: no host reduction
        if reduce_fn is not None:
            def tramp(user, vals, n):
                try:
                    a = np.ctypeslib.as_array(vals, shape=(n,))
                    reduce_fn(a)
                    return 0
                except Exception:  # pragma: no cover
                    import traceback
                    traceback.print_exc()
                    return 1
            cb = _lib.REDUCE_FN(tramp)
        self._median_cb = cb
        _lib.check(_lib.lib().smashx_set_median_slots(self._h, int(nslots), _ptr(sl), cb, None))

    def set_exchange(self, comm, out_peer, in_peer):
        """Native exchange (smashx_set_exchange): comm = a Comm (or None to unset); out_peer / in_peer = the rank owning the
        other end of every out / in boundary edge, in the order of halo_edges()."""
        op, ip = np.ascontiguousarray(out_peer, np.int32), np.ascontiguousarray(in_peer, np.int32)
        self._comm = comm
        _lib.check(_lib.lib().smashx_set_exchange(self._h, comm.handle if comm is not None else None, _ptr(op), _ptr(ip)))

    def set_options(self, opt):
        o = _lib.Options()
        o.denormalize_forward = int(bool(opt.denormalize_forward))
        o.optimize_start_step = int(opt.optimize_start_step)
        o.njf = len(opt.jobs_fun)
        for i, j in enumerate(opt.jobs_fun):
            if j not in JOBS_FUN:
                raise _lib.SmashxError(_lib.E_UNSUPPORTED, f"jobs_fun {j!r} is outside the hot path")
            o.jobs_fun[i] = JOBS_FUN[j]
            o.wjobs_fun[i] = float(opt.wjobs_fun[i])
        o.njr = len(opt.jreg_fun)
        for i, j in enumerate(opt.jreg_fun):
            o.jreg_fun[i] = JREG_FUN.get(j, 0)
            o.wjreg_fun[i] = float(opt.wjreg_fun[i])
        o.wjreg = float(opt.wjreg)
        for i in range(16):
            o.optim_parameters[i] = int(opt.optim_parameters[i])
            o.lb_parameters[i] = float(opt.lb_parameters[i])
            o.ub_parameters[i] = float(opt.ub_parameters[i])
        for i in range(8):
            o.optim_states[i] = int(opt.optim_states[i])
            o.lb_states[i] = float(opt.lb_states[i])
            o.ub_states[i] = float(opt.ub_states[i])
        wg = np.ascontiguousarray(opt.wgauge, np.float32) if self.ng else np.zeros(1, np.float32)
        o.wgauge = _ptr(wg)
        _lib.check(_lib.lib().smashx_set_options(self._h, C.byref(o)))

    # -- calls ---------------------------------------------------------------------------------
    def upload(self, parameters, states, parameters_bgd=None, states_bgd=None, only=None):
        """only = names of the fields that changed since the last upload (the others keep their device copies)."""
        P, k1 = _pack(parameters, PARAM_NAMES, _lib.Parameters, only)
        S, k2 = _pack(states, STATE_NAMES, _lib.States, only)
        PB, k3 = _pack(parameters_bgd, PARAM_NAMES, _lib.Parameters) if parameters_bgd is not None else (None, None)
        SB, k4 = _pack(states_bgd, STATE_NAMES, _lib.States) if states_bgd is not None else (None, None)
        _lib.check(_lib.lib().smashx_upload(self._h, C.byref(P), C.byref(PB) if PB is not None else None, C.byref(S),
                                            C.byref(SB) if SB is not None else None))

    # -- control vector of the calibration, packed / unpacked on the device (mw_optimize.f90:679-777) ----------------------------
    def control_size(self):
        return int(_lib.lib().smashx_control_size(self._h))

    def control_set(self, x):
        x = np.ascontiguousarray(x, np.float64)
        _lib.check(_lib.lib().smashx_control_set(self._h, _ptr(x)))

    def control_get(self):
        x = np.zeros(self.control_size(), np.float64)
        _lib.check(_lib.lib().smashx_control_get(self._h, _ptr(x)))
        return x

    def control_gradient(self):
        g = np.zeros(self.control_size(), np.float64)
        _lib.check(_lib.lib().smashx_control_gradient(self._h, _ptr(g)))
        return g

    def cost_and_qsim(self, output):
        """cost + discharge of the last sweep only (no field comes back)."""
        qs = np.zeros((self.ng, self.nt), np.float32, order="F") if self.ng else None
        costs = _lib.Costs()
        _lib.check(_lib.lib().smashx_download(self._h, 0, None, None, _ptr(qs), C.byref(costs), None, None, None))
        return _store_costs(output, qs, costs)

    def sweep(self, adjoint=False, cost_b=1.0):
        _lib.check(_lib.lib().smashx_sweep(self._h, bool(adjoint), cost_b))

    def timing(self):
        t = _lib.Timing()
        _lib.check(_lib.lib().smashx_get_timing(self._h, C.byref(t)))
        d = {k: getattr(t, k) for k, _ in _lib.Timing._fields_ if k != "cellsteps"}
        for i, k in enumerate(("vert_fwd", "route_fwd", "route_adj", "vert_adj")):
            d[k + "_cellsteps"] = float(t.cellsteps[i])
        return d

    def download(self, adjoint, parameters, states, output, parameters_b=None, states_b=None, only_b=None):
        """parameters / states None: nothing but cost, discharge and gradients comes back; only_b = the gradient fields wanted."""
        P, k1 = _pack(parameters, PARAM_NAMES, _lib.Parameters)
        S, k2 = _pack(states, STATE_NAMES, _lib.States)
        qs = np.zeros((self.ng, self.nt), np.float32, order="F") if self.ng else None
        costs = _lib.Costs()
        F = PB = SB = None
        kf = kp = ks = None
        if not adjoint and output is not None:
            F, kf = _pack(output.fstates, STATE_NAMES, _lib.States)
        if adjoint:
            PB, kp = _pack(parameters_b, PARAM_NAMES, _lib.Parameters, only_b)
            SB, ks = _pack(states_b, STATE_NAMES, _lib.States, only_b)
        _lib.check(_lib.lib().smashx_download(self._h, bool(adjoint), C.byref(P), C.byref(S), _ptr(qs), C.byref(costs),
                                              C.byref(F) if F is not None else None,
                                              C.byref(PB) if PB is not None else None,
                                              C.byref(SB) if SB is not None else None))
        return _store_costs(output, qs, costs)

    # -- ensemble ------------------------------------------------------------------------------
    def multiple_run(self, parameters, states, sample, ind_parameters_states, return_qsim=False, *, res_cost=None, res_qsim=None):
        """compute_multiple_run (mw_multiple_run.f90:68-119) on the plan's resident forcing, qobs and options: sample (nf, S),
        ind_parameters_states (nf) 1-based into the stacked md_constant order (parameters 1..16, states 17..24).  Returns
        res_cost (S,) or (res_cost, res_qsim (ng, nt, S)).  parameters / states are read only."""
        sample, ind = check_multiple_run(self.structure, self.ng, self.nt, sample, ind_parameters_states, res_cost, res_qsim)
        nf, S = sample.shape
        if res_cost is None:
            res_cost = np.zeros(S, np.float32)
        if res_qsim is None and return_qsim:
            res_qsim = np.zeros((self.ng, self.nt, S), np.float32, order="F")
        want_q = res_qsim is not None and res_qsim.size > 0
        P, k1 = _pack_const(parameters, PARAM_NAMES, _lib.Parameters)
        St, k2 = _pack_const(states, STATE_NAMES, _lib.States)
        _lib.check(_lib.lib().smashx_multiple_run(self._h, C.byref(P), C.byref(St), nf, _ptr(ind), _ptr(sample), S,
                                                  _ptr(res_cost), _ptr(res_qsim) if want_q else None))
        return (res_cost, res_qsim) if return_qsim else res_cost

    def multiple_run_info(self):
        """{batch, chunk, n_batches, n_chunks, device_ms} of the last multiple_run on this plan (smashx_multiple_run_info)."""
        info, ms = (C.c_int * 4)(), C.c_float(0.0)
        _lib.check(_lib.lib().smashx_multiple_run_info(self._h, info, C.byref(ms)))
        return {"batch": info[0], "chunk": info[1], "n_batches": info[2], "n_chunks": info[3], "device_ms": float(ms.value)}

    def uniform_costs(self, parameters, states, sample, ind_parameters_states, *, res_cost=None):
        """The cost of S spatially uniform candidates on the catchment-resident kernel (smashx_uniform_costs): the arguments and the
        result of multiple_run without the discharge.  Returns res_cost (S,).  parameters / states are read only."""
        sample, ind = check_multiple_run(self.structure, self.ng, self.nt, sample, ind_parameters_states, res_cost)
        nf, S = sample.shape
        if res_cost is None:
            res_cost = np.zeros(S, np.float32)
        P, k1 = _pack_const(parameters, PARAM_NAMES, _lib.Parameters)
        St, k2 = _pack_const(states, STATE_NAMES, _lib.States)
        _lib.check(_lib.lib().smashx_uniform_costs(self._h, C.byref(P), C.byref(St), nf, _ptr(ind), _ptr(sample), S, _ptr(res_cost)))
        return res_cost

    def uniform_costs_info(self):
        """{cells, levels, block, lds_bytes, device_ms} of the last uniform_costs on this plan (smashx_uniform_costs_info)."""
        info, ms = (C.c_int * 4)(), C.c_float(0.0)
        _lib.check(_lib.lib().smashx_uniform_costs_info(self._h, info, C.byref(ms)))
        return {"cells": info[0], "levels": info[1], "block": info[2], "lds_bytes": info[3], "device_ms": float(ms.value)}

    # -- interception capacity ---------------------------------------------------------------------
    def adjust_interception(self, day_index, ci=None):
        """adjust_interception_store (mw_interception_store.f90:19-160) on the plan's resident forcing: day_index (nt) is the 1-based
        day number of every step (smash_amd.day_index builds it), nday its last entry.  Returns the (nrow, ncol) plane of capacities:
        ci itself when given (a Fortran-ordered float32 plane; active cells the plan owns are overwritten, the others keep their
        values), else a new plane that holds ParametersDT's default everywhere else."""
        nday, day, ci = check_adjust_interception(self.structure, self.nrow, self.ncol, self.nt,
                                                  int(np.asarray(day_index).reshape(-1)[-1]) if np.size(day_index) else 0, day_index, ci)
        _lib.check(_lib.lib().smashx_adjust_interception(self._h, nday, _ptr(day), _ptr(ci)))
        return ci

    # -- catchment means of the forcing -------------------------------------------------------------
    def mean_forcing(self, mean_prcp=None, mean_pet=None, *, prcp=True, pet=True):
        """compute_mean_forcing (mw_forcing_statistic.f90:18-75) on the plan's resident forcing.  Returns (mean_prcp, mean_pet), each
        (ng, nt) float32 in Fortran order: the array given, fully overwritten, or a new one; prcp = False / pet = False leaves that
        field out (it is then not read on the device) and returns None in its place."""
        mp, me = check_mean_forcing(self.ng, self.nt, mean_prcp, mean_pet, prcp, pet)
        _lib.check(_lib.lib().smashx_mean_forcing(self._h, _ptr(mp), _ptr(me)))
        return mp, me

    # -- precipitation indices of the forcing -------------------------------------------------------
    def prcp_indices(self, flwdst, prcp_indices=None):
        """compute_prcp_indices (mw_forcing_statistic.f90:77-220) on the plan's resident rain.  flwdst: (nrow, ncol) float32 Fortran
        order (mesh.flwdst); prcp_indices: (4, ng, nt) float32 Fortran order, (std, d1, d2, vg), updated in place -- a step without rain
        keeps its entries -- or None for a new array prefilled with -1.  Returns the array."""
        dst, out = check_prcp_indices(self.nrow, self.ncol, self.ng, self.nt, flwdst, prcp_indices)
        _lib.check(_lib.lib().smashx_prcp_indices(self._h, _ptr(dst), _ptr(out)))
        return out

    # -- hyper maps on the device (include/smashx_hyper.h) -------------------------------------------
    def set_hyper_descriptors(self, mapping, descriptor):
        """input_data.descriptor (nrow, ncol, nd) float32 Fortran order and the mapping ("hyper-linear" / "hyper-polynomial") into HBM
        (smashx_hyper_set_descriptors); handing over what the plan already holds moves nothing.  descriptor = None drops them."""
        code, nd, desc = check_hyper_descriptors(self.nrow, self.ncol, mapping, descriptor)
        _lib.check(_lib.lib().smashx_hyper_set_descriptors(self._h, code, nd, _ptr(desc)))
        self._hyper_nh = None if desc is None else (1 + 2 * nd if code == HYPER["hyper-polynomial"] else 1 + nd)

    def hyper_upload(self, hyper_parameters, hyper_states):
        """The forward map on the device, in place of upload() in front of sweep(): hyper_parameters (nhyper, 16) and hyper_states
        (nhyper, 8), float32 Fortran order (Hyper_ParametersDT.matrix())."""
        hp, hs = check_hyper_matrices(getattr(self, "_hyper_nh", None), hyper_parameters, hyper_states)
        _lib.check(_lib.lib().smashx_hyper_upload(self._h, _ptr(hp), _ptr(hs)))

    def hyper_gradient(self, hyper_parameters_b=None, hyper_states_b=None):
        """After an adjoint sweep: (hyper_parameters_b (nhyper, 16), hyper_states_b (nhyper, 8)), the arrays given -- overwritten --
        or new ones."""
        nh = getattr(self, "_hyper_nh", None)
        if hyper_parameters_b is None and nh is not None:
            hyper_parameters_b = np.zeros((nh, len(PARAM_NAMES)), np.float32, order="F")
        if hyper_states_b is None and nh is not None:
            hyper_states_b = np.zeros((nh, len(STATE_NAMES)), np.float32, order="F")
        hpb, hsb = check_hyper_matrices(nh, hyper_parameters_b, hyper_states_b, writeable=True)
        _lib.check(_lib.lib().smashx_hyper_gradient(self._h, _ptr(hpb), _ptr(hsb)))
        return hpb, hsb

    def _mapped_fields(self, who, call, parameters, states):
        """hyper_fields / ann_fields: the planes of parameters / states, every one a writeable (nrow, ncol) array, handed to call"""
        P, k1 = _pack(parameters, PARAM_NAMES, _lib.Parameters)
        S, k2 = _pack(states, STATE_NAMES, _lib.States)
        for a in k1 + k2:
            if a.shape != (self.nrow, self.ncol) or not a.flags.writeable:
                raise _lib.SmashxError(_lib.E_ARG, f"{who}: every plane must be a writeable ({self.nrow}, {self.ncol}) array")
        _lib.check(call(self._h, C.byref(P), C.byref(S)))

    def hyper_fields(self, parameters=None, states=None):
        """The mapped fields of the last hyper_upload into the planes of parameters / states (either may be None): active cells are
        written, the others keep their values."""
        self._mapped_fields("hyper_fields", _lib.lib().smashx_hyper_fields, parameters, states)

    def hyper_info(self):
        """{nd, nhyper, chains, span, map_ms, gradient_ms} of the last hyper_upload / hyper_gradient on this plan (smashx_hyper_info)."""
        info, ms = (C.c_int * 4)(), (C.c_float * 2)()
        _lib.check(_lib.lib().smashx_hyper_info(self._h, info, ms))
        return {"nd": info[0], "nhyper": info[1], "chains": info[2], "span": info[3], "map_ms": float(ms[0]), "gradient_ms": float(ms[1])}


    # -- the ANN regionalisation on the device (include/smashx_ann.h) ------------------------------------
    def set_ann_descriptors(self, descriptor):
        """The NORMALISED descriptors (nrow, ncol, nd), float32 Fortran order, into HBM (smashx_ann_set_descriptors); handing over what
        the plan already holds moves nothing."""
        nd, desc = check_ann_descriptors(self.nrow, self.ncol, descriptor)
        _lib.check(_lib.lib().smashx_ann_set_descriptors(self._h, nd, _ptr(desc)))

    def set_ann_net(self, net, control_vector):
        """The graph of a smash_amd.Net and the fields its outputs go to: control_vector names parameters / states, one per output
        (smashx_ann_set_net).  Behind set_ann_descriptors, whose nd is the net's input width."""
        nd, kind, width, ncv, lower, upper = net.graph()
        field = check_ann_control_vector(control_vector, ncv)
        if lower is not None and lower.size != ncv:
            raise _lib.SmashxError(_lib.E_ARG, f"ann net: the scale layer has {lower.size} bounds, the network {ncv} outputs")
        _lib.check(_lib.lib().smashx_ann_set_net(self._h, len(kind), _ptr(kind), _ptr(width), ncv, _ptr(field), _ptr(lower), _ptr(upper)))
        self._ann_nw = int(sum((l.input_shape[0] + 1) * l.neurons for l in net._dense()))

    def ann_upload(self, weights):
        """The network at every active cell into the control fields, behind an upload() of the background fields and in front of
        sweep(): weights packed float64 (Net.weights())."""
        _lib.check(_lib.lib().smashx_ann_upload(self._h, _ptr(check_ann_weights(getattr(self, "_ann_nw", None), weights))))

    def ann_gradient(self, weights_b=None):
        """After an adjoint sweep: the gradient w.r.t. the packed weights, float64 (the array given -- overwritten -- or a new one)."""
        nw = getattr(self, "_ann_nw", None)
        if weights_b is None and nw is not None:
            weights_b = np.zeros(nw, np.float64)
        wb = check_ann_weights(nw, weights_b, writeable=True)
        _lib.check(_lib.lib().smashx_ann_gradient(self._h, _ptr(wb)))
        return wb

    def ann_fields(self, parameters=None, states=None):
        """The mapped control fields of the last ann_upload into the planes of parameters / states (either may be None): their active
        cells are written, everything else stays."""
        self._mapped_fields("ann_fields", _lib.lib().smashx_ann_fields, parameters, states)

    def ann_info(self):
        """{nd, nweights, span, lds_bytes, map_ms, gradient_ms} of the last ann_upload / ann_gradient on this plan (smashx_ann_info)."""
        info, ms = (C.c_int * 4)(), (C.c_float * 2)()
        _lib.check(_lib.lib().smashx_ann_info(self._h, info, ms))
        return {"nd": info[0], "nweights": info[1], "span": info[2], "lds_bytes": info[3], "map_ms": float(ms[0]), "gradient_ms": float(ms[1])}


def check_ann_descriptors(nrow, ncol, descriptor):
    """Argument checks of set_ann_descriptors, before anything reaches the C call: (nd, descriptor)"""
    d = descriptor
    if (not isinstance(d, np.ndarray) or d.ndim != 3 or d.shape[:2] != (nrow, ncol) or d.shape[2] < 1 or d.dtype != np.float32
            or not d.flags.f_contiguous):
        raise _lib.SmashxError(_lib.E_ARG, f"ann descriptors: a Fortran-ordered float32 array of shape ({nrow}, {ncol}, nd >= 1) expected")
    return d.shape[2], d


def check_ann_control_vector(control_vector, ncv):
    """names of parameters / states, one per output of the network -> their field numbers (0 .. 15 parameters, 16 .. 23 states), int32"""
    names = [str(k) for k in control_vector]
    both = list(PARAM_NAMES) + list(STATE_NAMES)
    if len(names) != ncv or len(set(names)) != len(names) or any(k not in both for k in names):
        raise _lib.SmashxError(_lib.E_ARG, f"ann control vector: {ncv} distinct names of parameters / states expected, got {names}")
    return np.array([both.index(k) for k in names], np.int32)


def check_ann_weights(nweights, weights, writeable=False):
    """Argument checks of ann_upload / ann_gradient: a contiguous float64 vector of the net's packed length"""
    if nweights is None:
        raise _lib.SmashxError(_lib.E_STATE, "ann weights: no net set (set_ann_net)")
    w = weights
    if (not isinstance(w, np.ndarray) or w.shape != (nweights,) or w.dtype != np.float64 or not w.flags.c_contiguous
            or (writeable and not w.flags.writeable)):
        raise _lib.SmashxError(_lib.E_ARG, f"ann weights: a {'writeable ' if writeable else ''}contiguous float64 vector of length {nweights} expected")
    return w


def check_hyper_descriptors(nrow, ncol, mapping, descriptor):
    """Argument checks of set_hyper_descriptors, before anything reaches the C call (an array of another shape, type or order would be
    read out of bounds or scrambled).  Returns (mapping code, nd, descriptor) ready for the call -- descriptor None (drop) gives
    (code, 1, None); raises SmashxError(E_ARG)."""
    def bad(msg):
        return _lib.SmashxError(_lib.E_ARG, "hyper descriptors: " + msg)
    if mapping not in HYPER:
        raise bad(f"mapping = {mapping!r}: hyper-linear or hyper-polynomial expected")
    if descriptor is None:
        return HYPER[mapping], 1, None
    if (not isinstance(descriptor, np.ndarray) or descriptor.ndim != 3 or descriptor.shape[:2] != (nrow, ncol)
            or descriptor.dtype != np.float32 or not descriptor.flags.f_contiguous):
        raise bad(f"descriptor must be a Fortran-ordered float32 array of shape ({nrow}, {ncol}, nd)")
    return HYPER[mapping], int(descriptor.shape[2]), descriptor


def check_hyper_matrices(nhyper, hyper_parameters, hyper_states, writeable=False):
    """Argument checks of hyper_upload / hyper_gradient: (nhyper, 16) and (nhyper, 8) float32 Fortran-ordered matrices, nhyper as the
    descriptors the plan holds give it (None: none set).  Returns the two arrays; raises SmashxError(E_STATE) without descriptors and
    SmashxError(E_ARG) for everything else."""
    def bad(msg):
        return _lib.SmashxError(_lib.E_ARG, "hyper matrices: " + msg)
    if nhyper is None:
        raise _lib.SmashxError(_lib.E_STATE, "hyper matrices: no descriptors set (set_hyper_descriptors)")
    for name, a, nf in (("hyper_parameters", hyper_parameters, len(PARAM_NAMES)), ("hyper_states", hyper_states, len(STATE_NAMES))):
        if (not isinstance(a, np.ndarray) or a.shape != (nhyper, nf) or a.dtype != np.float32 or not a.flags.f_contiguous
                or (writeable and not a.flags.writeable)):
            raise bad(f"{name} must be a {'writeable ' if writeable else ''}Fortran-ordered float32 array of shape ({nhyper}, {nf})")
    return hyper_parameters, hyper_states


# fields each structure reads, stacked md_constant order 1..24 (include/smashx.h: parameters 1..16, states 17..24)
FIELD_NAMES = tuple(PARAM_NAMES) + tuple(STATE_NAMES)
STRUCTURE_FIELDS = {
    "gr-a": ("cp", "cft", "exc", "lr", "hp", "hft", "hlr"),
    "gr-b": ("ci", "cp", "cft", "exc", "lr", "hi", "hp", "hft", "hlr"),
    "gr-c": ("ci", "cp", "cft", "cst", "exc", "lr", "hi", "hp", "hft", "hst", "hlr"),
    "gr-d": ("cp", "cft", "lr", "hp", "hft", "hlr"),
    "vic-a": ("b", "cusl1", "cusl2", "clsl", "ks", "ds", "dsm", "ws", "lr", "husl1", "husl2", "hlsl", "hlr"),
}


def check_multiple_run(structure, ng, nt, sample, ind_parameters_states, res_cost=None, res_qsim=None):
    """Argument checks of multiple_run, before anything reaches the device (a wrong shape handed to the C call would be read or
    written out of bounds).  Returns (sample, ind) ready for the call; raises SmashxError(E_ARG)."""
    def bad(msg):
        return _lib.SmashxError(_lib.E_ARG, "multiple_run: " + msg)
    if structure not in STRUCTURE_FIELDS:
        raise _lib.SmashxError(_lib.E_UNSUPPORTED, f"structure {structure!r} is not on the hot path yet")
    if not isinstance(sample, np.ndarray) or sample.ndim != 2:
        raise bad("sample must be a 2-D array (nfields, nsamples)")
    if sample.dtype != np.float32 or not sample.flags.f_contiguous:
        raise bad("sample must be a Fortran-ordered float32 array")
    nf, S = sample.shape
    if S < 1:
        raise bad("no sample (S < 1)")
    ind = np.asarray(ind_parameters_states)
    if ind.ndim != 1 or ind.shape[0] != nf or not np.issubdtype(ind.dtype, np.integer):
        raise bad(f"ind_parameters_states must hold {nf} integers, one per row of sample")
    ind = np.ascontiguousarray(ind, np.int32)
    if np.any(ind < 1) or np.any(ind > len(FIELD_NAMES)):
        raise bad(f"an index is outside 1..{len(FIELD_NAMES)}")
    if len(set(ind.tolist())) != nf:
        raise bad("an index is repeated")
    for i in ind:
        if FIELD_NAMES[i - 1] not in STRUCTURE_FIELDS[structure]:
            raise bad(f"field {FIELD_NAMES[i - 1]!r} (index {i}) is not used by {structure}")
    if res_cost is not None:
        if not isinstance(res_cost, np.ndarray) or res_cost.shape != (S,) or res_cost.dtype != np.float32 or not res_cost.flags.f_contiguous:
            raise bad(f"res_cost must be a contiguous float32 array of shape ({S},)")
    if res_qsim is not None and getattr(res_qsim, "size", 0) > 0:
        if not isinstance(res_qsim, np.ndarray) or res_qsim.shape != (ng, nt, S) or res_qsim.dtype != np.float32 or not res_qsim.flags.f_contiguous:
            raise bad(f"res_qsim must be empty or a Fortran-ordered float32 array of shape ({ng}, {nt}, {S})")
    return sample, ind


def compute_multiple_run(setup, mesh, input_data, parameters, states, output, sample, ind_parameters_states, res_cost, res_qsim):
    """Drop-in for mw_multiple_run::compute_multiple_run (mw_multiple_run.f90:68-119), same argument order: res_cost (S,) and
    -- unless its size is 0 -- res_qsim (ng, nt, S) are filled in place; parameters, states and output are left untouched."""
    if res_cost is None:
        raise _lib.SmashxError(_lib.E_ARG, "multiple_run: res_cost is None")
    sample, ind = check_multiple_run(setup.structure, mesh.ng, setup.ntime_step, sample, ind_parameters_states, res_cost,
                                     res_qsim if res_qsim is not None else np.zeros(0, np.float32))
    s = _solver_for(setup, mesh, input_data)
    s.multiple_run(parameters, states, sample, ind, res_cost=res_cost, res_qsim=res_qsim)
    return res_cost


def multiple_run(setup, mesh, input_data, parameters, states, sample, return_qsim=False):
    """Convenience form: sample = {field name: 1-D array of S values}.  Returns res_cost or (res_cost, res_qsim)."""
    if not isinstance(sample, dict) or not sample:
        raise _lib.SmashxError(_lib.E_ARG, "multiple_run: sample must be a non-empty dict {field name: values}")
    for k in sample:
        if k not in FIELD_NAMES:
            raise _lib.SmashxError(_lib.E_ARG, f"multiple_run: unknown field {k!r}")
    cols = [np.asarray(v, np.float32).reshape(-1) for v in sample.values()]
    if len({c.size for c in cols}) != 1:
        raise _lib.SmashxError(_lib.E_ARG, "multiple_run: the fields of sample differ in length")
    mat = np.asfortranarray(np.stack(cols, axis=0), dtype=np.float32)
    ind = np.array([FIELD_NAMES.index(k) + 1 for k in sample], np.int32)
    check_multiple_run(setup.structure, mesh.ng, setup.ntime_step, mat, ind)
    s = _solver_for(setup, mesh, input_data)
    return s.multiple_run(parameters, states, mat, ind, return_qsim=return_qsim)


def uniform_costs(setup, mesh, input_data, parameters, states, sample, ind_parameters_states, res_cost=None):
    """The cost of every column of sample (nfields, S) -- spatially uniform values of the fields ind_parameters_states, 1-based into
    the stacked md_constant order -- on the catchment-resident kernel: what compute_multiple_run returns as res_cost, for the few
    candidates of a uniform calibration on a small catchment (smashx_uniform_costs; SmashxError(E_UNSUPPORTED) beyond its limits)."""
    sample, ind = check_multiple_run(setup.structure, mesh.ng, setup.ntime_step, sample, ind_parameters_states, res_cost)
    s = _solver_for(setup, mesh, input_data)
    return s.uniform_costs(parameters, states, sample, ind, res_cost=res_cost)


# ---- interception capacity: mw_interception_store::adjust_interception_store (mw_interception_store.f90:19-160) -------------------
# structures with an interception store (smash/core/_constant.py STRUCTURE_ADJUST_CI)
STRUCTURE_ADJUST_CI = {"gr-a": False, "gr-b": True, "gr-c": True, "gr-d": False, "vic-a": False}


def day_index(start_time, end_time, dt):
    """The day number of every time step as _build_parameters forms it (smash/core/_build_model.py:238-248): the steps are
    start_time + dt, start_time + 2 dt, ... up to end_time (the first step is start_time + dt), a step belongs to the calendar day
    its time stamp falls on, and the days are numbered from 1 in order of appearance.  start_time / end_time: anything
    numpy.datetime64 takes ("2014-09-15 00:00", datetime, datetime64); dt in seconds.  Returns the int32 array (ntime_step);
    nday is its last entry."""
    t0, t1 = np.datetime64(start_time, "s"), np.datetime64(end_time, "s")
    step = int(dt)
    if step <= 0 or step != dt:
        raise _lib.SmashxError(_lib.E_ARG, f"day_index: dt = {dt!r} must be a positive whole number of seconds")
    nt = int((t1 - t0) // np.timedelta64(step, "s"))
    if nt < 1:
        raise _lib.SmashxError(_lib.E_ARG, "day_index: end_time is less than one time step after start_time")
    stamps = t0 + np.arange(1, nt + 1) * np.timedelta64(step, "s")
    days = stamps.astype("datetime64[D]")
    out = np.ones(nt, np.int32)
    out[1:] += np.cumsum(days[1:] != days[:-1])
    return out


def check_adjust_interception(structure, nrow, ncol, nt, nday, day_index, ci=None):
    """Argument checks of adjust_interception, before anything reaches the C call (a short day_index would be read out of bounds,
    a plane of another shape written out of bounds).  Returns (nday, day_index as int32, ci) ready for the call -- ci = None gives a
    new plane filled with ParametersDT's default; raises SmashxError(E_UNSUPPORTED) for a structure without an interception store
    and SmashxError(E_ARG) for everything else."""
    def bad(msg):
        return _lib.SmashxError(_lib.E_ARG, "adjust_interception: " + msg)
    if not STRUCTURE_ADJUST_CI.get(structure, False):
        raise _lib.SmashxError(_lib.E_UNSUPPORTED, f"adjust_interception: structure {structure!r} has no interception store")
    day = np.asarray(day_index)
    if day.ndim != 1 or not np.issubdtype(day.dtype, np.integer):
        raise bad("day_index must be a 1-D integer array")
    if day.shape[0] != nt:
        raise bad(f"day_index holds {day.shape[0]} entries, the run has {nt} time steps")
    if day[0] != 1:
        raise bad(f"day_index must start at 1 (it starts at {int(day[0])})")
    step = np.diff(day.astype(np.int64))
    if np.any((step != 0) & (step != 1)):
        t = int(np.flatnonzero((step != 0) & (step != 1))[0]) + 1
        raise bad(f"day_index must be non-decreasing in steps of 0 or 1 (entry {t} is {int(day[t])} after {int(day[t - 1])})")
    if isinstance(nday, bool) or not isinstance(nday, (int, np.integer)):
        raise bad("nday must be an integer")
    if int(day[-1]) != int(nday):
        raise bad(f"day_index ends at day {int(day[-1])}, nday = {int(nday)}")
    if ci is None:
        ci = np.full((nrow, ncol), PARAM_DEFAULTS["ci"], np.float32, order="F")
    elif not isinstance(ci, np.ndarray) or ci.shape != (nrow, ncol) or ci.dtype != np.float32 or not ci.flags.f_contiguous:
        raise bad(f"ci must be a Fortran-ordered float32 array of shape ({nrow}, {ncol})")
    return int(nday), np.ascontiguousarray(day, np.int32), ci


def adjust_interception_store(setup, mesh, input_data, parameters, nday, day_index):
    """Drop-in for mw_interception_store::adjust_interception_store (mw_interception_store.f90:19-160), same argument order:
    parameters.ci is overwritten on the active cells with the capacity, out of 0.1 ... 4.9 mm, whose sub-daily interception
    evaporation over the period comes closest to the one formed from daily totals.  The forcing is the one resident in HBM (it is
    uploaded first when the plan does not hold it yet)."""
    nday, day, ci = check_adjust_interception(setup.structure, mesh.nrow, mesh.ncol, setup.ntime_step, nday, day_index,
                                              np.asfortranarray(parameters.ci, dtype=np.float32))
    s = _solver_for(setup, mesh, input_data, options=False)
    parameters.ci = s.adjust_interception(day, ci)
    return parameters.ci


# ---- catchment means of the forcing: mw_forcing_statistic::compute_mean_forcing (mw_forcing_statistic.f90:18-75) -------------------
def check_mean_forcing(ng, nt, mean_prcp=None, mean_pet=None, prcp=True, pet=True):
    """Argument checks of mean_forcing, before anything reaches the C call (an array of another shape, type or order would be written
    out of bounds or scrambled).  Returns (mean_prcp, mean_pet) ready for the call: the caller's arrays, new (ng, nt) float32 Fortran
    arrays filled with -99 (mwd_input_data.f90:100-106) where none was given, None for a field that is left out.  Raises
    SmashxError(E_ARG)."""
    def bad(msg):
        return _lib.SmashxError(_lib.E_ARG, "mean_forcing: " + msg)
    if not prcp and not pet:
        raise bad("neither prcp nor pet is asked for")
    out = []
    for name, a, want in (("mean_prcp", mean_prcp, prcp), ("mean_pet", mean_pet, pet)):
        if not want:
            if a is not None:
                raise bad(f"{name} was given but the field is left out")
            out.append(None)
        elif a is None:
            out.append(np.full((ng, nt), -99.0, np.float32, order="F"))
        elif not isinstance(a, np.ndarray) or a.shape != (ng, nt) or a.dtype != np.float32 or not a.flags.f_contiguous or not a.flags.writeable:
            raise bad(f"{name} must be a writeable Fortran-ordered float32 array of shape ({ng}, {nt})")
        else:
            out.append(a)
    return out[0], out[1]


def compute_mean_forcing(setup, mesh, input_data):
    """Drop-in for mw_forcing_statistic::compute_mean_forcing (mw_forcing_statistic.f90:18-75), same argument order:
    input_data.mean_prcp / mean_pet (ng, nt) are overwritten with the mean, over the cells upstream of every gauge, of the values >= 0
    of every time step -- the reference's fp32 sum in column-major cell order, bit for bit.  The forcing is the one resident in HBM
    (it is uploaded first when the plan does not hold it yet).  Returns (mean_prcp, mean_pet)."""
    mp, me = check_mean_forcing(mesh.ng, setup.ntime_step, getattr(input_data, "mean_prcp", None), getattr(input_data, "mean_pet", None))
    if mesh.ng == 0:
        input_data.mean_prcp, input_data.mean_pet = mp, me
        return mp, me
    s = _solver_for(setup, mesh, input_data, options=False)
    input_data.mean_prcp, input_data.mean_pet = s.mean_forcing(mp, me)
    return input_data.mean_prcp, input_data.mean_pet


# ---- inputs of the signature-based criteria (mwd_cost.f90:82, 125-129) -----------------------------------------------------------------
def wants_signature(jobs_fun):
    return any(j in SIGNATURE_FUN for j in jobs_fun)


def check_signature_inputs(ng, nt, mean_prcp, mask_event=None):
    """Argument checks of set_signature_inputs, before anything reaches the C call (an array of another shape, type or order would be
    read out of bounds or scrambled).  Returns (mean_prcp, mask_event) ready for the call; raises SmashxError(E_ARG)."""
    def bad(msg):
        return _lib.SmashxError(_lib.E_ARG, "signature inputs: " + msg)
    if not isinstance(mean_prcp, np.ndarray) or mean_prcp.shape != (ng, nt) or mean_prcp.dtype != np.float32 or not mean_prcp.flags.f_contiguous:
        raise bad(f"mean_prcp must be a Fortran-ordered float32 array of shape ({ng}, {nt})")
    if mask_event is not None:
        if not isinstance(mask_event, np.ndarray) or mask_event.shape != (ng, nt) or mask_event.dtype != np.int32 or not mask_event.flags.f_contiguous:
            raise bad(f"mask_event must be a Fortran-ordered int32 array of shape ({ng}, {nt})")
        if mask_event.size and (mask_event.min() < 0 or mask_event.max() > nt):
            raise bad(f"mask_event holds entries outside 0..{nt} (0 outside events, 1..n inside)")
    return mean_prcp, mask_event


def signature_refusal(jobs_fun, wgauge, qobs, mean_prcp, mask_event, optimize_start_step):
    """The refusal rule of smashx_set_options for the signature criteria (include/smashx_signature.h), on the host: the reason, or None.
    The reference leaves num / den unassigned -- and then reads them -- for Crc when the rain summed over the steps with qobs >= 0 and
    mean_prcp >= 0 is not > 0, and for an Erc event of which that holds when no earlier event assigned them; whether that happens
    depends on qobs, mean_prcp and mask_event only.  Gauges with wgauge = 0 or without any qobs >= 0 are not evaluated."""
    s0 = int(optimize_start_step) - 1
    want = [j for j in jobs_fun if j in SIGNATURE_FUN]
    if not want:
        return None
    if mean_prcp is None:
        return "signature criteria read mean_prcp, which is missing"
    if mask_event is None and any(j[0] == "E" for j in want):
        return "Epf / Elt / Erc read mask_event, which is missing"
    qobs, po = np.asarray(qobs, np.float32)[:, s0:], np.asarray(mean_prcp, np.float32)[:, s0:]
    for g in range(qobs.shape[0]):
        if not (wgauge[g] > 0 or wgauge[g] < 0) or not np.any(qobs[g] >= 0):
            continue
        valid = (qobs[g] >= 0) & (po[g] >= 0)        # (qo is qobs times a positive factor)
        if "Crc" in want and not np.any(po[g][valid] > 0):
            return f"Crc at gauge {g + 1}: no precipitation > 0 on the steps with qobs >= 0 and mean_prcp >= 0"
        if "Erc" in want:
            mk = np.asarray(mask_event)[g, s0:]
            pos = np.flatnonzero(mk > 0)
            for i in range(1, (int(mk[pos[-1]]) if pos.size else 0) + 1):
                w = np.flatnonzero(mk == i)
                if w.size and np.any(po[g][w[0]:w[0] + w.size][valid[w[0]:w[0] + w.size]] > 0):
                    break
                return f"Erc at gauge {g + 1}, event {i}: no precipitation > 0 on its valid steps and no earlier event assigned the ratio"
    return None


# ---- precipitation indices: mw_forcing_statistic::compute_prcp_indices (mw_forcing_statistic.f90:77-220) -----------------------------
PRCP_INDICES = ("std", "d1", "d2", "vg")


def check_prcp_indices(nrow, ncol, ng, nt, flwdst, prcp_indices=None):
    """Argument checks of prcp_indices, before anything reaches the C call (an array of another shape, type or order would be read or
    written out of bounds or scrambled).  Returns (flwdst, prcp_indices) ready for the call: the caller's arrays, or a new
    (4, ng, nt) float32 Fortran array filled with -1 (smash/core/prcp_indices.py:112-116) where none was given.  Raises
    SmashxError(E_ARG)."""
    def bad(msg):
        return _lib.SmashxError(_lib.E_ARG, "prcp_indices: " + msg)
    if not isinstance(flwdst, np.ndarray) or flwdst.shape != (nrow, ncol) or flwdst.dtype != np.float32 or not flwdst.flags.f_contiguous:
        raise bad(f"flwdst must be a Fortran-ordered float32 array of shape ({nrow}, {ncol})")
    if prcp_indices is None:
        prcp_indices = np.full((4, ng, nt), -1.0, np.float32, order="F")
    elif (not isinstance(prcp_indices, np.ndarray) or prcp_indices.shape != (4, ng, nt) or prcp_indices.dtype != np.float32
          or not prcp_indices.flags.f_contiguous or not prcp_indices.flags.writeable):
        raise bad(f"prcp_indices must be a writeable Fortran-ordered float32 array of shape (4, {ng}, {nt})")
    return flwdst, prcp_indices


def compute_prcp_indices(setup, mesh, input_data, prcp_indices):
    """Drop-in for mw_forcing_statistic::compute_prcp_indices (mw_forcing_statistic.f90:77-220), same argument order: prcp_indices
    (4, ng, nt) is updated in place with (std, d1, d2, vg) of every gauge and step that has rain over the gauge's upstream cells --
    the reference's fp32 arithmetic bit for bit, its reading of the cell (gauge_row, gauge_row) included -- and left as passed on the
    others.  Reads mesh.flwdst and the rain resident in HBM (it is uploaded first when the plan does not hold it yet).  Returns the
    array."""
    dst, out = check_prcp_indices(mesh.nrow, mesh.ncol, mesh.ng, setup.ntime_step, mesh.flwdst, prcp_indices)
    if mesh.ng == 0:
        return out
    s = _solver_for(setup, mesh, input_data, options=False)
    return s.prcp_indices(dst, out)


def prcp_indices(setup, mesh, input_data):
    """Model.prcp_indices() of the reference (smash/core/prcp_indices.py:111-124): {"std", "d1", "d2", "vg"} -> (ng, nt) float32 arrays,
    from a prefill of -1 with every negative entry turned into NaN."""
    _, out = check_prcp_indices(mesh.nrow, mesh.ncol, mesh.ng, setup.ntime_step, mesh.flwdst, None)
    compute_prcp_indices(setup, mesh, input_data, out)
    out = np.where(out < 0, np.float32(np.nan), out)
    return dict(zip(PRCP_INDICES, out))


def _tangent_call(s, parameters, parameters_d, parameters_bgd, states, states_d, states_bgd, output, output_d):
    P, k1 = _pack(parameters, PARAM_NAMES, _lib.Parameters)
    PD, k2 = _pack(parameters_d, PARAM_NAMES, _lib.Parameters)
    PB, k3 = _pack(parameters_bgd, PARAM_NAMES, _lib.Parameters)
    S, k4 = _pack(states, STATE_NAMES, _lib.States)
    SD, k5 = _pack(states_d, STATE_NAMES, _lib.States)
    SB, k6 = _pack(states_bgd, STATE_NAMES, _lib.States)
    qs = np.zeros((s.ng, s.nt), np.float32, order="F") if s.ng else None
    qd = np.zeros((s.ng, s.nt), np.float32, order="F") if s.ng else None
    costs = _lib.Costs()
    cost_d = C.c_float(0.0)
    _lib.check(_lib.lib().smashx_forward_d(s._h, C.byref(P), C.byref(PD), C.byref(PB), C.byref(S), C.byref(SD), C.byref(SB),
                                           _ptr(qs), _ptr(qd), C.byref(costs), C.byref(cost_d)))
    cost = _store_costs(output, qs, costs)
    if output_d is not None and qd is not None:
        output_d.qsim = qd
    return cost, float(cost_d.value)


def invalidate_forcing(input_data):
    """The forcing arrays of input_data were edited in place: the next forward / forward_b / forward_d call uploads them again."""
    s = getattr(input_data, "_smashx_solver", None)
    if s is not None:
        s._fp = None
        s._forcing_external = False


def _solver_for(setup, mesh, input_data, options=True, **kw):
    s = getattr(input_data, "_smashx_solver", None)
    if s is not None and getattr(s, "_forcing_external", False):      # the caller placed the forcing in HBM itself (device blocks)
        fp = None
    else:
        fp = Solver.forcing_fingerprint(*((input_data.sparse_prcp, input_data.sparse_pet) if setup.sparse_storage
                                          else (input_data.prcp, input_data.pet)))
    if s is None or s._sig != Solver.signature(setup, mesh):
        s = Solver(setup, mesh, **kw)
        s._fp = None
        input_data._smashx_solver = s
    if fp is not None and getattr(s, "_fp", None) != fp:
        if setup.sparse_storage:
            s.set_forcing(input_data.sparse_prcp, input_data.sparse_pet, sparse=True)
        else:
            s.set_forcing(input_data.prcp, input_data.pet, sparse=False)
        s._fp = fp
    if not options:       # a call that reads nothing but the forcing (adjust_interception_store, compute_mean_forcing, compute_prcp_indices)
        return s
    if mesh.ng:
        s.set_qobs(input_data.qobs)
    if mesh.ng and wants_signature(setup.optimize.jobs_fun):
        # the criteria's inputs before the options, which decide the refusals on them; keyed on their contents like the forcing
        # (mask_event and mean_prcp are written in place by their producers)
        o = setup.optimize
        events = any(j in ("Epf", "Elt", "Erc") for j in o.jobs_fun)
        mp, mk = check_signature_inputs(mesh.ng, setup.ntime_step, getattr(input_data, "mean_prcp", None),
                                        getattr(o, "mask_event", None) if events else None)
        why = signature_refusal(o.jobs_fun, o.wgauge, input_data.qobs, mp, mk, o.optimize_start_step)
        if why is not None:
            raise _lib.SmashxError(_lib.E_UNSUPPORTED, why)
        key = (zlib.crc32(mp.tobytes(order="A")), None if mk is None else zlib.crc32(mk.tobytes(order="A")))
        if getattr(s, "_sig_key", None) != key:
            s.set_signature_inputs(mp, mk)
            s._sig_key = key
    s.set_options(setup.optimize)
    return s


def forward(setup, mesh, input_data, parameters, parameters_bgd, states, states_bgd, output, cost=None):
    """Drop-in for mw_forward::forward (mw_forward.f90:18-39).  Returns output.cost."""
    s = _solver_for(setup, mesh, input_data)
    s.upload(parameters, states, parameters_bgd, states_bgd)
    key = "sparse_" if setup.sparse_storage else ""
    dom = (getattr(output, key + "qsim_domain", None) if getattr(setup, "save_qsim_domain", False) else None,
           getattr(output, key + "net_prcp_domain", None) if getattr(setup, "save_net_prcp_domain", False) else None)
    if dom[0] is not None or dom[1] is not None:
        s.set_domain_outputs(dom[0], dom[1], setup.sparse_storage)
    try:
        s.sweep(False)
    finally:
        if dom[0] is not None or dom[1] is not None:
            s.set_domain_outputs(None, None)
    return s.download(False, parameters, states, output)


def forward_b(setup, mesh, input_data, parameters, parameters_b, parameters_bgd, parameters_bgd_b, states, states_b,
              states_bgd, states_bgd_b, output, output_b, cost=None, cost_b=1.0):
    """Drop-in for mw_forward::forward_b (mw_forward.f90:41-68): parameters_b / states_b are overwritten
    with the gradient of the cost (times cost_b); *_bgd_b and output_b are scratch in the reference and
    are left untouched here."""
    s = _solver_for(setup, mesh, input_data)
    s.upload(parameters, states, parameters_bgd, states_bgd)
    s.sweep(True, float(cost_b))
    return s.download(True, parameters, states, output, parameters_b, states_b)


def forward_d(setup, mesh, input_data, parameters, parameters_d, parameters_bgd, parameters_bgd_d, states, states_d,
              states_bgd, states_bgd_d, output, output_d, cost=None, cost_d=None):
    """Drop-in for mw_forward::forward_d (mw_forward.f90:70-97), the tangent-linear model: returns (cost, cost_d) and
    fills output.qsim / output_d.qsim.  *_bgd_d are passive in the reference and are ignored."""
    s = _solver_for(setup, mesh, input_data)
    return _tangent_call(s, parameters, parameters_d, parameters_bgd, states, states_d, states_bgd, output, output_d)


# ---- hyper mappings: mw_forward::hyper_forward / hyper_forward_b / hyper_forward_d (mw_forward.f90:99-181) -------------------------
def _hyper_map(setup, mesh, input_data, nfields, lb, ub):
    if setup.optimize.mapping not in HYPER:
        raise _lib.SmashxError(_lib.E_ARG, f"setup.optimize.mapping = {setup.optimize.mapping!r}: hyper-linear or hyper-polynomial expected")
    desc = np.asfortranarray(input_data.descriptor, dtype=np.float32)
    m = _lib.HyperMap(HYPER[setup.optimize.mapping], mesh.nrow, mesh.ncol, int(desc.shape[2]) if desc.ndim == 3 else 0, nfields,
                      _ptr(desc), None, None)
    keep = (desc, np.ascontiguousarray(lb, np.float32), np.ascontiguousarray(ub, np.float32))
    m.lb, m.ub = _ptr(keep[1]), _ptr(keep[2])
    return m, keep


def _plane_ptrs(fields, names):
    arr = (C.c_void_p * len(names))()
    for i, k in enumerate(names):
        a = getattr(fields, k)
        if not (a.dtype == np.float32 and a.flags.f_contiguous):
            a = np.asfortranarray(a, dtype=np.float32)
            setattr(fields, k, a)
        arr[i] = a.ctypes.data
    return arr


def _hyper_to_fields(setup, mesh, input_data, parameters, hyper_parameters, states, hyper_states, direction=None):
    """hyper_parameters_to_parameters + hyper_states_to_states (mwd_parameters_manipulation.f90:304-362, mwd_states_manipulation.f90:
    270-329) -- or, with direction = (hyper_parameters_d, parameters_d, hyper_states_d, states_d), their tangents (_D)."""
    L, o = _lib.lib(), setup.optimize
    for names, fields, hyp, lb, ub, k in ((PARAM_NAMES, parameters, hyper_parameters, o.lb_parameters, o.ub_parameters, 0),
                                          (STATE_NAMES, states, hyper_states, o.lb_states, o.ub_states, 2)):
        m, keep = _hyper_map(setup, mesh, input_data, len(names), lb, ub)
        h = hyp.matrix()
        if direction is None:
            _lib.check(L.smashx_hyper_map_forward(C.byref(m), _ptr(h), _plane_ptrs(fields, names)))
        else:
            hd = direction[k].matrix()
            _lib.check(L.smashx_hyper_map_d(C.byref(m), _ptr(h), _ptr(hd), _plane_ptrs(fields, names), _plane_ptrs(direction[k + 1], names)))


def _plain(setup):
    """base_hyper_forward knows neither denormalize_forward nor the regularisers (hyper_compute_cost: cost = jobs)."""
    s = setup.copy()
    s.optimize.denormalize_forward = False
    s.optimize.jreg_fun, s.optimize.wjreg_fun, s.optimize.wjreg = [], [], 0.0
    return s


def hyper_forward(setup, mesh, input_data, parameters, hyper_parameters, hyper_parameters_bgd, states, hyper_states, hyper_states_bgd,
                  output, cost=None):
    """Drop-in for mw_forward::hyper_forward (mw_forward.f90:99-123 -> base_hyper_forward, forward.f90:82-157): the descriptor ->
    field maps on the host (include/smashx.h "hyper mappings"), the time loop and the cost on the GPU.  parameters / states come back
    as the mapped fields / the FINAL states (forward.f90:150: no restore).  Returns output.cost."""
    _hyper_to_fields(setup, mesh, input_data, parameters, hyper_parameters, states, hyper_states)
    s = _solver_for(_plain(setup), mesh, input_data)
    s.upload(parameters, states, parameters, states)
    s.sweep(False)
    cost = s.download(False, None, None, output)
    for k in STATE_NAMES:
        getattr(states, k)[...] = getattr(output.fstates, k)
    return cost


def hyper_forward_b(setup, mesh, input_data, parameters, parameters_b, hyper_parameters, hyper_parameters_b, hyper_parameters_bgd,
                    states, states_b, hyper_states, hyper_states_b, hyper_states_bgd, output, output_b, cost=None, cost_b=1.0):
    """Drop-in for mw_forward::hyper_forward_b (mw_forward.f90:125-152 -> BASE_HYPER_FORWARD_B, forward_db.f90:11231-11560):
    hyper_parameters_b / hyper_states_b are overwritten with the gradient of the cost w.r.t. the coefficients (times cost_b);
    parameters_b / states_b hold the gradient w.r.t. the mapped fields."""
    L, o = _lib.lib(), setup.optimize
    _hyper_to_fields(setup, mesh, input_data, parameters, hyper_parameters, states, hyper_states)
    s = _solver_for(_plain(setup), mesh, input_data)
    s.upload(parameters, states, parameters, states)
    s.sweep(True, float(cost_b))
    cost = s.download(True, None, None, output, parameters_b, states_b)
    # (the gradient planes of fields the structure does not read come back as zeros: they add nothing to any sum)
    for names, grads, hyp, hyp_b, lb, ub in ((STATE_NAMES, states_b, hyper_states, hyper_states_b, o.lb_states, o.ub_states),
                                             (PARAM_NAMES, parameters_b, hyper_parameters, hyper_parameters_b, o.lb_parameters, o.ub_parameters)):
        m, keep = _hyper_map(setup, mesh, input_data, len(names), lb, ub)
        ptrs = _plane_ptrs(grads, names)
        hb = np.zeros((o.nhyper, len(names)), np.float32, order="F")
        _lib.check(L.smashx_hyper_map_b(C.byref(m), _ptr(hyp.matrix()), ptrs, _ptr(hb)))
        hyp_b.set_matrix(hb)
    return cost


def hyper_forward_d(setup, mesh, input_data, parameters, parameters_d, hyper_parameters, hyper_parameters_d, hyper_parameters_bgd,
                    states, states_d, hyper_states, hyper_states_d, hyper_states_bgd, output, output_d, cost=None, cost_d=None):
    """Drop-in for mw_forward::hyper_forward_d (mw_forward.f90:154-181 -> BASE_HYPER_FORWARD_D, forward_db.f90:11079-11162).
    Returns (cost, cost_d)."""
    _hyper_to_fields(setup, mesh, input_data, parameters, hyper_parameters, states, hyper_states,
                     direction=(hyper_parameters_d, parameters_d, hyper_states_d, states_d))
    s = _solver_for(_plain(setup), mesh, input_data)
    return _tangent_call(s, parameters, parameters_d, parameters, states, states_d, states, output, output_d)


def scalar_product_test(setup, mesh, input_data, parameters, states, output):
    """mw_adjoint_test::scalar_product_test (mw_adjoint_test.f90:26-105): <dY*, dY> = cost_b * cost_d against
    <dk*, dk> = sum(parameters_b * parameters_d) for dk = 1 on every parameter field and 0 on the states.
    Returns (sp1, sp2)."""
    from .types import OutputDT
    par_d, sta_d = parameters.copy(), states.copy()
    for k in PARAM_NAMES:
        getattr(par_d, k)[...] = 1.0
    for k in STATE_NAMES:
        getattr(sta_d, k)[...] = 0.0
    par_b, sta_b = parameters.copy(), states.copy()
    out_d, out_b = OutputDT(setup, mesh), OutputDT(setup, mesh)
    _, cost_d = forward_d(setup, mesh, input_data, parameters.copy(), par_d, parameters.copy(), parameters.copy(), states.copy(),
                          sta_d, states.copy(), states.copy(), output, out_d)
    forward_b(setup, mesh, input_data, parameters.copy(), par_b, parameters.copy(), parameters.copy(), states.copy(), sta_b,
              states.copy(), states.copy(), output, out_b, 0.0, 1.0)
    sp2 = float(sum(np.sum(getattr(par_b, k).astype(np.float64) * getattr(par_d, k)) for k in PARAM_NAMES))
    return 1.0 * cost_d, sp2


def gradient_test(setup, mesh, input_data, parameters, states, output, nstep=16):
    """mw_adjoint_test::gradient_test (mw_adjoint_test.f90:108-189): Ia = (Y(k + a dk) - Y(k)) / (a dk* . dk) for dk = 1 on
    every parameter field and a = 2^0 .. 2^-(nstep-1); Y = cost of a forward sweep, dk* = parameters_b of one adjoint sweep.
    Returns [(a, |Ia - 1|), ...] (the reference prints them)."""
    from .types import OutputDT
    bgd_p, bgd_s = parameters.copy(), states.copy()
    yk = np.float32(forward(setup, mesh, input_data, parameters.copy(), bgd_p, states.copy(), bgd_s, output))
    par_b, sta_b = parameters.copy(), states.copy()
    forward_b(setup, mesh, input_data, parameters.copy(), par_b, bgd_p, parameters.copy(), states.copy(), sta_b, bgd_s, states.copy(),
              output, OutputDT(setup, mesh), 0.0, 1.0)
    dot = np.float32(0.0)
    for k in PARAM_NAMES:                      # sum(parameters_b_matrix * dk), fp32 like the reference
        dot = np.float32(dot + np.sum(getattr(par_b, k), dtype=np.float32))
    res = []
    for n in range(nstep):
        an = np.float32(2.0 ** (-n))
        p = bgd_p.copy()
        for k in PARAM_NAMES:
            getattr(p, k)[...] = getattr(bgd_p, k) + an
        yadk = np.float32(forward(setup, mesh, input_data, p, bgd_p, states.copy(), bgd_s, output))
        ian = np.float32((yadk - yk) / (an * dot))
        res.append((float(an), float(abs(ian - np.float32(1.0)))))
    return res
