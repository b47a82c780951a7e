"""What the benchmarks of the set-up products on the resident forcing share (interception_bench.py, mean_forcing_bench.py,
prcp_indices_bench.py): the plan with its forcing built on the device, the stderr capture, the timed calls."""
import os
import re
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


class CapturedStderr:
    """what the process (the C library included) writes to file descriptor 2 while the block runs"""

    def __enter__(self):
        sys.stderr.flush()
        self.tmp = tempfile.TemporaryFile(mode="w+b")
        self.saved = os.dup(2)
        os.dup2(self.tmp.fileno(), 2)
        return self

    def __exit__(self, *exc):
        os.dup2(self.saved, 2)
        os.close(self.saved)
        self.tmp.seek(0)
        self.text = self.tmp.read().decode(errors="replace")
        self.tmp.close()


def plan_with_device_forcing(n, nt, ng, torch, dev):
    """gr-b on the synthetic n x n mesh with its first ng gauges (0: none), compact forcing built on the device block by block as
    bench.py builds it -> the synthetic mesh, the MeshDT, the Solver, its forcing_info() and the seconds all that took"""
    import bench
    import smash_amd
    from smash_amd import synth
    from smash_amd.solver import Solver
    t_setup = time.perf_counter()
    m = synth.make_mesh(n, n, ng=max(ng, 1))
    setup = smash_amd.SetupDT(0, ng, structure="gr-b", dt=3600.0, ntime_step=nt)
    if ng:
        mesh = smash_amd.MeshDT.from_synth(setup, m)
    else:
        mesh = smash_amd.MeshDT(setup, n, n, 0)
        mesh.dx, mesh.flwdir, mesh.flwacc, mesh.path, mesh.active_cell = m.dx, m.flwdir, m.flwacc, m.path, m.active_cell
        mesh.gauge_pos, mesh.area = np.zeros((0, 2), np.int32, order="F"), np.zeros(0, np.float32)
    sol = Solver(setup, mesh)
    sol.set_forcing_layout(compact=True, prcp_factor=0.1, pet_ratio=synth._pet_tables()[1], pet_hour0=0)
    rows, cols = sol.cell_order()
    d_rows = torch.from_numpy(rows.astype(np.int64)).to(dev)
    d_cols = torch.from_numpy(cols.astype(np.int64)).to(dev)
    tb = max(24, (1 << 26) // max(sol.ncells, 1) // 24 * 24)
    for t0 in range(0, nt, tb):
        t1 = min(nt, t0 + tb)
        prcp, pet = bench.forcing_block(d_rows, d_cols, t0, t1, dev)
        torch.cuda.synchronize()
        sol.set_forcing_device_block(t0, t1, prcp.data_ptr(), pet.data_ptr())
        del prcp, pet
    del d_rows, d_cols
    torch.cuda.empty_cache()
    return m, mesh, sol, sol.forcing_info(), time.perf_counter() - t_setup


def timed(call, pattern, reps):
    """reps calls after one warm-up (code object load, lists built and uploaded): wall time of each, and the device time and launches the
    library reports under SMASHX_VERBOSE (pattern's groups ms and launches) -> the figures, the last call's match"""
    wall, device, last = [], [], None
    for rep in range(reps + 1):
        with CapturedStderr() as cap:
            t0 = time.perf_counter()
            call()
            w = time.perf_counter() - t0
        mt = re.search(pattern, cap.text)
        if mt is None:
            raise SystemExit("the library did not report its device time (SMASHX_VERBOSE): " + cap.text[-500:])
        if rep == 0:
            first = w
        else:
            wall.append(w); device.append(float(mt.group("ms")) * 1e-3); last = mt
    return {"first_call_wall_s": round(first, 4), "wall_s_median": round(statistics.median(wall), 4), "wall_s_all": [round(v, 4) for v in wall],
            "device_s_median": round(statistics.median(device), 4), "device_s_all": [round(v, 4) for v in device],
            "launches": int(last.group("launches"))}, last
