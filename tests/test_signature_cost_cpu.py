"""CPU: the signature-based criteria (Crc, Cfp2/10/50/90, Epf, Elt, Erc; mwd_cost.f90:772-970).  No device is needed: the numpy
restatement tests/signature_util.py is pinned bit for bit to what the compiled reference computed on hand-made series
(tests/golden/signature_cost/functions.npz, recorded by tests/golden/make_signature_cost.py), and the host side of the feature -- the
codes, the new header, the argument checks and the refusal rule -- is checked against it."""
import os
import re

import numpy as np
import pytest

import signature_util as su
import test_abi_header_cpu as ah

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
FUN = su.load_functions()


def test_new_codes_in_jobs_fun():
    """the eight criteria have codes after SMASHX_LOGARITHMIC, the same in the binding, the header and the recorder"""
    from smash_amd import _lib
    assert [_lib.JOBS_FUN[k] for k in su.NAMES] == list(range(7, 15))
    assert tuple(_lib.SIGNATURE_FUN) == su.NAMES and {k: _lib.JOBS_FUN[k] for k in su.CODES} == su.CODES
    with open(os.path.join(ROOT, "include", "smashx.h")) as f:
        hc = ah.parse(f.read())["constants"]
    assert hc["SMASHX_CFP10"] == _lib.JOBS_FUN["Cfp10"] == 9
    assert {"SMASHX_" + k.upper(): v for k, v in _lib.JOBS_FUN.items()}.items() <= hc.items()


def test_signature_header_matches_the_binding():
    """include/smashx_signature.h against _lib.SIGNATURE_PROTOTYPES with the parser and the type rules of tests/test_abi_header_cpu.py;
    smashx.h brings the header along, after smashx_prcp.h"""
    from smash_amd import _lib
    with open(os.path.join(ROOT, "include", "smashx_signature.h")) as f:
        text = f.read()
    h = ah.parse(text)
    assert h["leftovers"] == [] and h["structs"] == {} and h["callbacks"] == {}
    assert [k for k in h["constants"] if k != "SMASHX_SIGNATURE_H"] == []
    assert not re.search(r"\b(struct|enum|typedef)\b", ah.strip(text)[1])
    calls = re.findall(r"\bsmashx_[a-z_0-9]+\s*\(", ah.strip(text)[1])
    assert len(calls) == len(h["functions"]) == 2
    assert sorted(h["functions"]) == sorted(_lib.SIGNATURE_PROTOTYPES) and _lib.SIGNATURE_SYMBOLS == list(_lib.SIGNATURE_PROTOTYPES)
    others = set(_lib.PROTOTYPES) | set(_lib.SETUP_PROTOTYPES) | set(_lib.FORCING_PROTOTYPES) | set(_lib.PRCP_PROTOTYPES)
    assert not set(_lib.SIGNATURE_PROTOTYPES) & others
    findings = []
    for name, ((rbase, rptr), params) in h["functions"].items():
        restype, argtypes = _lib.SIGNATURE_PROTOTYPES[name]
        assert not rptr and restype is ah.SCALARS[rbase], name
        assert len(params) == len(argtypes), name
        for (pname, base, pointer, length), t in zip(params, argtypes):
            ah.check_type(f"{name}({pname})", t, base, pointer, length, h, _lib, findings, param=True)
    assert findings == []
    assert [q[:3] for q in h["functions"]["smashx_set_signature_inputs"][1]] == [
        ("plan", "smashx_plan", True), ("mean_prcp", "float", True), ("mask_event", "int", True)]
    with open(os.path.join(ROOT, "include", "smashx.h")) as f:
        hdr = f.read()
    assert hdr.count('#include "smashx_signature.h"') == 1
    assert hdr.index('#include "smashx_prcp.h"') < hdr.index('#include "smashx_signature.h"')


@pytest.mark.parametrize("case", sorted(FUN))
def test_restatement_is_the_reference_bit_for_bit(case):
    """signature, SIGNATURE_B (res_b = 1) and SIGNATURE_D of the compiled reference, every criterion it can evaluate on the series"""
    c = FUN[case]
    assert c["crit"], case
    for nm, (res, qs_b, res_d) in c["crit"].items():
        mine = su._walk(c["po"], c["qo"], c["qs"], c["mask"], nm, c["qs_d"])
        assert su.same_bits(mine[0], res), (nm, mine[0], res)
        assert su.same_bits(mine[1], qs_b), (nm, np.flatnonzero(mine[1] != qs_b))
        assert su.same_bits(mine[2], res_d), (nm, mine[2], res_d)
    for nm in su.NAMES:
        assert (nm in c["crit"]) != su.refused(c["po"], c["qo"], c["mask"], nm), nm


def test_fixtures_hold_the_cases_they_are_for():
    """the properties the series were made for, read off the fixture itself"""
    c = FUN["tie_zeros"]
    seeds = tuple(np.flatnonzero(c["crit"]["Cfp2"][1]))
    assert len(seeds) == 2 and all(c["qs"][k] == 0 for k in seeds)                          # a tie across the Cfp2 position ...
    assert seeds != tuple(sorted(su.stable_points(c["qo"], c["qs"], su.PCT["Cfp2"])))       # ... that tells the heap sort from a stable one
    assert {FUN[k]["qo"].size for k in FUN} >= {1, 63, 64, 65, 129, 200}
    for case, n in (("compact1", 1), ("compact2", 2), ("frac_integer", 51)):
        c = FUN[case]
        assert np.count_nonzero((c["qo"] >= 0) & (c["qs"] >= 0)) == n
    n = 51
    for p in su.PCT.values():
        frac = np.float32(np.float32(n - 1) * p) + np.float32(1)
        assert frac == int(frac)
    c = FUN["events200"]
    ev = su.events(c["mask"])
    assert len(ev) == 8 and ev[-1][0] + ev[-1][1] == 200 and su.events(FUN["len63"]["mask"])[0][0] == 0
    folds = [su._event_fold(c["po"], c["qo"], c["qs"], a, n) for a, n in ev]
    assert folds[1][6] == 0 and folds[1][2] == 0          # an event without a valid step
    assert folds[2][2] > 0 and folds[3][2] == 0           # sum_po = 0 after a valid event: Erc carries num / den over
    assert folds[4][7] == 0 and folds[5][8] == 0          # imax_qs = 0, imax_po = 0
    a, n = ev[6]
    assert np.any(c["mask"][a:a + n] != 7) and np.count_nonzero(c["mask"] == 7) == n       # an extent that is not the event's own steps
    assert np.any(c["qo"] < 0) and np.any(c["po"] < 0)
    # the carried num / den matter: without event 4 the Erc value differs
    m2 = c["mask"].copy()
    m2[m2 == 4] = 0
    m2[m2 > 4] -= 1
    assert su.signature(c["po"], c["qo"], c["qs"], m2, "Erc") != c["crit"]["Erc"][0]


def test_check_signature_inputs():
    from smash_amd import SmashxError, _lib, check_signature_inputs
    ng, nt = 2, 5
    mp = np.zeros((ng, nt), np.float32, order="F")
    mk = np.zeros((ng, nt), np.int32, order="F")
    assert check_signature_inputs(ng, nt, mp, mk) == (mp, mk) and check_signature_inputs(ng, nt, mp)[1] is None
    bad_masks = [mk.astype(np.int64), np.ascontiguousarray(mk), np.zeros((ng, nt + 1), np.int32, order="F"), mk.tolist()]
    neg = mk.copy(); neg[0, 0] = -1
    big = mk.copy(); big[1, 2] = nt + 1
    for m in bad_masks + [neg, big]:
        with pytest.raises(SmashxError) as e:
            check_signature_inputs(ng, nt, mp, m)
        assert e.value.code == _lib.E_ARG
    for a in (None, mp.astype(np.float64), np.ascontiguousarray(mp), np.zeros((ng + 1, nt), np.float32, order="F")):
        with pytest.raises(SmashxError) as e:
            check_signature_inputs(ng, nt, a, mk)
        assert e.value.code == _lib.E_ARG


def test_refusal_rule():
    """smash_amd.signature_refusal is the rule of include/smashx_signature.h: it refuses exactly where the restated routine reads an
    unassigned num / den, looks at nothing but qobs, mean_prcp and mask_event from optimize_start_step on, and skips gauges that
    compute_jobs skips"""
    from smash_amd import signature_refusal
    rng = np.random.default_rng(3)
    nt = 40
    seen = set()
    for trial in range(200):
        po = np.where(rng.random(nt) < 0.7, 0.0, rng.random(nt)).astype(np.float32)
        if trial % 10 == 0:
            po[:] = 0.0                                  # a dry series: Crc has nothing to divide by
        po[rng.random(nt) < 0.2] = -99.0
        qo = rng.random(nt).astype(np.float32)
        qo[rng.random(nt) < 0.3] = -99.0
        mask = np.zeros(nt, np.int32)
        for i, a in enumerate(sorted(rng.choice(nt - 6, 3, replace=False))):
            mask[a:a + 5] = i + 1
        s0 = int(rng.integers(0, 10))
        for nm in su.NAMES:
            want = su.refused(po[s0:], qo[s0:], mask[s0:], nm)
            got = signature_refusal([nm], [1.0], qo[None, :], po[None, :], mask[None, :], s0 + 1)
            assert (got is not None) == want, (trial, nm, got)
            seen.add((nm, want))
    assert ("Crc", True) in seen and ("Erc", True) in seen and ("Erc", False) in seen and ("Crc", False) in seen
    assert not any(r for nm, r in seen if nm not in ("Crc", "Erc"))
    dry = np.full((1, nt), -99.0, np.float32)
    q = np.ones((1, nt), np.float32)
    assert signature_refusal(["nse", "Crc"], [1.0], q, dry, None, 1) is not None            # the -99 prefill of mean_prcp
    assert signature_refusal(["nse", "Crc"], [0.0], q, dry, None, 1) is None                # wgauge = 0: not evaluated
    assert signature_refusal(["nse", "Crc"], [1.0], -q, dry, None, 1) is None               # no qobs >= 0: not evaluated
    assert signature_refusal(["nse"], [1.0], q, None, None, 1) is None
    assert signature_refusal(["Cfp2"], [1.0], q, None, None, 1) is not None                 # no mean_prcp at all
    assert signature_refusal(["Epf"], [1.0], q, np.ones((1, nt), np.float32), None, 1) is not None     # an E* criterion without mask_event


def test_optimize_setup_has_mask_event():
    import smash_amd
    s = smash_amd.SetupDT(0, 3, ntime_step=7)
    m = s.optimize.mask_event
    assert m.shape == (3, 7) and m.dtype == np.int32 and m.flags.f_contiguous and not m.any()
    assert s.copy().optimize.mask_event is not m


# outputs of the end-to-end fixtures whose default-build bar (golden_util.tol of the recorded flag-to-flag noise) is above golden_util.CAP:
# a sanity bar, no parity claim -- their parity is asserted in the exact-libm build, bit for bit.  Pinned so that the list cannot grow
# silently (tests/test_oracle_golden.py does the same for the golden fixtures).
SANITY_ONLY = {"gr_a_cance_28x28x1440__all": ["b_cft", "b_cp", "b_exc", "b_hft", "b_hp", "b_lr"],
               "gr_a_cance_28x28x1440__median": ["b_hft"],
               "gr_b_16x16x96_nse_gaps__all": [],
               "gr_b_16x16x96_nse_gaps__median": ["b_cp", "b_hp"]}


def test_sanity_only_outputs_are_pinned():
    import golden_util as gu
    for case in su.E2E_CASES:
        for tag in ("all", "median"):
            z = su.load_e2e(case, tag)
            got = sorted(k[len("noise_"):] for k in z.files if k.startswith("noise_") and gu.sanity_only(float(np.max(z[k]))))
            assert got == SANITY_ONLY[f"{case}__{tag}"], (case, tag, got)


def test_fixture_sizes():
    for f in os.listdir(su.DIR):
        assert os.path.getsize(os.path.join(su.DIR, f)) < 1 << 20, f
    assert re.fullmatch(r"[a-z_0-9]+", "functions")
