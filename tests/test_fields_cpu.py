"""CPU: the field table of the host driver (smash_amd/csrc/sx_fields.h) -- which fields each structure reads, which device slot holds
each, which are states and which live on the routing stream -- printed by tests/csrc/sx_fields_check.cpp and checked against the
structures' field lists (golden_util) and the SMASHX_P_* / SMASHX_S_* order of include/smashx.h."""
import os
import subprocess

import pytest

import golden_util as gu
from test_abi_header_cpu import HEADER, parse

HERE = os.path.dirname(os.path.abspath(__file__))
EXE = os.path.join(HERE, "csrc", "sx_fields_check")
STRUCTURES = {1: "gr-a", 2: "gr-b", 3: "gr-c", 4: "gr-d", 5: "vic-a"}


@pytest.fixture(scope="module")
def table():
    src = [os.path.join(HERE, "csrc", "sx_fields_check.cpp"), os.path.join(HERE, "..", "smash_amd", "csrc", "sx_fields.h"), HEADER]
    if not os.path.exists(EXE) or os.path.getmtime(EXE) < max(os.path.getmtime(s) for s in src):
        r = subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-o", EXE, src[0]], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-1500:]
    out = subprocess.run([EXE], capture_output=True, text=True, check=True).stdout.split("\n")
    rows = [ln.split() for ln in out if ln]
    sizes = [int(v) for v in next(r for r in rows if r[0] == "sizes")[1:]]
    slots = {(int(r[1]), int(r[2])): tuple(int(v) for v in r[3:]) for r in rows if r[0] == "slot"}      # (st, slot) -> field, state, routing
    fields = {(int(r[1]), int(r[2])): tuple(int(v) for v in r[3:]) for r in rows if r[0] == "field"}    # (st, field) -> slot, state, routing
    seed = [int(v) for v in next(r for r in rows if r[0] == "seed")[1:]]
    return sizes, slots, fields, seed


@pytest.fixture(scope="module")
def names():
    """field index 0..23 -> name, from the enumerators of the header: parameters, then states"""
    c = parse(open(HEADER).read())["constants"]
    gnp, gns = c["SMASHX_GNP"], c["SMASHX_GNS"]
    par = {v: k[len("SMASHX_P_"):].lower() for k, v in c.items() if k.startswith("SMASHX_P_")}
    sta = {v: k[len("SMASHX_S_"):].lower() for k, v in c.items() if k.startswith("SMASHX_S_")}
    assert sorted(par) == list(range(gnp)) and sorted(sta) == list(range(gns))
    return [par[i] for i in range(gnp)] + [sta[i] for i in range(gns)], gnp


def test_sizes(table, names):
    (gnp, gns, nfields, npslots, nslots), slots, fields, _ = table
    assert (gnp, gnp + gns, nfields) == (names[1], len(names[0]), len(names[0]))
    assert (npslots, nslots) == (9, 14)
    assert len(slots) == 5 * nslots and len(fields) == 5 * nfields


@pytest.mark.parametrize("st", sorted(STRUCTURES))
def test_structure_reads_its_fields(table, names, st):
    (_, _, nfields, npslots, nslots), slots, fields, _ = table
    name, gnp = names
    used = [f for f in range(nfields) if fields[st, f][0] >= 0]
    assert {name[f] for f in used if f < gnp} == set(gu.STRUCT_PARAMS[STRUCTURES[st]])
    assert {name[f] for f in used if f >= gnp} == set(gu.STRUCT_STATES[STRUCTURES[st]])
    for f in range(nfields):
        slot, is_state, _ = fields[st, f]
        assert is_state == int(f >= gnp), name[f]
        if slot >= 0:                                        # field -> slot -> field is the identity, and a state sits in a state slot
            assert slots[st, slot][0] == f, name[f]
            assert slots[st, slot][1] == is_state == int(slot >= npslots), name[f]
    for s in range(nslots):                                  # slot -> field -> slot, and no field in two slots
        f = slots[st, s][0]
        assert f == -1 or fields[st, f][0] == s, s
    assert len({slots[st, s][0] for s in range(nslots)} - {-1}) == len(used)


@pytest.mark.parametrize("st", sorted(STRUCTURES))
def test_exactly_lr_and_hlr_live_on_the_routing_stream(table, names, st):
    (_, _, nfields, _, nslots), slots, fields, _ = table
    name, _ = names
    assert {name[f] for f in range(nfields) if fields[st, f][2]} == {"lr", "hlr"}
    assert {name[slots[st, s][0]] for s in range(nslots) if slots[st, s][2]} == {"lr", "hlr"}


def test_seed_order_names_every_slot_once(table):
    (_, _, _, _, nslots), _, _, seed = table
    assert sorted(seed) == list(range(nslots))
