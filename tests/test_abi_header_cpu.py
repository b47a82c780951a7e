"""CPU: the ctypes binding (smash_amd/_lib.py) against include/smashx.h, read as text.

The header is regular enough for regular expressions: comments and preprocessor lines are stripped, then every statement is either an
enum, a struct typedef, a callback typedef, an opaque typedef or a function prototype.  `compare(text, binding)` returns a list of
findings (strings that name the offender); the tests expect none on the real header and at least one on edited copies of it, and
count what the parser found against the header's own text so that a declaration it skips fails here instead of passing."""
import ctypes as C
import os
import re

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
HEADER = os.path.join(ROOT, "include", "smashx.h")

SCALARS = {"int": C.c_int, "long": C.c_long, "long long": C.c_longlong, "unsigned": C.c_uint, "float": C.c_float, "double": C.c_double,
           "unsigned char": C.c_ubyte}
CALLBACKS = {"smashx_halo_fn": "HALO_FN", "smashx_reduce_fn": "REDUCE_FN"}
N_FUNCTIONS, N_STRUCTS = 56, 9


def strip(text):
    """the header without comments; returns (with preprocessor lines, without them)"""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    return text, re.sub(r"^[ \t]*#[^\n]*$", " ", text, flags=re.M)


def parse_declarators(decl):
    """'const float* a, b[4]' -> [(name, base type, is pointer, array length or None), ...]; the length stays a token"""
    first, *rest = [d.strip() for d in decl.split(",")]
    m = re.fullmatch(r"(.*?[\w\*])\s*(\b\w+)\s*(?:\[(\w+)\])?", first, flags=re.S)
    if not m:
        raise ValueError(f"cannot parse declaration {decl!r}")
    base, out = m.group(1), [(m.group(2), m.group(3))]
    for d in rest:
        m2 = re.fullmatch(r"(\w+)\s*(?:\[(\w+)\])?", d)
        if not m2:
            raise ValueError(f"cannot parse declarator {d!r} of {decl!r}")
        out.append((m2.group(1), m2.group(2)))
    pointer = "*" in base
    base = " ".join(base.replace("*", " ").replace("const", " ").split())
    return [(name, base, pointer, length) for name, length in out]


def parse(text):
    """-> dict(constants, structs, functions, leftovers).  structs: name -> [(field, base, pointer, length)];
    functions: name -> (return (base, pointer), [(param, base, pointer, length)]); leftovers: statements nothing recognised."""
    with_pp, code = strip(text)
    constants = {k: int(v) for k, v in re.findall(r"^[ \t]*#[ \t]*define[ \t]+(SMASHX_\w+)[ \t]+(-?\d+)[ \t]*$", with_pp, flags=re.M)}
    leftovers = []

    def take_enum(m):
        items = [i.strip() for i in m.group(1).split(",") if i.strip()]
        for i in items:
            mm = re.fullmatch(r"(\w+)\s*=\s*(-?\d+)", i)
            if mm:
                constants[mm.group(1)] = int(mm.group(2))
            else:
                leftovers.append("enumerator " + i)
        return " "
    code = re.sub(r"\benum\s*\{(.*?)\}\s*;", take_enum, code, flags=re.S)
    structs = {}

    def take_struct(m):
        fields = []
        for decl in m.group(1).split(";"):
            if decl.strip():
                fields += parse_declarators(decl.strip())
        structs[m.group(2)] = fields
        return " "
    code = re.sub(r"\btypedef\s+struct\s*\{(.*?)\}\s*(\w+)\s*;", take_struct, code, flags=re.S)
    callbacks = {name: [p for a in args.split(",") for p in parse_declarators(a.strip())]
                 for name, args in re.findall(r"\btypedef\s+int\s*\(\s*\*\s*(\w+)\s*\)\s*\(([^)]*)\)\s*;", code)}
    code = re.sub(r"\btypedef\s+int\s*\(\s*\*\s*\w+\s*\)\s*\([^)]*\)\s*;", " ", code)
    code = re.sub(r"\btypedef\s+struct\s+(\w+)\s+\1\s*;", " ", code)
    code = re.sub(r'\bextern\s+"C"\s*\{', " ", code)
    functions = {}
    for stmt in code.split(";"):
        stmt = stmt.strip().lstrip("}").strip()        # (the brace that closes extern "C")
        if not stmt:
            continue
        m = re.fullmatch(r"(.*?[\w\*])\s*(\bsmashx_\w+)\s*\((.*)\)", stmt, flags=re.S)
        if not m or m.group(2) in functions:
            leftovers.append(" ".join(stmt.split())[:80])
            continue
        ret = m.group(1)
        args = m.group(3).strip()
        params = [] if args in ("", "void") else [p for a in args.split(",") for p in parse_declarators(a.strip())]
        functions[m.group(2)] = ((" ".join(ret.replace("*", " ").replace("const", " ").split()), "*" in ret), params)
    return dict(constants=constants, structs=structs, functions=functions, leftovers=leftovers, callbacks=callbacks)


def is_pointer_type(t):
    return t in (C.c_void_p, C.c_char_p) or (isinstance(t, type) and issubclass(t, C._Pointer))


def check_type(where, t, base, pointer, length, h, binding, findings, param):
    """one header declarator (field or parameter) against its ctypes type t"""
    if length is not None and not param:                       # an array field: element type x length
        n = int(length) if length.isdigit() else h["constants"].get(length)
        if not (isinstance(t, type) and issubclass(t, C.Array)) or t._length_ != n:
            findings.append(f"{where}: the header has an array of {length}, the binding {t}")
            return
        t = t._type_
    elif length is not None:
        pointer = True                                         # an array parameter is a pointer
    if base in CALLBACKS:
        if t is not C.c_void_p and t is not getattr(binding, CALLBACKS[base]):
            findings.append(f"{where}: the header has the callback {base}, the binding {t}")
    elif pointer:
        if not is_pointer_type(t):
            findings.append(f"{where}: the header has a pointer ({base}*), the binding {t}")
        elif issubclass(t, C._Pointer) and base in binding.STRUCTS and t._type_ is not binding.STRUCTS[base]:
            findings.append(f"{where}: the header points to {base}, the binding to {t._type_.__name__}")
    elif base not in SCALARS:
        findings.append(f"{where}: type {base!r} of the header is not understood")
    elif t is not SCALARS[base]:
        findings.append(f"{where}: the header has {base}, the binding {getattr(t, '__name__', t)}")


def compare(text, binding):
    """every difference between the header text and the binding, as a list of strings"""
    h = parse(text)
    findings = ["header statement not understood: " + s for s in h["leftovers"]]
    # functions
    for name in sorted(set(h["functions"]) ^ set(binding.PROTOTYPES)):
        findings.append(f"{name}: " + ("declared in the header, missing from PROTOTYPES" if name in h["functions"] else "in PROTOTYPES, not in the header"))
    for name, ((rbase, rptr), params) in h["functions"].items():
        if name not in binding.PROTOTYPES:
            continue
        restype, argtypes = binding.PROTOTYPES[name]
        want = C.c_char_p if (rbase, rptr) == ("char", True) else SCALARS.get(rbase) if not rptr else None
        if restype is not want or want is None:
            findings.append(f"{name}: returns {rbase}{'*' if rptr else ''} in the header, restype is {restype}")
        if len(params) != len(argtypes):
            findings.append(f"{name}: {len(params)} parameters in the header, {len(argtypes)} argtypes")
            continue
        for (pname, base, pointer, length), t in zip(params, argtypes):
            check_type(f"{name}({pname})", t, base, pointer, length, h, binding, findings, param=True)
    for name, params in h["callbacks"].items():
        fn = getattr(binding, CALLBACKS.get(name, ""), None)
        if fn is None or fn._restype_ is not C.c_int or len(fn._argtypes_) != len(params):
            findings.append(f"{name}: callback of the header without a matching CFUNCTYPE")
            continue
        for (pname, base, pointer, length), t in zip(params, fn._argtypes_):
            check_type(f"{name}({pname})", t, base, pointer, length, h, binding, findings, param=True)
    # structs
    for name in sorted(set(h["structs"]) ^ set(binding.STRUCTS)):
        findings.append(f"{name}: " + ("struct of the header without a ctypes class" if name in h["structs"] else "in STRUCTS, not in the header"))
    for name, fields in h["structs"].items():
        if name not in binding.STRUCTS:
            continue
        mine = binding.STRUCTS[name]._fields_
        if [f[0] for f in fields] != [f[0] for f in mine]:
            findings.append(f"{name}: fields {[f[0] for f in fields]} in the header, {[f[0] for f in mine]} in the binding")
            continue
        for (fname, base, pointer, length), (_, t) in zip(fields, mine):
            check_type(f"{name}.{fname}", t, base, pointer, length, h, binding, findings, param=False)
    # constants
    for cname, value in expected_constants(h["constants"], binding, findings).items():
        if cname not in h["constants"]:
            findings.append(f"{cname}: not defined in the header")
        elif h["constants"][cname] != value:
            findings.append(f"{cname}: {h['constants'][cname]} in the header, {value} in the binding")
    return findings


def expected_constants(hc, binding, findings):
    """header name -> the binding's value, for every constant the binding states; whole families of the header (error codes, structure,
    cost, regulariser, hyper-mapping, task and function ids) must be covered"""
    def key(k):
        return k.upper().replace("-", "_")
    out = {"SMASHX_ABI_VERSION": binding.ABI_VERSION, "SMASHX_GNP": binding.GNP, "SMASHX_GNS": binding.GNS,
           "SMASHX_COMM_ID_BYTES": binding.COMM_ID_BYTES, "SMASHX_OK": binding.E_OK, "SMASHX_FN_COUNT": binding.FN_COUNT}
    out.update({"SMASHX_" + k: getattr(binding, k) for k in dir(binding) if k.startswith(("E_", "LBFGSB_")) and k != "E_OK"})
    for table, prefix in ((binding.STRUCTURES, ""), (binding.JOBS_FUN, ""), (binding.JREG_FUN, ""), (binding.HYPER, ""), (binding.FN, "FN_")):
        out.update({"SMASHX_" + prefix + key(k): v for k, v in table.items()})
    for family in (r"SMASHX_E_\w+", r"SMASHX_(GR|VIC)_\w+", r"SMASHX_HYPER_\w+", r"SMASHX_LBFGSB_\w+", r"SMASHX_FN_\w+"):
        for cname in hc:
            if re.fullmatch(family, cname) and cname not in out:
                findings.append(f"{cname}: defined in the header, missing from the binding")
    return out


def _header():
    with open(HEADER) as f:
        return f.read()


def test_parser_sees_every_declaration():
    """counts taken from the header's own text, not from the binding"""
    text = _header()
    h = parse(text)
    assert h["leftovers"] == []
    code = strip(text)[1]
    code = re.sub(r"\btypedef\s+int\s*\(\s*\*\s*\w+\s*\)\s*\([^)]*\)\s*;", " ", code)
    calls = re.findall(r"\bsmashx_[a-z_0-9]+\s*\(", code)
    assert len(calls) == len(h["functions"]) == N_FUNCTIONS, (len(calls), len(h["functions"]))
    assert len(h["structs"]) == len(re.findall(r"\btypedef\s+struct\s*\{", code)) == N_STRUCTS, sorted(h["structs"])
    assert sorted(h["callbacks"]) == sorted(CALLBACKS)
    assert "smashx_plan" not in h["structs"] and "smashx_lbfgsb" not in h["structs"]
    # declarations that name several fields, and the arrays of pointers
    names = [f[0] for f in h["structs"]["smashx_config"]]
    assert names[:3] == ["structure", "nrow", "ncol"] and names[-1] == "tile"
    opt = {f[0]: f for f in h["structs"]["smashx_options"]}
    assert opt["ub_parameters"] == ("ub_parameters", "float", False, "SMASHX_GNP") and opt["ub_states"][3] == "SMASHX_GNS"
    assert h["structs"]["smashx_parameters"] == [("f", "float", True, "SMASHX_GNP")]
    assert h["structs"]["smashx_states"] == [("f", "float", True, "SMASHX_GNS")]
    assert len(h["structs"]["smashx_timing"]) == 24
    enumerators = sum(len([i for i in body.split(",") if i.strip()]) for body in re.findall(r"\benum\s*\{(.*?)\}", code, flags=re.S))
    defines = len(re.findall(r"^[ \t]*#[ \t]*define[ \t]+SMASHX_\w+[ \t]+\S", strip(text)[0], flags=re.M))
    assert len(h["constants"]) == enumerators + defines, (len(h["constants"]), enumerators, defines)


def test_binding_matches_the_header():
    from smash_amd import _lib
    findings = compare(_header(), _lib)
    assert findings == [], "\n".join(findings)
    assert _lib.SYMBOLS == list(_lib.PROTOTYPES)


def _edit(text, old, new):
    assert text.count(old) == 1, old
    return text.replace(old, new)


def test_comparison_bites():
    """three in-memory edits of the header, each of which the comparison must report"""
    from smash_amd import _lib
    text = _header()
    swapped = _edit(_edit(_edit(text, "float cost_ms;", "float @;"), "float route_adj_ms;", "float cost_ms;"), "float @;", "float route_adj_ms;")
    found = compare(swapped, _lib)
    assert found and all("smashx_timing" in f for f in found), found
    widened = _edit(text, "int smashx_sweep(smashx_plan* plan, int adjoint,", "int smashx_sweep(smashx_plan* plan, long long adjoint,")
    found = compare(widened, _lib)
    assert found and all("smashx_sweep(adjoint)" in f for f in found), found
    dropped = _edit(text, "smashx_states* states, float* qsim,\n                    smashx_costs* costs, smashx_states* fstates,",
                    "smashx_states* states,\n                    smashx_costs* costs, smashx_states* fstates,")
    found = compare(dropped, _lib)
    assert found and all("smashx_download" in f for f in found), found


def test_loaded_library_carries_the_table():
    """after lib() every exported function has exactly the table's restype and argtypes: nothing runs on ctypes' defaults"""
    import __graft_entry__
    __graft_entry__.build()
    from smash_amd import _lib
    L = _lib.lib()
    for name, (restype, argtypes) in _lib.PROTOTYPES.items():
        fn = getattr(L, name)
        assert fn.restype is restype, name
        assert fn.argtypes is not None and list(fn.argtypes) == list(argtypes), name
    assert L.smashx_abi_sizes(None) == _lib.ABI_VERSION
