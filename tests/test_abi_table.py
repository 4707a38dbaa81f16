"""CPU (no GPU needed): pdp_amd/abi.py - the one Python mirror of the C ABI - held against include/*.h, parsed once: the names every header declares, every prototype
argument by argument, every struct field by field, every integer constant, and the symbols the built libraries export.  The parser is as small as the headers allow
and refuses what it does not understand: a header that defeats it fails these tests, it is never skipped."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
SCALARS = {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64, "double": C.c_double}
FLOAT = r"-?\d+\.\d*(?:[eE][-+]?\d+)?"


def parse_header(text):
    """dict(defines {name: int}, structs {pdp_x: [(field, base type, pointer?, array length or None)]}, prototypes {pdp_f: ((base, pointer?), [(base, pointer?), ...])},
    calls: the set of pdp_* names followed by a parenthesis - what the per-feature tests used to collect)"""
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    defines = {}
    for name, value in re.findall(r"^[ \t]*#[ \t]*define[ \t]+(PDP_\w+)(.*)$", code, flags=re.M):
        value = value.strip()
        if re.fullmatch(r"\(?-?\d+\)?", value):
            defines[name] = int(value.strip("()"))
        else:
            assert value == "" or re.fullmatch(FLOAT, value), "#define %s %s: neither an include guard, an integer nor a float" % (name, value)
    structs = {}

    def one_struct(match):
        fields = []
        for decl in filter(None, (d.strip() for d in match.group(1).split(";"))):
            base, rest = re.fullmatch(r"(?:const\s+)?(\w+)\b(.*)", decl, flags=re.S).groups()
            for d in rest.split(","):
                stars, field, length = re.fullmatch(r"\s*(\**)\s*(\w+)\s*(?:\[(\d+)\])?\s*", d).groups()
                fields.append((field, base, bool(stars), int(length) if length else None))
        structs[match.group(2)] = fields
        return ""
    code = re.sub(r"typedef\s+struct\s*\w*\s*\{(.*?)\}\s*(pdp_\w+)\s*;", one_struct, code, flags=re.S)
    code = re.sub(r"^[ \t]*#.*$", "", code, flags=re.M).replace('extern "C" {', "")

    def one_type(text):                                                             # "const double* x" -> ("double", True); "int B" -> ("int", False); "void" -> ("void", False)
        base = re.fullmatch(r"\s*(?:const\s+)?(\w+)\b[\w\s\*]*", text).group(1)
        return base, "*" in text
    prototypes = {}
    for statement in filter(None, (s.strip(" \t\n}") for s in code.split(";"))):
        ret, name, params = re.fullmatch(r"([\w\s\*]+?)\b(pdp_\w+)\s*\((.*)\)", statement, flags=re.S).groups()
        assert name not in prototypes, name
        prototypes[name] = (one_type(ret), [] if params.strip() == "void" else [one_type(q) for q in params.split(",")])
    return dict(defines=defines, structs=structs, prototypes=prototypes, calls=set(re.findall(r"\b(pdp_[a-z0-9_]+)\s*\(", code)))


@pytest.fixture(scope="module")
def headers():
    return {f: parse_header(open(os.path.join(INCLUDE, f)).read()) for f in sorted(os.listdir(INCLUDE))}


@pytest.fixture(scope="module")
def abi():
    from pdp_amd import abi
    return abi


def mirror(abi, struct):
    return getattr(abi, "".join(w.capitalize() for w in struct.split("_")))         # pdp_oc_ms_opts -> PdpOcMsOpts


def agrees(abi, base, pointer, ctype):
    """int, int32_t, int64_t and double exactly (void: None); char* is c_char_p; a pointer to a pdp_* struct is POINTER of its mirror; any other pointer is c_void_p
    or some POINTER"""
    if not pointer:
        return ctype is None if base == "void" else ctype is SCALARS[base]
    if base == "char":
        return ctype is C.c_char_p
    if base.startswith("pdp_"):
        return ctype is C.POINTER(mirror(abi, base))
    return ctype is C.c_void_p or (isinstance(ctype, type) and issubclass(ctype, C._Pointer))


def test_every_header_is_in_the_table_with_the_names_it_declares(headers, abi):
    assert set(headers) == set(abi.ENTRY_POINTS)
    for h, parsed in headers.items():
        assert list(parsed["prototypes"]) == list(abi.entry_points(h)), h           # the same names in the header's order
        assert set(parsed["prototypes"]) == parsed["calls"], h                     # (and the parser missed nothing that looks like a declaration)
        for library, table in abi.ENTRY_POINTS[h]:
            assert library in ("core", "model") and table
    assert len(headers["pdp_hip.h"]["prototypes"]) == 33                            # include/pdp_hip.h stays pinned: new entry points come in extension headers
    every = [name for h in headers for name in abi.entry_points(h)]
    assert len(every) == len(set(every)) == len(abi.entry_points())           # pairwise disjoint
    assert set(abi.entry_points(library="core")) | set(abi.entry_points(library="model")) == set(every)
    assert not set(abi.entry_points(library="core")) & set(abi.entry_points(library="model"))
    assert [library for library, _ in abi.ENTRY_POINTS["pdp_hip.h"]] == ["core", "model"] and "pdp_cp_grad_contract_batched" in abi.entry_points("pdp_hip.h", "core")
    assert list(abi.entry_points("pdp_hip_lm_prior.h", "core")) == ["pdp_lm_update_prior_batched", "pdp_lm_covariance_batched"] and not abi.entry_points("pdp_hip_lm.h", "model")


def test_every_prototype_agrees_with_the_table_argument_by_argument(headers, abi):
    checked = 0
    for h, parsed in headers.items():
        table = abi.entry_points(h)
        for name, ((rbase, rpointer), params) in parsed["prototypes"].items():
            restype, argtypes = table[name]
            assert agrees(abi, rbase, rpointer, restype), (name, "returns", rbase, restype)
            assert len(argtypes) == len(params), (name, len(argtypes), len(params))
            for k, ((base, pointer), ctype) in enumerate(zip(params, argtypes)):
                assert agrees(abi, base, pointer, ctype), (name, k, base, pointer, ctype)
                checked += 1
    assert checked > 400                                                           # (41 prototypes, 406 parameters today)


def test_every_struct_agrees_with_its_mirror_field_by_field(headers, abi):
    structs = {name: fields for parsed in headers.values() for name, fields in parsed["structs"].items()}
    mirrors = {k for k, v in vars(abi).items() if isinstance(v, type) and issubclass(v, C.Structure)}
    assert len(structs) == sum(len(parsed["structs"]) for parsed in headers.values())
    assert {mirror(abi, name).__name__ for name in structs} == mirrors
    for name, fields in structs.items():
        got = mirror(abi, name)._fields_
        assert [f[0] for f in fields] == [f[0] for f in got], name
        for (field, base, pointer, length), (_, ctype) in zip(fields, got):
            if length is not None:                                                  # an array of scalars: element type and length
                assert not pointer and issubclass(ctype, C.Array) and ctype._type_ is SCALARS[base] and ctype._length_ == length, (name, field)
            elif not pointer and base.startswith("pdp_"):                           # a struct by value
                assert ctype is mirror(abi, base), (name, field)
            else:
                assert agrees(abi, base, pointer, ctype) and not (pointer and base.startswith("pdp_")), (name, field, base, ctype)


def test_every_integer_constant_is_the_headers_define(headers, abi):
    defines = {}
    for parsed in headers.values():
        assert not set(parsed["defines"]) & set(defines)
        defines.update(parsed["defines"])
    mine = {k: v for k, v in vars(abi).items() if k.startswith("PDP_") and k.isupper() and isinstance(v, int)}
    assert mine == defines and len(defines) >= 42
    assert sorted(abi.PDP_E) == [-4, -3, -2, -1] and all(abi.PDP_E[defines[k]].startswith(k + " ") for k in ("PDP_E_ARG", "PDP_E_SIZE", "PDP_E_LAUNCH", "PDP_E_MODE"))
    lm = sorted((v, k[len("PDP_LM_"):]) for k, v in headers["pdp_hip_lm.h"]["defines"].items() if k.startswith("PDP_LM_"))
    assert [v for v, _ in lm] == list(range(6)) and abi.LM_STATES == [k for _, k in lm] == ["START", "ACTIVE", "CONVERGED", "STALLED", "BUDGET", "FAILED"]


def test_runtime_binds_from_the_table_and_still_exports_what_callers_use(abi):
    from pdp_amd import runtime
    for name in ("PdpMat", "PdpLqrProblem", "PdpModelInfo", "PdpOcAuxsys", "PdpOcSolveOpts", "PdpOcMsOpts", "PdpOcSensOut", "PdpLmSchedule", "PdpLmState", "PdpLmPrior",
                 "PdpPolicy", "PDP_E", "LM_STATES"):
        assert getattr(runtime, name) is getattr(abi, name), name
    pol = runtime.make_policy("mlp", layers=[3, 2])
    assert (pol.kind, runtime.make_policy("poly", pivots=[0.0, 1.0]).kind) == (abi.PDP_POLICY_MLP, abi.PDP_POLICY_POLY)


def test_the_built_libraries_export_the_names_the_table_gives_them(abi):
    import __graft_entry__ as g
    g.build()
    from pdp_amd import codegen, runtime, zoo
    core_names, model_names = abi.entry_points(library="core"), abi.entry_points(library="model")
    core = runtime.load_core()
    for name, (restype, argtypes) in core_names.items():
        fn = getattr(core, name)                                                   # (AttributeError: not exported)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes), name
    assert b"gfx950" in core.pdp_hip_version()
    assert not [name for name in model_names if hasattr(C.CDLL(codegen.CORE_LIB_PATH), name)]
    for kind, value in (("irl", abi.PDP_KIND_OC), ("oc", abi.PDP_KIND_CP), ("sysid", abi.PDP_KIND_SYSID)):      # an OC, a ControlPlanning and a SysID model
        path = codegen.build_problem(zoo.make_problem("cartpole", kind))[0]
        raw = C.CDLL(path)
        assert not [name for name in model_names if not hasattr(raw, name)], kind
        assert not [name for name in core_names if hasattr(raw, name)], kind
        mdl = runtime.load_model(path)
        assert mdl.kind == value
        for name, (restype, argtypes) in model_names.items():
            fn = getattr(mdl.lib, name)
            assert fn.restype is restype and list(fn.argtypes) == list(argtypes), (kind, name)
