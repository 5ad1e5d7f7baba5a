"""camouflage_multimodal_amd/_lib.py restates the C headers under include/; this file holds the restatement to their text (CPU only,
needs the built library for the export check).

Per header: every `ret camo_name(args);` declaration is parsed from the comment-stripped text and compared with _lib.PROTOTYPES --
the names, the return type and every argument, by KIND (class, size, signedness; pointee of a pointer), not by ctypes class identity
(on Linux c_int32 is c_int and c_uint64 is c_size_t).  Once: the four struct typedefs against their mirrors' _fields_, the mirrored
constants against the headers' macros and enumerators, the comparison itself against three deliberate mistakes, and the stub that
INTEGRATION.md 4 tells an integrator to copy against the ABI version and CamoDims.
"""
import ctypes as C
import functools
import glob
import os
import re

import pytest

from camouflage_multimodal_amd import _lib
from conftest import ROOT

HEADERS = sorted(os.path.basename(p) for p in glob.glob(os.path.join(ROOT, "include", "*.h")))
MIRRORS = {"camo_dims_t": _lib.CamoDims, "camo_rg_dims_t": _lib.CamoRgDims, "camo_options_t": _lib.CamoOptions, "camo_plan_t": _lib.CamoPlan}
# C scalar -> (class, bytes): i signed integer, u unsigned integer, f floating point
SCALARS = {"int": ("i", 4), "int32_t": ("i", 4), "int64_t": ("i", 8), "uint8_t": ("u", 1), "uint32_t": ("u", 4), "uint64_t": ("u", 8),
           "size_t": ("u", C.sizeof(C.c_void_p)), "float": ("f", 4), "double": ("f", 8)}
# constant of _lib -> the macro or enumerator it mirrors (RG_NPARAMS, RGT_NGRADS and RGB_VAR_BOUND are expressions in the headers:
# test_host_logic.py, test_rg_train.py and test_rg_batch.py hold those)
CONSTANTS = {n: "CAMO_" + n for n in (
    "ABI_VERSION", "FWD_INFERENCE", "FLAG_ATTN_MAPS", "FWD_FUSED_MAPS", "SUMSQ_FLOATS", "FUSION_CROSS_ATTENTION", "FUSION_LATE", "PREC_F32",
    "PREC_BF16", "NPARAMS_CROSS", "NPARAMS_LATE", "CALL_FORWARD", "CALL_BACKWARD", "CALL_TRAIN", "RG_MAX_LABELS", "RGB_TILE_SLOTS", "RGD_NPARAMS",
    "RGD_MAX_CHANNELS", "RGD_FIX_BITS")}

# a declaration starts where the previous one, a struct / enum or `extern "C" {` ended
DECL = re.compile(r"(?<=[;{}])\s*((?:const\s+)?\w+[\s*]+)(camo_[a-z_0-9]+)\s*\(([^()]*)\)\s*;")
STRUCT = re.compile(r"\btypedef\s+struct\s+\w+\s*\{([^{}]*)\}\s*(\w+)\s*;")


@functools.lru_cache(maxsize=None)
def code(header):
    """The header without its comments."""
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    return re.sub(r"//[^\n]*", " ", text)


def c_kind(ctype):
    """Kind of a C type as written ("const float* const*", "int32_t", "camo_dims_t*")."""
    t = re.sub(r"\bconst\b", "", ctype).replace(" ", "").replace("\t", "").replace("\n", "")
    base, stars = t.rstrip("*"), len(t) - len(t.rstrip("*"))
    if stars == 0:
        return ("void",) if base == "void" else SCALARS[base]
    if base == "char" and stars == 1:
        return ("str",)
    if stars == 1 and base in MIRRORS:
        return ("ptr", MIRRORS[base])
    assert not base.endswith("_t") or base in SCALARS, f"{ctype}: a struct without a mirror"
    return ("ptr", SCALARS.get(base) if stars == 1 else None)


def py_kind(t):
    """Kind of a ctypes restype / argtype."""
    if t is None:
        return ("void",)
    if t is C.c_char_p:
        return ("str",)
    if t is C.c_void_p:
        return ("ptr", None)
    if isinstance(t, type) and issubclass(t, C._Pointer):
        return ("ptr", t._type_ if issubclass(t._type_, C.Structure) else py_kind(t._type_))
    code_ = t._type_
    assert isinstance(code_, str) and code_ in "bhilqBHILQfd", t
    return ("f" if code_ in "fd" else "i" if code_.islower() else "u", C.sizeof(t))


def agree(c, py):
    """Does the ctypes kind `py` bind the C kind `c`?  A struct pointer takes POINTER of its mirror; any other pointer takes c_void_p or
    POINTER of the pointee's scalar; everything else takes its own kind."""
    if c[0] != "ptr" or py[0] != "ptr" or (isinstance(c[1], type) or isinstance(py[1], type)):
        return c == py
    return py[1] is None or py[1] == c[1]


def split_type(arg):
    m = re.fullmatch(r"\s*(.*?[\s*])(\w+)\s*", arg, re.S)
    assert m, f"unnamed or unparsed argument {arg!r}"
    return m.group(1)


def declarations(header):
    """[(name, return type, [argument types])] of every function the header declares, in its order, as C text."""
    out = []
    for ret, name, args in DECL.findall(";" + "\n".join(l for l in code(header).split("\n") if not l.lstrip().startswith("#"))):
        out.append((name, ret, [] if args.strip() in ("", "void") else [split_type(a) for a in args.split(",")]))
    return out


def mismatches(decl, entry):
    """What is wrong with one PROTOTYPES entry against the parsed declaration of the same function ([] = nothing)."""
    (name, ret, args), (pname, restype, argtypes) = decl, entry
    bad = [] if name == pname else [f"{pname} in the place of {name}"]
    if not agree(c_kind(ret), py_kind(restype)):
        bad.append(f"{name}: returns {ret.strip()}, bound as {restype}")
    if len(args) != len(argtypes):
        bad.append(f"{name}: {len(args)} arguments, {len(argtypes)} bound")
    for i, (a, t) in enumerate(zip(args, argtypes)):
        if not agree(c_kind(a), py_kind(t)):
            bad.append(f"{name}: argument {i} is {a.strip()}, bound as {t}")
    return bad


@pytest.mark.parametrize("header", HEADERS)
def test_prototypes_are_the_headers_declarations(header):
    assert header in _lib.PROTOTYPES, f"include/{header} has no entry in _lib.PROTOTYPES"
    table, decls = _lib.PROTOTYPES[header], declarations(header)
    assert len(decls) == len(re.findall(r"\b(camo_[a-z_0-9]+)\s*\(", code(header))), "the strict parser skipped a declaration"
    names = [d[0] for d in decls]
    assert set(names) == set(_lib.symbols(header)) and len(names) == len(table) == len(set(names)), set(names) ^ set(_lib.symbols(header))
    assert names == list(_lib.symbols(header)), "the table keeps the header's order"
    bad = [b for d, e in zip(decls, table) for b in mismatches(d, e)]
    assert not bad, "\n".join(bad)
    assert os.path.exists(_lib.LIB_PATH), "run `python -m camouflage_multimodal_amd.build` first"
    raw = C.CDLL(_lib.LIB_PATH)
    for s in names:
        assert hasattr(raw, s), f"{s} is declared and not exported"


def test_the_table_covers_the_headers_and_nothing_else():
    assert list(_lib.PROTOTYPES) and set(_lib.PROTOTYPES) == set(HEADERS)
    every = [n for h in _lib.PROTOTYPES for n in _lib.symbols(h)]
    assert len(every) == len(set(every))
    assert _lib.SYMBOLS == _lib.symbols("camo_fusion.h")


def test_struct_mirrors_are_the_headers_structs():
    found = {}
    for header in HEADERS:
        for body, name in STRUCT.findall(code(header)):
            fields = []
            for member in filter(None, (m.strip() for m in body.split(";"))):
                m = re.fullmatch(r"(\w+[\s*]+)(\w+(?:\s*,\s*\w+)*)", member, re.S)            # `int32_t front, front_rt`
                assert m, member
                names = re.split(r"\s*,\s*", m.group(2))
                assert len(names) == 1 or "*" not in m.group(1), member                       # (a star binds to one name only)
                fields += [(n, m.group(1)) for n in names]
            assert name not in found
            found[name] = fields
    assert set(found) == set(MIRRORS)
    for name, mirror in MIRRORS.items():
        assert [n for n, _ in found[name]] == [f[0] for f in mirror._fields_], name
        for (n, ctype), (_, t) in zip(found[name], mirror._fields_):
            assert agree(c_kind(ctype), py_kind(t)), (name, n, ctype, t)
    assert C.sizeof(_lib.CamoDims) == 40 and _lib.CamoDims.options.offset == 32               # LP64: 7 x 4 bytes, padding, the pointer


def header_constants():
    """{macro or enumerator: int} of every header; None where the value is not an integer literal, a (1 << n) or a count up from one."""
    def literal(s):
        m = re.fullmatch(r"\(\s*1\s*<<\s*(\d+)\s*\)", s)
        return 1 << int(m.group(1)) if m else int(s) if re.fullmatch(r"-?\d+", s) else None
    vals = {}
    for header in HEADERS:
        for name, value in re.findall(r"^[ \t]*#[ \t]*define[ \t]+(CAMO_\w+)[ \t]+(\S.*?)[ \t]*$", code(header), re.M):
            assert name not in vals, name
            vals[name] = literal(value)
        for body in re.findall(r"\benum\s*\w*\s*\{([^{}]*)\}", code(header)):
            nxt = 0
            for item in filter(None, (i.strip() for i in body.split(","))):
                name, eq, expr = (s.strip() for s in item.partition("="))
                assert name not in vals, name
                vals[name] = literal(expr) if eq else nxt
                nxt = None if vals[name] is None else vals[name] + 1
    return vals


def test_constants_are_the_headers_values():
    vals = header_constants()
    for py, c in CONSTANTS.items():
        assert c in vals, f"{c} is in no header"
        assert vals[c] is not None, f"{c} is neither an integer literal nor (1 << n)"
        assert getattr(_lib, py) == vals[c], (py, getattr(_lib, py), vals[c])
    assert vals["CAMO_RGD_MAX_PIXELS"] == 1 << 30 and vals["CAMO_E_HIP"] == -4 and vals["CAMO_RGT_NGRADS"] is None     # the parser itself


def test_the_comparison_reports_a_wrong_entry():
    """No library call is made with the wrong types: the entries below are copies that are only compared."""
    header, name = "camo_rg_train_bn.h", "camo_rg_loss_backward_bn"
    decl = next(d for d in declarations(header) if d[0] == name)
    _, restype, argtypes = entry = next(e for e in _lib.PROTOTYPES[header] if e[0] == name)
    assert len(argtypes) == 27 and mismatches(decl, entry) == []
    rg, i32, f32 = C.POINTER(_lib.CamoRgDims), C.c_int32, C.c_float
    assert argtypes[0] is rg and argtypes[1] is i32 and argtypes[16] is f32
    dropped = mismatches(decl, (name, restype, argtypes[:5] + argtypes[6:]))
    assert any("27 arguments, 26 bound" in b for b in dropped)
    assert mismatches(decl, (name, restype, argtypes[:1] + (f32,) + argtypes[2:])) == [f"{name}: argument 1 is int32_t, bound as {f32}"]
    assert mismatches(decl, (name, restype, argtypes[:16] + (i32,) + argtypes[17:])) == [f"{name}: argument 16 is float, bound as {i32}"]
    other = C.POINTER(_lib.CamoDims)
    assert mismatches(decl, (name, restype, (other,) + argtypes[1:])) == [f"{name}: argument 0 is const camo_rg_dims_t*, bound as {other}"]
    assert mismatches(decl, (name, restype, (C.c_void_p,) + argtypes[1:]))                    # a struct pointer is held to its mirror
    assert mismatches(decl, (name, C.c_size_t, argtypes)) and mismatches(decl, (name, C.c_uint32, argtypes))
    assert mismatches(decl, (name, restype, argtypes[:11] + (C.c_int64,) + argtypes[12:]))     # the size of an integer
    assert mismatches(decl, (name, restype, argtypes[:2] + (C.POINTER(i32),) + argtypes[3:]))  # const float* const* is no int32_t*
    assert mismatches(decl, ("camo_rg_loss_backward", restype, argtypes))


def test_the_documented_stub_is_the_current_abi():
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    section = doc.split("\n## 4. ")[1].split("\n## 5. ")[0]
    block = section.split("```python\n")[1].split("```")[0]
    stated = re.search(r"camo_abi_version\(\)\s*==\s*(\d+)", block)
    assert stated and int(stated.group(1)) == _lib.ABI_VERSION
    assert f"ABI version {_lib.ABI_VERSION} " in section and not re.search(rf"ABI version (?!{_lib.ABI_VERSION}\b)\d+", section)
    fields = re.search(r"class CamoDims\(C\.Structure\):.*?_fields_ = \[(.*?)\]", block, re.S).group(1)
    stub = re.findall(r'\("(\w+)",\s*C\.(\w+)\)', fields)
    assert [n for n, _ in stub] == [f[0] for f in _lib.CamoDims._fields_]
    for (n, t), (_, mirror) in zip(stub, _lib.CamoDims._fields_):
        a, b = py_kind(mirror), py_kind(getattr(C, t))
        assert a == b or a[0] == b[0] == "ptr", n                                             # (the stub passes no options: a void* will do)
    assert "_lib.PROTOTYPES" in section and "tests/test_abi_binding.py" in section


def test_a_symbol_the_library_lacks_is_named(monkeypatch):
    monkeypatch.setattr(_lib, "_lib", None)                                                   # (bind afresh; the loaded binding comes back afterwards)
    monkeypatch.setitem(_lib.PROTOTYPES, "camo_absent.h", (("camo_absent", C.c_int32, ()),))
    with pytest.raises(_lib.CamoError, match=r"does not export camo_absent \(include/camo_absent\.h\).*rebuild"):
        _lib.lib()
    assert _lib._lib is None
