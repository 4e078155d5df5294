"""
The ctypes binding (setk_amd/_ffi.py) held to the header it binds (include/setk_hip.h), on the CPU:
every prototype of _ffi.PROTOTYPES against the declaration (argument count, the kind of every
argument, structure pointers by class, the return type), every structure against its typedef
(names, order and kinds of the fields, and sizeof / offsetof as the host compiler lays it out), every
constant against its #define.  A prototype that is one int short or a field out of order otherwise
passes every test without a device and corrupts a call on one.  No device library is loaded.
"""
import ctypes
import os
import re
import subprocess

import pytest

from setk_amd import _ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "setk_hip.h")

SCALARS = {"int": ctypes.c_int, "size_t": ctypes.c_size_t, "long long": ctypes.c_longlong,
           "float": ctypes.c_float, "double": ctypes.c_double}
HANDLES = ("setk_handle_t", "setk_comm_t")
# the #defines that no code of the binding needs
UNBOUND = {"SETK_ABI_VERSION", "SETK_COMM_ID_BYTES", "SETK_COMM_SUM", "SETK_COMM_MAX"}
# name table of the module -> the prefix of its #defines
NAME_TABLES = {"SSL_BACKENDS": "SETK_SSL_", "SPATIAL_KINDS": "SETK_SPATIAL_", "NS_KINDS": "SETK_NS_",
               "KALDI_KINDS": "SETK_KALDI_"}


def _class_of(struct):
    """setk_simu_recipe -> _ffi.SimuRecipe"""
    return getattr(_ffi, "".join(w.capitalize() for w in struct[len("setk_"):].split("_")))


def _is_pointer(t):
    return t in (ctypes.c_void_p, ctypes.c_char_p) or (isinstance(t, type) and issubclass(t, ctypes._Pointer))


def _agrees(decl, t, structs):
    """Whether the ctypes type `t` is the kind the C declaration `decl` (type and stars, no name)
    asks for; None when it is: otherwise what was expected."""
    if "*" in decl or "[" in decl or decl.split()[-1] in HANDLES:
        m = re.fullmatch(r"const (setk_\w+)\s*\*", decl)
        if m and m.group(1) in structs:
            want = ctypes.POINTER(_class_of(m.group(1)))
            return None if t is want else want.__name__
        return None if _is_pointer(t) else "a pointer type"
    assert decl in SCALARS, f"a kind of declaration this test does not know: {decl!r}"
    return None if t is SCALARS[decl] else SCALARS[decl].__name__


@pytest.fixture(scope="module")
def header():
    text = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    protos = {}
    for ret, name, args in re.findall(r"^(const char\s*\*|int)\s+(setk_\w+)\s*\(([^)]*)\)\s*;", text, re.M):
        args = [] if args.strip() == "void" else [" ".join(a.split()) for a in args.split(",")]
        # (type and stars, name): `const float* const* audio`, `int info[3]`
        protos[name] = (re.sub(r"\s*\*", "*", ret),
                        [re.fullmatch(r"(.*?)(\w+)((?:\[\w*\])?)", a).groups() for a in args])
    structs = {}
    for name, body in re.findall(r"typedef struct (setk_\w+) \{(.*?)\}\s*\1\s*;", text, re.S):
        fields = []
        for decl in filter(None, (" ".join(d.split()) for d in body.split(";"))):
            first, *more = [d.strip() for d in decl.split(",")]
            base, field = re.fullmatch(r"(.*?)(\w+)", first).groups()
            fields.append((base.strip(), field))
            for d in more:  # `double alpha, alpha_s`, `const double *w_mcra, *w_local`
                fields.append((base.replace("*", "").strip() + ("*" if d.startswith("*") else ""), d.lstrip("* ")))
        structs[name] = fields
    defines = {name: int(value, 0) for name, value in
               re.findall(r"^#define\s+(SETK_\w+)\s+\(?(-?(?:0x[0-9a-fA-F]+|\d+))\)?\s*$", text, re.M)}
    assert protos and structs and defines, "include/setk_hip.h did not parse"
    return protos, structs, defines


def test_every_prototype_matches_its_declaration(header):
    protos, structs, _ = header
    assert list(_ffi.PROTOTYPES) == list(protos)  # all of them, in the header's order
    assert _ffi.exported_symbols() == list(protos)
    for name, (ret, args) in protos.items():
        restype, argtypes = _ffi.PROTOTYPES[name]
        want = {"const char*": ctypes.c_char_p, "int": ctypes.c_int}[ret]
        assert restype is want, f"{name}: returns {ret}, declared as {restype.__name__}"
        assert len(argtypes) == len(args), f"{name}: {len(argtypes)} argument types, the header has {len(args)}"
        for k, ((decl, arg, dim), t) in enumerate(zip(args, argtypes)):
            want = _agrees(decl.strip() + dim, t, structs)
            assert want is None, f"{name}: argument {k} ({decl}{arg}{dim}) is {t.__name__}, not {want}"


def test_every_structure_matches_its_typedef(header, tmp_path):
    _, structs, _ = header
    assert len(structs) >= 7
    for name, fields in structs.items():
        cls = _class_of(name)
        assert [f for _, f in fields] == [f[0] for f in cls._fields_], f"{name}: field names / order"
        for (decl, field), (_, t) in zip(fields, cls._fields_):
            want = _agrees(decl, t, structs)
            assert want is None, f"{name}.{field} ({decl}) is {t.__name__}, not {want}"
    # the layout as the host compiler of tools/hoststub/build.sh sees it
    lines = ['#include <stdio.h>', '#include "setk_hip.h"', "int main(void) {"]
    for name, fields in structs.items():
        lines.append(f'  printf("{name} %zu\\n", sizeof({name}));')
        lines += [f'  printf("{name}.{f} %zu\\n", offsetof({name}, {f}));' for _, f in fields]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines + ["  return 0;", "}", ""]))
    cc = re.search(r"^(\S+/clang) ", open(os.path.join(ROOT, "tools", "hoststub", "build.sh")).read(), re.M).group(1)
    r = subprocess.run([cc, "-I", os.path.dirname(HEADER), str(src), "-o", str(tmp_path / "layout")],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(tmp_path / "layout")], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    measured = {k: int(v) for k, v in (line.split() for line in r.stdout.splitlines())}
    for name, fields in structs.items():
        cls = _class_of(name)
        assert ctypes.sizeof(cls) == measured[name], f"sizeof({name})"
        for _, f in fields:
            assert getattr(cls, f).offset == measured[f"{name}.{f}"], f"offsetof({name}, {f})"


def test_every_constant_matches_its_define(header):
    _, _, defines = header
    covered = set()
    for name, value in defines.items():  # SETK_OK, SETK_FLAG_BAN -> FLAG_BAN
        for mine in (name, name[len("SETK_"):]):
            if hasattr(_ffi, mine):
                assert getattr(_ffi, mine) == value, f"{name} is {value}, _ffi.{mine} is {getattr(_ffi, mine)}"
                covered.add(name)
    for table, prefix in NAME_TABLES.items():  # SETK_SSL_SRP -> SSL_BACKENDS["srp"]
        theirs = {n: v for n, v in defines.items() if n.startswith(prefix) and n not in covered}
        mine = getattr(_ffi, table)
        assert {prefix + k.upper(): v for k, v in mine.items()} == theirs, f"_ffi.{table} against {prefix}*"
        covered |= set(theirs)
    assert len(covered) >= 20
    assert set(defines) - covered == UNBOUND, "a #define without a counterpart in _ffi.py"
