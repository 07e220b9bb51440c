"""The tests' one reader of include/letkf_amd.h: the text without comments, the integer #defines, the declared entries with
return type and parameters, the argument structs field by field, and the layout gcc gives those structs.  Everything is
read once per process."""
import ctypes as C
import functools
import os
import re
import subprocess
import tempfile

from __graft_entry__ import ROOT

INCLUDE = os.path.join(ROOT, "include")
SCALARS = {"int": C.c_int, "int32_t": C.c_int32, "uint32_t": C.c_uint32, "int64_t": C.c_int64, "double": C.c_double}
KINDS = {"i32": C.c_int32, "u32": C.c_uint32, "i64": C.c_int64, "f64": C.c_double, "ptr": C.c_void_p}


@functools.lru_cache(None)
def text():
    """the header without its comments"""
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(INCLUDE, "letkf_amd.h")).read(), flags=re.S)


@functools.lru_cache(None)
def defines():
    """{name: value} of every `#define NAME integer` (negative values stand in parentheses)"""
    return {n: int(v) for n, v in re.findall(r"^#define (\w+) \(?(-?\d+)\)?\s*$", text(), flags=re.M)}


@functools.lru_cache(None)
def entries():
    """{name: (return type, [parameter declaration, ...])} of every function the header declares, in its order"""
    out = {}
    for ret, name, params in re.findall(r"^(int|void|const char \*)\s*(letkf_\w+)\s*\(([^)]*)\)\s*;", text(), flags=re.M):
        out[name] = (ret.strip(), [] if params.strip() == "void" else [" ".join(p.split()) for p in params.split(",")])
    return out


def declared_params(name):
    assert name in entries(), f"{name} not declared"
    return entries()[name][1]


def ctype_of(param):
    """the ctypes type of one C parameter declaration (pointers of any kind as void *)"""
    if "*" in param:
        return C.c_void_p
    return SCALARS[param.replace("const ", "").split()[0]]


def argtypes_of(name):
    return [ctype_of(p) for p in declared_params(name)]


def restype_of(name):
    return {"int": C.c_int, "void": None, "const char *": C.c_char_p}[entries()[name][0]]


@functools.lru_cache(None)
def structs():
    """{name: [(kind, field, count), ...]} for every `typedef struct { ... } name;`: kind in i32 / u32 / i64 / f64 / ptr, count
    the length of an array field (`double tracer_cv[8]`: 8) and None otherwise"""
    out = {}
    for m in re.finditer(r"typedef struct \{(.*?)\}\s*(\w+);", text(), flags=re.S):
        fields = []
        for decl in m.group(1).split(";"):
            decl = decl.strip()
            if not decl:
                continue
            base = re.search(r"\b(uint32_t|int32_t|int64_t|double)\b", decl)
            assert base, decl
            base = {"uint32_t": "u32", "int32_t": "i32", "int64_t": "i64", "double": "f64"}[base.group(1)]
            for part in re.sub(r"\b(const|u?int32_t|int64_t|double)\b", "", decl).split(","):
                name, count = re.fullmatch(r"(\w+)(?:\[(\d+)\])?", part.replace("*", "").strip()).groups()
                fields.append(("ptr" if "*" in part else base, name, int(count) if count else None))
        out[m.group(2)] = fields
    return out


def c_structs():
    """structs() as the Fortran mirror is compared with it: [(kind, field), ...], a uint32_t mask as i32"""
    return {s: [("i32" if k == "u32" else k, n) for k, n, _ in fields] for s, fields in structs().items()}


def field_ctype(kind, count):
    return KINDS[kind] * count if count else KINDS[kind]


@functools.lru_cache(None)
def layout():
    """{struct: (sizeof, {field: offsetof})} as gcc lays the header's structs out: one program for all of them"""
    lines = []
    for s, fields in structs().items():
        lines.append(f'printf("{s} %zu\\n", sizeof({s}));')
        lines += [f'printf("{s}.{n} %zu\\n", offsetof({s}, {n}));' for _, n, _ in fields]
    code = '#include <stdio.h>\n#include <stddef.h>\n#include "letkf_amd.h"\nint main(){' + "".join(lines) + "return 0;}\n"
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "s.c"), os.path.join(d, "s")
        open(src, "w").write(code)
        subprocess.check_call(["gcc", "-I", INCLUDE, src, "-o", exe])
        printed = dict(line.split() for line in subprocess.check_output([exe]).decode().splitlines())
    return {s: (int(printed[s]), {n: int(printed[f"{s}.{n}"]) for _, n, _ in fields}) for s, fields in structs().items()}


def sizeof(struct):
    return layout()[struct][0]


def offsetof(struct, field):
    return layout()[struct][1][field]
