"""The tests' one reader of the headers under include/ (letkf_amd.h unless another is named): the text without comments, the
integer #defines, the declared entries with return type and parameters, the argument structs field by field, and the layout
gcc gives those structs -- each read once per header and process.  Beside it the readers of the headers' three mirrors: the
BIND(C) types of a Fortran module, the symbols a built library exports, and the entries' definitions in the csrc units."""
import ctypes as C
import functools
import os
import re
import subprocess
import tempfile

from __graft_entry__ import PKG_DIR, ROOT

INCLUDE = os.path.join(ROOT, "include")
CSRC = os.path.join(PKG_DIR, "csrc")
MAIN = "letkf_amd.h"
SCALARS = {"int": C.c_int, "int32_t": C.c_int32, "uint32_t": C.c_uint32, "int64_t": C.c_int64, "double": C.c_double}
KINDS = {"i32": C.c_int32, "u32": C.c_uint32, "i64": C.c_int64, "f64": C.c_double, "f32": C.c_float, "ptr": C.c_void_p}
BASES = {"uint32_t": "u32", "int32_t": "i32", "int64_t": "i64", "double": "f64", "float": "f32"}


@functools.lru_cache(None)
def text(header=MAIN):
    """the header without its comments"""
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(INCLUDE, header)).read(), flags=re.S)


@functools.lru_cache(None)
def defines(header=MAIN):
    """{name: value} of every `#define NAME integer` (negative values stand in parentheses)"""
    return {n: int(v) for n, v in re.findall(r"^#define (\w+) \(?(-?\d+)\)?\s*$", text(header), flags=re.M)}


@functools.lru_cache(None)
def entries(header=MAIN):
    """{name: (return type, [parameter declaration, ...])} of every function the header declares, in its order"""
    out = {}
    for ret, name, params in re.findall(r"^(int|void|const char \*)\s*(letkf_\w+)\s*\(([^)]*)\)\s*;", text(header), flags=re.M):
        out[name] = (ret.strip(), [] if params.strip() == "void" else [" ".join(p.split()) for p in params.split(",")])
    return out


def declared_params(name, header=MAIN):
    assert name in entries(header), f"{name} not declared"
    return entries(header)[name][1]


def ctype_of(param):
    """the ctypes type of one C parameter declaration (pointers of any kind as void *)"""
    if "*" in param:
        return C.c_void_p
    return SCALARS[param.replace("const ", "").split()[0]]


def argtypes_of(name, header=MAIN):
    return [ctype_of(p) for p in declared_params(name, header)]


def restype_of(name, header=MAIN):
    return {"int": C.c_int, "void": None, "const char *": C.c_char_p}[entries(header)[name][0]]


@functools.lru_cache(None)
def structs(header=MAIN):
    """{name: [(kind, field, count), ...]} for every `typedef struct { ... } name;`: kind in i32 / u32 / i64 / f64 / f32 / ptr,
    count the length of an array field (`double tracer_cv[8]`: 8) and None otherwise"""
    out = {}
    for m in re.finditer(r"typedef struct \{(.*?)\}\s*(\w+);", text(header), flags=re.S):
        fields = []
        for decl in m.group(1).split(";"):
            decl = decl.strip()
            if not decl:
                continue
            base = re.search(r"\b(" + "|".join(BASES) + r")\b", decl)
            assert base, decl
            for part in re.sub(r"\b(const|" + "|".join(BASES) + r")\b", "", decl).split(","):
                name, count = re.fullmatch(r"(\w+)(?:\[(\d+)\])?", part.replace("*", "").strip()).groups()
                fields.append(("ptr" if "*" in part else BASES[base.group(1)], name, int(count) if count else None))
        out[m.group(2)] = fields
    return out


def c_structs(header=MAIN):
    """structs() as a Fortran mirror is compared with it (fortran_types): a uint32_t mask as i32"""
    return {s: [("i32" if k == "u32" else k, n, c) for k, n, c in fields] for s, fields in structs(header).items()}


def field_ctype(kind, count):
    return KINDS[kind] * count if count else KINDS[kind]


@functools.lru_cache(None)
def layout(header=MAIN):
    """{struct: (sizeof, {field: offsetof})} as gcc lays the header's structs out: one program for all of them"""
    lines = []
    for s, fields in structs(header).items():
        lines.append(f'printf("{s} %zu\\n", sizeof({s}));')
        lines += [f'printf("{s}.{n} %zu\\n", offsetof({s}, {n}));' for _, n, _ in fields]
    code = f'#include <stdio.h>\n#include <stddef.h>\n#include "{header}"\nint main(void){{' + "".join(lines) + "return 0;}\n"
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "s.c"), os.path.join(d, "s")
        open(src, "w").write(code)
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", INCLUDE, src, "-o", exe])
        printed = dict(line.split() for line in subprocess.check_output([exe]).decode().splitlines())
    return {s: (int(printed[s]), {n: int(printed[f"{s}.{n}"]) for _, n, _ in fields}) for s, fields in structs(header).items()}


def sizeof(struct, header=MAIN):
    return layout(header)[struct][0]


def offsetof(struct, field, header=MAIN):
    return layout(header)[struct][1][field]


def fortran_types(src):
    """{name: [(kind, field, count), ...]} for every `TYPE, BIND(C) :: name` of a Fortran source, as c_structs() gives them"""
    out = {}
    for m in re.finditer(r"TYPE, BIND\(C\) :: (\w+)\n(.*?)END TYPE", src, flags=re.S):
        fields = []
        for line in re.sub(r"&\s*\n", " ", m.group(2)).splitlines():
            line = line.split("!")[0]
            if "::" not in line:
                continue
            decl, names = line.split("::")
            kind = [k for k, t in (("i32", "c_int32_t"), ("i64", "c_int64_t"), ("f64", "c_double"), ("f32", "c_float"),
                                   ("ptr", "c_ptr")) if t in decl]
            assert len(kind) == 1, line
            for n in names.split(","):
                name, count = re.fullmatch(r"(\w+)(?:\((\d+)\))?", n.strip()).groups()
                fields.append((kind[0], name, int(count) if count else None))
        out[m.group(1)] = fields
    return out


def exported(lib_path):
    """the letkf_* functions a built library defines and exports"""
    out = subprocess.check_output(["nm", "-D", "--defined-only", lib_path], text=True)
    return {line.split()[-1] for line in out.splitlines() if " T letkf_" in line}


@functools.lru_cache(None)
def definitions(csrc=CSRC):
    """{entry: [(unit, head, close), ...]}: every definition of a letkf_* function at file level in the .hip and .cpp units --
    what stands between its parameter list and its body, and the line that closes the body"""
    out = {}
    for unit in sorted(os.listdir(csrc)):
        if not unit.endswith((".hip", ".cpp")):
            continue
        src = open(os.path.join(csrc, unit)).read()
        for m in re.finditer(r'^(?:extern "C" )?(?:int|void|const char\*) (letkf_\w+)\(([^)]*)\)([^;{]*)\{', src, flags=re.M):
            close = re.compile(r"^\}.*$", flags=re.M).search(src, m.end()).group(0)
            out.setdefault(m.group(1), []).append((unit, m.group(3).strip(), close.strip()))
    return out
