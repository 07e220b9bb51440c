"""The third companion header include/letkf_amd_obsope.h and its mirrors, without a device: the ctypes structures against the
header field by field and against gcc's layout, the exported entry and its signature table, the four tables kept apart, the
Fortran BIND(C) types in C order, and the new Fortran module under amdflang."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import pytest

from __graft_entry__ import PKG_DIR, ROOT, load_package

HEADER = os.path.join(ROOT, "include", "letkf_amd_obsope.h")
FDIR = os.path.join(PKG_DIR, "fortran")
FC = "/opt/rocm/bin/amdflang"
CTYPE = {"i32": C.c_int32, "i64": C.c_int64, "f64": C.c_double, "ptr": C.c_void_p}


@pytest.fixture(scope="module")
def pkg():
    p = load_package()
    p.build()
    return p


def header_text():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def header_fields(struct):
    body = re.search(r"typedef struct \{([^{}]*)\}\s*" + struct + ";", header_text()).group(1)
    out = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        base = re.match(r"(const\s+)?(int32_t|int64_t|double)\s+", decl)
        assert base, decl
        kind = {"int32_t": "i32", "int64_t": "i64", "double": "f64"}[base.group(2)]
        for name in decl[base.end():].split(","):
            name = name.strip()
            out.append(("ptr", name.lstrip("* ")) if name.startswith("*") else (kind, name))
    return out


@pytest.mark.parametrize("struct,mirror", [("letkf_obsope_fields", "ObsopeFields"), ("letkf_obsope_params", "ObsopeParams")])
def test_ctypes_mirror_is_the_header_and_has_gccs_layout(pkg, struct, mirror):
    fields = header_fields(struct)
    cls = getattr(pkg, mirror)
    assert [(n, CTYPE[k]) for k, n in fields] == list(cls._fields_)
    names = [n for _, n in fields]
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "letkf_amd_obsope.h"\nint main(void) {\n'
           f'  printf("%zu\\n", sizeof({struct}));\n' +
           "".join(f'  printf("%zu\\n", offsetof({struct}, {n}));\n' for n in names) + "  return 0;\n}\n")
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "layout.c"), "w").write(src)
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(d, "layout.c"),
                               "-o", os.path.join(d, "layout")])
        out = [int(v) for v in subprocess.check_output([os.path.join(d, "layout")], text=True).split()]
    assert out[0] == C.sizeof(cls)
    assert out[1:] == [getattr(cls, n).offset for n in names]


def test_the_library_exports_the_entry_as_the_header_declares_it(pkg):
    decl = dict(re.findall(r"^int\s+(letkf_\w+)\s*\(([^)]*)\)\s*;", header_text(), flags=re.M))
    assert set(decl) == set(pkg.OBSOPE_ARGTYPES) == {"letkf_obsope_dev"}
    lib = C.CDLL(pkg.LIB_PATH)
    for name, params in decl.items():
        assert hasattr(lib, name), name
        want = [C.c_void_p if "*" in p else {"int32_t": C.c_int32, "int64_t": C.c_int64}[p.split()[0]] for p in params.split(",")]
        assert pkg.OBSOPE_ARGTYPES[name] == want, name
        assert getattr(pkg.lib(), name).argtypes == want
    assert int(re.search(r"#define LETKF_AMD_OBSOPE_VERSION (\d+)", header_text()).group(1)) == pkg.OBSOPE_VERSION == 1
    assert callable(pkg.Context.obsope)


def test_the_four_tables_are_pairwise_disjoint(pkg):
    tables = (pkg.ARGTYPES, pkg.INTERP_ARGTYPES, pkg.INTERP_WINDOW_ARGTYPES, pkg.OBSOPE_ARGTYPES)
    for n, a in enumerate(tables):
        for b in tables[n + 1:]:
            assert not set(a) & set(b)
    assert list(pkg.EXPORTS) == list(pkg.ARGTYPES)                  # the main header's list stays the main header's
    main = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "letkf_amd.h")).read(), flags=re.S)
    assert "obsope_dev" not in main and "#define LETKF_AMD_ABI_VERSION 11" in main


def fortran_fields(src, name):
    body = re.search(r"TYPE, BIND\(C\) :: " + name + r"\n(.*?)END TYPE", src, flags=re.S).group(1)
    out = []
    for line in body.splitlines():
        line = line.split("!")[0]
        if "::" not in line:
            continue
        decl, names = line.split("::")
        kind = "i32" if "c_int32_t" in decl else "i64" if "c_int64_t" in decl else "f64" if "c_double" in decl else "ptr"
        out += [(kind, n.strip()) for n in names.split(",")]
    return out


def test_fortran_types_list_the_fields_in_c_order():
    src = open(os.path.join(FDIR, "letkf_obsope_amd.f90")).read()
    for struct in ("letkf_obsope_fields", "letkf_obsope_params"):
        assert fortran_fields(src, struct) == header_fields(struct)
    assert set(re.findall(r"BIND\(C, name='(letkf_\w+)'\)", src)) == {"letkf_obsope_dev"}
    assert re.search(r"SUBROUTINE obsope_amd\(ctx, prm, nfile, off, elm, typ, lev, ri, rj, fields, n1, n2, set, idx, qc, ensval", src)
    drv = open(os.path.join(FDIR, "obsope_driver.f90")).read()
    assert drv.index("CALL obsope_amd") < drv.index("CALL set_letkf_obs_amd(ctx")     # the operator reads the files first


@pytest.mark.skipif(not os.path.exists(FC), reason="amdflang not present")
def test_the_fortran_module_compiles_with_amdflang():
    with tempfile.TemporaryDirectory() as d:
        for f in ("letkf_amd_api.f90", "letkf_obsope_amd.f90"):
            subprocess.check_call([FC, "-O2", "-fPIC", "-c", os.path.join(FDIR, f), "-o", os.path.join(d, f[:-4] + ".o")], cwd=d)
        assert os.path.exists(os.path.join(d, "letkf_obsope_amd.mod"))
