"""The companion header include/letkf_amd_interp.h and its mirrors, without a device: the coarse set of an axis against its
definition, the two exported entries, the ctypes mirror of letkf_interp_args against gcc's layout (a small C program compiled
here), the Fortran BIND(C) type field by field in C order, and the new Fortran module under amdflang."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import pytest

from __graft_entry__ import PKG_DIR, ROOT, load_package

HEADER = os.path.join(ROOT, "include", "letkf_amd_interp.h")
FDIR = os.path.join(PKG_DIR, "fortran")
FC = "/opt/rocm/bin/amdflang"


@pytest.fixture(scope="module")
def pkg():
    p = load_package()
    p.build()
    return p


def header_text():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def header_fields():
    """[(kind, name)] of letkf_interp_args in the header's order"""
    body = re.search(r"typedef struct \{(.*?)\}\s*letkf_interp_args;", header_text(), flags=re.S).group(1)
    out = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        base = {"int32_t": "i32", "int64_t": "i64", "double": "f64"}[re.search(r"\b(int32_t|int64_t|double)\b", decl).group(1)]
        for part in re.sub(r"\b(const|int32_t|int64_t|double)\b", "", decl).split(","):
            out.append(("ptr" if "*" in part else base, part.replace("*", "").strip()))
    return out


@pytest.mark.parametrize("n", [1, 2, 5, 7, 8])
@pytest.mark.parametrize("stride", [1, 2, 3, 4, 8])
def test_coarse_axis_is_the_strided_set_with_the_end(pkg, n, stride):
    want = sorted(set(range(0, n, stride)) | {n - 1})
    assert list(pkg.interp_coarse_axis(n, stride)) == want
    cnt = C.c_int32(-1)
    assert pkg.lib().letkf_interp_coarse_axis(n, stride, None, C.byref(cnt)) == 0 and cnt.value == len(want)


def test_coarse_axis_refuses_bad_arguments(pkg):
    cnt = C.c_int32(-1)
    for n, s in ((0, 1), (5, 0), (-1, 2)):
        assert pkg.lib().letkf_interp_coarse_axis(n, s, None, C.byref(cnt)) == -1


def test_the_library_exports_both_entries_as_the_header_declares_them(pkg):
    decl = dict((name, params) for name, params in re.findall(r"^int\s+(letkf_\w+)\s*\(([^)]*)\)\s*;", header_text(), flags=re.M))
    assert set(decl) == set(pkg.INTERP_ARGTYPES) == {"letkf_interp_coarse_axis", "letkf_das_interp_dev"}
    lib = C.CDLL(pkg.LIB_PATH)
    for name, params in decl.items():
        assert hasattr(lib, name), name
        want = [C.c_void_p if "*" in p else {"int32_t": C.c_int32, "int64_t": C.c_int64}[p.split()[0]] for p in params.split(",")]
        assert pkg.INTERP_ARGTYPES[name] == want, name
        assert getattr(pkg.lib(), name).argtypes == want
    assert int(re.search(r"#define LETKF_AMD_INTERP_VERSION (\d+)", header_text()).group(1)) == pkg.INTERP_VERSION == 1
    assert not set(pkg.INTERP_ARGTYPES) & set(pkg.ARGTYPES)           # the main table stays the main header's
    assert not [a for a in dir(pkg.Context) if a.startswith("OPT_") and "INTERP" in a]


def test_ctypes_mirror_has_gccs_layout(pkg):
    fields = header_fields()
    kinds = {"i32": C.c_int32, "i64": C.c_int64, "f64": C.c_double, "ptr": C.c_void_p}
    assert [(n, kinds[kd]) for kd, n in fields] == list(pkg.InterpArgs._fields_)
    names = [n for _, n in fields]
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "letkf_amd_interp.h"\nint main(void) {\n'
           '  printf("%zu\\n", sizeof(letkf_interp_args));\n' +
           "".join(f'  printf("%zu\\n", offsetof(letkf_interp_args, {n}));\n' for n in names) + "  return 0;\n}\n")
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "layout.c"), "w").write(src)
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(d, "layout.c"),
                               "-o", os.path.join(d, "layout")])
        out = [int(v) for v in subprocess.check_output([os.path.join(d, "layout")], text=True).split()]
    assert out[0] == C.sizeof(pkg.InterpArgs)
    assert out[1:] == [getattr(pkg.InterpArgs, n).offset for n in names]


def fortran_fields(src):
    body = re.search(r"TYPE, BIND\(C\) :: letkf_interp_args\n(.*?)END TYPE", src, flags=re.S).group(1)
    out = []
    for line in body.splitlines():
        line = line.split("!")[0]
        if "::" not in line:
            continue
        decl, names = line.split("::")
        kind = "i32" if "c_int32_t" in decl else "i64" if "c_int64_t" in decl else "f64" if "c_double" in decl else "ptr"
        out += [(kind, n.strip()) for n in names.split(",")]
    return out


def test_fortran_type_lists_the_fields_in_c_order():
    src = open(os.path.join(FDIR, "letkf_interp_amd.f90")).read()
    assert fortran_fields(src) == header_fields()
    assert set(re.findall(r"BIND\(C, name='(letkf_\w+)'\)", src)) == {"letkf_interp_coarse_axis", "letkf_das_interp_dev"}
    assert re.search(r"SUBROUTINE das_letkf_interp_amd\(ctx, args, tables, nx, ny, nlev, stride_x, stride_y", src)


@pytest.mark.skipif(not os.path.exists(FC), reason="amdflang not present")
def test_the_fortran_module_compiles_with_amdflang():
    with tempfile.TemporaryDirectory() as d:
        for f in ("letkf_amd_api.f90", "letkf_interp_amd.f90"):
            subprocess.check_call([FC, "-O2", "-fPIC", "-c", os.path.join(FDIR, f), "-o", os.path.join(d, f[:-4] + ".o")], cwd=d)
        assert os.path.exists(os.path.join(d, "letkf_interp_amd.mod"))
