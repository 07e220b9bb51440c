"""The fourth companion header include/letkf_amd_monit.h and its mirrors, without a device: the ctypes structures against the
header field by field and against gcc's layout, the exported entries and their signature table, the five tables kept apart,
the entries' own host unit behind the exception barrier, the Fortran BIND(C) types in C order, the new Fortran module under
amdflang, and letkf_monit_type against the reference's list."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import _monit as M
from __graft_entry__ import PKG_DIR, ROOT, load_package

HEADER = os.path.join(ROOT, "include", "letkf_amd_monit.h")
FDIR = os.path.join(PKG_DIR, "fortran")
CSRC = os.path.join(PKG_DIR, "csrc")
FC = "/opt/rocm/bin/amdflang"
CTYPE = {"i32": C.c_int32, "i64": C.c_int64, "f64": C.c_double, "ptr": C.c_void_p}
ENTRIES = {"letkf_state_to_history_dev", "letkf_monit_obs_dev", "letkf_monit_type"}
STRUCTS = [("letkf_hist_state", "HistState"), ("letkf_monit_params", "MonitParams"), ("letkf_obsdep", "Obsdep")]


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


@pytest.mark.parametrize("struct,mirror", STRUCTS)
def test_ctypes_mirror_is_the_header_and_has_gccs_layout(pkg, struct, mirror):
    fields = header_fields(struct)
    cls = getattr(pkg, mirror)
    assert [(n, CTYPE[k]) for k, n in fields] == list(cls._fields_)
    names = [n for _, n in fields]
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "letkf_amd_monit.h"\nint main(void) {\n'
           f'  printf("%zu\\n", sizeof({struct}));\n' +
           "".join(f'  printf("%zu\\n", offsetof({struct}, {n}));\n' for n in names) + "  return 0;\n}\n")
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "layout.c"), "w").write(src)
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(d, "layout.c"),
                               "-o", os.path.join(d, "layout")])
        out = [int(v) for v in subprocess.check_output([os.path.join(d, "layout")], text=True).split()]
    assert out[0] == C.sizeof(cls)
    assert out[1:] == [getattr(cls, n).offset for n in names]


def test_the_library_exports_the_entries_as_the_header_declares_them(pkg):
    decl = dict(re.findall(r"^int\s+(letkf_\w+)\s*\(([^)]*)\)\s*;", header_text(), flags=re.M))
    assert set(decl) == set(pkg.MONIT_ARGTYPES) == ENTRIES
    lib = C.CDLL(pkg.LIB_PATH)
    for name, params in decl.items():
        assert hasattr(lib, name), name
        want = [C.c_void_p if "*" in p else {"int32_t": C.c_int32, "int64_t": C.c_int64}[p.split()[0]] for p in params.split(",")]
        assert pkg.MONIT_ARGTYPES[name] == want, name
        assert getattr(pkg.lib(), name).argtypes == want
    assert int(re.search(r"#define LETKF_AMD_MONIT_VERSION (\d+)", header_text()).group(1)) == pkg.MONIT_VERSION == 1
    assert '#include "letkf_amd_obsope.h"' in header_text()
    assert callable(pkg.Context.state_to_history) and callable(pkg.Context.monit_obs) and callable(pkg.monit_type)
    out = subprocess.check_output(["nm", "-D", "--defined-only", pkg.LIB_PATH], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if " T letkf_" in line}
    every = set(pkg.ARGTYPES) | set(pkg.INTERP_ARGTYPES) | set(pkg.INTERP_WINDOW_ARGTYPES) | set(pkg.OBSOPE_ARGTYPES) | ENTRIES
    assert ENTRIES <= exported and exported <= every, sorted(exported - every)


def test_the_five_tables_are_pairwise_disjoint(pkg):
    tables = (pkg.ARGTYPES, pkg.INTERP_ARGTYPES, pkg.INTERP_WINDOW_ARGTYPES, pkg.OBSOPE_ARGTYPES, pkg.MONIT_ARGTYPES)
    for n, a in enumerate(tables):
        for b in tables[n + 1:]:
            assert not set(a) & set(b)
    assert list(pkg.EXPORTS) == list(pkg.ARGTYPES)                  # the main header's list stays the main header's
    main = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "letkf_amd.h")).read(), flags=re.S)
    assert "#define LETKF_AMD_ABI_VERSION 11" in main
    assert not [n for n in ENTRIES if n in main]


def test_each_entry_is_defined_once_in_its_own_host_unit_behind_the_barrier():
    defs = {}
    for f in sorted(os.listdir(CSRC)):
        if not f.endswith(".hip"):
            continue
        src = open(os.path.join(CSRC, f)).read()
        for m in re.finditer(r"^(?:int|void|const char\*) (letkf_\w+)\(([^)]*)\)([^;{]*)\{", src, flags=re.M):
            if m.group(1) in ENTRIES:
                close = re.compile(r"^\}.*$", flags=re.M).search(src, m.end()).group(0)
                defs.setdefault(m.group(1), []).append((f, m.group(3).strip(), close.strip()))
    assert set(defs) == ENTRIES
    for name, where in defs.items():
        assert len(where) == 1, (name, where)
        unit, head, close = where[0]
        assert unit == "letkf_monit_entry.hip" and head == "try" and close == f"}} LETKF_ENTRY_END({name})", (name, where)
    unit = open(os.path.join(CSRC, "letkf_monit_entry.hip")).read()
    assert "__global__" not in unit and "hipLaunchKernelGGL" not in unit
    assert '#include "letkf_api_internal.h"' in unit
    mk = open(os.path.join(PKG_DIR, "Makefile")).read()
    units = re.search(r"^UNITS\s*:=(.*)$", mk, flags=re.M).group(1).split()
    assert "letkf_monit" in units and "letkf_monit_entry" in units
    assert re.search(r"^FLAGS_letkf_monit\s*:=\s*-ffp-contract=off\s*$", mk, flags=re.M)
    assert "letkf_amd_monit.h" in mk and "letkf_monit_dev.h" in mk


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
    src = open(os.path.join(FDIR, "letkf_monit_amd.f90")).read()
    for struct, _ in STRUCTS:
        assert fortran_fields(src, struct) == header_fields(struct)
    assert set(re.findall(r"BIND\(C, name='(letkf_\w+)'\)", src)) == ENTRIES
    assert re.search(r"SUBROUTINE state_to_history_amd\(ctx, st, layout, v3d, v2d, ierr\)", src)
    assert re.search(r"SUBROUTINE monit_obs_amd\(ctx, mprm, prm, nfile, off, elm, typ, lev, ri, rj, dat, fields, nn, key, set, idx, rec, &\n"
                     r"\s+nobs, bias, rmse, monit_type, ierr\)", src)
    assert re.search(r"SUBROUTINE monit_print_amd\(nobs, bias, rmse, monit_type\)", src)
    assert [int(x) for x in re.search(r"elem_uid_monit\(nid_obs_monit\) = &\n\s+\(/([^/]*)/\)", src).group(1).split(",")] == M.ELEM_UID.tolist()
    assert re.findall(r"'([ \w]{3})'", re.search(r"obelmlist\(nid_obs_monit\) = &\n\s+\(/([^/]*)/\)", src).group(1)) == M.OBELMLIST
    drv = open(os.path.join(FDIR, "monit_driver.f90")).read()
    assert drv.index("CALL state_to_history_amd") < drv.index("CALL monit_obs_amd") < drv.index("CALL monit_print_amd")
    assert "monit_driver" in open(os.path.join(FDIR, "Makefile")).read()


@pytest.mark.skipif(not os.path.exists(FC), reason="amdflang not present")
def test_the_fortran_module_compiles_with_amdflang():
    with tempfile.TemporaryDirectory() as d:
        for f in ("letkf_amd_api.f90", "letkf_obsope_amd.f90", "letkf_monit_amd.f90"):
            subprocess.check_call([FC, "-O2", "-fPIC", "-c", os.path.join(FDIR, f), "-o", os.path.join(d, f[:-4] + ".o")], cwd=d)
        assert os.path.exists(os.path.join(d, "letkf_monit_amd.mod"))


@pytest.mark.parametrize("radar,h08", [(0, 0), (1, 0), (0, 1), (1, 1)])
def test_monit_type_is_the_references_list(pkg, radar, h08):
    """common_obs_scale.f90:1821-1837, the names spelled out here: U V T Tv Q PS; + REF RE0 Vr; + H08; RH and PRH never"""
    on = ["  U", "  V", "  T", " Tv", "  Q", " PS"] + (["REF", "RE0", " Vr"] if radar else []) + (["H08"] if h08 else [])
    want = np.array([1 if n in on else 0 for n in M.OBELMLIST], dtype=np.int32)
    got = pkg.monit_type(M.ELEM_UID, radar, h08)
    assert np.array_equal(got, want) and np.array_equal(M.monit_type(M.ELEM_UID, radar, h08), want)
    assert got[M.OBELMLIST.index(" RH")] == 0 and got[M.OBELMLIST.index("PRH")] == 0
    assert np.array_equal(pkg.monit_type(M.ELEM_UID[::-1].copy(), radar, h08), want[::-1])      # by id, not by position
    with pytest.raises(pkg.LetkfError):
        pkg.monit_type(np.zeros(33, dtype=np.int32), radar, h08)
