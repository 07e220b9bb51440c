"""The twelfth companion header include/letkf_amd_tcvital.h and its mirrors, without a device: the checks
tests/test_nobsout_binding.py makes for the eleventh, made here for this one with the same readers (tests/_header.py) -- its units
lie in csrc/tcvital/ and its library and driver hang on goals of their own (DESIGN.md sections 17 and 22).  Beside them the goals'
plans, read from `make -n`."""
import ctypes as C
import os
import re
import subprocess

import pytest

import _header
from __graft_entry__ import PKG_DIR, load_package

FDIR = os.path.join(PKG_DIR, "fortran")
FC = "/opt/rocm/bin/amdflang"
HEADER = "letkf_amd_tcvital.h"
ENTRIES = {"letkf_tcvital_rows_dev", "letkf_tcvital_search_dev", "letkf_tcvital_fill_dev"}
STRUCTS = {"letkf_tcvital_params": "TcvitalParams"}
UNITS = os.path.join(_header.CSRC, "tcvital")
UNIT, KERNELS = "letkf_tcvital_entry.hip", "letkf_tcvital.hip"
MODULE, CHAIN = "letkf_tcvital_amd", ["letkf_amd_api", "letkf_obsope_amd"]
OTHER_LIBS = ("LIB_PATH", "OSSE_LIB_PATH", "OBSSIM_LIB_PATH", "SUPEROB_LIB_PATH", "OBSSCAN_LIB_PATH", "MAPPROJ_LIB_PATH", "OBSFILE_LIB_PATH",
              "NOBSOUT_LIB_PATH")
OTHER_GOALS = ("obsscan", "mapproj", "obsfile", "nobsout")
PKG = os.path.realpath(PKG_DIR)


@pytest.fixture(scope="module")
def pkg():
    p = load_package()
    p.build()
    return p


def test_ctypes_mirrors_are_the_header_and_have_gccs_layout(pkg):
    structs = _header.structs(HEADER)
    assert set(structs) == set(STRUCTS)
    for struct, fields in structs.items():
        cls = getattr(pkg, STRUCTS[struct])
        assert [(n, _header.field_ctype(k, cnt)) for k, n, cnt in fields] == list(cls._fields_), struct
        assert _header.sizeof(struct, HEADER) == C.sizeof(cls) == 48, struct
        assert [_header.offsetof(struct, n, HEADER) for _, n, _ in fields] == [getattr(cls, n).offset for _, n, _ in fields], struct


def test_the_entries_are_typed_as_the_header_declares_them(pkg):
    table = pkg.TCVITAL_SIGNATURES
    assert set(_header.entries(HEADER)) == set(table) == ENTRIES
    lib = pkg.tcvital_lib()
    for name in ENTRIES:
        want = _header.argtypes_of(name, HEADER)
        assert table[name] == want, name
        assert getattr(lib, name).argtypes == want and getattr(lib, name).restype is C.c_int, name
        assert _header.restype_of(name, HEADER) is C.c_int, name
    defines = _header.defines(HEADER)
    assert defines["LETKF_AMD_TCVITAL_VERSION"] == pkg.TCVITAL_VERSION == 1
    assert (defines["LETKF_TCVITAL_ID_TCX"], defines["LETKF_TCVITAL_ID_TCY"], defines["LETKF_TCVITAL_ID_TCP"], defines["LETKF_TCVITAL_QC_BAD"]) == \
        (pkg.TCVITAL_ID_TCX, pkg.TCVITAL_ID_TCY, pkg.TCVITAL_ID_TCP, pkg.TCVITAL_QC_BAD) == (99991, 99992, 99993, 50)
    assert '#include "letkf_amd_obsope.h"' in _header.text(HEADER)                       # for letkf_obsope_fields
    assert _header.defines()["LETKF_AMD_ABI_VERSION"] == 11
    assert "const letkf_obsope_fields *f" in _header.declared_params("letkf_tcvital_search_dev", HEADER)
    raw = open(os.path.join(_header.INCLUDE, HEADER)).read()
    for said in ("WHERE THE REFERENCE IS NOT FOLLOWED", "(1)", "(2)", "(3)", "(4)", "(5)", "obsope_tools.f90:1105"):   # the five departures
        assert said in raw, said


def test_the_entries_are_exported_by_their_library_and_by_no_other(pkg):
    for path in OTHER_LIBS:
        assert not _header.exported(getattr(pkg, path)) & ENTRIES, path
    sat = pkg.TCVITAL_LIB_PATH
    assert _header.exported(sat) == ENTRIES
    assert os.path.dirname(sat) == os.path.dirname(pkg.LIB_PATH)
    dyn = subprocess.check_output(["readelf", "-d", sat], text=True)
    assert "[libletkf_amd.so]" in dyn and "$ORIGIN" in dyn and not [g for g in OTHER_GOALS if g in dyn]


def test_the_table_is_disjoint_from_the_others_and_no_other_header_names_its_entries(pkg):
    others = [getattr(pkg, t) for t in dir(pkg) if t.endswith("ARGTYPES")] + [pkg.MAPPROJ_SIGNATURES, pkg.OBSFILE_SIGNATURES,
                                                                             pkg.NOBSOUT_SIGNATURES]
    assert len(others) == 12
    for t in others:
        assert not set(t) & ENTRIES
    for h in sorted(os.listdir(_header.INCLUDE)):
        if h != HEADER:
            assert not [n for n in ENTRIES if re.search(rf"\b{n}\b", _header.text(h))], h
            assert not [n for n in _header.entries(h) if re.search(rf"\b{n}\b", _header.text(HEADER))], h
    # the operator's header is as it was: its sentence stays true of that entry
    assert "H08, TC vitals, rain and USE_RADAR_PSEUDO_RH are not covered: qc 90" in open(os.path.join(_header.INCLUDE, "letkf_amd_obsope.h")).read()
    assert "tcvital" not in open(os.path.join(_header.INCLUDE, _header.MAIN)).read()


def test_each_entry_is_defined_once_in_its_unit_behind_the_barrier():
    defs = _header.definitions(UNITS)
    assert set(defs) == ENTRIES
    assert not set(_header.definitions()) & ENTRIES
    for name in ENTRIES:
        assert defs[name] == [(UNIT, "try", f"}} LETKF_ENTRY_END({name})")], (name, defs[name])
    src = open(os.path.join(UNITS, UNIT)).read()
    assert "__global__" not in src and "hipLaunchKernelGGL" not in src and "<<<" not in src
    assert '#include "letkf_api_internal.h"' in src and '#include "letkf_tcvital_dev.h"' in src
    kernels = re.sub(r"//.*", "", open(os.path.join(UNITS, KERNELS)).read())
    assert "atomic" not in kernels and kernels.count("__global__") == 5                  # tile, pick; scan, pick; fill
    assert '#include "letkf_obsope_point_dev.h"' in kernels and "kGg" in kernels and "kRd" in kernels   # prsadj's constants are the operator's
    assert "9.81" not in kernels and "287.05" not in kernels


def test_fortran_types_list_the_fields_in_c_order():
    src = open(os.path.join(FDIR, MODULE + ".f90")).read()
    assert _header.fortran_types(src) == _header.c_structs(HEADER)
    assert set(re.findall(r"BIND\(C, name='(letkf_\w+)'\)", src)) == ENTRIES
    assert re.findall(r"^\s*USE (\w+)", src, flags=re.M) == CHAIN[-1:]
    drv = open(os.path.join(FDIR, "tcvital_driver.f90")).read()
    for name in ENTRIES:
        assert name + "(" in drv, name


@pytest.mark.skipif(not os.path.exists(FC), reason="amdflang not present")
def test_the_fortran_module_compiles_with_amdflang(tmp_path):
    for f in CHAIN + [MODULE]:
        subprocess.check_call([FC, "-O2", "-fPIC", "-c", os.path.join(FDIR, f + ".f90"), "-o", str(tmp_path / (f + ".o"))], cwd=tmp_path)
    assert (tmp_path / (MODULE + ".mod")).exists()


def test_the_python_mirror_has_the_three_entries(pkg):
    for name in ("tcvital_rows", "tcvital_search", "tcvital_fill"):
        assert callable(getattr(pkg.Context, name)), name


# ---- the build: what `make tcvital` would do, and that the default goals do not reach it
def plan(directory, *args):
    out = subprocess.check_output(["make", "-n", "--no-print-directory", "-C", directory, *args], text=True)
    return [line.split() for line in out.replace("\\\n", " ").splitlines() if not line.startswith("make")]


def test_the_goal_builds_the_ninth_library_as_a_satellite(pkg):
    cmds = plan(PKG, "-B", "tcvital")
    cc = {os.path.basename(w[w.index("-o") + 1])[:-2]: w for w in cmds if "-c" in w and "/obj_tcvital/" in w[w.index("-o") + 1]}
    assert set(cc) == {"letkf_tcvital", "letkf_tcvital_entry"}
    for u, w in cc.items():
        assert w[w.index("-c") + 1].endswith(f"csrc/tcvital/{u}.hip") and "--offload-arch=gfx950" in w and "-save-temps=obj" in w, w
        assert f"-I{PKG}/csrc" in w and not [x for x in w if "fast-math" in x or x == "-Ofast"], w
    assert "-ffp-contract=off" in cc["letkf_tcvital"]                                    # the disc test rounds term by term
    links = {os.path.basename(w[w.index("-o") + 1]): (n, w) for n, w in enumerate(cmds) if "-shared" in w}
    assert set(links) == {"libletkf_amd.so", "libletkf_amd_tcvital.so"}
    at, w = links["libletkf_amd_tcvital.so"]
    objdir = os.path.join(PKG, "lib", "obj_tcvital")
    assert sorted(x for x in w if x.endswith(".o")) == sorted(os.path.join(objdir, u + ".o") for u in cc)
    audit = cmds[at - 1]
    assert audit[0] == "python3" and audit[1].endswith("tools/isa_exec_audit.py") and audit[-2:] == ["--dir", objdir], audit
    assert "-lletkf_amd" in w and "-Wl,-rpath,'$ORIGIN'" in w and f"-L{PKG}/lib" in w and at > links["libletkf_amd.so"][0]


def test_the_default_goals_do_not_reach_it_and_a_twin_has_none(pkg):
    for args in (("-B",), ("-B", "CHECKED=1"), ("-B", "PROF=1")) + tuple(("-B", g) for g in OTHER_GOALS):
        assert not [w for w in plan(PKG, *args) if "tcvital" in " ".join(w)], args
    for args in (("-B",),) + tuple(("-B", g) for g in OTHER_GOALS):
        assert not [w for w in plan(FDIR, *args) if "tcvital" in " ".join(w)], args
    assert plan(PKG, "tcvital") == [], "the tree is not up to date"
    for own_header in ("/csrc/tcvital/letkf_tcvital_dev.h", "/../include/letkf_amd_tcvital.h"):
        own = {os.path.basename(w[w.index("-o") + 1]) for w in plan(PKG, "-W", PKG + own_header, "tcvital") if "-c" in w}
        assert own == {"letkf_tcvital.o", "letkf_tcvital_entry.o"}, own_header
        for goal in ("all",) + OTHER_GOALS:
            assert not plan(PKG, "-W", PKG + own_header, goal), (own_header, goal)      # no unit of the other libraries is built against it


@pytest.mark.skipif(not os.path.exists(FC), reason="amdflang not present")
def test_the_fortran_goal_links_the_driver_with_its_library_first():
    cmds = [w for w in plan(FDIR, "-B", "tcvital") if "-c" not in w and "-o" in w]
    assert [w[w.index("-o") + 1] for w in cmds] == ["tcvital_driver"]
    w = cmds[0]
    assert [x for x in w if x.startswith("-lletkf")] == ["-lletkf_amd_tcvital", "-lletkf_amd"] and "-lamdhip64" in w
    assert [x for x in w if x.endswith(".o")] == ["letkf_tcvital_amd.o", "letkf_obsope_amd.o", "letkf_amd_api.o"]


def test_the_one_build_call_makes_the_goals():
    src = open(os.path.join(PKG_DIR, "__init__.py")).read()
    assert '"-C", HERE, "tcvital"]' in src and "TCVITAL_LIB_PATH,)" in src.split("stale =")[0]
    entry = open(os.path.join(os.path.dirname(PKG_DIR), "__graft_entry__.py")).read()
    assert 'os.path.join(PKG_DIR, "fortran"), "tcvital"]' in entry and "pkg.tcvital_lib()" in entry
