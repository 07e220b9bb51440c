"""The eighth companion header include/letkf_amd_obsscan.h and its mirrors, without a device: the checks
test_companion_bindings.py makes for every row of its table, made here for this one companion with the same readers
(tests/_header.py) -- its units lie in csrc/obsscan/ and its library and driver hang on goals of their own, so it has no row in
that table.  Beside them what the build owes this companion: the goal's plan, read from `make -n`."""
import ctypes as C
import os
import re
import subprocess

import pytest

import _header
from __graft_entry__ import PKG_DIR, load_package

FDIR = os.path.join(PKG_DIR, "fortran")
FC = "/opt/rocm/bin/amdflang"
HEADER = "letkf_amd_obsscan.h"
ENTRIES = {"letkf_obsscan_dev", "letkf_obsscan_rows", "letkf_obsscan_slot_bounds", "letkf_obsope_slot_dev"}
STRUCTS = {"letkf_obsscan_params": "ObsscanParams", "letkf_obsscan_out": "ObsscanOut", "letkf_obsscan_lists": "ObsscanLists"}
UNITS = os.path.join(_header.CSRC, "obsscan")
UNIT = "letkf_obsscan_entry.hip"
MODULE, CHAIN = "letkf_obsscan_amd", ["letkf_amd_api", "letkf_obsope_amd"]
OTHER_LIBS = ("LIB_PATH", "OSSE_LIB_PATH", "OBSSIM_LIB_PATH", "SUPEROB_LIB_PATH")
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
        assert _header.sizeof(struct, HEADER) == C.sizeof(cls), struct
        assert [_header.offsetof(struct, n, HEADER) for _, n, _ in fields] == [getattr(cls, n).offset for _, n, _ in fields], struct


def test_the_entries_are_typed_as_the_header_declares_them(pkg):
    table = pkg.OBSSCAN_ARGTYPES
    assert set(_header.entries(HEADER)) == set(table) == ENTRIES
    lib = pkg.obsscan_lib()
    for name in ENTRIES:
        want = _header.argtypes_of(name, HEADER)
        assert table[name] == want, name
        assert getattr(lib, name).argtypes == want and getattr(lib, name).restype is C.c_int, name
        assert _header.restype_of(name, HEADER) is C.c_int, name
    defines = _header.defines(HEADER)
    assert defines["LETKF_AMD_OBSSCAN_VERSION"] == pkg.OBSSCAN_VERSION == 1
    assert defines["LETKF_OBSSCAN_MAX_BUCKETS"] == pkg.OBSSCAN_MAX_BUCKETS == 2 ** 22
    assert (defines["LETKF_OBSSCAN_QC_TIME"], defines["LETKF_OBSSCAN_QC_OUT_H"]) == (pkg.IQC_TIME, pkg.IQC_OUT_H) == (97, 98)
    assert '#include "letkf_amd_obsope.h"' in _header.text(HEADER)
    assert _header.defines()["LETKF_AMD_ABI_VERSION"] == 11


def test_the_entries_are_exported_by_their_library_and_by_no_other(pkg):
    for path in OTHER_LIBS:
        assert not _header.exported(getattr(pkg, path)) & ENTRIES, path
    sat = pkg.OBSSCAN_LIB_PATH
    assert _header.exported(sat) == ENTRIES
    assert os.path.dirname(sat) == os.path.dirname(pkg.LIB_PATH)
    dyn = subprocess.check_output(["readelf", "-d", sat], text=True)
    assert "[libletkf_amd.so]" in dyn and "$ORIGIN" in dyn


def test_the_table_is_disjoint_from_the_other_eight_and_no_other_header_names_its_entries(pkg):
    others = [getattr(pkg, t) for t in dir(pkg) if t.endswith("ARGTYPES") and t != "OBSSCAN_ARGTYPES"]
    assert len(others) == 8
    for t in others:
        assert not set(t) & ENTRIES
    for h in sorted(os.listdir(_header.INCLUDE)):
        if h != HEADER:
            assert not [n for n in ENTRIES if re.search(rf"\b{n}\b", _header.text(h))], h
            assert not [n for n in _header.entries(h) if re.search(rf"\b{n}\b", _header.text(HEADER))], h


def test_each_entry_is_defined_once_in_its_unit_behind_the_barrier():
    defs = _header.definitions(UNITS)
    assert set(defs) == ENTRIES
    assert not set(_header.definitions()) & ENTRIES
    for name in ENTRIES:
        assert defs[name] == [(UNIT, "try", f"}} LETKF_ENTRY_END({name})")], (name, defs[name])
    src = open(os.path.join(UNITS, UNIT)).read()
    assert "__global__" not in src and "hipLaunchKernelGGL" not in src and "<<<" not in src
    assert '#include "letkf_api_internal.h"' in src


def test_fortran_types_list_the_fields_in_c_order():
    src = open(os.path.join(FDIR, MODULE + ".f90")).read()
    assert _header.fortran_types(src) == _header.c_structs(HEADER)
    assert set(re.findall(r"BIND\(C, name='(letkf_\w+)'\)", src)) == ENTRIES
    assert re.findall(r"^\s*USE (\w+)", src, flags=re.M) == CHAIN
    for routine in ("obsscan_amd", "obsope_slot_amd"):
        assert re.search(rf"SUBROUTINE {routine}\(", src), routine


@pytest.mark.skipif(not os.path.exists(FC), reason="amdflang not present")
def test_the_fortran_module_compiles_with_amdflang(tmp_path):
    for f in CHAIN + [MODULE]:
        subprocess.check_call([FC, "-O2", "-fPIC", "-c", os.path.join(FDIR, f + ".f90"), "-o", str(tmp_path / (f + ".o"))], cwd=tmp_path)
    assert (tmp_path / (MODULE + ".mod")).exists()


def test_the_driver_scans_then_runs_the_operator_slot_by_slot_then_sets_the_observations(pkg):
    assert callable(pkg.Context.obsscan) and callable(pkg.Context.obsope_slot)
    drv = open(os.path.join(FDIR, "obsscan_driver.f90")).read()
    assert drv.index("CALL obsscan_amd") < drv.index("CALL obsope_slot_amd") < drv.index("CALL set_letkf_obs_amd")
    assert re.search(r"DO islot = s0, s1\n.*\n\s*CALL obsope_slot_amd", drv)


# ---- the build: what `make obsscan` would do, and that the default goal does not reach it
def plan(directory, *args):
    out = subprocess.check_output(["make", "-n", "--no-print-directory", "-C", directory, *args], text=True)
    return [line.split() for line in out.replace("\\\n", " ").splitlines() if not line.startswith("make")]


def test_the_goal_builds_the_fifth_library_as_a_satellite(pkg):
    cmds = plan(PKG, "-B", "obsscan")
    cc = {os.path.basename(w[w.index("-o") + 1])[:-2]: w for w in cmds if "-c" in w and "/obj_obsscan/" in w[w.index("-o") + 1]}
    assert set(cc) == {"letkf_obsscan", "letkf_obsscan_entry"}
    for u, w in cc.items():
        assert w[w.index("-c") + 1].endswith(f"csrc/obsscan/{u}.hip") and "--offload-arch=gfx950" in w and "-save-temps=obj" in w, w
    assert {u for u, w in cc.items() if "-ffp-contract=off" in w} == {"letkf_obsscan"}
    links = {os.path.basename(w[w.index("-o") + 1]): (n, w) for n, w in enumerate(cmds) if "-shared" in w}
    assert set(links) == {"libletkf_amd.so", "libletkf_amd_obsscan.so"}
    at, w = links["libletkf_amd_obsscan.so"]
    objdir = os.path.join(PKG, "lib", "obj_obsscan")
    assert sorted(x for x in w if x.endswith(".o")) == sorted(os.path.join(objdir, u + ".o") for u in cc)
    audit = cmds[at - 1]
    assert audit[0] == "python3" and audit[1].endswith("tools/isa_exec_audit.py") and audit[-2:] == ["--dir", objdir], audit
    assert "-lletkf_amd" in w and "-Wl,-rpath,'$ORIGIN'" in w and f"-L{PKG}/lib" in w and at > links["libletkf_amd.so"][0]


def test_the_default_goals_do_not_reach_it_and_a_twin_has_none(pkg):
    for args in (("-B",), ("-B", "CHECKED=1"), ("-B", "PROF=1")):
        assert not [w for w in plan(PKG, *args) if "obsscan" in " ".join(w)], args
    assert not [w for w in plan(FDIR, "-B") if "obsscan" in " ".join(w)]
    assert plan(PKG, "obsscan") == [], "the tree is not up to date"
    own = {os.path.basename(w[w.index("-o") + 1]) for w in plan(PKG, "-W", PKG + "/csrc/obsscan/letkf_obsscan_dev.h", "obsscan") if "-c" in w}
    assert own == {"letkf_obsscan.o", "letkf_obsscan_entry.o"}
    assert not plan(PKG, "-W", PKG + "/../include/letkf_amd_obsscan.h", "all")       # no unit of the four libraries is built against it


@pytest.mark.skipif(not os.path.exists(FC), reason="amdflang not present")
def test_the_fortran_goal_links_the_driver_with_its_library_first():
    cmds = [w for w in plan(FDIR, "-B", "obsscan") if "-c" not in w and "-o" in w]
    assert [w[w.index("-o") + 1] for w in cmds] == ["obsscan_driver"]
    w = cmds[0]
    assert [x for x in w if x.startswith("-lletkf")] == ["-lletkf_amd_obsscan", "-lletkf_amd"] and "-lamdhip64" in w
    assert [x for x in w if x.endswith(".o")] == ["letkf_obsscan_amd.o", "letkf_obsope_amd.o", "letkf_obs_amd.o", "letkf_tools_amd.o",
                                                  "letkf_amd_api.o"]
