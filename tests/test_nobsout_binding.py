"""The eleventh companion header include/letkf_amd_nobsout.h and its mirrors, without a device: the checks
tests/test_obsfile_binding.py makes for the tenth, made here for this one with the same readers (tests/_header.py) -- its units lie
in csrc/nobsout/ and its library and driver hang on goals of their own (DESIGN.md sections 17 and 21).  Beside them the goals' plans,
read from `make -n`, and that the main library exports what its tables say and nothing new."""
import ctypes as C
import os
import re
import subprocess

import pytest

import _header
from __graft_entry__ import PKG_DIR, load_package

FDIR = os.path.join(PKG_DIR, "fortran")
FC = "/opt/rocm/bin/amdflang"
HEADER = "letkf_amd_nobsout.h"
ENTRIES = {"letkf_das_columns_nobs_dev", "letkf_nobs_fields_dev"}
STRUCTS = {"letkf_nobsout_params": "NobsoutParams"}
UNITS = os.path.join(_header.CSRC, "nobsout")
UNIT, KERNELS = "letkf_nobsout_entry.hip", "letkf_nobsout.hip"
MODULE, CHAIN = "letkf_nobsout_amd", ["letkf_amd_api"]
OTHER_LIBS = ("LIB_PATH", "OSSE_LIB_PATH", "OBSSIM_LIB_PATH", "SUPEROB_LIB_PATH", "OBSSCAN_LIB_PATH", "MAPPROJ_LIB_PATH", "OBSFILE_LIB_PATH")
OTHER_GOALS = ("obsscan", "mapproj", "obsfile")
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
    table = pkg.NOBSOUT_SIGNATURES
    assert set(_header.entries(HEADER)) == set(table) == ENTRIES
    lib = pkg.nobsout_lib()
    for name in ENTRIES:
        want = _header.argtypes_of(name, HEADER)
        assert table[name] == want, name
        assert getattr(lib, name).argtypes == want and getattr(lib, name).restype is C.c_int, name
        assert _header.restype_of(name, HEADER) is C.c_int, name
    defines = _header.defines(HEADER)
    assert defines["LETKF_AMD_NOBSOUT_VERSION"] == pkg.NOBSOUT_VERSION == 1
    assert (defines["LETKF_NOBSOUT_MAX_CTYPE"], defines["LETKF_NOBSOUT_MAX_OBTYPE"], defines["LETKF_NOBSOUT_NFIELDS"]) == \
        (pkg.NOBSOUT_MAX_CTYPE, pkg.NOBSOUT_MAX_OBTYPE, pkg.NOBSOUT_NFIELDS) == (64, 32, 11)
    assert '#include "letkf_amd.h"' in _header.text(HEADER)
    assert _header.defines()["LETKF_AMD_ABI_VERSION"] == 11
    # the new entry takes the old one's parameters, in its order, and two more
    old = _header.declared_params("letkf_das_columns_dev")
    new = _header.declared_params("letkf_das_columns_nobs_dev", HEADER)
    assert new[:len(old)] == old and new[len(old):] == ["int32_t *nobs_ctype", "double *cutd_ctype"]
    raw = open(os.path.join(_header.INCLUDE, HEADER)).read()
    assert ":399-400" in raw and "iv3d_t" in raw                                         # the class the reference reads is named


def test_the_entries_are_exported_by_their_library_and_by_no_other(pkg):
    for path in OTHER_LIBS:
        assert not _header.exported(getattr(pkg, path)) & ENTRIES, path
    sat = pkg.NOBSOUT_LIB_PATH
    assert _header.exported(sat) == ENTRIES
    assert os.path.dirname(sat) == os.path.dirname(pkg.LIB_PATH)
    dyn = subprocess.check_output(["readelf", "-d", sat], text=True)
    assert "[libletkf_amd.so]" in dyn and "$ORIGIN" in dyn and not [g for g in OTHER_GOALS if g in dyn]


def test_the_main_library_exports_what_its_tables_say(pkg):
    main = set()
    for t in (pkg.ARGTYPES, pkg.INTERP_ARGTYPES, pkg.INTERP_WINDOW_ARGTYPES, pkg.OBSOPE_ARGTYPES, pkg.MONIT_ARGTYPES):
        main |= set(t)
    assert _header.exported(pkg.LIB_PATH) == main
    assert "letkf_das_columns_dev" in main and not main & ENTRIES
    # letkf_amd.h does not know the companion, and letkf_das_args is what it was
    assert "nobs_ctype" not in [n for _, n, _ in _header.structs()["letkf_das_args"]]
    assert "nobsout" not in open(os.path.join(_header.INCLUDE, _header.MAIN)).read()


def test_the_table_is_disjoint_from_the_others_and_no_other_header_names_its_entries(pkg):
    others = [getattr(pkg, t) for t in dir(pkg) if t.endswith("ARGTYPES")] + [pkg.MAPPROJ_SIGNATURES, pkg.OBSFILE_SIGNATURES]
    assert len(others) == 11
    for t in others:
        assert not set(t) & ENTRIES
    raw = open(os.path.join(_header.INCLUDE, HEADER)).read()                             # comments included
    for h in sorted(os.listdir(_header.INCLUDE)):
        if h != HEADER:
            assert not [n for n in ENTRIES if re.search(rf"\b{n}\b", _header.text(h))], h
            if h != _header.MAIN:                                                         # (the main loop and the search are named)
                assert not [n for n in _header.entries(h) if re.search(rf"\b{n}\b", raw)], h


def test_each_entry_is_defined_once_in_its_unit_behind_the_barrier():
    defs = _header.definitions(UNITS)
    assert set(defs) == ENTRIES
    assert not set(_header.definitions()) & ENTRIES
    for name in ENTRIES:
        assert defs[name] == [(UNIT, "try", f"}} LETKF_ENTRY_END({name})")], (name, defs[name])
    src = open(os.path.join(UNITS, UNIT)).read()
    assert "__global__" not in src and "hipLaunchKernelGGL" not in src and "<<<" not in src
    assert '#include "letkf_api_internal.h"' in src and '#include "letkf_nobsout_dev.h"' in src
    assert "das_columns_impl(" in src                                                    # the main loop is the main library's
    kernels = re.sub(r"//.*", "", open(os.path.join(UNITS, KERNELS)).read())
    assert "atomic" not in kernels and kernels.count("__global__") == 3
    assert '#include "letkf_search_dev.h"' in kernels and "search_dev::kDistZeroFac" in kernels   # the library's one literal
    # the old entry is the shared function with no diagnostics, and no kernel moved into the host unit
    das = open(os.path.join(_header.CSRC, "letkf_api_das.hip")).read()
    assert "return das_columns_impl(c, g, t, nij1, nlev, rig, rjg, rlev, rz, list_bytes, nobs_out, nullptr);" in das
    assert "__global__" not in das


def test_fortran_types_list_the_fields_in_c_order():
    src = open(os.path.join(FDIR, MODULE + ".f90")).read()
    assert _header.fortran_types(src) == _header.c_structs(HEADER)
    assert set(re.findall(r"BIND\(C, name='(letkf_\w+)'\)", src)) == ENTRIES
    assert re.findall(r"^\s*USE (\w+)", src, flags=re.M) == CHAIN[-1:]
    assert re.search(r"SUBROUTINE nobs_fields_amd\(", src)
    drv = open(os.path.join(FDIR, "nobsout_driver.f90")).read()
    assert "letkf_das_columns_nobs_dev(" in drv and "CALL nobs_fields_amd(" in drv and "letkf_das_columns_dev(" not in drv
    # das_letkf_amd itself stays as it is
    tools = open(os.path.join(FDIR, "letkf_tools_amd.f90")).read()
    assert "letkf_das_columns_dev(" in tools and "nobsout" not in tools and "letkf_das_columns_nobs_dev" not in tools


@pytest.mark.skipif(not os.path.exists(FC), reason="amdflang not present")
def test_the_fortran_module_compiles_with_amdflang(tmp_path):
    for f in CHAIN + [MODULE]:
        subprocess.check_call([FC, "-O2", "-fPIC", "-c", os.path.join(FDIR, f + ".f90"), "-o", str(tmp_path / (f + ".o"))], cwd=tmp_path)
    assert (tmp_path / (MODULE + ".mod")).exists()


def test_the_python_mirror_has_the_two_entries(pkg):
    for name in ("das_columns_nobs", "nobs_fields"):
        assert callable(getattr(pkg.Context, name)), name
    import inspect
    old = list(inspect.signature(pkg.Context.das_columns).parameters)
    new = list(inspect.signature(pkg.Context.das_columns_nobs).parameters)
    assert new == old + ["nobs_ctype", "cutd_ctype"]


# ---- the build: what `make nobsout` would do, and that the default goals do not reach it
def plan(directory, *args):
    out = subprocess.check_output(["make", "-n", "--no-print-directory", "-C", directory, *args], text=True)
    return [line.split() for line in out.replace("\\\n", " ").splitlines() if not line.startswith("make")]


def test_the_goal_builds_the_eighth_library_as_a_satellite(pkg):
    cmds = plan(PKG, "-B", "nobsout")
    cc = {os.path.basename(w[w.index("-o") + 1])[:-2]: w for w in cmds if "-c" in w and "/obj_nobsout/" in w[w.index("-o") + 1]}
    assert set(cc) == {"letkf_nobsout", "letkf_nobsout_entry"}
    for u, w in cc.items():
        assert w[w.index("-c") + 1].endswith(f"csrc/nobsout/{u}.hip") and "--offload-arch=gfx950" in w and "-save-temps=obj" in w, w
        assert f"-I{PKG}/csrc" in w and not [x for x in w if "fast-math" in x or x == "-Ofast"], w
    links = {os.path.basename(w[w.index("-o") + 1]): (n, w) for n, w in enumerate(cmds) if "-shared" in w}
    assert set(links) == {"libletkf_amd.so", "libletkf_amd_nobsout.so"}
    at, w = links["libletkf_amd_nobsout.so"]
    objdir = os.path.join(PKG, "lib", "obj_nobsout")
    assert sorted(x for x in w if x.endswith(".o")) == sorted(os.path.join(objdir, u + ".o") for u in cc)
    audit = cmds[at - 1]
    assert audit[0] == "python3" and audit[1].endswith("tools/isa_exec_audit.py") and audit[-2:] == ["--dir", objdir], audit
    assert "-lletkf_amd" in w and "-Wl,-rpath,'$ORIGIN'" in w and f"-L{PKG}/lib" in w and at > links["libletkf_amd.so"][0]


def test_the_default_goals_do_not_reach_it_and_a_twin_has_none(pkg):
    for args in (("-B",), ("-B", "CHECKED=1"), ("-B", "PROF=1")) + tuple(("-B", g) for g in OTHER_GOALS):
        assert not [w for w in plan(PKG, *args) if "nobsout" in " ".join(w)], args
    for args in (("-B",),) + tuple(("-B", g) for g in OTHER_GOALS):
        assert not [w for w in plan(FDIR, *args) if "nobsout" in " ".join(w)], args
    assert plan(PKG, "nobsout") == [], "the tree is not up to date"
    for own_header in ("/csrc/nobsout/letkf_nobsout_dev.h", "/../include/letkf_amd_nobsout.h"):
        own = {os.path.basename(w[w.index("-o") + 1]) for w in plan(PKG, "-W", PKG + own_header, "nobsout") if "-c" in w}
        assert own == {"letkf_nobsout.o", "letkf_nobsout_entry.o"}, own_header
        for goal in ("all",) + OTHER_GOALS:
            assert not plan(PKG, "-W", PKG + own_header, goal), (own_header, goal)      # no unit of the other libraries is built against it
    # the shared function's declaration is every host unit's: a change to it rebuilds the new units too
    rebuilt = {os.path.basename(w[w.index("-o") + 1]) for w in plan(PKG, "-W", PKG + "/csrc/letkf_api_internal.h", "nobsout") if "-c" in w}
    assert {"letkf_api_das.o", "letkf_nobsout_entry.o"} <= rebuilt


@pytest.mark.skipif(not os.path.exists(FC), reason="amdflang not present")
def test_the_fortran_goal_links_the_driver_with_its_library_first():
    cmds = [w for w in plan(FDIR, "-B", "nobsout") if "-c" not in w and "-o" in w]
    assert [w[w.index("-o") + 1] for w in cmds] == ["nobsout_driver"]
    w = cmds[0]
    assert [x for x in w if x.startswith("-lletkf")] == ["-lletkf_amd_nobsout", "-lletkf_amd"] and "-lamdhip64" in w
    assert [x for x in w if x.endswith(".o")] == ["letkf_nobsout_amd.o", "letkf_amd_api.o"]


def test_the_one_build_call_makes_the_goals():
    src = open(os.path.join(PKG_DIR, "__init__.py")).read()
    assert '"-C", HERE, "nobsout"]' in src and "NOBSOUT_LIB_PATH)" in src.split("stale =")[0]
    entry = open(os.path.join(os.path.dirname(PKG_DIR), "__graft_entry__.py")).read()
    assert 'os.path.join(PKG_DIR, "fortran"), "nobsout"]' in entry and "pkg.nobsout_lib()" in entry
