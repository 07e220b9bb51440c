"""The thirteenth companion header include/letkf_amd_h08.h and its mirrors, without a device: the checks
tests/test_tcvital_binding.py makes for the twelfth, made here for this one with the same readers (tests/_header.py) -- its units
lie in csrc/h08/ and its library and driver hang on goals of their own (DESIGN.md sections 17 and 23).  Beside them the goals'
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
HEADER = "letkf_amd_h08.h"
ENTRIES = {"letkf_h08_count", "letkf_h08_bytes", "letkf_h08_decode_dev", "letkf_h08_encode_dev", "letkf_h08_select_dev",
           "letkf_h08_profiles_dev", "letkf_h08_rows_dev"}
STRUCTS = {"letkf_h08_params": ("H08Params", 224), "letkf_h08_profiles": ("H08Profiles", 32)}
UNITS = os.path.join(_header.CSRC, "h08")
UNIT, KERNELS = "letkf_h08_entry.hip", "letkf_h08.hip"
MODULE, CHAIN = "letkf_h08_amd", ["letkf_amd_api", "letkf_obsope_amd", "letkf_mapproj_amd", "letkf_obsfile_amd"]
OTHER_LIBS = ("LIB_PATH", "OSSE_LIB_PATH", "OBSSIM_LIB_PATH", "SUPEROB_LIB_PATH", "OBSSCAN_LIB_PATH", "MAPPROJ_LIB_PATH", "OBSFILE_LIB_PATH",
              "NOBSOUT_LIB_PATH", "TCVITAL_LIB_PATH")
OTHER_GOALS = ("obsscan", "mapproj", "obsfile", "nobsout", "tcvital")
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
        cls = getattr(pkg, STRUCTS[struct][0])
        assert [(n, _header.field_ctype(k, cnt)) for k, n, cnt in fields] == list(cls._fields_), struct
        assert _header.sizeof(struct, HEADER) == C.sizeof(cls) == STRUCTS[struct][1], struct
        assert [_header.offsetof(struct, n, HEADER) for _, n, _ in fields] == [getattr(cls, n).offset for _, n, _ in fields], struct
    p = pkg.h08_params(nlev=5, ch_use=(1, 0, 1, 0, 1, 0, 1, 0, 1, 2))
    assert (p.nlev, list(p.ch_use), p.sub_lon, p.r_pol, p.r_sat, p.ell_tan, p.ell_ecc, p.cldsky_thrs) == \
        (5, [1, 0, 1, 0, 1, 0, 1, 0, 1, 2], 140.7, 6356.7523e3, 42164.0e3, 0.993305616, 0.00669438444, -5.0)


def test_the_entries_are_typed_as_the_header_declares_them(pkg):
    table = pkg.H08_SIGNATURES
    assert set(_header.entries(HEADER)) == set(table) == ENTRIES
    lib = pkg.h08_lib()
    for name in ENTRIES:
        want = _header.argtypes_of(name, HEADER)
        assert table[name] == want, name
        assert getattr(lib, name).argtypes == want and getattr(lib, name).restype is C.c_int, name
        assert _header.restype_of(name, HEADER) is C.c_int, name
    defines = _header.defines(HEADER)
    assert defines["LETKF_AMD_H08_VERSION"] == pkg.H08_VERSION == 1
    assert (defines["LETKF_H08_NCH"], defines["LETKF_H08_ID"], defines["LETKF_H08_QC_BAD"]) == \
        (pkg.H08_NCH, pkg.H08_ID, pkg.H08_QC_BAD) == (10, 8800, 50)
    text = _header.text(HEADER)
    assert '#include "letkf_amd_obsope.h"' in text and '#include "letkf_amd_obsfile.h"' in text
    assert _header.defines()["LETKF_AMD_ABI_VERSION"] == 11
    assert "const letkf_obsope_fields *f" in _header.declared_params("letkf_h08_profiles_dev", HEADER)
    assert "const letkf_obsfile_cols *cols" in _header.declared_params("letkf_h08_decode_dev", HEADER)
    raw = open(os.path.join(_header.INCLUDE, HEADER)).read()
    for said in ("WHERE THE REFERENCE IS NOT FOLLOWED", "(1)", "(2)", "(3)", "(4)", "(5)", "(6)", "common_obs_scale.f90:2777-3110",
                 "scale_H08_fwd.F90:518-632", "obsope_tools.f90:512-646", "nv2dd >= 9"):
        assert said in raw, said


def test_the_entries_are_exported_by_their_library_and_by_no_other(pkg):
    for path in OTHER_LIBS:
        assert not _header.exported(getattr(pkg, path)) & ENTRIES, path
    sat = pkg.H08_LIB_PATH
    assert _header.exported(sat) == ENTRIES
    assert os.path.dirname(sat) == os.path.dirname(pkg.LIB_PATH)
    dyn = subprocess.check_output(["readelf", "-d", sat], text=True)
    assert "[libletkf_amd.so]" in dyn and "$ORIGIN" in dyn and not [g for g in OTHER_GOALS if g in dyn]


def test_the_table_is_disjoint_from_the_others_and_no_other_header_names_its_entries(pkg):
    assert not [t for t in dir(pkg) if t.endswith("ARGTYPES") and "H08" in t]
    others = [getattr(pkg, t) for t in dir(pkg) if t.endswith("ARGTYPES")] + [pkg.MAPPROJ_SIGNATURES, pkg.OBSFILE_SIGNATURES,
                                                                             pkg.NOBSOUT_SIGNATURES, pkg.TCVITAL_SIGNATURES]
    assert len(others) == 13
    for t in others:
        assert not set(t) & ENTRIES
    for h in sorted(os.listdir(_header.INCLUDE)):
        if h != HEADER:
            assert not [n for n in ENTRIES if re.search(rf"\b{n}\b", _header.text(h))], h
            assert not [n for n in _header.entries(h) if re.search(rf"\b{n}\b", _header.text(HEADER))], h
    # the headers that said H08 was out of reach point here now; no declaration of theirs changed
    inc = lambda h: open(os.path.join(_header.INCLUDE, h)).read()
    for h in ("letkf_amd_obsfile.h", "letkf_amd_obsope.h", "letkf_amd_obsmake.h", "letkf_amd_monit.h"):
        assert "letkf_amd_h08.h" in inc(h), h
    assert "H08, TC vitals, rain and USE_RADAR_PSEUDO_RH are not covered: qc 90" in inc("letkf_amd_obsope.h")
    assert "read_obs_H08" in inc("letkf_amd_obsfile.h") and "is NOT handled" not in inc("letkf_amd_obsfile.h")
    assert "h08_" not in inc(_header.MAIN).replace("h08_min_cld_member", "").replace("h08_limit_lev", "").replace("h08_bt_min", "") \
        .replace("h08_lev", "").replace("h08_val2", "")


def test_each_entry_is_defined_once_in_its_unit_behind_the_barrier():
    defs = _header.definitions(UNITS)
    assert set(defs) == ENTRIES
    assert not set(_header.definitions()) & ENTRIES
    for name in ENTRIES:
        assert defs[name] == [(UNIT, "try", f"}} LETKF_ENTRY_END({name})")], (name, defs[name])
    src = open(os.path.join(UNITS, UNIT)).read()
    assert "__global__" not in src and "hipLaunchKernelGGL" not in src and "<<<" not in src
    assert '#include "letkf_api_internal.h"' in src and '#include "letkf_h08_dev.h"' in src
    assert "scan_ws(" in src and "scan_offsets(" in src                                  # the selection is on the main library's scan
    kernels = re.sub(r"//.*", "", open(os.path.join(UNITS, KERNELS)).read())
    assert "atomic" not in kernels and kernels.count("__global__") == 7          # decode, total, encode; mark, fill; profiles; rows
    assert '#include "letkf_obsope_point_dev.h"' in kernels and "ceil_split(" in kernels and "term2(" in kernels
    assert '#include "letkf_lane_dev.h"' in kernels and "wave_max(" in kernels and "wave_min(" in kernels


def test_fortran_types_list_the_fields_in_c_order():
    src = open(os.path.join(FDIR, MODULE + ".f90")).read()
    assert _header.fortran_types(src) == _header.c_structs(HEADER)
    assert set(re.findall(r"BIND\(C, name='(letkf_\w+)'\)", src)) == ENTRIES
    assert re.findall(r"^\s*USE (\w+)", src, flags=re.M) == ["letkf_obsope_amd", "letkf_obsfile_amd"]
    drv = open(os.path.join(FDIR, "h08_driver.f90")).read()
    for name in ENTRIES - {"letkf_h08_bytes"}:
        assert name + "(" in drv, name


@pytest.mark.skipif(not os.path.exists(FC), reason="amdflang not present")
def test_the_fortran_module_compiles_with_amdflang(tmp_path):
    for f in CHAIN + [MODULE]:
        subprocess.check_call([FC, "-O2", "-fPIC", "-c", os.path.join(FDIR, f + ".f90"), "-o", str(tmp_path / (f + ".o"))], cwd=tmp_path)
    assert (tmp_path / (MODULE + ".mod")).exists()


def test_the_python_mirror_has_the_entries(pkg):
    for name in ("h08_decode", "h08_encode", "h08_select", "h08_profiles", "h08_rows"):
        assert callable(getattr(pkg.Context, name)), name
    assert pkg.h08_count(640) == 10 and pkg.h08_bytes(10) == 640
    with pytest.raises(pkg.LetkfError):
        pkg.h08_count(100)


# ---- the build: what `make h08` would do, and that the default goals do not reach it
def plan(directory, *args):
    out = subprocess.check_output(["make", "-n", "--no-print-directory", "-C", directory, *args], text=True)
    return [line.split() for line in out.replace("\\\n", " ").splitlines() if not line.startswith("make")]


def test_the_goal_builds_the_tenth_library_as_a_satellite(pkg):
    cmds = plan(PKG, "-B", "h08")
    cc = {os.path.basename(w[w.index("-o") + 1])[:-2]: w for w in cmds if "-c" in w and "/obj_h08/" in w[w.index("-o") + 1]}
    assert set(cc) == {"letkf_h08", "letkf_h08_entry"}
    for u, w in cc.items():
        assert w[w.index("-c") + 1].endswith(f"csrc/h08/{u}.hip") and "--offload-arch=gfx950" in w and "-save-temps=obj" in w, w
        assert f"-I{PKG}/csrc" in w and not [x for x in w if "fast-math" in x or x == "-Ofast"], w
    assert "-ffp-contract=off" in cc["letkf_h08"]                                        # every product and sum rounds on its own
    links = {os.path.basename(w[w.index("-o") + 1]): (n, w) for n, w in enumerate(cmds) if "-shared" in w}
    assert set(links) == {"libletkf_amd.so", "libletkf_amd_h08.so"}
    at, w = links["libletkf_amd_h08.so"]
    objdir = os.path.join(PKG, "lib", "obj_h08")
    assert sorted(x for x in w if x.endswith(".o")) == sorted(os.path.join(objdir, u + ".o") for u in cc)
    audit = cmds[at - 1]
    assert audit[0] == "python3" and audit[1].endswith("tools/isa_exec_audit.py") and audit[-2:] == ["--dir", objdir], audit
    assert "-lletkf_amd" in w and "-Wl,-rpath,'$ORIGIN'" in w and f"-L{PKG}/lib" in w and at > links["libletkf_amd.so"][0]


def test_the_default_goals_do_not_reach_it_and_a_twin_has_none(pkg):
    for args in (("-B",), ("-B", "CHECKED=1"), ("-B", "PROF=1")) + tuple(("-B", g) for g in OTHER_GOALS):
        assert not [w for w in plan(PKG, *args) if "h08" in " ".join(w)], args
    for args in (("-B",),) + tuple(("-B", g) for g in OTHER_GOALS):
        assert not [w for w in plan(FDIR, *args) if "h08" in " ".join(w)], args
    assert plan(PKG, "h08") == [], "the tree is not up to date"
    for own_header in ("/csrc/h08/letkf_h08_dev.h", "/../include/letkf_amd_h08.h"):
        own = {os.path.basename(w[w.index("-o") + 1]) for w in plan(PKG, "-W", PKG + own_header, "h08") if "-c" in w}
        assert own == {"letkf_h08.o", "letkf_h08_entry.o"}, own_header
        for goal in ("all",) + OTHER_GOALS:
            assert not plan(PKG, "-W", PKG + own_header, goal), (own_header, goal)      # no unit of the other libraries is built against it


@pytest.mark.skipif(not os.path.exists(FC), reason="amdflang not present")
def test_the_fortran_goal_links_the_driver_with_its_library_first():
    cmds = [w for w in plan(FDIR, "-B", "h08") if "-c" not in w and "-o" in w]
    assert [w[w.index("-o") + 1] for w in cmds] == ["h08_driver"]
    w = cmds[0]
    assert [x for x in w if x.startswith("-lletkf")] == ["-lletkf_amd_h08", "-lletkf_amd_obsfile", "-lletkf_amd_mapproj", "-lletkf_amd"]
    assert "-lamdhip64" in w
    assert [x for x in w if x.endswith(".o")] == ["letkf_h08_amd.o", "letkf_obsfile_amd.o", "letkf_mapproj_amd.o", "letkf_obsope_amd.o",
                                                   "letkf_amd_api.o"]


def test_the_one_build_call_makes_the_goals():
    src = open(os.path.join(PKG_DIR, "__init__.py")).read()
    assert '"-C", HERE, "h08"]' in src and "(H08_LIB_PATH,)" in src.split("stale =")[0]
    entry = open(os.path.join(os.path.dirname(PKG_DIR), "__graft_entry__.py")).read()
    assert 'os.path.join(PKG_DIR, "fortran"), "h08"]' in entry and "pkg.h08_lib()" in entry
    assert entry.index('"fortran"), "tcvital"]') < entry.index('"fortran"), "h08"]') and entry.index("pkg.tcvital_lib()") < entry.index("pkg.h08_lib()")
