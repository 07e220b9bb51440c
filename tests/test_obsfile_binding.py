"""The tenth companion header include/letkf_amd_obsfile.h and its mirrors, without a device: the checks
tests/test_mapproj_binding.py makes for the ninth, made here for this one with the same readers (tests/_header.py) -- its units lie
in csrc/obsfile/ and its library and driver hang on goals of their own.  Beside them the goals' plans, read
from `make -n`, and the two host entries."""
import ctypes as C
import os
import re
import subprocess

import pytest

import _header
import _obsfile as O
from __graft_entry__ import PKG_DIR, load_package

FDIR = os.path.join(PKG_DIR, "fortran")
FC = "/opt/rocm/bin/amdflang"
HEADER = "letkf_amd_obsfile.h"
ENTRIES = {"letkf_obsfile_count", "letkf_obsfile_bytes", "letkf_obs_decode_dev", "letkf_obs_encode_dev", "letkf_obsda_assemble_dev",
           "letkf_obsda_encode_dev", "letkf_obsdep_encode_dev"}
STRUCTS = {"letkf_obsfile_cols": "ObsfileCols", "letkf_obsfile_params": "ObsfileParams", "letkf_obsda_params": "ObsdaParams",
           "letkf_obsda_cols": "ObsdaCols", "letkf_obsfile_rows": "ObsfileRows"}
UNITS = os.path.join(_header.CSRC, "obsfile")
UNIT, KERNELS = "letkf_obsfile_entry.hip", "letkf_obsfile.hip"
MODULE, CHAIN = "letkf_obsfile_amd", ["letkf_amd_api", "letkf_mapproj_amd"]
OTHER_LIBS = ("LIB_PATH", "OSSE_LIB_PATH", "OBSSIM_LIB_PATH", "SUPEROB_LIB_PATH", "OBSSCAN_LIB_PATH", "MAPPROJ_LIB_PATH")
PKG = os.path.realpath(PKG_DIR)
LETKF_E_INVALID = _header.defines()["LETKF_E_INVALID"]


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
    table = pkg.OBSFILE_SIGNATURES
    assert set(_header.entries(HEADER)) == set(table) == ENTRIES
    lib = pkg.obsfile_lib()
    for name in ENTRIES:
        want = _header.argtypes_of(name, HEADER)
        assert table[name] == want, name
        assert getattr(lib, name).argtypes == want and getattr(lib, name).restype is C.c_int, name
        assert _header.restype_of(name, HEADER) is C.c_int, name
    defines = _header.defines(HEADER)
    assert defines["LETKF_AMD_OBSFILE_VERSION"] == pkg.OBSFILE_VERSION == 1
    assert [defines["LETKF_OBSFILE_" + n] for n in ("CONV", "RADAR", "OBSDA", "DEP")] == [1, 2, 3, 4]
    assert (pkg.OBSFILE_CONV, pkg.OBSFILE_RADAR, pkg.OBSFILE_OBSDA, pkg.OBSFILE_DEP) == (O.CONV, O.RADAR, O.OBSDA, O.DEP) == (1, 2, 3, 4)
    assert defines["LETKF_OBSFILE_TILE_ROWS"] == pkg.OBSFILE_TILE_ROWS and defines["LETKF_OBSFILE_TILE_MEMBERS"] == pkg.OBSFILE_TILE_MEMBERS
    assert defines["LETKF_OBSFILE_MAX_MEMBERS"] == pkg.OBSFILE_MAX_MEMBERS == 2 ** 16 and defines["LETKF_OBSFILE_TYP_RADAR"] == pkg.OBSFILE_TYP_RADAR == 22
    assert '#include "letkf_amd_mapproj.h"' in _header.text(HEADER)
    assert _header.defines()["LETKF_AMD_ABI_VERSION"] == 11
    assert "read_obs_H08" in open(os.path.join(_header.INCLUDE, HEADER)).read()          # the format that stays out is named
    # the kernel's tile is the header's
    dev = open(os.path.join(UNITS, "letkf_obsfile_dev.h")).read()
    assert "kTileRows = LETKF_OBSFILE_TILE_ROWS" in dev and "kTileMembers = LETKF_OBSFILE_TILE_MEMBERS" in dev


def test_the_entries_are_exported_by_their_library_and_by_no_other(pkg):
    for path in OTHER_LIBS:
        assert not _header.exported(getattr(pkg, path)) & ENTRIES, path
    sat = pkg.OBSFILE_LIB_PATH
    assert _header.exported(sat) == ENTRIES
    assert os.path.dirname(sat) == os.path.dirname(pkg.LIB_PATH)
    dyn = subprocess.check_output(["readelf", "-d", sat], text=True)
    assert "[libletkf_amd.so]" in dyn and "$ORIGIN" in dyn and "obsscan" not in dyn and "mapproj" not in dyn


def test_the_table_is_disjoint_from_the_others_and_no_other_header_names_its_entries(pkg):
    others = [getattr(pkg, t) for t in dir(pkg) if t.endswith("ARGTYPES")] + [pkg.MAPPROJ_SIGNATURES]
    assert len(others) == 10
    for t in others:
        assert not set(t) & ENTRIES
    raw = open(os.path.join(_header.INCLUDE, HEADER)).read()                             # comments included
    for h in sorted(os.listdir(_header.INCLUDE)):
        if h != HEADER:
            assert not [n for n in ENTRIES if re.search(rf"\b{n}\b", _header.text(h))], h
            assert not [n for n in _header.entries(h) if re.search(rf"\b{n}\b", raw)], h


def test_each_entry_is_defined_once_in_its_unit_behind_the_barrier():
    defs = _header.definitions(UNITS)
    assert set(defs) == ENTRIES
    assert not set(_header.definitions()) & ENTRIES
    for name in ENTRIES:
        assert defs[name] == [(UNIT, "try", f"}} LETKF_ENTRY_END({name})")], (name, defs[name])
    src = open(os.path.join(UNITS, UNIT)).read()
    assert "__global__" not in src and "hipLaunchKernelGGL" not in src and "<<<" not in src
    assert '#include "letkf_api_internal.h"' in src and '#include "letkf_obsfile_dev.h"' in src
    assert "scan_ws(" in src and "scan_offsets(" in src                                  # the compaction uses the main library's scan
    kernels = re.sub(r"//.*", "", open(os.path.join(UNITS, KERNELS)).read())
    assert '#include "mapproj/letkf_mapproj_point.h"' in kernels and "lc_forward" in kernels
    assert "atomic" not in kernels and kernels.count("__global__") == 9
    assemble = kernels[kernels.index("void __launch_bounds__(kBlock) assemble_kernel"):kernels.index("count_total_kernel")]
    assert "__shared__ uint32_t tile[kTileMembers * P]" in assemble and "__syncthreads()" in assemble


def test_fortran_types_list_the_fields_in_c_order():
    src = open(os.path.join(FDIR, MODULE + ".f90")).read()
    assert _header.fortran_types(src) == _header.c_structs(HEADER)
    assert set(re.findall(r"BIND\(C, name='(letkf_\w+)'\)", src)) == ENTRIES
    assert re.findall(r"^\s*USE (\w+)", src, flags=re.M) == CHAIN[-1:]
    for routine in ("obsfile_count_amd", "obs_decode_amd", "obs_encode_amd", "obsda_assemble_amd", "obsda_encode_amd", "obsdep_encode_amd"):
        assert re.search(rf"SUBROUTINE {routine}\(", src), routine
    drv = open(os.path.join(FDIR, "obsfile_driver.f90")).read()
    assert drv.count("access='sequential'") >= 6 and drv.count("access='stream'") >= 2 and "WRITE (u) wk" in drv and "READ (u, iostat=ierr) wk" in drv


@pytest.mark.skipif(not os.path.exists(FC), reason="amdflang not present")
def test_the_fortran_module_compiles_with_amdflang(tmp_path):
    for f in CHAIN + [MODULE]:
        subprocess.check_call([FC, "-O2", "-fPIC", "-c", os.path.join(FDIR, f + ".f90"), "-o", str(tmp_path / (f + ".o"))], cwd=tmp_path)
    assert (tmp_path / (MODULE + ".mod")).exists()


def test_the_python_mirror_has_the_six_entries_and_the_two_conveniences(pkg):
    for name in ("obs_decode", "obs_encode", "obsda_assemble", "obsda_encode", "obsdep_encode", "read_obs_file", "read_obsda_files"):
        assert callable(getattr(pkg.Context, name)), name
    assert callable(pkg.obsfile_count) and callable(pkg.obsfile_bytes) and callable(pkg.obsfile_rows)


# ---- the build: what `make obsfile` would do, and that the default goals do not reach it
def plan(directory, *args):
    out = subprocess.check_output(["make", "-n", "--no-print-directory", "-C", directory, *args], text=True)
    return [line.split() for line in out.replace("\\\n", " ").splitlines() if not line.startswith("make")]


def test_the_goal_builds_the_seventh_library_as_a_satellite(pkg):
    cmds = plan(PKG, "-B", "obsfile")
    cc = {os.path.basename(w[w.index("-o") + 1])[:-2]: w for w in cmds if "-c" in w and "/obj_obsfile/" in w[w.index("-o") + 1]}
    assert set(cc) == {"letkf_obsfile", "letkf_obsfile_entry"}
    for u, w in cc.items():
        assert w[w.index("-c") + 1].endswith(f"csrc/obsfile/{u}.hip") and "--offload-arch=gfx950" in w and "-save-temps=obj" in w, w
        assert f"-I{PKG}/csrc" in w and not [x for x in w if "fast-math" in x or x == "-Ofast"], w
    assert "-ffp-contract=off" in cc["letkf_obsfile"]                                     # where letkf_mapproj_point.h is compiled
    links = {os.path.basename(w[w.index("-o") + 1]): (n, w) for n, w in enumerate(cmds) if "-shared" in w}
    assert set(links) == {"libletkf_amd.so", "libletkf_amd_obsfile.so"}
    at, w = links["libletkf_amd_obsfile.so"]
    objdir = os.path.join(PKG, "lib", "obj_obsfile")
    assert sorted(x for x in w if x.endswith(".o")) == sorted(os.path.join(objdir, u + ".o") for u in cc)
    audit = cmds[at - 1]
    assert audit[0] == "python3" and audit[1].endswith("tools/isa_exec_audit.py") and audit[-2:] == ["--dir", objdir], audit
    assert "-lletkf_amd" in w and "-Wl,-rpath,'$ORIGIN'" in w and f"-L{PKG}/lib" in w and at > links["libletkf_amd.so"][0]


def test_the_default_goals_do_not_reach_it_and_a_twin_has_none(pkg):
    for args in (("-B",), ("-B", "CHECKED=1"), ("-B", "PROF=1"), ("-B", "obsscan"), ("-B", "mapproj")):
        assert not [w for w in plan(PKG, *args) if "obsfile" in " ".join(w)], args
    for args in (("-B",), ("-B", "obsscan"), ("-B", "mapproj")):
        assert not [w for w in plan(FDIR, *args) if "obsfile" in " ".join(w)], args
    assert plan(PKG, "obsfile") == [], "the tree is not up to date"
    for own_header in ("/csrc/obsfile/letkf_obsfile_dev.h", "/../include/letkf_amd_obsfile.h"):
        own = {os.path.basename(w[w.index("-o") + 1]) for w in plan(PKG, "-W", PKG + own_header, "obsfile") if "-c" in w}
        assert own == {"letkf_obsfile.o", "letkf_obsfile_entry.o"}, own_header
        for goal in ("all", "obsscan", "mapproj"):
            assert not plan(PKG, "-W", PKG + own_header, goal), (own_header, goal)     # no unit of the other libraries is built against it


@pytest.mark.skipif(not os.path.exists(FC), reason="amdflang not present")
def test_the_fortran_goal_links_the_driver_with_its_libraries_first():
    cmds = [w for w in plan(FDIR, "-B", "obsfile") if "-c" not in w and "-o" in w]
    assert [w[w.index("-o") + 1] for w in cmds] == ["obsfile_driver"]
    w = cmds[0]
    assert [x for x in w if x.startswith("-lletkf")] == ["-lletkf_amd_obsfile", "-lletkf_amd_mapproj", "-lletkf_amd"] and "-lamdhip64" in w
    assert [x for x in w if x.endswith(".o")] == ["letkf_obsfile_amd.o", "letkf_mapproj_amd.o", "letkf_amd_api.o"]


# ---- the host entries: no device is touched
def test_count_and_bytes_are_the_statements(pkg):
    for fmt, nrecs in ((O.CONV, (8,)), (O.RADAR, (7, 8)), (O.OBSDA, (4, 6)), (O.DEP, (11,))):
        for nrec in nrecs:
            for rows in (0, 1, 7, 2 ** 24):
                nbytes = 4 * (O.HEAD_WORDS[fmt] + rows * (nrec + 2))
                assert pkg.obsfile_bytes(fmt, nrec, rows) == nbytes and pkg.obsfile_count(fmt, nrec, nbytes) == rows == O.count(fmt, nrec, nbytes)
            for nbytes in (4 * O.HEAD_WORDS[fmt] + 4, 4 * O.HEAD_WORDS[fmt] + 4 * (nrec + 2) + 1, 4 * O.HEAD_WORDS[fmt] - 4):
                assert O.count(fmt, nrec, nbytes) is None
                with pytest.raises(pkg.LetkfError, match="whole number of records|nbytes"):
                    pkg.obsfile_count(fmt, nrec, nbytes)
    n = C.c_int64(55)
    lib = pkg.obsfile_lib()
    for fmt, nrec in ((0, 8), (5, 8), (O.CONV, 7), (O.RADAR, 6), (O.OBSDA, 5), (O.DEP, 8)):
        assert lib.letkf_obsfile_count(fmt, nrec, 0, C.addressof(n)) == LETKF_E_INVALID and n.value == 55
        assert lib.letkf_obsfile_bytes(fmt, nrec, 0, C.addressof(n)) == LETKF_E_INVALID and n.value == 55
        assert re.search("format|nrec", pkg.lib().letkf_amd_last_error().decode())
    assert lib.letkf_obsfile_count(O.CONV, 8, 40, None) == LETKF_E_INVALID and lib.letkf_obsfile_bytes(O.CONV, 8, 1, None) == LETKF_E_INVALID
