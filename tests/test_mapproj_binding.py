"""The ninth companion header include/letkf_amd_mapproj.h and its mirrors, without a device: the checks
test_companion_bindings.py makes for every row of its table, made here for this one companion with the same readers
(tests/_header.py) -- its units lie in csrc/mapproj/ and its library and driver hang on goals of their own, so it has no row in
that table.  Beside them the goal's plan, read from `make -n`, and the three host entries
(letkf_mapproj_setup and the one-point helpers) against the truth of tests/_mapproj.py, with every refusal of the setup."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import _header
import _mapproj as M
from __graft_entry__ import PKG_DIR, load_package

FDIR = os.path.join(PKG_DIR, "fortran")
FC = "/opt/rocm/bin/amdflang"
HEADER = "letkf_amd_mapproj.h"
ENTRIES = {"letkf_mapproj_setup", "letkf_phys2ij_dev", "letkf_ij2phys_dev", "letkf_mapproj_grid_dev", "letkf_phys2ij_host",
           "letkf_ij2phys_host"}
STRUCTS = {"letkf_mapproj_params": "MapprojParams", "letkf_mapproj": "Mapproj"}
UNITS = os.path.join(_header.CSRC, "mapproj")
UNIT = "letkf_mapproj_entry.hip"
MODULE, CHAIN = "letkf_mapproj_amd", ["letkf_amd_api"]
OTHER_LIBS = ("LIB_PATH", "OSSE_LIB_PATH", "OBSSIM_LIB_PATH", "SUPEROB_LIB_PATH", "OBSSCAN_LIB_PATH")
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
    table = pkg.MAPPROJ_SIGNATURES
    assert set(_header.entries(HEADER)) == set(table) == ENTRIES
    lib = pkg.mapproj_lib()
    for name in ENTRIES:
        want = _header.argtypes_of(name, HEADER)
        assert table[name] == want, name
        assert getattr(lib, name).argtypes == want and getattr(lib, name).restype is C.c_int, name
        assert _header.restype_of(name, HEADER) is C.c_int, name
    defines = _header.defines(HEADER)
    assert defines["LETKF_AMD_MAPPROJ_VERSION"] == pkg.MAPPROJ_VERSION == 1
    assert defines["LETKF_MAPPROJ_LC"] == pkg.MAPPROJ_LC == 1
    floats = dict(re.findall(r"^#define (LETKF_MAPPROJ_\w+) ([0-9.e]+)\s*$", _header.text(HEADER), flags=re.M))
    assert float(floats["LETKF_MAPPROJ_RADIUS_SCALE"]) == pkg.MAPPROJ_RADIUS_SCALE == M.RADIUS == 6.37122e6
    assert float(floats["LETKF_MAPPROJ_PI_REF"]) == pkg.MAPPROJ_PI_REF == M.PI_REF == 3.1415926535
    assert '#include "letkf_amd.h"' in _header.text(HEADER)
    assert _header.defines()["LETKF_AMD_ABI_VERSION"] == 11


def test_the_entries_are_exported_by_their_library_and_by_no_other(pkg):
    for path in OTHER_LIBS:
        assert not _header.exported(getattr(pkg, path)) & ENTRIES, path
    sat = pkg.MAPPROJ_LIB_PATH
    assert _header.exported(sat) == ENTRIES
    assert os.path.dirname(sat) == os.path.dirname(pkg.LIB_PATH)
    dyn = subprocess.check_output(["readelf", "-d", sat], text=True)
    assert "[libletkf_amd.so]" in dyn and "$ORIGIN" in dyn and "obsscan" not in dyn


def test_the_table_is_disjoint_from_the_other_nine_and_no_other_header_names_its_entries(pkg):
    others = [getattr(pkg, t) for t in dir(pkg) if t.endswith("ARGTYPES")]
    assert len(others) == 9
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
    # the point functions: one header, for the host and the device, which both units include
    point = open(os.path.join(UNITS, "letkf_mapproj_point.h")).read()
    assert point.count("__host__ __device__ inline") >= 6
    for unit in (UNIT, "letkf_mapproj.hip"):
        assert '#include "letkf_mapproj_point.h"' in open(os.path.join(UNITS, unit)).read(), unit
    kernels = re.sub(r"//.*", "", open(os.path.join(UNITS, "letkf_mapproj.hip")).read())
    assert kernels.count("__global__") == 3 and "__shared__" not in kernels and "atomic" not in kernels


def test_fortran_types_list_the_fields_in_c_order():
    src = open(os.path.join(FDIR, MODULE + ".f90")).read()
    assert _header.fortran_types(src) == _header.c_structs(HEADER)
    assert set(re.findall(r"BIND\(C, name='(letkf_\w+)'\)", src)) == ENTRIES
    assert re.findall(r"^\s*USE (\w+)", src, flags=re.M) == CHAIN
    for routine in ("mapproj_setup_amd", "phys2ij_amd", "ij2phys_amd", "mapproj_grid_amd"):
        assert re.search(rf"SUBROUTINE {routine}\(", src), routine


@pytest.mark.skipif(not os.path.exists(FC), reason="amdflang not present")
def test_the_fortran_module_compiles_with_amdflang(tmp_path):
    for f in CHAIN + [MODULE]:
        subprocess.check_call([FC, "-O2", "-fPIC", "-c", os.path.join(FDIR, f + ".f90"), "-o", str(tmp_path / (f + ".o"))], cwd=tmp_path)
    assert (tmp_path / (MODULE + ".mod")).exists()


def test_the_driver_projects_then_scans(pkg):
    assert callable(pkg.Context.phys2ij) and callable(pkg.Context.ij2phys) and callable(pkg.Context.mapproj_grid)
    drv = open(os.path.join(FDIR, "mapproj_driver.f90")).read()
    drv = drv[drv.index("PROGRAM mapproj_driver"):]
    assert drv.index("CALL mapproj_setup_amd") < drv.index("CALL phys2ij_amd") < drv.index("CALL obsscan_amd")
    assert "hipMemcpyDeviceToHost" not in drv[drv.index("CALL phys2ij_amd"):drv.index("CALL obsscan_amd")]   # ri / rj stay there


# ---- the build: what `make mapproj` would do, and that the default goal does not reach it
def plan(directory, *args):
    out = subprocess.check_output(["make", "-n", "--no-print-directory", "-C", directory, *args], text=True)
    return [line.split() for line in out.replace("\\\n", " ").splitlines() if not line.startswith("make")]


def test_the_goal_builds_the_sixth_library_as_a_satellite(pkg):
    cmds = plan(PKG, "-B", "mapproj")
    cc = {os.path.basename(w[w.index("-o") + 1])[:-2]: w for w in cmds if "-c" in w and "/obj_mapproj/" in w[w.index("-o") + 1]}
    assert set(cc) == {"letkf_mapproj", "letkf_mapproj_entry"}
    for u, w in cc.items():
        assert w[w.index("-c") + 1].endswith(f"csrc/mapproj/{u}.hip") and "--offload-arch=gfx950" in w and "-save-temps=obj" in w, w
        assert "-ffp-contract=off" in w and not [x for x in w if "fast-math" in x or x == "-Ofast"], w
    links = {os.path.basename(w[w.index("-o") + 1]): (n, w) for n, w in enumerate(cmds) if "-shared" in w}
    assert set(links) == {"libletkf_amd.so", "libletkf_amd_mapproj.so"}
    at, w = links["libletkf_amd_mapproj.so"]
    objdir = os.path.join(PKG, "lib", "obj_mapproj")
    assert sorted(x for x in w if x.endswith(".o")) == sorted(os.path.join(objdir, u + ".o") for u in cc)
    audit = cmds[at - 1]
    assert audit[0] == "python3" and audit[1].endswith("tools/isa_exec_audit.py") and audit[-2:] == ["--dir", objdir], audit
    assert "-lletkf_amd" in w and "-Wl,-rpath,'$ORIGIN'" in w and f"-L{PKG}/lib" in w and at > links["libletkf_amd.so"][0]


def test_the_default_goals_do_not_reach_it_and_a_twin_has_none(pkg):
    for args in (("-B",), ("-B", "CHECKED=1"), ("-B", "PROF=1"), ("-B", "obsscan")):
        assert not [w for w in plan(PKG, *args) if "mapproj" in " ".join(w)], args
    assert not [w for w in plan(FDIR, "-B") if "mapproj" in " ".join(w)]
    assert not [w for w in plan(FDIR, "-B", "obsscan") if "mapproj" in " ".join(w)]
    assert plan(PKG, "mapproj") == [], "the tree is not up to date"
    for own_header in ("/csrc/mapproj/letkf_mapproj_dev.h", "/csrc/mapproj/letkf_mapproj_point.h", "/../include/letkf_amd_mapproj.h"):
        own = {os.path.basename(w[w.index("-o") + 1]) for w in plan(PKG, "-W", PKG + own_header, "mapproj") if "-c" in w}
        assert own == {"letkf_mapproj.o", "letkf_mapproj_entry.o"}, own_header
        assert not plan(PKG, "-W", PKG + own_header, "all"), own_header       # no unit of the other libraries is built against it
        assert not plan(PKG, "-W", PKG + own_header, "obsscan"), own_header


@pytest.mark.skipif(not os.path.exists(FC), reason="amdflang not present")
def test_the_fortran_goal_links_the_driver_with_its_libraries_first():
    cmds = [w for w in plan(FDIR, "-B", "mapproj") if "-c" not in w and "-o" in w]
    assert [w[w.index("-o") + 1] for w in cmds] == ["mapproj_driver"]
    w = cmds[0]
    assert [x for x in w if x.startswith("-lletkf")] == ["-lletkf_amd_mapproj", "-lletkf_amd_obsscan", "-lletkf_amd"] and "-lamdhip64" in w
    assert [x for x in w if x.endswith(".o")] == ["letkf_mapproj_amd.o", "letkf_obsscan_amd.o", "letkf_obsope_amd.o", "letkf_amd_api.o"]


# ---- the host entries: no device is touched
@pytest.mark.parametrize("name", list(M.configs()))
def test_setup_derives_the_constants_of_the_truth(pkg, name):
    p = M.configs()[name]
    proj, q, t = pkg.mapproj_setup(**M.setup_args(p)), M.setup(p), M.mp_setup(p)
    assert (proj.type, proj.reserved0, proj.hemisphere) == (1, 0, q["h"])
    for k, b in M.bound_constants(p, t).items():
        assert M.err(getattr(proj, k), t[k]) <= b, k
    assert (proj.radius, proj.cxg1, proj.cyg1, proj.dx, proj.dy) == (p["radius"], p["cxg1"], p["cyg1"], p["dx"], p["dy"])


@pytest.mark.parametrize("name", list(M.configs()))
def test_the_host_helpers_agree_with_the_truth(pkg, name):
    p = M.configs()[name]
    proj, t = pkg.mapproj_setup(**M.setup_args(p)), M.mp_setup(p)
    lon, lat = M.points(7, 40, south=name == "south")
    got = [pkg.phys2ij_host(proj, float(a), float(b), rotc=True) for a, b in zip(lon, lat)]
    fwd = dict(ri=np.array([g[0] for g in got]), rj=np.array([g[1] for g in got]), rotc=np.array([g[2] for g in got]))
    M.check_rows(None, p, fwd, M.mp_phys2ij(t, lon, lat), name)
    assert [pkg.phys2ij_host(proj, float(a), float(b)) for a, b in zip(lon, lat)] == [g[:2] for g in got]     # without rotc
    back = [pkg.ij2phys_host(proj, g[0], g[1], rotc=True) for g in got]
    inv = dict(lon=np.array([g[0] for g in back]), lat=np.array([g[1] for g in back]), rotc=np.array([g[2] for g in back]))
    M.check_phys(inv, M.mp_ij2phys(t, fwd["ri"], fwd["rj"]), name)
    assert np.abs(inv["lon"] - lon).max() <= 2 * M.BOUND_DEG and np.abs(inv["lat"] - lat).max() <= 2 * M.BOUND_DEG
    # the undefined inputs, as the header decides them
    for a, b in ((np.nan, 35.0), (135.0, np.nan), (np.inf, 35.0), (135.0, np.inf), (135.0 + 720.0, 35.0)):
        ri, rj, rotc = pkg.phys2ij_host(proj, a, b, rotc=True)
        assert np.isnan(ri) and np.isnan(rj) and np.isnan(rotc[0]) and np.isnan(rotc[1]), (a, b)


REFUSALS = [
    (dict(type=0), "type"), (dict(type=2), "type"), (dict(type=-1), "type"),
    (dict(lc_lat1=37.5, lc_lat2=32.5), "lc_lat1"), (dict(lc_lat1=35.0, lc_lat2=35.0), "lc_lat1"),
    (dict(lc_lat1=-30.0, lc_lat2=30.0), "lc_lat1 + lc_lat2"),
    (dict(lc_lat2=90.0), "lc_lat"), (dict(lc_lat1=-90.0, lc_lat2=-30.0), "lc_lat"), (dict(lc_lat2=np.nan), "lc_lat"),
    (dict(basepoint_lat=90.0), "basepoint_lat"), (dict(basepoint_lat=-90.0), "basepoint_lat"), (dict(basepoint_lat=np.nan), "basepoint_lat"),
    (dict(basepoint_lon=np.inf), "basepoint_lon"), (dict(basepoint_x=np.nan), "basepoint_x"), (dict(cyg1=np.inf), "cyg1"),
    (dict(radius=0.0), "radius"), (dict(radius=-1.0), "radius"), (dict(radius=np.inf), "radius"), (dict(radius=np.nan), "radius"),
    (dict(dx=0.0), "dx"), (dict(dx=np.nan), "dx"), (dict(dy=-1000.0), "dy"), (dict(dy=np.inf), "dy"),
]


@pytest.mark.parametrize("change,word", REFUSALS, ids=[f"{list(c)[0]}={list(c.values())[0]}-{n}" for n, (c, _) in enumerate(REFUSALS)])
def test_setup_refuses_and_writes_nothing(pkg, change, word):
    args = dict(M.setup_args(M.configs()["BDA_d3_1km_9p_bf20"]), **change)
    with pytest.raises(pkg.LetkfError, match=re.escape(word)):
        pkg.mapproj_setup(**args)
    # ... through the C entry: the code, and proj as it was
    p, proj = pkg.MapprojParams(), pkg.Mapproj()
    p.type = args.pop("type", 1)
    for k, v in args.items():
        setattr(p, k, v)
    C.memset(C.addressof(proj), 0x5A, C.sizeof(proj))
    before = bytes(proj)
    assert pkg.mapproj_lib().letkf_mapproj_setup(C.addressof(p), C.addressof(proj)) == LETKF_E_INVALID
    assert bytes(proj) == before


def test_the_host_entries_refuse_null_and_a_proj_that_setup_did_not_make(pkg):
    lib, good = pkg.mapproj_lib(), pkg.mapproj_setup(**M.setup_args(M.configs()["BDA_d3_1km_9p_bf20"]))
    p = pkg.MapprojParams()
    assert lib.letkf_mapproj_setup(None, C.addressof(good)) == LETKF_E_INVALID
    assert lib.letkf_mapproj_setup(C.addressof(p), None) == LETKF_E_INVALID
    a, b = C.c_double(7.0), C.c_double(7.0)
    for entry in (lib.letkf_phys2ij_host, lib.letkf_ij2phys_host):
        assert entry(None, 135.0, 35.0, C.addressof(a), C.addressof(b), None) == LETKF_E_INVALID
        assert entry(C.addressof(good), 135.0, 35.0, None, C.addressof(b), None) == LETKF_E_INVALID
        assert entry(C.addressof(good), 135.0, 35.0, C.addressof(a), None, None) == LETKF_E_INVALID
        for field, value in (("type", 0), ("hemisphere", 0.0), ("c", 0.0), ("c", 1.5), ("fact", np.nan), ("radius", -1.0), ("dx", 0.0),
                             ("dy", np.inf), ("pole_y", np.nan)):
            bad = pkg.Mapproj.from_buffer_copy(bytes(good))
            setattr(bad, field, value)
            assert entry(C.addressof(bad), 135.0, 35.0, C.addressof(a), C.addressof(b), None) == LETKF_E_INVALID, field
            assert field in pkg.lib().letkf_amd_last_error().decode(), field
        assert (a.value, b.value) == (7.0, 7.0)
