"""The companion headers include/letkf_amd_*.h and their mirrors, without a device -- one table, written out here, and the
same checks for every row of it: the ctypes structures against the header field by field and against gcc's layout, the
entries against the package's signature table and the loaded functions, the version, the library that exports the entries
(and that no other does), their definition behind the exception barrier in the unit named here, the Fortran BIND(C) types in
C order and the Fortran module under amdflang.  What only one companion has stays in that companion's own test file."""
import collections
import ctypes as C
import os
import re
import subprocess

import pytest

import _header
from __graft_entry__ import PKG_DIR, load_package

FDIR = os.path.join(PKG_DIR, "fortran")
FC = "/opt/rocm/bin/amdflang"

# table: the package's signature table (<table>_ARGTYPES) and version constant (<table>_VERSION); the header's macro is
# LETKF_AMD_<table>_VERSION.  lib: the package's path constant and loader of the library that exports the entries.  unit: where
# every entry is defined as a function-try-block, but for those in plain.  chain: the modules the Fortran module USEs, in
# compile order.
Companion = collections.namedtuple("Companion", "header entries structs table includes lib loader unit plain module chain")
MAIN_LIB, OSSE, OBSSIM, SUPEROB = ("LIB_PATH", "lib"), ("OSSE_LIB_PATH", "osse_lib"), ("OBSSIM_LIB_PATH", "obssim_lib"), \
    ("SUPEROB_LIB_PATH", "superob_lib")
# the two axis helpers are integer arithmetic on the caller's arrays beside the kernels that use the same rule: they allocate
# nothing and call nothing that throws, and are plain functions
COMPANIONS = {c.header[len("letkf_amd_"):-2]: c for c in (
    Companion("letkf_amd_interp.h", {"letkf_interp_coarse_axis", "letkf_das_interp_dev"}, {"letkf_interp_args": "InterpArgs"},
              "INTERP", "letkf_amd.h", *MAIN_LIB, "letkf_api_das.hip", {"letkf_interp_coarse_axis": "letkf_interp.hip"},
              "letkf_interp_amd", ["letkf_amd_api"]),
    Companion("letkf_amd_interp_window.h", {"letkf_interp_window_axis", "letkf_das_interp_window_dev"},
              {"letkf_interp_window": "InterpWindow"}, "INTERP_WINDOW", "letkf_amd_interp.h", *MAIN_LIB, "letkf_api_das.hip",
              {"letkf_interp_window_axis": "letkf_interp.hip"}, "letkf_interp_window_amd", ["letkf_amd_api", "letkf_interp_amd"]),
    Companion("letkf_amd_obsope.h", {"letkf_obsope_dev"}, {"letkf_obsope_fields": "ObsopeFields", "letkf_obsope_params": "ObsopeParams"},
              "OBSOPE", "letkf_amd.h", *MAIN_LIB, "letkf_api_obs.hip", {}, "letkf_obsope_amd", ["letkf_amd_api"]),
    Companion("letkf_amd_monit.h", {"letkf_state_to_history_dev", "letkf_monit_obs_dev", "letkf_monit_type"},
              {"letkf_hist_state": "HistState", "letkf_monit_params": "MonitParams", "letkf_obsdep": "Obsdep"},
              "MONIT", "letkf_amd_obsope.h", *MAIN_LIB, "letkf_monit_entry.hip", {}, "letkf_monit_amd",
              ["letkf_amd_api", "letkf_obsope_amd"]),
    Companion("letkf_amd_obsmake.h", {"letkf_rand_create", "letkf_rand_destroy", "letkf_rand_set_chunk", "letkf_rand_res53",
                                      "letkf_randn_dev", "letkf_obsmake_slot_dev", "letkf_obsmake_noise_dev"},
              {"letkf_obsmake_slot": "ObsmakeSlot", "letkf_obsmake_err": "ObsmakeErr"},
              "OBSMAKE", "letkf_amd_obsope.h", *OSSE, "letkf_obsmake_entry.hip", {}, "letkf_obsmake_amd",
              ["letkf_amd_api", "letkf_obsope_amd"]),
    Companion("letkf_amd_obssim.h", {"letkf_obssim_dev"}, {"letkf_obssim_params": "ObssimParams", "letkf_obssim_out": "ObssimOut"},
              "OBSSIM", "letkf_amd_obsope.h", *OBSSIM, "letkf_obssim_entry.hip", {}, "letkf_obssim_amd",
              ["letkf_amd_api", "letkf_obsope_amd"]),
    Companion("letkf_amd_superob.h", {"letkf_superob_dev", "letkf_superob_default_methods", "letkf_superob_slot_priority"},
              {"letkf_superob_params": "SuperobParams", "letkf_superob_out": "SuperobOut"},
              "SUPEROB", "letkf_amd.h", *SUPEROB, "letkf_superob_entry.hip", {}, "letkf_superob_amd", ["letkf_amd_api"]),
)}
LIBS = (MAIN_LIB, OSSE, OBSSIM, SUPEROB)
each = pytest.mark.parametrize("c", COMPANIONS.values(), ids=list(COMPANIONS))


@pytest.fixture(scope="module")
def pkg():
    p = load_package()
    p.build()
    return p


@each
def test_ctypes_mirrors_are_the_header_and_have_gccs_layout(pkg, c):
    structs = _header.structs(c.header)
    assert set(structs) == set(c.structs)
    for struct, fields in structs.items():
        cls = getattr(pkg, c.structs[struct])
        assert [(n, _header.field_ctype(k, cnt)) for k, n, cnt in fields] == list(cls._fields_), struct
        assert _header.sizeof(struct, c.header) == C.sizeof(cls), struct
        assert [_header.offsetof(struct, n, c.header) for _, n, _ in fields] == [getattr(cls, n).offset for _, n, _ in fields], struct


@each
def test_the_entries_are_typed_as_the_header_declares_them(pkg, c):
    table = getattr(pkg, c.table + "_ARGTYPES")
    assert set(_header.entries(c.header)) == set(table) == c.entries
    lib = getattr(pkg, c.loader)()
    for name in c.entries:
        want = _header.argtypes_of(name, c.header)
        assert table[name] == want, name
        assert getattr(lib, name).argtypes == want and getattr(lib, name).restype is C.c_int, name
        assert _header.restype_of(name, c.header) is C.c_int, name
    assert _header.defines(c.header)[f"LETKF_AMD_{c.table}_VERSION"] == getattr(pkg, c.table + "_VERSION") == 1
    assert f'#include "{c.includes}"' in _header.text(c.header)
    assert _header.defines()["LETKF_AMD_ABI_VERSION"] == 11


@each
def test_the_entries_are_exported_by_their_library_and_by_no_other(pkg, c):
    for path, _ in LIBS:
        got = _header.exported(getattr(pkg, path)) & c.entries
        assert got == (c.entries if path == c.lib else set()), path
    if c.lib != "LIB_PATH":             # a satellite: nothing else in it, beside the main library, which it finds there
        sat = getattr(pkg, c.lib)
        assert _header.exported(sat) == c.entries
        assert os.path.dirname(sat) == os.path.dirname(pkg.LIB_PATH)
        dyn = subprocess.check_output(["readelf", "-d", sat], text=True)
        assert "[libletkf_amd.so]" in dyn and "$ORIGIN" in dyn


def test_the_main_library_exports_its_tables_and_nothing_else(pkg):
    every = set(pkg.ARGTYPES).union(*(c.entries for c in COMPANIONS.values() if c.lib == "LIB_PATH"))
    assert _header.exported(pkg.LIB_PATH) == every


def test_the_eight_tables_are_pairwise_disjoint(pkg):
    tables = [pkg.ARGTYPES] + [getattr(pkg, c.table + "_ARGTYPES") for c in COMPANIONS.values()]
    assert len(tables) == 8
    for n, a in enumerate(tables):
        for b in tables[n + 1:]:
            assert not set(a) & set(b)
    assert list(pkg.EXPORTS) == list(pkg.ARGTYPES)                  # the main header's list stays the main header's
    headers = [_header.MAIN] + [c.header for c in COMPANIONS.values()]
    for c in COMPANIONS.values():
        for h in headers:
            if h != c.header:
                assert not [n for n in c.entries if re.search(rf"\b{n}\b", _header.text(h))], (c.header, h)


@each
def test_each_entry_is_defined_once_in_its_unit_behind_the_barrier(c):
    defs = _header.definitions()
    for name in c.entries:
        assert len(defs.get(name, ())) == 1, (name, defs.get(name))
        unit, head, close = defs[name][0]
        if name in c.plain:
            assert (unit, head, close) == (c.plain[name], "", "}"), (name, defs[name])
        else:
            assert (unit, head, close) == (c.unit, "try", f"}} LETKF_ENTRY_END({name})"), (name, defs[name])
    src = open(os.path.join(_header.CSRC, c.unit)).read()
    assert "__global__" not in src and "hipLaunchKernelGGL" not in src and "<<<" not in src
    assert '#include "letkf_api_internal.h"' in src


def test_only_the_two_axis_helpers_stand_outside_the_barrier():
    assert set().union(*(c.plain for c in COMPANIONS.values())) == {"letkf_interp_coarse_axis", "letkf_interp_window_axis"}


@each
def test_fortran_types_list_the_fields_in_c_order(c):
    src = open(os.path.join(FDIR, c.module + ".f90")).read()
    assert _header.fortran_types(src) == _header.c_structs(c.header)
    assert set(re.findall(r"BIND\(C, name='(letkf_\w+)'\)", src)) == c.entries
    assert re.findall(r"^\s*USE (\w+)", src, flags=re.M) == c.chain


@pytest.mark.skipif(not os.path.exists(FC), reason="amdflang not present")
@each
def test_the_fortran_module_compiles_with_amdflang(c, tmp_path):
    for f in c.chain + [c.module]:
        subprocess.check_call([FC, "-O2", "-fPIC", "-c", os.path.join(FDIR, f + ".f90"), "-o", str(tmp_path / (f + ".o"))], cwd=tmp_path)
    assert (tmp_path / (c.module + ".mod")).exists()
