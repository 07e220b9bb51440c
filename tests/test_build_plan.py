"""What `make` would do, read from `make -n` in the built tree and not from the Makefiles' text: which units each of the four
libraries links, with which flags they are compiled, the audit directly before every link, no satellite beside a twin, which
objects a changed header rebuilds, and the Fortran drivers with their libraries in link order.  No GPU, nothing is built."""
import os
import re
import subprocess

import pytest

from __graft_entry__ import PKG_DIR, load_package

PKG = os.path.realpath(PKG_DIR)          # (as make's own $(abspath ...) names the tree)
UNITS = {
    "": {"letkf_kernels", "letkf_wave", "letkf_wave2", "letkf_trio", "letkf_trivial", "letkf_eig", "letkf_staged", "letkf_gram",
         "letkf_krylov", "letkf_search", "letkf_obsprep", "letkf_setobs", "letkf_post", "letkf_setup", "letkf_exchange", "letkf_efso",
         "letkf_locadv", "letkf_efsonorm", "letkf_obsanal", "letkf_interp", "letkf_obsope", "letkf_monit", "letkf_api",
         "letkf_api_error", "letkf_api_das", "letkf_api_efso", "letkf_api_search", "letkf_api_obs", "letkf_api_grid",
         "letkf_monit_entry"},
    "_osse": {"letkf_obsmake", "letkf_obsmake_entry", "letkf_sfmt"},
    "_obssim": {"letkf_obssim", "letkf_obssim_entry"},
    "_superob": {"letkf_superob", "letkf_superob_entry"},
}
HOST_ONLY = {"letkf_sfmt"}
EVERY_HIP = {(f"obj{lib}", u) for lib, units in UNITS.items() for u in units - HOST_ONLY}
# a satellite's own headers, and some of those every unit of all four libraries is built against
OWN_HEADERS = {"_osse": ["../include/letkf_amd_obsmake.h", "csrc/letkf_obsmake_dev.h", "csrc/letkf_sfmt.h"],
               "_obssim": ["../include/letkf_amd_obssim.h", "csrc/letkf_obssim_dev.h"],
               "_superob": ["../include/letkf_amd_superob.h", "csrc/letkf_superob_dev.h"]}
MAIN_HEADERS = ["../include/letkf_amd.h", "../include/letkf_amd_obsope.h", "../include/letkf_amd_monit.h", "csrc/letkf_api_internal.h",
                "csrc/letkf_obsope_point_dev.h", "csrc/letkf_monit_dev.h", "csrc/letkf_device.h"]
DRIVERS = {"shim": None, "das": None, "das_letkf": None, "letkf_analysis": None, "efso": None, "obsanal": None, "efso_locadv": None,
           "efso_norm": None, "interp": None, "interp_window": None, "obsope": None, "monit": None, "obsmake": "osse",
           "obssim": "obssim", "superob": "superob"}


@pytest.fixture(scope="module", autouse=True)
def built():
    load_package().build()


def plan(directory, *args):
    """the commands of `make -n args`, one per entry (a continued line joined), each split into words"""
    out = subprocess.check_output(["make", "-n", "--no-print-directory", "-C", directory, *args], text=True)
    return [line.split() for line in out.replace("\\\n", " ").splitlines() if not line.startswith("make")]


def compiles(cmds):
    """{(object directory's name, unit): words} of the compile commands"""
    out = {}
    for w in cmds:
        if "-c" in w:
            obj = w[w.index("-o") + 1]
            key = (os.path.basename(os.path.dirname(obj)), os.path.basename(obj)[:-len(".o")])
            assert key not in out, key
            out[key] = w
    return out


def links(cmds):
    """{library's file name: (position among the commands, words)} of the link commands"""
    return {os.path.basename(w[w.index("-o") + 1]): (n, w) for n, w in enumerate(cmds) if "-shared" in w}


@pytest.fixture(scope="module")
def whole():
    return plan(PKG, "-B")


def test_each_library_links_exactly_its_units_with_the_audit_directly_before(whole):
    ln = links(whole)
    assert set(ln) == {f"libletkf_amd{lib}.so" for lib in UNITS}
    for n, a in enumerate(UNITS.values()):
        for b in list(UNITS.values())[n + 1:]:
            assert not a & b
    assert set(compiles(whole)) == {(f"obj{lib}", u) for lib, units in UNITS.items() for u in units}
    for lib, units in UNITS.items():
        at, w = ln[f"libletkf_amd{lib}.so"]
        objdir = os.path.join(PKG, "lib", f"obj{lib}")
        objects = [x for x in w if x.endswith(".o")]
        assert sorted(objects) == sorted(os.path.join(objdir, u + ".o") for u in units), lib
        audit = whole[at - 1]
        assert audit[0] == "python3" and audit[1].endswith("tools/isa_exec_audit.py") and audit[-2:] == ["--dir", objdir], (lib, audit)
        if lib:                        # a satellite finds the main library beside itself
            assert "-lletkf_amd" in w and "-Wl,-rpath,'$ORIGIN'" in w and f"-L{PKG}/lib" in w, w
            assert at > ln["libletkf_amd.so"][0]
        else:
            assert not [x for x in w if x.startswith("-lletkf")]


def test_the_flags_of_single_units_reach_their_compile_lines_and_no_other(whole):
    cc = compiles(whole)
    with_flag = lambda flag: {u for (_, u), w in cc.items() if flag in w}
    assert with_flag("-ffp-contract=off") == {"letkf_obsope", "letkf_monit", "letkf_obsmake", "letkf_obssim", "letkf_superob"}
    assert with_flag("-amdgpu-sched-strategy=max-memory-clause") == {"letkf_wave2"}
    assert {u for _, u in cc} - with_flag("--offload-arch=gfx950") == HOST_ONLY == {u for _, u in cc} - with_flag("-save-temps=obj")
    for (_, u), w in cc.items():
        assert w[w.index("-c") + 1].endswith(f"csrc/{u}" + (".cpp" if u in HOST_ONLY else ".hip")), w


@pytest.mark.parametrize("twin,name", [("CHECKED=1", "checked"), ("PROF=1", "prof")])
def test_a_twin_builds_no_satellite(twin, name):
    cmds = plan(PKG, "-B", twin)
    assert set(links(cmds)) == {f"libletkf_amd_{name}.so"}
    assert set(compiles(cmds)) == {(f"obj_{name}", u) for u in UNITS[""]}
    assert not [w for w in cmds if re.search(r"obj_(osse|obssim|superob)|libletkf_amd_(osse|obssim|superob)", " ".join(w))]


@pytest.mark.parametrize("lib,header", [(lib, h) for lib, hs in OWN_HEADERS.items() for h in hs] + [(None, h) for h in MAIN_HEADERS])
def test_a_changed_header_rebuilds_what_is_built_against_it(lib, header):
    """make -W pretends the file is new: a satellite's own header rebuilds that satellite alone, one of the main library's every
    .hip unit of all four"""
    assert plan(PKG, "all") == [], "the tree is not up to date"
    rebuilt = set(compiles(plan(PKG, "-W", PKG + "/" + header, "all")))      # (the path as the Makefile spells it)
    if lib:
        assert rebuilt and rebuilt <= {(f"obj{lib}", u) for u in UNITS[lib]} and rebuilt >= {(f"obj{lib}", u) for u in UNITS[lib] - HOST_ONLY}
    else:
        assert rebuilt == EVERY_HIP


def test_every_fortran_driver_is_built_with_its_satellite_library_first():
    cmds = [w for w in plan(os.path.join(PKG, "fortran"), "-B") if "-c" not in w and "-o" in w]
    built = {w[w.index("-o") + 1]: w for w in cmds}
    assert set(built) == {d + "_driver" for d in DRIVERS} and len(cmds) == len(DRIVERS)
    for d, sat in DRIVERS.items():
        w = built[d + "_driver"]
        ours = [x for x in w if x.startswith("-lletkf")]
        assert ours == ([f"-lletkf_amd_{sat}"] if sat else []) + ["-lletkf_amd"], (d, ours)
        assert ("-lamdhip64" in w) == (d != "shim")
