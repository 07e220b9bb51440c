"""No C++ exception leaves a C entry: every entry the headers declare is defined once -- the main header's in one of the
letkf_api*.hip units, the companions' where test_companion_bindings.py names them -- as a function-try-block that LETKF_ENTRY_END
closes (read from the sources), and the barrier behind that macro maps what is thrown
to LETKF_E_INVALID with its text (a stand-alone host program built from letkf_api_error.hip alone).  No GPU, no library."""
import os
import re
import subprocess
import textwrap

import _header
from __graft_entry__ import PKG_DIR
from test_companion_bindings import COMPANIONS

CSRC = os.path.join(PKG_DIR, "csrc")
# the two entries without a barrier: they take no context, allocate nothing and are what a caller reads after a failure
EXEMPT = {"letkf_amd_abi_version", "letkf_amd_last_error"}


def test_every_entry_is_defined_once_behind_the_barrier():
    defs = _header.definitions()
    api = {u for where in defs.values() for u, _, _ in where if u.startswith("letkf_api")}
    assert len(api) >= 7, sorted(api)
    for unit in api:
        assert "__global__" not in open(os.path.join(CSRC, unit)).read(), f"{unit}: a kernel in a unit of the host API"
    main = set(_header.entries())
    assert len(main) == 59 and EXEMPT <= main
    # the companions' entries, with their units, are test_companion_bindings.py's; here: they and the main header's are all there is
    companions = set().union(*(c.entries for c in COMPANIONS.values()))
    assert not main & companions
    missing = sorted((main | companions) - set(defs))
    assert not missing, f"declared, but defined in no unit: {missing}"
    assert not sorted(set(defs) - main - companions), f"defined as an entry, but declared in no header: {sorted(set(defs) - main - companions)}"
    for name in sorted(main):
        assert len(defs[name]) == 1, (name, [u for u, _, _ in defs[name]])
        unit, head, close = defs[name][0]
        assert unit in api, (name, unit)
        if name in EXEMPT:
            assert head == "" and unit == "letkf_api_error.hip", (name, unit, head)
            continue
        assert head == "try", f"{unit}: {name} is no function-try-block"
        want = f"}} LETKF_ENTRY_END({name})" if name != "letkf_core_c" else f"}} LETKF_ENTRY_END_TO({name}, if (status) *status =)"
        assert close == want, f"{unit}: {name} closes with {close!r}"
    # the macro itself: one handler for everything, through the one barrier function
    err_h = open(os.path.join(CSRC, "letkf_api_error.h")).read()
    assert re.search(r"#define LETKF_ENTRY_END_TO\(name, \.\.\.\) catch \(\.\.\.\) \{ __VA_ARGS__ letkf::api::fail_exception\(#name\); \}", err_h)
    assert "#define LETKF_ENTRY_END(name) LETKF_ENTRY_END_TO(name, return)" in err_h


MAIN = textwrap.dedent(r"""
    #include <cstdio>
    #include <cstring>
    #include <new>
    #include <stdexcept>
    #include "letkf_api_error.h"

    static int thrower(int what) try {
      if (what == 0) throw std::bad_alloc();
      if (what == 1) throw std::length_error("vector::_M_default_append");
      if (what == 2) throw 7;
      return letkf::api::fail(LETKF_E_HIP, "no exception");
    } LETKF_ENTRY_END(thrower)

    static void thrower_status(int what, int* status) try {
      if (what == 0) throw std::bad_alloc();
      *status = LETKF_OK;
    } LETKF_ENTRY_END_TO(thrower_status, if (status) *status =)

    int main() {
      for (int what = 0; what < 4; ++what) {
        const int rc = thrower(what);
        std::printf("%d|%d|%s\n", what, rc, letkf_amd_last_error());
      }
      int st = 12345;
      thrower_status(0, &st);
      std::printf("4|%d|%s\n", st, letkf_amd_last_error());
      thrower_status(0, nullptr);
      thrower_status(1, &st);
      std::printf("5|%d|%s\n", st, letkf_amd_last_error());
      return 0;
    }
""")


def test_the_barrier_maps_what_is_thrown(tmp_path):
    main = tmp_path / "main.cpp"
    main.write_text(MAIN)
    exe = tmp_path / "barrier"
    # the error unit as plain C++: a host compiler builds it alone, no HIP header in reach
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", CSRC, str(main), "-x", "c++",
                           os.path.join(CSRC, "letkf_api_error.hip"), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert not r.stderr, r.stderr
    lines = [line.split("|", 2) for line in r.stdout.splitlines()]
    inv, hip = str(_header.defines()["LETKF_E_INVALID"]), str(_header.defines()["LETKF_E_HIP"])
    assert lines[0][:2] == ["0", inv] and lines[0][2] == "thrower: std::bad_alloc", lines[0]
    assert lines[1] == ["1", inv, "thrower: vector::_M_default_append"], lines[1]
    assert lines[2] == ["2", inv, "thrower: unknown exception"], lines[2]
    assert lines[3] == ["3", hip, "no exception"], lines[3]                      # (a later fail() replaces the text)
    assert lines[4] == ["4", inv, "thrower_status: std::bad_alloc"], lines[4]    # the code goes to *status
    assert lines[5] == ["5", "0", "thrower_status: std::bad_alloc"], lines[5]    # (success leaves the text alone)
    assert len(lines) == 6

