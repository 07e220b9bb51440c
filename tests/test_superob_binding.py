"""The seventh companion header include/letkf_amd_superob.h and its mirrors, without a device: the ctypes structures against the
header field by field and against gcc's layout, the entries and their signature table, the eight tables kept apart, the entries
exported by superob's library and by none of the other three, the device entry in its own host unit behind the exception
barrier, the fourth library in the Makefile with the audit before the link, the Fortran BIND(C) types in C order, and the two
host-only helpers against the statement."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import _superob as S
from __graft_entry__ import PKG_DIR, ROOT, load_package

HEADER = os.path.join(ROOT, "include", "letkf_amd_superob.h")
FDIR = os.path.join(PKG_DIR, "fortran")
CSRC = os.path.join(PKG_DIR, "csrc")
CTYPE = {"i32": C.c_int32, "i64": C.c_int64, "f64": C.c_double, "ptr": C.c_void_p}
ENTRIES = {"letkf_superob_dev", "letkf_superob_default_methods", "letkf_superob_slot_priority"}
STRUCTS = [("letkf_superob_params", "SuperobParams"), ("letkf_superob_out", "SuperobOut")]


@pytest.fixture(scope="module")
def pkg():
    p = load_package()
    p.build()
    return p


def header_text():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def header_fields(struct):
    """[(kind, name)] in declaration order"""
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
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "letkf_amd_superob.h"\nint main(void) {\n'
           f'  printf("%zu\\n", sizeof({struct}));\n' +
           "".join(f'  printf("%zu\\n", offsetof({struct}, {n}));\n' for n in names) + "  return 0;\n}\n")
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "layout.c"), "w").write(src)
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(d, "layout.c"),
                               "-o", os.path.join(d, "layout")])
        out = [int(v) for v in subprocess.check_output([os.path.join(d, "layout")], text=True).split()]
    assert out[0] == C.sizeof(cls)
    assert out[1:] == [getattr(cls, n).offset for n in names]


def exported(path):
    out = subprocess.check_output(["nm", "-D", "--defined-only", path], text=True)
    return {line.split()[-1] for line in out.splitlines() if " T letkf_" in line}


def test_superobs_library_exports_the_entries_and_the_other_three_do_not(pkg):
    decl = dict(re.findall(r"^int\s+(letkf_\w+)\s*\(([^)]*)\)\s*;", header_text(), flags=re.M))
    assert set(decl) == set(pkg.SUPEROB_ARGTYPES) == ENTRIES
    lib = pkg.superob_lib()
    for name, params in decl.items():
        want = [C.c_void_p if "*" in p else {"int32_t": C.c_int32, "int64_t": C.c_int64}[p.split()[0]] for p in params.split(",")]
        assert pkg.SUPEROB_ARGTYPES[name] == want, name
        assert getattr(lib, name).argtypes == want and getattr(lib, name).restype == C.c_int
    assert int(re.search(r"#define LETKF_AMD_SUPEROB_VERSION (\d+)", header_text()).group(1)) == pkg.SUPEROB_VERSION == 1
    assert '#include "letkf_amd.h"' in header_text()
    assert callable(pkg.Context.superob)
    assert exported(pkg.SUPEROB_LIB_PATH) == ENTRIES
    for other in (pkg.LIB_PATH, pkg.OSSE_LIB_PATH, pkg.OBSSIM_LIB_PATH):
        assert not exported(other) & ENTRIES, other
    assert os.path.dirname(pkg.SUPEROB_LIB_PATH) == os.path.dirname(pkg.LIB_PATH)
    dyn = subprocess.check_output(["readelf", "-d", pkg.SUPEROB_LIB_PATH], text=True)
    assert "[libletkf_amd.so]" in dyn and "$ORIGIN" in dyn
    assert int(re.search(r"#define LETKF_AMD_ABI_VERSION (\d+)", open(os.path.join(ROOT, "include", "letkf_amd.h")).read()).group(1)) == 11


def test_the_eight_tables_are_pairwise_disjoint(pkg):
    tables = (pkg.ARGTYPES, pkg.INTERP_ARGTYPES, pkg.INTERP_WINDOW_ARGTYPES, pkg.OBSOPE_ARGTYPES, pkg.MONIT_ARGTYPES,
              pkg.OBSMAKE_ARGTYPES, pkg.OBSSIM_ARGTYPES, pkg.SUPEROB_ARGTYPES)
    for n, a in enumerate(tables):
        for b in tables[n + 1:]:
            assert not set(a) & set(b)
    for h in ("letkf_amd.h", "letkf_amd_obsope.h", "letkf_amd_monit.h", "letkf_amd_obsmake.h", "letkf_amd_obssim.h"):
        text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", h)).read(), flags=re.S)
        assert not [n for n in ENTRIES if n in text]


def test_the_entries_are_defined_once_in_their_own_host_unit_behind_the_barrier():
    defs = {}
    for f in sorted(os.listdir(CSRC)):
        if not f.endswith((".hip", ".cpp")):
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
        assert unit == "letkf_superob_entry.hip" and head == "try" and close == f"}} LETKF_ENTRY_END({name})", (name, where)
    unit = open(os.path.join(CSRC, "letkf_superob_entry.hip")).read()
    assert "__global__" not in unit and "hipLaunchKernelGGL" not in unit and "<<<" not in unit
    assert '#include "letkf_api_internal.h"' in unit
    kernels = open(os.path.join(CSRC, "letkf_superob.hip")).read()
    assert len(re.findall(r"__global__[^;{]*\bsuperob_select_kernel\(", kernels)) == 1      # one select kernel for both stages
    assert "superob_select_kernel<true>" in kernels and "superob_select_kernel<false>" in kernels


def test_the_makefile_has_a_fourth_library_with_lists_of_its_own_and_the_audit_before_the_link():
    mk = open(os.path.join(PKG_DIR, "Makefile")).read()
    units = re.search(r"^UNITS\s*:=(.*)$", mk, flags=re.M).group(1).split()
    osse = re.search(r"^OSSE_UNITS\s*:=(.*)$", mk, flags=re.M).group(1).split()
    sim = re.search(r"^SIM_UNITS\s*:=(.*)$", mk, flags=re.M).group(1).split()
    sup = re.search(r"^SUP_UNITS\s*:=(.*)$", mk, flags=re.M).group(1).split()
    assert sup == ["letkf_superob", "letkf_superob_entry"] and not set(sup) & (set(units) | set(osse) | set(sim))
    assert osse == ["letkf_obsmake", "letkf_obsmake_entry", "letkf_sfmt"] and sim == ["letkf_obssim", "letkf_obssim_entry"]
    assert re.search(r"^SUP_OBJDIR\s*:=", mk, flags=re.M) and re.search(r"^SUP_OUT\s*:=.*libletkf_amd_superob\.so$", mk, flags=re.M)
    assert re.search(r"^FLAGS_letkf_superob\s*:=\s*-ffp-contract=off\s*$", mk, flags=re.M)
    assert "letkf_amd_superob.h" in mk and "letkf_superob_dev.h" in mk
    assert re.search(r"^\$\(SUP_OUT\):.*\n\tpython3 \$\(AUDIT\) -q --dir \$\(SUP_OBJDIR\)\n\t.*-lletkf_amd .*\$\$ORIGIN", mk, flags=re.M)
    assert re.search(r"^all: \$\(SUP_OUT\)$", mk, flags=re.M)
    production, twins = re.search(r"^ifeq \(\$\(OUT\),\$\(HERE\)lib/libletkf_amd\.so\)\n(.*?)^else\n(.*?)^endif", mk, flags=re.M | re.S).groups()
    assert "$(SUP_OUT)" in production and twins.strip() == "all: $(OUT)"                    # the twins have none


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
    src = open(os.path.join(FDIR, "letkf_superob_amd.f90")).read()
    for struct, _ in STRUCTS:
        assert fortran_fields(src, struct) == header_fields(struct)
    assert set(re.findall(r"BIND\(C, name='(letkf_\w+)'\)", src)) == ENTRIES
    assert re.search(r"SUBROUTINE superob_amd\(", src)
    drv = open(os.path.join(FDIR, "superob_driver.f90")).read()
    assert drv.rindex("CALL superob_amd") < drv.rindex("letkf_ctx_synchronize") < drv.rindex("WRITE (uo)")
    assert "access='sequential'" in drv
    assert "superob_driver" in open(os.path.join(FDIR, "Makefile")).read()


def test_the_host_helpers_are_the_statements(pkg):
    for nslots, nbslot in ((7, 4), (1, 1), (4, 1), (64, 33), (5, 5), (6, 3)):
        assert [int(s) for s in pkg.superob_slot_priority(nslots, nbslot)] == S.slot_priority(nslots, nbslot)
    assert [int(s) for s in pkg.superob_slot_priority(7, 4)] == [4, 3, 5, 2, 6, 1, 7]
    for nobtype, nid in ((24, 16), (4, 4), (32, 32), (1, 1)):
        for a, b in zip(pkg.superob_default_methods(nobtype, nid), S.default_methods(nobtype, nid)):
            assert a.shape == (nid, nobtype) and np.array_equal(a, b)
    for bad in ((0, 1), (65, 1), (3, 0), (3, 4)):
        with pytest.raises(pkg.LetkfError):
            pkg.superob_slot_priority(*bad)
    for bad in ((0, 4), (33, 4), (4, 0), (4, 33)):
        with pytest.raises(pkg.LetkfError):
            pkg.superob_default_methods(*bad)
    assert pkg.SUPEROB_SURFACE_TYPES == S.SURFACE_TYPES == sum(1 << (t - 1) for t in (8, 9, 10, 11, 15))
