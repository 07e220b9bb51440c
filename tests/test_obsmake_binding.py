"""The fifth companion header include/letkf_amd_obsmake.h and its mirrors, without a device: the ctypes structures against the
header field by field and against gcc's layout, the entries and their signature table, the six tables kept apart, the entries
exported by the library of the OSSE tools and NOT by the main one, their own host unit behind the exception barrier, the
second library in the Makefile, the Fortran BIND(C) types in C order and the new Fortran module under amdflang."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import pytest

from __graft_entry__ import PKG_DIR, ROOT, load_package

HEADER = os.path.join(ROOT, "include", "letkf_amd_obsmake.h")
FDIR = os.path.join(PKG_DIR, "fortran")
CSRC = os.path.join(PKG_DIR, "csrc")
FC = "/opt/rocm/bin/amdflang"
CTYPE = {"i32": C.c_int32, "i64": C.c_int64, "f64": C.c_double, "ptr": C.c_void_p}
ENTRIES = {"letkf_rand_create", "letkf_rand_destroy", "letkf_rand_set_chunk", "letkf_rand_res53", "letkf_randn_dev",
           "letkf_obsmake_slot_dev", "letkf_obsmake_noise_dev"}
STRUCTS = [("letkf_obsmake_slot", "ObsmakeSlot"), ("letkf_obsmake_err", "ObsmakeErr")]


@pytest.fixture(scope="module")
def pkg():
    p = load_package()
    p.build()
    return p


def header_text():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def header_fields(struct):
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
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "letkf_amd_obsmake.h"\nint main(void) {\n'
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


def test_the_osse_library_exports_the_entries_and_the_main_one_does_not(pkg):
    decl = dict(re.findall(r"^int\s+(letkf_\w+)\s*\(([^)]*)\)\s*;", header_text(), flags=re.M))
    assert set(decl) == set(pkg.OBSMAKE_ARGTYPES) == ENTRIES
    lib = pkg.osse_lib()
    for name, params in decl.items():
        want = [C.c_void_p if "*" in p else {"int32_t": C.c_int32, "int64_t": C.c_int64}[p.split()[0]] for p in params.split(",")]
        assert pkg.OBSMAKE_ARGTYPES[name] == want, name
        assert getattr(lib, name).argtypes == want and getattr(lib, name).restype == C.c_int
    assert int(re.search(r"#define LETKF_AMD_OBSMAKE_VERSION (\d+)", header_text()).group(1)) == pkg.OBSMAKE_VERSION == 1
    assert '#include "letkf_amd_obsope.h"' in header_text()
    assert callable(pkg.Context.randn) and callable(pkg.Context.obsmake_slot) and callable(pkg.Context.obsmake_noise) and callable(pkg.Rand)
    assert exported(pkg.OSSE_LIB_PATH) == ENTRIES
    assert not exported(pkg.LIB_PATH) & ENTRIES
    assert os.path.dirname(pkg.OSSE_LIB_PATH) == os.path.dirname(pkg.LIB_PATH)
    dyn = subprocess.check_output(["readelf", "-d", pkg.OSSE_LIB_PATH], text=True)
    assert "[libletkf_amd.so]" in dyn and "$ORIGIN" in dyn


def test_the_six_tables_are_pairwise_disjoint(pkg):
    tables = (pkg.ARGTYPES, pkg.INTERP_ARGTYPES, pkg.INTERP_WINDOW_ARGTYPES, pkg.OBSOPE_ARGTYPES, pkg.MONIT_ARGTYPES,
              pkg.OBSMAKE_ARGTYPES)
    for n, a in enumerate(tables):
        for b in tables[n + 1:]:
            assert not set(a) & set(b)
    assert list(pkg.EXPORTS) == list(pkg.ARGTYPES)
    for h in ("letkf_amd.h", "letkf_amd_obsope.h", "letkf_amd_monit.h"):
        text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", h)).read(), flags=re.S)
        assert not [n for n in ENTRIES if n in text]


def test_each_entry_is_defined_once_in_its_own_host_unit_behind_the_barrier():
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
        assert unit == "letkf_obsmake_entry.hip" and head == "try" and close == f"}} LETKF_ENTRY_END({name})", (name, where)
    unit = open(os.path.join(CSRC, "letkf_obsmake_entry.hip")).read()
    assert "__global__" not in unit and "hipLaunchKernelGGL" not in unit
    assert '#include "letkf_api_internal.h"' in unit
    sfmt = open(os.path.join(CSRC, "letkf_sfmt.cpp")).read()
    assert "#include <hip" not in sfmt and "__global__" not in sfmt and "__device__" not in sfmt          # host only
    mk = open(os.path.join(PKG_DIR, "Makefile")).read()
    units = re.search(r"^UNITS\s*:=(.*)$", mk, flags=re.M).group(1).split()
    osse = re.search(r"^OSSE_UNITS\s*:=(.*)$", mk, flags=re.M).group(1).split()
    assert osse == ["letkf_obsmake", "letkf_obsmake_entry", "letkf_sfmt"] and not set(osse) & set(units)
    assert re.search(r"^FLAGS_letkf_obsmake\s*:=\s*-ffp-contract=off\s*$", mk, flags=re.M)
    assert "letkf_amd_obsmake.h" in mk and "letkf_obsmake_dev.h" in mk and "-lletkf_amd" in mk
    assert re.search(r"^\$\(OSSE_OUT\):.*\n\tpython3 \$\(AUDIT\) -q --dir \$\(OSSE_OBJDIR\)\n", mk, flags=re.M)   # the audit before the link
    assert re.search(r"^all: \$\(OUT\) \$\(OSSE_OUT\)$", mk, flags=re.M)


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
    src = open(os.path.join(FDIR, "letkf_obsmake_amd.f90")).read()
    for struct, _ in STRUCTS:
        assert fortran_fields(src, struct) == header_fields(struct)
    assert set(re.findall(r"BIND\(C, name='(letkf_\w+)'\)", src)) == ENTRIES
    assert re.search(r"SUBROUTINE obsmake_slot_amd\(", src) and re.search(r"SUBROUTINE obsmake_noise_amd\(", src)
    drv = open(os.path.join(FDIR, "obsmake_driver.f90")).read()
    assert drv.rindex("CALL obsmake_slot_amd") < drv.rindex("CALL rand_create_amd") < drv.rindex("CALL obsmake_noise_amd")
    assert "obsmake_driver" in open(os.path.join(FDIR, "Makefile")).read()


@pytest.mark.skipif(not os.path.exists(FC), reason="amdflang not present")
def test_the_fortran_module_compiles_with_amdflang():
    with tempfile.TemporaryDirectory() as d:
        for f in ("letkf_amd_api.f90", "letkf_obsope_amd.f90", "letkf_obsmake_amd.f90"):
            subprocess.check_call([FC, "-O2", "-fPIC", "-c", os.path.join(FDIR, f), "-o", os.path.join(d, f[:-4] + ".o")], cwd=d)
        assert os.path.exists(os.path.join(d, "letkf_obsmake_amd.mod"))
