"""The sixth companion header include/letkf_amd_obssim.h and its mirrors, without a device: the ctypes structures against the
header field by field and against gcc's layout, the entry and its signature table, the seven tables kept apart, the entry
exported by the simulator's library and by neither of the other two, its own host unit behind the exception barrier, the third
library in the Makefile, the Fortran BIND(C) types in C order, the new Fortran module under amdflang, and the one header that
holds the point physics both kernels use."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import pytest

from __graft_entry__ import PKG_DIR, ROOT, load_package

HEADER = os.path.join(ROOT, "include", "letkf_amd_obssim.h")
FDIR = os.path.join(PKG_DIR, "fortran")
CSRC = os.path.join(PKG_DIR, "csrc")
FC = "/opt/rocm/bin/amdflang"
CTYPE = {"i32": C.c_int32, "i64": C.c_int64, "f64": C.c_double, "ptr": C.c_void_p}
ENTRIES = {"letkf_obssim_dev"}
STRUCTS = [("letkf_obssim_params", "ObssimParams"), ("letkf_obssim_out", "ObssimOut")]


@pytest.fixture(scope="module")
def pkg():
    p = load_package()
    p.build()
    return p


def header_text():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def header_fields(struct):
    """[(kind, name, count)]: count > 0 for an array member"""
    body = re.search(r"typedef struct \{([^{}]*)\}\s*" + struct + ";", header_text()).group(1)
    out = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        base = re.match(r"(const\s+)?(int32_t|int64_t|double|float)\s+", decl)
        assert base, decl
        kind = {"int32_t": "i32", "int64_t": "i64", "double": "f64", "float": "f32"}[base.group(2)]
        for name in decl[base.end():].split(","):
            name = name.strip()
            arr = re.match(r"(\w+)\[(\d+)\]$", name)
            if name.startswith("*"):
                out.append(("ptr", name.lstrip("* "), 0))
            elif arr:
                out.append((kind, arr.group(1), int(arr.group(2))))
            else:
                out.append((kind, name, 0))
    return out


@pytest.mark.parametrize("struct,mirror", STRUCTS)
def test_ctypes_mirror_is_the_header_and_has_gccs_layout(pkg, struct, mirror):
    fields = header_fields(struct)
    cls = getattr(pkg, mirror)
    assert [(n, CTYPE[k] * c if c else CTYPE[k]) for k, n, c in fields] == list(cls._fields_)
    names = [n for _, n, _ in fields]
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "letkf_amd_obssim.h"\nint main(void) {\n'
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


def test_the_simulators_library_exports_the_entry_and_the_other_two_do_not(pkg):
    decl = dict(re.findall(r"^int\s+(letkf_\w+)\s*\(([^)]*)\)\s*;", header_text(), flags=re.M))
    assert set(decl) == set(pkg.OBSSIM_ARGTYPES) == ENTRIES
    lib = pkg.obssim_lib()
    for name, params in decl.items():
        want = [C.c_void_p if "*" in p else {"int32_t": C.c_int32, "int64_t": C.c_int64}[p.split()[0]] for p in params.split(",")]
        assert pkg.OBSSIM_ARGTYPES[name] == want, name
        assert getattr(lib, name).argtypes == want and getattr(lib, name).restype == C.c_int
    assert int(re.search(r"#define LETKF_AMD_OBSSIM_VERSION (\d+)", header_text()).group(1)) == pkg.OBSSIM_VERSION == 1
    assert '#include "letkf_amd_obsope.h"' in header_text()
    assert callable(pkg.Context.obssim)
    assert exported(pkg.OBSSIM_LIB_PATH) == ENTRIES
    assert not exported(pkg.LIB_PATH) & ENTRIES and not exported(pkg.OSSE_LIB_PATH) & ENTRIES
    assert os.path.dirname(pkg.OBSSIM_LIB_PATH) == os.path.dirname(pkg.LIB_PATH)
    dyn = subprocess.check_output(["readelf", "-d", pkg.OBSSIM_LIB_PATH], text=True)
    assert "[libletkf_amd.so]" in dyn and "$ORIGIN" in dyn
    assert int(re.search(r"#define LETKF_AMD_ABI_VERSION (\d+)", open(os.path.join(ROOT, "include", "letkf_amd.h")).read()).group(1)) == 11


def test_the_seven_tables_are_pairwise_disjoint(pkg):
    tables = (pkg.ARGTYPES, pkg.INTERP_ARGTYPES, pkg.INTERP_WINDOW_ARGTYPES, pkg.OBSOPE_ARGTYPES, pkg.MONIT_ARGTYPES,
              pkg.OBSMAKE_ARGTYPES, pkg.OBSSIM_ARGTYPES)
    for n, a in enumerate(tables):
        for b in tables[n + 1:]:
            assert not set(a) & set(b)
    for h in ("letkf_amd.h", "letkf_amd_obsope.h", "letkf_amd_monit.h", "letkf_amd_obsmake.h"):
        text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", h)).read(), flags=re.S)
        assert not [n for n in ENTRIES if n in text]


def test_the_entry_is_defined_once_in_its_own_host_unit_behind_the_barrier():
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
        assert unit == "letkf_obssim_entry.hip" and head == "try" and close == f"}} LETKF_ENTRY_END({name})", (name, where)
    unit = open(os.path.join(CSRC, "letkf_obssim_entry.hip")).read()
    assert "__global__" not in unit and "hipLaunchKernelGGL" not in unit
    assert '#include "letkf_api_internal.h"' in unit
    mk = open(os.path.join(PKG_DIR, "Makefile")).read()
    units = re.search(r"^UNITS\s*:=(.*)$", mk, flags=re.M).group(1).split()
    osse = re.search(r"^OSSE_UNITS\s*:=(.*)$", mk, flags=re.M).group(1).split()
    sim = re.search(r"^SIM_UNITS\s*:=(.*)$", mk, flags=re.M).group(1).split()
    assert sim == ["letkf_obssim", "letkf_obssim_entry"] and not set(sim) & (set(units) | set(osse))
    assert re.search(r"^SIM_OBJDIR\s*:=", mk, flags=re.M) and re.search(r"^SIM_OUT\s*:=.*libletkf_amd_obssim\.so$", mk, flags=re.M)
    assert re.search(r"^FLAGS_letkf_obssim\s*:=\s*-ffp-contract=off\s*$", mk, flags=re.M)
    assert "letkf_amd_obssim.h" in mk and "letkf_obssim_dev.h" in mk and "letkf_obsope_point_dev.h" in mk
    assert re.search(r"^\$\(SIM_OUT\):.*\n\tpython3 \$\(AUDIT\) -q --dir \$\(SIM_OBJDIR\)\n\t.*-lletkf_amd .*\$\$ORIGIN", mk, flags=re.M)   # the audit before the link
    assert re.search(r"^all: \$\(SIM_OUT\)$", mk, flags=re.M) and re.search(r"^all: \$\(OUT\) \$\(OSSE_OUT\)$", mk, flags=re.M)


def test_the_point_physics_lives_in_one_header_both_kernels_include():
    for unit in ("letkf_obsope.hip", "letkf_obssim.hip"):
        assert '#include "letkf_obsope_point_dev.h"' in open(os.path.join(CSRC, unit)).read(), unit
    hdr = open(os.path.join(CSRC, "letkf_obsope_point_dev.h")).read()
    for name in ("calc_ref_vr", "ceil_split", "term2", "term3", "radar_azimuth", "radar_distance", "radar_elevation"):
        assert re.search(r"__device__ inline \w+ " + name + r"\(", hdr), name
        for f in os.listdir(CSRC):
            if f.endswith(".hip"):
                assert not re.search(r"__device__[^;{]*\b" + name + r"\(", open(os.path.join(CSRC, f)).read()), (name, f)
    for f in os.listdir(CSRC):
        if f.endswith(".hip"):
            assert not re.search(r'#include\s+"[^"]*\.hip"', open(os.path.join(CSRC, f)).read()), f


def fortran_fields(src, name):
    body = re.search(r"TYPE, BIND\(C\) :: " + name + r"\n(.*?)END TYPE", src, flags=re.S).group(1)
    out = []
    for line in body.splitlines():
        line = line.split("!")[0]
        if "::" not in line:
            continue
        decl, names = line.split("::")
        kind = ("i32" if "c_int32_t" in decl else "i64" if "c_int64_t" in decl else "f64" if "c_double" in decl else
                "f32" if "c_float" in decl else "ptr")
        for n in names.split(","):
            arr = re.match(r"\s*(\w+)\((\d+)\)\s*$", n)
            out.append((kind, arr.group(1), int(arr.group(2))) if arr else (kind, n.strip(), 0))
    return out


def test_fortran_types_list_the_fields_in_c_order():
    src = open(os.path.join(FDIR, "letkf_obssim_amd.f90")).read()
    for struct, _ in STRUCTS:
        assert fortran_fields(src, struct) == header_fields(struct)
    assert set(re.findall(r"BIND\(C, name='(letkf_\w+)'\)", src)) == ENTRIES
    assert re.search(r"SUBROUTINE obssim_cal_amd\(", src)
    drv = open(os.path.join(FDIR, "obssim_driver.f90")).read()
    assert drv.rindex("CALL state_to_history_amd") < drv.rindex("CALL obssim_cal_amd") < drv.rindex("WRITE (uo, rec=irec)")
    assert "access='direct'" in drv
    assert "obssim_driver" in open(os.path.join(FDIR, "Makefile")).read()


@pytest.mark.skipif(not os.path.exists(FC), reason="amdflang not present")
def test_the_fortran_module_compiles_with_amdflang():
    with tempfile.TemporaryDirectory() as d:
        for f in ("letkf_amd_api.f90", "letkf_obsope_amd.f90", "letkf_obssim_amd.f90"):
            subprocess.check_call([FC, "-O2", "-fPIC", "-c", os.path.join(FDIR, f), "-o", os.path.join(d, f[:-4] + ".o")], cwd=d)
        assert os.path.exists(os.path.join(d, "letkf_obssim_amd.mod"))
