"""The second companion header include/letkf_amd_interp_window.h and its mirrors, without a device: the coarse lines a window
needs against their definition in plain Python (exhaustively on small domains), sharding.interp_tile_window against the same
definition, the two exported entries, the ctypes mirror of letkf_interp_window against gcc's layout, the Fortran BIND(C) type
in C order, the new Fortran module under amdflang, and the three signature tables kept apart."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

from __graft_entry__ import PKG_DIR, ROOT, load_package

HEADER = os.path.join(ROOT, "include", "letkf_amd_interp_window.h")
FDIR = os.path.join(PKG_DIR, "fortran")
FC = "/opt/rocm/bin/amdflang"


@pytest.fixture(scope="module")
def pkg():
    p = load_package()
    p.build()
    return p


def header_text():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def header_fields():
    body = re.search(r"typedef struct \{(.*?)\}\s*letkf_interp_window;", header_text(), flags=re.S).group(1)
    out = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            assert decl.startswith("int32_t "), decl
            out += [("i32", n.strip()) for n in decl[len("int32_t "):].split(",")]
    return out


def lattice(gn, s):
    """L of the header: {0, s, 2s, ...} united with {gn - 1}"""
    return sorted(set(range(0, gn, s)) | {gn - 1})


def needed(gn, s, p, q):
    """the global lines the owned range [p, q] needs, by the header's three clauses"""
    L = lattice(gn, s)
    run = [l for l in L if p <= l <= q]
    if p not in L:
        run.append(max(l for l in L if l < p))
    if q not in L:
        run.append(min(l for l in L if l > q))
    return sorted(run)


def corners(lines, i):
    """the existing cell rule on a run of lines (tests/_interp.py corners_of, one axis): [(weight, line)] of non-zero weight,
    near corner first"""
    ix = np.array(lines)
    ca = max(int(np.searchsorted(ix, i, side="right")) - 1, 0)
    a, b = int(ix[ca]), int(ix[min(ca + 1, len(ix) - 1)])
    w = (i - a) / (b - a) if b > a else 0.0
    return [(wt, l) for wt, l in ((1.0 - w, a), (w, b)) if wt != 0.0]


def raw_axis(pkg, gn, s, g0, n, o0, on):
    idx = np.full(on + 2, -9, dtype=np.int32)
    cnt = C.c_int32(-1)
    rc = pkg.lib().letkf_interp_window_axis(gn, s, g0, n, o0, on, idx.ctypes.data_as(C.c_void_p), C.byref(cnt))
    return rc, cnt.value, idx


def test_window_axis_is_the_definition_for_every_owned_range(pkg):
    """gn <= 14, strides 1..8, every [p, q]: once in the minimal array and once in a larger one (the whole domain); the run is
    contiguous in L, and the cell rule on it gives every owned point the global lattice's corners, weights and corner order"""
    ncase = 0
    for gn in range(1, 15):
        for s in range(1, 9):
            L = lattice(gn, s)
            assert list(pkg.interp_coarse_axis(gn, s)) == L
            for p in range(gn):
                for q in range(p, gn):
                    want = needed(gn, s, p, q)
                    assert want == L[L.index(want[0]):L.index(want[-1]) + 1]            # a contiguous run of L
                    g0 = min(want[0], p)
                    n = max(want[-1], q) - g0 + 1
                    for a0, an in ((g0, n), (0, gn)):
                        rc, cnt, idx = raw_axis(pkg, gn, s, a0, an, p - a0, q - p + 1)
                        assert rc == 0 and cnt == len(want), (gn, s, p, q, a0, an)
                        assert [int(v) + a0 for v in idx[:cnt]] == want
                        assert (idx[cnt:] == -9).all()
                        only = C.c_int32(-1)
                        assert pkg.lib().letkf_interp_window_axis(gn, s, a0, an, p - a0, q - p + 1, None, C.byref(only)) == 0
                        assert only.value == cnt
                    assert [int(v) + g0 for v in pkg.interp_window_axis(gn, s, g0, n, p - g0, q - p + 1)] == want
                    for i in range(p, q + 1):
                        assert corners(want, i) == corners(L, i), (gn, s, p, q, i)
                    # every cell of the run holds an owned point
                    ncel = max(len(want) - 1, 1)
                    for c in range(ncel):
                        a, b = want[c], want[min(c + 1, len(want) - 1)]
                        end = b if c == ncel - 1 else b - 1
                        assert max(a, p) <= min(end, q), (gn, s, p, q, c)
                    ncase += 1
    assert ncase == 8 * sum(gn * (gn + 1) // 2 for gn in range(1, 15))


def test_window_axis_refuses_a_needed_line_outside_the_arrays(pkg):
    E = -1
    # gn = 14, stride 4: L = 0 4 8 12 13.  Owned [5, 6] needs 4 and 8.
    assert raw_axis(pkg, 14, 4, 4, 5, 1, 2)[0] == 0                         # arrays [4, 8]
    assert raw_axis(pkg, 14, 4, 5, 4, 0, 2)[0] == E                         # arrays [5, 8]: 4 is missing
    assert raw_axis(pkg, 14, 4, 4, 4, 1, 2)[0] == E                         # arrays [4, 7]: 8 is missing
    assert raw_axis(pkg, 14, 4, 5, 2, 0, 2)[0] == E                         # the owned range alone
    # owned [13, 13], the domain's closing line, needs nothing else; owned [12, 12] neither
    assert raw_axis(pkg, 14, 4, 13, 1, 0, 1)[:2] == (0, 1)
    assert raw_axis(pkg, 14, 4, 12, 1, 0, 1)[:2] == (0, 1)
    with pytest.raises(pkg.LetkfError):
        pkg.interp_window_axis(14, 4, 5, 4, 0, 2)


def test_window_axis_refuses_bad_arguments(pkg):
    ok = (14, 4, 4, 5, 1, 2)
    assert raw_axis(pkg, *ok)[0] == 0
    for pos, val in ((0, 0), (1, 0), (2, -1), (2, 10), (3, 0), (4, -1), (4, 4), (5, 0), (5, 5)):
        bad = list(ok)
        bad[pos] = val
        assert raw_axis(pkg, *bad)[0] == -1, bad
    assert pkg.lib().letkf_interp_window_axis(*ok, None, None) == -1


def test_interp_tile_window_gives_the_minimal_rectangle_and_the_halo_columns(pkg):
    import importlib
    sharding = importlib.import_module("scale_letkf_amd.sharding")
    for nx_g, ny_g, px, py, sx, sy in ((7, 5, 2, 2, 2, 2), (7, 5, 2, 2, 3, 2), (7, 5, 2, 2, 8, 8), (24, 24, 2, 2, 3, 2), (13, 9, 3, 2, 4, 3)):
        tiles = sharding.tile_partition(nx_g, ny_g, px * py)
        assert sharding.tile_grid(px * py) == (px, py)
        for pj in range(py):
            for pi in range(px):
                i0, i1, j0, j1 = tiles[pi + px * pj]
                w = sharding.interp_tile_window(nx_g, ny_g, px, py, pi, pj, sx, sy)
                lx, ly = needed(nx_g, sx, i0, i1 - 1), needed(ny_g, sy, j0, j1 - 1)
                assert w["gi0"] == min(lx[0], i0) and w["gi0"] + w["nx"] - 1 == max(lx[-1], i1 - 1)
                assert w["gj0"] == min(ly[0], j0) and w["gj0"] + w["ny"] - 1 == max(ly[-1], j1 - 1)
                assert w["window"] == (nx_g, ny_g, w["gi0"], w["gj0"], i0 - w["gi0"], j0 - w["gj0"], i1 - i0, j1 - j0)
                win = w["window"]
                assert list(pkg.interp_window_axis(nx_g, sx, win[2], w["nx"], win[4], win[6])) == w["lines_x"] == [l - w["gi0"] for l in lx]
                assert list(pkg.interp_window_axis(ny_g, sy, win[3], w["ny"], win[5], win[7])) == w["lines_y"] == [l - w["gj0"] for l in ly]
                assert sorted(w["halo"]) == sorted((i, j) for i in lx for j in ly if not (i0 <= i < i1 and j0 <= j < j1))


def test_the_library_exports_both_entries_as_the_header_declares_them(pkg):
    decl = dict((name, params) for name, params in re.findall(r"^int\s+(letkf_\w+)\s*\(([^)]*)\)\s*;", header_text(), flags=re.M))
    assert set(decl) == set(pkg.INTERP_WINDOW_ARGTYPES) == {"letkf_interp_window_axis", "letkf_das_interp_window_dev"}
    lib = C.CDLL(pkg.LIB_PATH)
    for name, params in decl.items():
        assert hasattr(lib, name), name
        want = [C.c_void_p if "*" in p else {"int32_t": C.c_int32, "int64_t": C.c_int64}[p.split()[0]] for p in params.split(",")]
        assert pkg.INTERP_WINDOW_ARGTYPES[name] == want, name
        assert getattr(pkg.lib(), name).argtypes == want
    assert int(re.search(r"#define LETKF_AMD_INTERP_WINDOW_VERSION (\d+)", header_text()).group(1)) == pkg.INTERP_WINDOW_VERSION == 1
    assert not [a for a in dir(pkg.Context) if a.startswith("OPT_") and "INTERP" in a]
    assert callable(pkg.Context.das_interp_window)


def test_the_three_tables_are_pairwise_disjoint(pkg):
    tables = (pkg.ARGTYPES, pkg.INTERP_ARGTYPES, pkg.INTERP_WINDOW_ARGTYPES)
    for n, a in enumerate(tables):
        for b in tables[n + 1:]:
            assert not set(a) & set(b)
    assert list(pkg.EXPORTS) == list(pkg.ARGTYPES)                  # the main header's list stays the main header's
    assert pkg.INTERP_VERSION == 1 and set(pkg.INTERP_ARGTYPES) == {"letkf_interp_coarse_axis", "letkf_das_interp_dev"}


def test_ctypes_mirror_has_gccs_layout(pkg):
    fields = header_fields()
    assert [(n, C.c_int32) for _, n in fields] == list(pkg.InterpWindow._fields_)
    names = [n for _, n in fields]
    assert names == ["gnx", "gny", "gi0", "gj0", "oi0", "oj0", "onx", "ony"]
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "letkf_amd_interp_window.h"\nint main(void) {\n'
           '  printf("%zu\\n", sizeof(letkf_interp_window));\n' +
           "".join(f'  printf("%zu\\n", offsetof(letkf_interp_window, {n}));\n' for n in names) + "  return 0;\n}\n")
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "layout.c"), "w").write(src)
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(d, "layout.c"),
                               "-o", os.path.join(d, "layout")])
        out = [int(v) for v in subprocess.check_output([os.path.join(d, "layout")], text=True).split()]
    assert out[0] == C.sizeof(pkg.InterpWindow)
    assert out[1:] == [getattr(pkg.InterpWindow, n).offset for n in names]


def fortran_fields(src):
    body = re.search(r"TYPE, BIND\(C\) :: letkf_interp_window\n(.*?)END TYPE", src, flags=re.S).group(1)
    out = []
    for line in body.splitlines():
        line = line.split("!")[0]
        if "::" not in line:
            continue
        decl, names = line.split("::")
        kind = "i32" if "c_int32_t" in decl else "i64" if "c_int64_t" in decl else "f64" if "c_double" in decl else "ptr"
        out += [(kind, n.strip()) for n in names.split(",")]
    return out


def test_fortran_type_lists_the_fields_in_c_order():
    src = open(os.path.join(FDIR, "letkf_interp_window_amd.f90")).read()
    assert fortran_fields(src) == header_fields()
    assert set(re.findall(r"BIND\(C, name='(letkf_\w+)'\)", src)) == {"letkf_interp_window_axis", "letkf_das_interp_window_dev"}
    assert re.search(r"SUBROUTINE das_letkf_interp_window_amd\(ctx, args, tables, nx, ny, nlev, stride_x, stride_y", src)
    # the first companion's module is used, not restated
    assert "USE letkf_interp_amd" in src and "letkf_interp_coarse_axis" not in src


@pytest.mark.skipif(not os.path.exists(FC), reason="amdflang not present")
def test_the_fortran_module_compiles_with_amdflang():
    with tempfile.TemporaryDirectory() as d:
        for f in ("letkf_amd_api.f90", "letkf_interp_amd.f90", "letkf_interp_window_amd.f90"):
            subprocess.check_call([FC, "-O2", "-fPIC", "-c", os.path.join(FDIR, f), "-o", os.path.join(d, f[:-4] + ".o")], cwd=d)
        assert os.path.exists(os.path.join(d, "letkf_interp_window_amd.mod"))
