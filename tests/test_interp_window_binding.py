"""What only the second companion header include/letkf_amd_interp_window.h has (the checks every companion shares are in
test_companion_bindings.py): the coarse lines a window needs against their definition in plain Python (exhaustively on small
domains), sharding.interp_tile_window against the same definition, and the Fortran routine on top of the first companion's."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from __graft_entry__ import PKG_DIR, load_package

FDIR = os.path.join(PKG_DIR, "fortran")


@pytest.fixture(scope="module")
def pkg():
    p = load_package()
    p.build()
    return p


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


def test_the_fortran_routine_uses_the_first_companions_module(pkg):
    src = open(os.path.join(FDIR, "letkf_interp_window_amd.f90")).read()
    assert [n for n, _ in pkg.InterpWindow._fields_] == ["gnx", "gny", "gi0", "gj0", "oi0", "oj0", "onx", "ony"]
    assert not [a for a in dir(pkg.Context) if a.startswith("OPT_") and "INTERP" in a] and callable(pkg.Context.das_interp_window)
    assert re.search(r"SUBROUTINE das_letkf_interp_window_amd\(ctx, args, tables, nx, ny, nlev, stride_x, stride_y", src)
    # the first companion's module is used, not restated
    assert "USE letkf_interp_amd" in src and "letkf_interp_coarse_axis" not in src
