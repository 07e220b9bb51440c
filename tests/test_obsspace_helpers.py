"""tests/_obsspace.py against the oracle's C functions, without a GPU: the flag every hand-built threshold row must get, the mesh
cell of every hand-built coordinate (the clamps taken as doubles: NaN, the infinities and magnitudes beyond 2^31 included), the
arithmetic of the departure's kld routes, and that the case builders produce what tests/test_gpu_obs_argspace.py says it runs."""
import numpy as np
import pytest

import _obsspace as S
from _obsprep import QcParams


def test_routes_at_160_kib():
    assert S.route_thresholds() == [(319, 320), (1279, 1280)]
    assert [S.departure_route(k) for k in (1, 7, 318, 319, 320, 323, 1001, 1279, 1280, 5000)] == \
        ["tile64"] * 4 + ["tile16"] * 4 + ["global"] * 2
    for lds in (64 * 1024, 64 * 1024 + 8 * 64, 160 * 1024):        # the rule, not one figure: a route changes at each pair only
        pairs = S.route_thresholds(lds)
        routes = [S.departure_route(k, lds) for k in range(1, 3000)]
        assert [(k, k + 1) for k in range(1, 2999) if routes[k - 1] != routes[k]] == pairs


@pytest.mark.parametrize("h08", [0, 1])
def test_threshold_rows_get_the_flags_stated(h08):
    r = S.threshold_rows(h08)
    prm = S.params(QcParams, S.TK, True, h08=h08)
    prm.h08_val2 = 1 if h08 else None
    ens, val, qc, v2 = S.oracle_departure(prm, r)
    bad = [(n, int(q), int(w)) for n, q, w in zip(r["name"], qc, r["want"]) if q != w]
    assert not bad, bad
    at = [i for i, n in enumerate(r["name"]) if n.endswith(" at")]
    assert len(at) == 8 + (2 if h08 else 0)
    for i in at:                                   # `exactly at` is exact: |y - mean| == GE * err in the oracle's own arithmetic
        ge = abs(val[i]) / r["err"][i]
        assert ge == float(int(ge * 2)) / 2 and ge >= 1.0, (r["name"][i], ge)
    skipped = r["qc"] > 0
    assert S.same_bits(ens[skipped], r["ens"][skipped]) and np.all(S.bits(val[skipped]) == S.CANARY)
    early = np.isin(qc, (S.QC_BAD, S.QC_REFMEM, S.QC_OTYPE))
    assert early.sum() >= 5 and np.all(S.bits(val[early]) == S.CANARY)         # rejected before the mean: val not written
    assert np.all(S.bits(ens[:, S.TK + 1:]) == S.CANARY)


def test_radar_switches_off():
    r = S.threshold_rows(0)
    prm = S.params(QcParams, S.TK, True, use_radar_ref=0, use_radar_vr=0)
    qc = S.oracle_departure(prm, r)[2]
    radar = np.isin(r["elm"], (S.ID_REF, S.ID_REF0, S.ID_VR)) & (r["qc"] <= 0)
    assert radar.sum() >= 20 and np.all(qc[radar] == S.QC_OTYPE) and np.array_equal(qc[~radar], r["want"][~radar])


def test_kld_cases_take_every_route():
    assert {S.departure_route(c[2]) for c in S.KLD_CASES} == {"tile64", "tile16", "global"}
    assert {(319, False, 319, 70), (320, False, 320, 70), (1279, False, 1279, 70), (1280, False, 1280, 70)} <= set(S.KLD_CASES)


@pytest.mark.parametrize("k,det,kld,nobs", S.KLD_CASES)
def test_dep_rows_take_every_branch(k, det, kld, nobs):
    r = S.kld_rows(k, kld, nobs)
    prm = S.params(QcParams, k, det, h08=1)
    prm.h08_val2 = 1
    ens, val, qc, v2 = S.oracle_departure(prm, r)
    live = r["qc"] <= 0
    assert {0, -1, S.QC_GROSS, S.QC_REFMEM, S.QC_BAD} <= set(qc[live].tolist()) and (r["qc"] > 0).sum() > 5
    assert S.same_bits(ens[:, k + 1:], r["ens"][:, k + 1:]) and S.same_bits(ens[~live], r["ens"][~live])
    assert not S.same_bits(v2, r["val2"])
    qc0 = S.oracle_departure(S.params(QcParams, k, det, h08=0), r)[2]        # the default build: 8800 rows are ordinary rows
    assert {0, S.QC_GROSS, S.QC_REFMEM, S.QC_BAD} <= set(qc0[live].tolist())


@pytest.mark.parametrize("fix", [0, 1])
@pytest.mark.parametrize("nctype", [1, 3])
@pytest.mark.parametrize("ngrd", S.NGRD_PAIRS)
@pytest.mark.parametrize("rank", [(0, 0), (2, 1)])
def test_mesh_rows_fall_in_the_cells_stated(ngrd, nctype, fix, rank):
    w = S.mesh_world(ngrd, nctype, fix, rank)
    r = S.mesh_rows(w)
    n_cell, key, ns = S.oracle_sort(w, r)
    good = np.nonzero(r["qc"] == 0)[0]
    assert ns == len(good) and np.all(key[ns:] == S.ICANARY)
    coff = np.concatenate([[0], np.cumsum(w["ngrd_i"].astype(np.int64) * w["ngrd_j"])])
    cell = np.array([coff[r["ctype"][n]] + np.dot(S.cell_np(w, r["ctype"][n], r["ri"][n], r["rj"][n]),
                                                  (1, w["ngrd_i"][r["ctype"][n]])) for n in good])
    order = np.lexsort((good, cell))               # by cell, then by row number
    assert np.array_equal(key[:ns], good[order])
    assert np.array_equal(n_cell, np.bincount(cell, minlength=w["ncell"]))
    if nctype > 1:
        assert n_cell[coff[nctype - 1]:].sum() == 0 and (r["ctype"] == nctype - 1).sum() > 0     # a type with rows, none accepted
    assert n_cell.max() >= 40                      # many rows in one cell
    # the hand-built points: a boundary belongs to the cell below it, the wild ones to an edge cell
    gi, gj = int(w["ngrd_i"][0]), int(w["ngrd_j"][0])
    assert S.cell_np(w, 0, np.inf, -np.inf) == (gi - 1, 0) and S.cell_np(w, 0, np.nan, np.nan) == (0, 0)
    assert S.cell_np(w, 0, 3.0e9, 1e300) == (gi - 1, gj - 1) and S.cell_np(w, 0, -3.0e9, -1e300) == (0, 0)
    i0 = rank[0] * S.NLON + S.IHALO + 0.5
    if gi % 2 == 0:
        mid = i0 + S.NLON / 2
        assert [S.cell_np(w, 0, x, 0.0)[0] for x in (S.DN(mid), mid, S.UP(mid))] == [gi // 2 - 1, gi // 2 - 1, gi // 2]


@pytest.mark.parametrize("px,py", [(3, 2), (1, 4)])
@pytest.mark.parametrize("fix", [0, 1])
def test_plan_world_reaches_past_the_neighbour(px, py, fix):
    w = S.plan_world(px, py, fix, empty_rank=px * py - 1)
    assert w["n_all"][-1].sum() == 0 and w["n_all"][0].sum() > 500
    tot = []
    for me in range(px * py):
        ac, src, nt = S.oracle_plan(w, me, w["total"])
        assert 0 < nt <= w["total"] and np.all(src[nt:] == S.ICANARY) and ac[-1] == nt
        tot.append(nt)
        assert S.oracle_plan(w, me, nt)[2] == nt and S.oracle_plan(w, me, nt - 1)[2] == -1
    if px == 3:                                    # type 1 reaches 7 cells in i: rank 0 holds rows of rank 2, two subdomains away
        ac, src, nt = S.oracle_plan(w, 0, w["total"])
        first2 = int(w["n_all"][:2].sum())
        own2 = int(w["n_all"][2].sum())
        assert np.any((src[:nt] >= first2) & (src[:nt] < first2 + own2))
