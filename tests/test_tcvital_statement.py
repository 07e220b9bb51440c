"""tests/_tcvital.py, the numpy restatement of the TC vitals (include/letkf_amd_tcvital.h) and the fixtures of
tests/test_gpu_tcvital.py, pinned so that no device test can hide behind them: every seeded fixture has a clear winner, the exact
fixtures are exact in any order of the sums, and a decomposed grid gives the undivided one.  No device."""
import numpy as np
import pytest

import _tcvital as T


def whole(name):
    nlon, nlat, ih, jh, nmem, seed = T.FIXTURES[name]
    v, ci, cj = T.low_fixture(nlon, nlat, ih, jh, nmem, seed)
    return nlon, nlat, ih, jh, nmem, v, ci, cj


@pytest.mark.parametrize("name", sorted(T.FIXTURES))
def test_every_member_of_every_fixture_has_a_clear_winner(name):
    """128 eps = 2.8e-14 would do for the location to be exact under the device tests' 64 eps on s; the fixtures keep 1e-9."""
    nlon, nlat, ih, jh, nmem, v, ci, cj = whole(name)
    p = T.params()
    worst = np.inf
    for m in range(nmem):
        for centre in range(nmem):                                    # the device tests search every member around one centre
            g = T.gap(v[m], nlon, nlat, ih, jh, p, ci[centre], cj[centre])
            worst = min(worst, g)
    print(f"{name}: worst relative gap {worst:.3e}")
    assert worst >= 1.0e-9
    assert 128 * T.EPS < 1.0e-9


def test_every_search_the_device_tests_hold_to_a_location_has_a_clear_winner():
    """... also under the disc that cuts the grid, and where the lowest cell is a NaN"""
    worst = np.inf
    for name, over, centre in T.SEARCHES:
        nlon, nlat, ih, jh, nmem, v, ci, cj = whole(name)
        for m in range(nmem):
            worst = min(worst, T.gap(v[m], nlon, nlat, ih, jh, T.params(**over), ci[centre], cj[centre]))
    nlon, nlat, ih, jh, nmem = T.FIXTURES["main"][:5]
    v, p, ritc, rjtc = T.nothing_cases()["nan minimum"]
    for m in range(nmem):
        worst = min(worst, T.gap(v[m], nlon, nlat, ih, jh, p, ritc, rjtc))
    print(f"worst relative gap {worst:.3e}")
    assert worst >= 1.0e-9


@pytest.mark.parametrize("name", sorted(T.FIXTURES))
def test_the_fixtures_are_what_the_issue_of_the_search_needs(name):
    nlon, nlat, ih, jh, nmem, v, ci, cj = whole(name)
    topo = v[:, T.IV_TOPO]
    assert 0.6 < (topo != 0.0).mean() < 0.8                           # terrain on about 70 % of the cells
    assert (np.abs(ci - np.round(ci)) > 0.05).all() and (np.abs(cj - np.round(cj)) > 0.05).all()   # centres off the lattice
    assert len({(round(a, 6), round(b, 6)) for a, b in zip(ci, cj)}) == nmem                        # ... one per member
    # the winner lies near the member's own centre and the pressure there is a cyclone's
    p = T.params()
    for m in range(nmem):
        (tcx, tcy, mslp), (ig, jg) = T.search_member(v[m], nlon, nlat, ih, jh, p, ci[m], cj[m])
        assert abs(ig - ci[m]) < 3 and abs(jg - cj[m]) < 3 and 960.0e2 < mslp < 1000.0e2
        assert tcx == (ig - 1.0) * p["dx"] + p["cxg1"] and tcy == (jg - 1.0) * p["dy"] + p["cyg1"]


def test_topography_zero_leaves_ps_bit_for_bit_and_reads_nothing_else():
    v = T.exact_fixture(9, 7, 2, 2, 1, [(4, 3)])
    assert np.array_equal(T.slp(v[0]), v[0, T.IV_PS]) and np.isnan(v[0, T.IV_T2M]).all()


def test_the_exact_fixtures_are_exact_in_any_order_of_the_sums():
    nlon, nlat, ih, jh = 37, 29, 2, 2
    dips = [(8, 10), (34, 10), (14, 16), (14, 22)]
    v = T.exact_fixture(nlon, nlat, ih, jh, 2, dips)
    assert (v[:, T.IV_PS] == np.round(v[:, T.IV_PS])).all() and v[:, T.IV_PS].max() < 2.0 ** 40 / 45
    for m in range(2):
        a = T.slp(v[m])
        s = T.smoothed(v[m], nlon, nlat, ih, jh)
        rng = np.random.default_rng(m)
        for j, i in [(9, 7), (9, 33), (15, 13), (21, 13), (10, 8), (0, 0), (28, 36)]:      # 0-based interior cells
            blk = a[j:j + 5, i:i + 5]                                                        # (the halo is 2: the 5 x 5 block)
            c, s3 = blk[2, 2], None
            for order in range(3):
                t5, t3 = rng.permutation(blk.ravel()), rng.permutation(blk[1:4, 1:4].ravel())
                s5, s3 = 0.0, 0.0
                for x in t5:
                    s5 += x
                for x in t3:
                    s3 += x
                assert (c * 5.0 + (s3 - c) * 3.0 + (s5 - s3)) / 45.0 == s[j, i]
        # four cells share the minimum; the winner is the lowest j, then the lowest i
        low = s.min()
        assert sorted((int(i) + 1, int(j) + 1) for j, i in np.argwhere(s == low)) == sorted(dips)
        (_, _, mslp), cell = T.search_member(v[m], nlon, nlat, ih, jh, T.params(), 18.0, 15.0)
        assert cell == (8, 10) and mslp == low == 101000.0 - (4500.0 + 45.0 * m) * 5.0 / 45.0


def test_the_rim_of_the_disc_is_inside_and_one_ulp_less_is_not():
    nlon, nlat, ih, jh = 37, 29, 2, 2
    v = T.exact_fixture(nlon, nlat, ih, jh, 1, [(20 + 3, 12 + 4)])
    p = T.params(tc_search_dis=10000.0)
    _, cell = T.search_member(v[0], nlon, nlat, ih, jh, p, 20.0, 12.0)
    assert cell == (23, 16)
    p["tc_search_dis"] = np.nextafter(10000.0, 0.0)
    _, cell = T.search_member(v[0], nlon, nlat, ih, jh, p, 20.0, 12.0)
    assert cell is not None and cell != (23, 16)


def test_nothing_to_find():
    nlon, nlat, ih, jh = 12, 10, 2, 2
    v, ci, cj = T.low_fixture(nlon, nlat, ih, jh, 2, 5)
    none = [[T.NONE] * 3] * 2
    assert T.search(v, nlon, nlat, ih, jh, T.params(tc_search_dis=6000.0), 40.0, 40.0).tolist() == none      # disc outside
    assert T.search(v, nlon, nlat, ih, jh, T.params(tc_search_dis=0.0), 5.5, 5.0).tolist() == none           # off a cell
    assert T.search(v, nlon, nlat, ih, jh, T.params(tc_search_dis=0.0), 5.0, 5.0)[0, 2] < T.CAP              # on a cell: that cell
    assert T.search(v, nlon, nlat, ih, jh, T.params(), np.nan, 5.0).tolist() == none
    assert T.search(v, nlon, nlat, ih, jh, T.params(), 5.0, np.nan).tolist() == none
    w = v.copy()
    w[:, T.IV_PS] = np.nan
    assert T.search(w, nlon, nlat, ih, jh, T.params(), 5.0, 5.0).tolist() == none                           # a NaN s never wins


def test_a_two_by_two_decomposition_gives_the_undivided_grid():
    nlon, nlat, ih, jh, nmem, v, ci, cj = whole("seams")
    sub_i, sub_j = nlon // 2, nlat // 2
    p = T.params()
    for centre in range(nmem):
        one = T.search(v, nlon, nlat, ih, jh, p, ci[centre], cj[centre])
        cands = []
        for rank in range(4):
            ri, rj = rank % 2, rank // 2
            q = dict(p, i_off=ri * sub_i, j_off=rj * sub_j)
            cands.append(T.search(T.cut(v, ri, rj, sub_i, sub_j, ih, jh), sub_i, sub_j, ih, jh, q, ci[centre], cj[centre]))
        cands = np.array(cands)
        assert (cands[:, :, 2] < T.NONE).sum() >= nmem + 1                     # (more than one rank has a candidate)
        qc, ens = np.full(5, 90, dtype=np.int32), np.zeros((5, nmem))
        T.fill(cands, [1, 2, 3], True, qc, ens, 0)
        assert np.array_equal(ens[1:4].T.view(np.int64), one.view(np.int64)) and qc.tolist() == [90, 0, 0, 0, 90]


def test_fill_and_rows():
    cand = np.array([[[1.0, 2.0, 990.0e2], [T.NONE] * 3], [[3.0, 4.0, 990.0e2], [5.0, 6.0, 1100.0e2]]])
    qc, ens = np.array([0, 90, 90, 90], dtype=np.int32), np.zeros((4, 3))
    T.fill(cand, [1, -1, 3], True, qc, ens, 1)
    assert ens[1].tolist() == [0.0, 1.0, T.UNDEF] and not ens[2].any() and ens[3].tolist() == [0.0, 990.0e2, T.UNDEF]
    assert qc.tolist() == [0, 50, 90, 50]                              # ties: the lowest rank; 1100 hPa itself is not below the cap
    qc = np.array([0, 90, 10, 0], dtype=np.int32)
    T.fill(cand[:, :1], [1, 2, 3], False, qc, ens, 0)
    assert qc.tolist() == [0, 90, 10, 0]
    elm = np.array([T.ID_TCX, 2819, T.ID_TCY, T.ID_TCP, T.ID_TCX, 3073], dtype=np.int32)
    dif = np.array([5.0, 0.0, 0.0, 0.0, 0.0, 0.0])
    assert T.rows(elm, dif, -1.0, 0.0)[0].tolist() == [5, 3, 4] and T.rows(elm, dif, -1.0, 0.0)[1]
    assert not T.rows(elm, dif, 0.0, 1.0)[1] and not T.rows(elm[:4], dif[:4], -1.0, 1.0)[1]
    assert T.rows(elm[:3], dif[:3], -1.0, 1.0)[0].tolist() == [1, 3, 0]
