"""The statement of superob (tests/_superob.py), without a device: its two forms of the temporal stage and of the cell grouping
agree, superob_select on hand-worked cases, the slot priority, and the margin that makes the device comparison exact -- every
pair of method-1 candidates of every group of every fixture has identical coordinates or distances more than 1e-9 apart."""
import math

import numpy as np
import pytest

import _superob as S

M = S.uniform_methods


def same_result(a, b):
    assert set(a) == set(b)
    for name in a:
        x, y = np.asarray(a[name]), np.asarray(b[name])
        assert x.dtype == y.dtype and x.shape == y.shape, name
        assert x.tobytes() == y.tobytes(), name


def row(err, ri=2.0, rj=2.0, rk=2.0, dat=1.0):
    return [10.0 * ri, 20.0 * rj, 30.0 * rk, dat, err, ri, rj, rk]


@pytest.mark.parametrize("t", [1, 2])
@pytest.mark.parametrize("v,h", [(2, 3), (1, 1), (3, 2), (0, 0)])
def test_the_two_forms_of_the_temporal_stage_agree(v, h, t):
    case = S.base_case(seed=5, n=1500)
    m = M(4, 4, v=v, t=t, h=h)
    same_result(S.superob(case, m), S.superob(case, m, temporal=S.temporal_by_class))


@pytest.mark.parametrize("v,t,h", [(2, 1, 3), (0, 0, 1), (1, 2, 0), (3, 0, 2)])
def test_the_cell_grouping_agrees_with_brute_force_over_the_cells(v, t, h):
    case = S.base_case(seed=6, n=300, special=False)
    m = M(4, 4, v=v, t=t, h=h)
    same_result(S.superob(case, m), S.superob(case, m, brute=True))


def test_select_on_errs_2_1_1_3():
    g = [row(2.0, 2.4, 2.0, 2.0, 1.0), row(1.0, 2.3, 2.0, 2.0, 2.0), row(1.0, 2.1, 2.0, 2.0, 4.0), row(3.0, 2.0, 2.0, 2.0, 8.0)]
    (one,) = S.superob_select(g, 2, 2, 2, 1)
    assert one == g[2]                                           # the closer of the two rows of smallest err
    (two,) = S.superob_select(g, 2, 2, 2, 2)
    assert two[S.DAT] == (((0.0 + 1.0) + 2.0) + 4.0 + 8.0) / 4.0 and two[S.ERR] == 1.0
    assert two[S.RI] == ((((0.0 + 2.4) + 2.3) + 2.1) + 2.0) / 4.0
    (three,) = S.superob_select(g, 2, 2, 2, 3)
    assert three[S.DAT] == 3.0 and three[S.ERR] == 1.0 and three[S.RI] == ((0.0 + 2.3) + 2.1) / 2.0
    assert three[S.LON] == ((0.0 + 23.0) + 21.0) / 2.0
    assert S.superob_select(g, 2, 2, 2, 0) == g and S.superob_select(g[:1], 2, 2, 2, 3) == g[:1]


def test_select_takes_the_first_of_an_exact_tie_and_a_strictly_smaller_err_restarts():
    g = [row(1.0, 2.25, dat=1.0), row(1.0, 2.25, dat=2.0), row(1.0, 2.5, dat=3.0)]
    assert S.superob_select(g, 2, 2, 2, 1) == [g[0]]
    g = [row(1.0, 2.0, dat=1.0), row(0.5, 2.4, dat=2.0), row(1.0, 2.0, dat=3.0)]
    assert S.superob_select(g, 2, 2, 2, 1) == [g[1]] and S.superob_select(g, 2, 2, 2, 3) == [g[1]]


def test_select_with_every_err_at_or_above_1e20f_and_with_a_nan():
    big = S.BIG
    assert big == float(np.float32(1e20)) and big != 1e20
    g = [row(1e30, dat=1.0), row(math.inf, dat=2.0), row(1e21, dat=5.0)]
    for method in (1, 3):                                        # nothing is used: the first row stays
        assert S.superob_select(g, 2, 2, 2, method) == [g[0]]
    (two,) = S.superob_select(g, 2, 2, 2, 2)                     # all are averaged, err is the start value
    assert two[S.DAT] == 8.0 / 3.0 and two[S.ERR] == big
    g = [row(big, dat=1.0), row(1e30, dat=2.0), row(big, dat=5.0)]
    (three,) = S.superob_select(g, 2, 2, 2, 3)                   # == the start value joins the list
    assert three[S.DAT] == 3.0 and three[S.ERR] == big
    g = [row(math.nan, dat=1.0), row(2.0, dat=2.0), row(math.nan, dat=4.0)]
    assert S.superob_select(g, 2, 2, 2, 3) == [g[1]] and S.superob_select(g, 2, 2, 2, 1) == [g[1]]
    (two,) = S.superob_select(g, 2, 2, 2, 2)
    assert two[S.DAT] == 7.0 / 3.0 and two[S.ERR] == 2.0
    g = [row(math.nan, dat=1.0), row(math.nan, dat=2.0)]
    (one,) = S.superob_select(g, 2, 2, 2, 1)
    assert one[S.DAT] == 1.0 and math.isnan(one[S.ERR])


def test_select_drops_dz_at_k_0():
    g = [row(1.0, 2.3, 2.0, 0.1), row(1.0, 2.2, 2.0, 9.0)]
    assert S.superob_select(g, 2, 2, 0, 1) == [g[1]]             # surface: rk does not count
    assert S.superob_select(g, 2, 2, 1, 1) == [g[0]]
    assert S.distance(g[1], 2, 2, 0) < 0.21 < 8.0 < S.distance(g[1], 2, 2, 1)


def test_slot_priority():
    assert S.slot_priority(7, 4) == [4, 3, 5, 2, 6, 1, 7]
    assert S.slot_priority(1, 1) == [1]
    assert S.slot_priority(4, 1) == [1, 2, 3, 4]


def test_default_methods_are_the_references():
    g, v, t, h = S.default_methods(24, 16)
    assert not g.any()
    assert [int(x) for x in v[0]] == [2, 0, 0, 0, 2, 2] + [0] * 18
    assert [int(x) for x in t[3]] == [0, 0, 0, 0, 1, 1, 0, 1, 2, 2] + [0] * 14
    assert [int(x) for x in h[15]] == [0, 3, 3, 3, 0, 0] + [3] * 18


FIXTURES = [("base", lambda: S.base_case()), ("cell63", lambda: S.big_cell_case(63)), ("cell64", lambda: S.big_cell_case(64)),
            ("cell65", lambda: S.big_cell_case(65)), ("cell1025", lambda: S.big_cell_case(1025)),
            ("cell3000", lambda: S.big_cell_case(3000)), ("wide", lambda: S.wide_case()), ("dense", lambda: S.dense_case())]


@pytest.mark.parametrize("name,make", FIXTURES, ids=[f[0] for f in FIXTURES])
def test_every_method_1_group_of_the_fixtures_is_tied_exactly_or_clearly_apart(name, make):
    case = make()
    nid, nobtype = len(case["elem_uid"]), case["nobtype"]
    seen = [0, math.inf]

    def hook(g, i, j, k, method):
        gap = S.method1_margin(g, i, j, k)
        seen[0] += 1
        seen[1] = min(seen[1], gap)
        assert gap > 1e-9, (g, i, j, k)

    # the groups method 1 sees: the raw rows of a record (v = 1), of a cell (h = 1), and a cell of rows that stage 2 averaged
    for v, h in ((1, 1), (2, 1), (3, 1)) if name != "dense" else ((2, 1),):
        S.superob(case, S.uniform_methods(nid, nobtype, v=v, t=1, h=h), hook=hook)
    assert seen[0] > 0
    print(f"{name}: {seen[0]} groups, smallest relative gap {seen[1]:.3e}")
