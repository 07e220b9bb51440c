"""letkf_superob_dev against the statement (tests/_superob.py), bit for bit on every output: the integers and the doubles alike,
no tolerance.  The fixtures are small pools of points, so that exact ties and temporal duplicates abound; the statement's own
test asserts the margin that makes method 1's comparison of distances exact."""
import numpy as np
import pytest
import torch

import _superob as S

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env():
    from _gpu import ctx, pkg
    return pkg, ctx(), torch.device("cuda:0")


@pytest.fixture(scope="module")
def base():
    return S.base_case()


@pytest.fixture(scope="module")
def base_rows(base, env):
    return S.device_rows(base, env[2])


def check(env, case, methods, rows=None, obsnum=True):
    want = S.superob(case, methods)
    got = S.run_device(env[1], case, methods, env[2], obsnum=obsnum, rows=rows)
    if not obsnum:
        want.pop("obsnum")
    S.assert_same_bits(got, want)
    return got, want


@pytest.mark.parametrize("t", [0, 1, 2])
@pytest.mark.parametrize("v", [0, 1, 2, 3])
@pytest.mark.parametrize("h", [0, 1, 2, 3])
def test_base_set_under_every_method(env, base, base_rows, h, v, t):
    """5 x 4 x 3, 3 slots (the first empty), nbslot 2, 4 types, 4 elements: records of 2, 63, 64, 65 and 1001 rows, one ending
    its slot, one the table, one with mm = 0, one interrupted; every coordinate edge; surface types and elm > 9999; typ 0,
    nobtype + 1, an unknown id; NaN / inf coordinates"""
    got, want = check(env, base, S.uniform_methods(4, 4, v=v, t=t, h=h), rows=base_rows)
    assert 0 < int(want["nout"][0]) < len(base["rows"]["elm"])
    qc = set(int(q) for q in want["qc1"])
    assert qc >= {0, 2, 3, 5, 6} and (9 in qc) == (v > 0)
    assert want["counts"][6] > 0 and (want["counts"][4] > 0) == (t > 0)


def test_base_set_under_tables_that_differ_by_type_and_element(env, base, base_rows):
    rng = np.random.default_rng(11)
    methods = (rng.integers(0, 2, (4, 4)) * (rng.random((4, 4)) < 0.3), rng.integers(0, 4, (4, 4)), rng.integers(0, 3, (4, 4)),
               rng.integers(0, 4, (4, 4)))
    got, want = check(env, base, methods, rows=base_rows)
    assert want["counts"][1] > 0                                  # method_g drops something
    for g, v, t, h in ((1, 2, 1, 3),):                            # every row dropped
        got, want = check(env, base, S.uniform_methods(4, 4, g=g, v=v, t=t, h=h), rows=base_rows)
        assert int(got["nout"][0]) == 0 and not got["slot_off_out"].any()


@pytest.mark.parametrize("m", [63, 64, 65, 1025, 3000])
@pytest.mark.parametrize("v,t,h", [(0, 1, 3), (2, 2, 1), (0, 0, 2)])
def test_one_cell_of_many_rows(env, m, v, t, h):
    case = S.big_cell_case(m)
    got, want = check(env, case, S.uniform_methods(4, 4, v=v, t=t, h=h))
    assert int(want["nout"][0]) < m // 2


def test_more_than_2_to_32_cells(env):
    """3000 x 3000 x 100 with 7 slots, 24 types and 16 elements; nothing may be sized by the number of cells"""
    case = S.wide_case()
    assert 7 * 24 * 16 * 101 * 3000 * 3000 > 2 ** 32
    for methods in (S.default_methods(24, 16), S.uniform_methods(16, 24, v=3, t=1, h=1)):
        got, want = check(env, case, methods)
        assert len({(int(a), int(b), int(c)) for a, b, c in zip(want["slot"], want["typ"], want["elm"])}) > 500


def test_200000_rows_twice_with_identical_bits(env):
    case = S.dense_case()
    methods = S.uniform_methods(4, 4, v=2, t=1, h=3)
    rows = S.device_rows(case, env[2])
    got, want = check(env, case, methods, rows=rows)
    again = S.run_device(env[1], case, methods, env[2], rows=rows)
    S.assert_same_bits(again, got)
    assert int(got["counts"][5]) > 50000 and got["obsnum"][3].sum() == got["nout"][0]


def test_no_rows_and_no_obsnum(env, base, base_rows):
    empty = {"rows": {n: a[:0] for n, a in base["rows"].items()}, "slot_off": np.zeros(4, dtype=np.int64), "grid": base["grid"],
             "nbslot": 2, "elem_uid": base["elem_uid"], "nobtype": 4, "surface_typ_mask": 0x8}
    got, want = check(env, empty, S.uniform_methods(4, 4, v=2, t=1, h=3))
    assert int(got["nout"][0]) == 0 and not got["counts"].any() and not got["obsnum"].any()
    check(env, base, S.uniform_methods(4, 4, v=2, t=1, h=3), rows=base_rows, obsnum=False)


def test_the_host_helpers_are_the_statements(env):
    pkg = env[0]
    for nslots, nbslot in ((7, 4), (1, 1), (4, 1), (64, 33), (5, 5)):
        assert list(pkg.superob_slot_priority(nslots, nbslot)) == S.slot_priority(nslots, nbslot)
    for nobtype, nid in ((24, 16), (4, 4), (32, 32), (1, 1)):
        for a, b in zip(pkg.superob_default_methods(nobtype, nid), S.default_methods(nobtype, nid)):
            assert np.array_equal(a, b)
