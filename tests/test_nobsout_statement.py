"""tests/_nobsout.py, the numpy statement of NOBS_OUT (scale/letkf/letkf_tools.f90:1380-1389, :440-447, :768-778), held to cases
made by hand.  No device."""
import numpy as np
import pytest

import _nobsout as N

# five combined types: ref and re0 of the radar (type 22), u and v of ADPUPA (type 1), T of AIRCFT (type 4)
ELM_U = [9, 10, 1, 2, 3]
TYP = [22, 22, 1, 1, 4]


def test_two_ctypes_of_one_report_type_are_summed_into_that_types_row():
    nobs = np.array([[0, 0, 5, 7, 2], [1, 0, 0, 3, 0]], dtype=np.int32)
    w = N.work3dn(nobs, None, ELM_U, TYP)
    assert w.shape == (2, 30)
    assert w[0, 0] == 12 and w[1, 0] == 3                       # type 1 = u + v
    assert w[0, 3] == 2 and w[1, 3] == 0                        # type 4
    assert w[0, 21] == 0 and w[1, 21] == 1                      # type 22 = ref + re0
    others = [r for r in range(24) if r not in (0, 3, 21)]
    assert not w[:, others].any()


def test_the_three_radar_rows_and_their_cutoffs():
    elm_u, typ = [9, 10, 11, 3], [22, 22, 22, 1]
    nobs = np.array([[12, 4, 6, 9]], dtype=np.int32)
    cutd = np.array([[1234.5, 0.25, 77.0, 999.0]])
    w = N.work3dn(nobs, cutd, elm_u, typ)
    assert w[0, 24:27].tolist() == [12.0, 4.0, 6.0]
    assert w[0, 27:30].tolist() == [1234.5, 0.25, 77.0]
    assert w[0, 21] == 22 and w[0, 0] == 9
    f = N.fields(w)
    assert f.shape == (1, 11)
    assert f[0].tolist() == [9.0, 0.0, 0.0, 0.0, 22.0, 12.0, 4.0, 6.0, 1234.5, 0.25, 77.0]
    # without cut-offs the three rows are zero and the counts stay
    w0 = N.work3dn(nobs, None, elm_u, typ)
    assert not w0[0, 27:30].any() and np.array_equal(w0[:, :27], w[:, :27])


def test_a_combination_absent_from_the_table_is_zero():
    # no vr ctype; a vr of another report type is not the radar's
    elm_u, typ = [9, 11], [22, 3]
    w = N.work3dn(np.array([[5, 8]], dtype=np.int32), np.array([[10.0, 20.0]]), elm_u, typ)
    assert w[0, 24:30].tolist() == [5.0, 0.0, 0.0, 10.0, 0.0, 0.0]
    assert w[0, 2] == 8 and w[0, 21] == 5
    assert N.fields(w)[0].tolist() == [0.0, 8.0, 0.0, 0.0, 5.0, 5.0, 0.0, 0.0, 10.0, 0.0, 0.0]


@pytest.mark.parametrize("criterion", [1, 2, 3])
def test_a_merged_group_is_counted_on_its_master_only(criterion):
    hori_loc = np.array([4000.0, 3000.0, 6000.0, 8000.0, 5000.0])
    groups = [[0, 1], [2], [3], [4]]
    nobs0, cutd0 = N.defaults(5, groups, hori_loc, criterion)
    assert not nobs0.any() and cutd0[1] == 0.0
    if criterion == 1:
        assert cutd0[0] == 4000.0 * float(np.float32(3.651483717)) and cutd0[2] == 6000.0 * N.DIST_ZERO_FAC
        assert N.DIST_ZERO_FAC == 3.6514837741851807
    else:
        assert not cutd0.any()
    # the group's 12 selected rows stand on the master (ref); re0 keeps 0 and its cut-off 0 (:1633-1640)
    nobs, cutd = nobs0.copy(), cutd0.copy()
    nobs[0], cutd[0] = 12, 2500.0
    w = N.work3dn(nobs[None], cutd[None], ELM_U, TYP)
    assert w[0, 24:27].tolist() == [12.0, 0.0, 0.0] and w[0, 27:30].tolist() == [2500.0, 0.0, 0.0]
    assert w[0, 21] == 12
    # a point without any local observation still carries the default cut-off of the master
    w = N.work3dn(nobs0[None], cutd0[None], ELM_U, TYP)
    assert not w[0, :27].any() and w[0, 27] == cutd0[0] and w[0, 28] == 0.0


@pytest.mark.parametrize("nobtype", [24, 32])
def test_the_rows_follow_nobtype(nobtype):
    rng = np.random.default_rng(nobtype)
    elm_u = [9, 10, 11, 1, 2, 3, 4]
    typ = [22, 22, 22, 1, 1, nobtype, 8]
    nobs = rng.integers(0, 100, (6, 7)).astype(np.int32)
    cutd = rng.uniform(0.0, 1.0e4, (6, 7))
    w = N.work3dn(nobs, cutd, elm_u, typ, nobtype=nobtype)
    assert w.shape == (6, nobtype + 6)
    assert np.array_equal(w[:, nobtype - 1], nobs[:, 5]) and np.array_equal(w[:, 0], nobs[:, 3] + nobs[:, 4])
    assert np.array_equal(w[:, nobtype:nobtype + 3], nobs[:, :3]) and np.array_equal(w[:, nobtype + 3:], cutd[:, :3])
    assert w[:, :nobtype].sum() == nobs.sum()                    # every count stands in exactly one type row
    f = N.fields(w, nobtype=nobtype)
    assert np.array_equal(f[:, 3], nobs[:, 6]) and np.array_equal(f[:, 4], nobs[:, :3].sum(axis=1))
    assert np.array_equal(f[:, 5:], w[:, nobtype:])
    f2 = N.fields(w, nobtype=nobtype, pick=(nobtype, 1, 1, 8, 22))
    assert np.array_equal(f2[:, 0], nobs[:, 5]) and np.array_equal(f2[:, 1], f2[:, 2])
