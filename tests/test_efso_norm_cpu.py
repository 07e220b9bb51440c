"""CPU-side checks of EFSO's forecast-error norm and impact summary (include/letkf_amd.h section 13): the header declares
both entries and letkf_efso_norm_params, the library exports them, the Python binding's ctypes signatures and struct are
the header's, and the numpy restatement tests/_efso_norm.py is the reference's lnorm / print_obsense loops."""
import ctypes as C

import numpy as np
import pytest

import _efso_norm as en
from __graft_entry__ import load_package
from _header import argtypes_of, declared_params, defines, offsetof, sizeof, structs

ENTRIES = ("letkf_efso_norm_dev", "letkf_efso_summary_dev")


@pytest.fixture(scope="module")
def pkg():
    p = load_package()
    p.build()
    return p


def test_header_declares_both_entries_and_the_struct():
    assert "letkf_efso_norm_params" in structs()
    assert declared_params("letkf_efso_norm_dev")[1] == "const letkf_efso_norm_params *prm"
    assert declared_params("letkf_efso_summary_dev")[0] == "letkf_ctx *ctx"
    assert defines()["LETKF_AMD_ABI_VERSION"] == 11


def test_library_exports_both(pkg):
    lib = C.CDLL(pkg.LIB_PATH)
    for name in ENTRIES:
        assert hasattr(lib, name)
        assert name in pkg.EXPORTS
    assert callable(pkg.Context.efso_norm) and callable(pkg.Context.efso_summary)


def test_ctypes_signatures_match_the_header(pkg):
    lib = pkg.lib()
    for name in ENTRIES:
        want = argtypes_of(name)
        assert pkg.ARGTYPES[name] == want, name
        assert getattr(lib, name).argtypes == want
        assert getattr(lib, name).restype is C.c_int


def test_struct_matches_the_compiled_c_layout(pkg):
    fields = [f for f, _ in pkg.EfsoNormParams._fields_]
    assert sizeof("letkf_efso_norm_params") == C.sizeof(pkg.EfsoNormParams)
    assert [offsetof("letkf_efso_norm_params", f) for f in fields] == [getattr(pkg.EfsoNormParams, f).offset for f in fields]


def pressure_columns(rng, nij1, nlev, k):
    """total fields of a pressure variable: decreasing with level, members scattered around the column's profile"""
    prof = 1.0e5 * np.exp(-np.linspace(0.0, 2.5, nlev))[:, None] * rng.uniform(0.97, 1.03, nij1)[None, :]
    return prof.ravel()[:, None] + 50.0 * rng.standard_normal((nij1 * nlev, k))


def case(seed, nij1, nlev, k, nv):
    rng = np.random.default_rng(seed)
    fcst = rng.standard_normal((nij1 * nlev, k, nv)) * rng.uniform(0.5, 5.0, nv) + rng.uniform(-10.0, 300.0, nv)
    fcst[:, :, 4] = pressure_columns(rng, nij1, nlev, k)
    fcer = rng.standard_normal((nij1 * nlev, nv)) * 0.1
    return rng, fcst, fcer


@pytest.mark.parametrize("k,nlev,tar,box,wg,wmoist", [(2, 3, (1, 64), False, False, 1.0), (20, 6, (2, 4), True, True, 0.0),
                                                      (50, 5, (1, 5), True, False, 1.0), (7, 1, (1, 1), False, True, 0.5)])
def test_restatement_is_lnorm(k, nlev, tar, box, wg, wmoist):
    nij1, nv = 23, 11
    rng, fcst, fcer = case(k, nij1, nlev, k, nv)
    wg1 = rng.uniform(0.5, 1.5, nij1) if wg else None
    lon, lat = (rng.uniform(0.0, 360.0, nij1), rng.uniform(-90.0, 90.0, nij1)) if box else (None, None)
    bx = (90.0, 270.0, -30.0, 60.0)
    fo, eo, mean, bad = en.norm(fcst, fcer, nij1, tar_lev=tar, wg1=wg1, lon=lon, lat=lat, box=bx, wmoist=wmoist)
    assert not bad.any()
    r, _ = en.dp_over_ps(mean[:, 4].reshape(nlev, nij1))
    fl, el = en.lnorm_loops(fcst, fcer, nij1, r, tar_lev=tar, wg1=wg1, lon1=lon, lat1=lat, box=bx, wmoist=wmoist)
    assert np.array_equal(fo.view(np.int64), fl.view(np.int64))
    assert np.array_equal(eo.view(np.int64), el.view(np.int64))
    live = en.region(nij1, nlev, tar[0], tar[1], lon, lat, bx)
    assert np.all(fo[~live] == 0) and np.all(fo[live][:, :, [2, 4, 6, 7, 8, 9, 10]] == 0)
    if live.any():
        assert np.abs(fo[live][:, :, [0, 1, 3]]).min() > 0
        assert (np.abs(fo[live][:, :, 5]).min() > 0) == (wmoist > 0)


def test_fcer_assembly_order():
    rng, fcst, _ = case(3, 10, 4, 5, 11)
    xf, xg, xa = (rng.standard_normal((40, 11)) * 3 for _ in range(3))
    _, eo, _, _ = en.norm(fcst, None, 10, xf=xf, xg=xg, xa=xa)
    want = (0.5 * (xf + xg) - xa) / 4.0
    _, eo2, _, _ = en.norm(fcst, want, 10)
    assert np.array_equal(eo, eo2)


def test_half_level_rule():
    rng = np.random.default_rng(5)
    nij1 = 31
    for nlev in (2, 3, 10, 60):
        pb = pressure_columns(rng, nij1, nlev, 1)[:, 0].reshape(nlev, nij1)
        dp, ps, ptop = en.half_levels(pb)
        assert np.allclose(dp.sum(axis=0), ps - ptop, rtol=1e-13, atol=0)
        assert np.all(dp > 0) and np.all(ptop >= 0)
        assert np.allclose(ps, pb[0] + 0.5 * (pb[0] - pb[1]))
        r, bad = en.dp_over_ps(pb)
        assert not bad.any() and np.all(r > 0) and np.all(r < 1)
        # a column whose pressure increases with level is rejected
        pb2 = pb.copy()
        pb2[:, 7] = pb2[::-1, 7]
        assert en.dp_over_ps(pb2)[1].tolist() == [i == 7 for i in range(nij1)]
    # a clipped top: p_{L+1/2} = 0 when the extrapolation goes below 0
    dp, ps, ptop = en.half_levels(np.array([[1000.0], [500.0], [10.0]]))
    assert ptop[0] == 0.0 and dp[-1, 0] == 0.5 * (500.0 + 10.0)
    assert en.dp_over_ps(np.array([[1000.0], [1000.0]]))[1][0]          # dp = 0 at level 1
    assert en.dp_over_ps(np.ones((1, 3)))[0].tolist() == [[1.0, 1.0, 1.0]]


def edge_rows(rng, nobs, nterm, nobtype, elem_uid, latbound):
    elm = rng.choice(list(elem_uid) + [9999, -1], nobs).astype(np.int32)
    typ = rng.integers(-1, nobtype + 3, nobs).astype(np.int32)
    lat = rng.choice([latbound, -latbound, np.nextafter(latbound, 99), np.nextafter(-latbound, -99), 0.0, 45.0, -45.0,
                      90.0, -90.0], nobs)
    qc = rng.choice([0, 0, 0, 1, 3], nobs).astype(np.int32)
    obsense = rng.standard_normal((nobs, nterm))
    obsense[rng.random((nobs, nterm)) < 0.1] = 0.0
    return obsense, elm, typ, lat, qc


@pytest.mark.parametrize("nterm", [1, 3, 4])
def test_summary_restatement_is_print_obsense(nterm):
    rng = np.random.default_rng(nterm)
    elem_uid = [2819, 2820, 3073, 3330, 3331, 14593, 4001]
    nobtype, latbound = 5, 20.0
    obsense, elm, typ, lat, qc = edge_rows(rng, 3000, nterm, nobtype, elem_uid, latbound)
    for q in (None, qc):
        got = en.summary(obsense, elm, typ, lat, elem_uid, nobtype, latbound, q)
        want = en.summary_loops(obsense, elm, typ, lat, elem_uid, nobtype, latbound, q)
        for g, w in zip(got, want):
            assert g.shape == w.shape and np.array_equal(np.asarray(g).view(np.int64 if g.dtype == np.float64 else np.int32),
                                                         np.asarray(w).view(np.int64 if w.dtype == np.float64 else np.int32))
        assert got[0].sum() == np.count_nonzero(en.bins(elm, typ, lat, elem_uid, nobtype, latbound, q) >= 0)
    # the edges: lat = +-latbound is TR, typ = nobtype + 1 is OTHERS, unknown elements and typ 0 are skipped
    one = np.ones((4, 1))
    c, _, _ = en.summary(one, np.array([2819, 2819, 2819, 9]), np.array([nobtype + 1, 1, 0, 1]),
                         np.array([latbound, -latbound, 50.0, 0.0]), elem_uid, nobtype, latbound)
    assert c[1, nobtype, 0] == 1 and c[1, 0, 0] == 1 and c.sum() == 2


def test_table_formats():
    assert en.fortran_e12_5(123.456) == " 0.12346E+03"
    assert en.fortran_e12_5(-0.00123449) == "-0.12345E-02"
    assert en.fortran_e12_5(0.0) == " 0.00000E+00"
    assert en.fortran_e12_5(9.999996) == " 0.10000E+02"
    count = np.zeros((3, 3, 2), np.int32)
    ssum = np.zeros((1, 3, 3, 2))
    nneg = np.zeros((1, 3, 3, 2), np.int32)
    count[1, 0, 1], ssum[0, 1, 0, 1], nneg[0, 1, 0, 1] = 4, -2.5, 3
    lines = en.table_lines(count, ssum, nneg, 10, ["ADPUPA", "AIRCFT"], ["U", "T"])
    assert lines[1] == " TOTAL NUMBER OF OBSERVATIONS:        10"
    assert lines[5] == "ADPUPA  TOTAL        4 -0.25000E+01    75.00"
    assert lines[6] == "ADPUPA TR T          4 -0.25000E+01    75.00"
    assert en.table_lines(count, ssum, nneg, 0, ["ADPUPA", "AIRCFT"], ["U", "T"]) == []
