"""CPU-side checks of EFSO's localisation advection (include/letkf_amd.h section 12): the header declares both entries at
ABI 11, the library exports them, the Python binding's ctypes signatures are the header's, and the numpy restatement
tests/_efso_locadv.py has the properties of the reference's loc_advection."""
import ctypes as C

import numpy as np
import pytest

import _efso_locadv as la
from __graft_entry__ import load_package
from _header import argtypes_of, declared_params, defines

ENTRIES = ("letkf_efso_locadv_dev", "letkf_efso_search_dev")


@pytest.fixture(scope="module")
def pkg():
    p = load_package()
    p.build()
    return p


def test_header_declares_both_entries_at_abi_11():
    assert defines()["LETKF_AMD_ABI_VERSION"] == 11
    for name in ENTRIES:
        declared_params(name)
    assert declared_params("letkf_efso_search_dev")[1] == "const letkf_efso_args *args"


def test_library_exports_both(pkg):
    lib = C.CDLL(pkg.LIB_PATH)
    for name in ENTRIES:
        assert hasattr(lib, name)
        assert name in pkg.EXPORTS
    assert pkg.lib().letkf_amd_abi_version() == 11


def test_ctypes_signatures_match_the_header(pkg):
    lib = pkg.lib()
    for name in ENTRIES:
        want = argtypes_of(name)
        assert pkg.ARGTYPES[name] == want, name
        assert getattr(lib, name).argtypes == want
        assert getattr(lib, name).restype is C.c_int
    assert len(pkg.ARGTYPES["letkf_efso_locadv_dev"]) == 15 and len(pkg.ARGTYPES["letkf_efso_search_dev"]) == 9


def test_context_methods_exist(pkg):
    assert callable(pkg.Context.efso_locadv) and callable(pkg.Context.efso_search)


def test_zero_rate_broadcasts_the_column_position_exactly():
    rng = np.random.default_rng(1)
    nij1, nlev = 37, 6
    rig, rjg = rng.uniform(3.0, 40.0, nij1), rng.uniform(3.0, 30.0, nij1)
    u0, v0, u1, v1 = la.shear_winds(rng, nij1, nlev)
    for rate, eft in ((0.0, 6.0), (0.5, 0.0), (-0.0, 3.0)):
        ri, rj = la.advect(rig, rjg, u0, v0, u1, v1, rate, eft, 1000.0, 1000.0)
        assert np.array_equal(ri, np.tile(rig, nlev)) and np.array_equal(rj, np.tile(rjg, nlev))


def test_eastward_wind_moves_the_centre_west_and_northward_south():
    nij1, nlev = 5, 3
    rig, rjg = np.full(nij1, 20.0), np.full(nij1, 15.0)
    z = np.zeros(nij1 * nlev)
    w = np.full(nij1 * nlev, 10.0)
    ri, rj = la.advect(rig, rjg, w, z, w, z, 0.5, 1.0, 1000.0, 1000.0)
    assert np.all(ri < 20.0) and np.array_equal(rj, np.full(nij1 * nlev, 15.0))
    assert np.allclose(ri, 20.0 - 10.0 * 0.5 * 3600.0 / 1000.0)          # 18 cells upstream
    ri, rj = la.advect(rig, rjg, z, w, z, w, 0.5, 1.0, 1000.0, 2000.0)
    assert np.array_equal(ri, np.full(nij1 * nlev, 20.0)) and np.all(rj < 15.0)
    assert np.allclose(rj, 15.0 - 10.0 * 0.5 * 3600.0 / 2000.0)
    # a negative rate (or wind) moves the other way
    ri, _ = la.advect(rig, rjg, w, z, w, z, -0.5, 1.0, 1000.0, 1000.0)
    assert np.all(ri > 20.0)


def test_shear_displaces_levels_differently_and_bounds():
    rng = np.random.default_rng(2)
    nij1, nlev = 20, 10
    rig, rjg = rng.uniform(3.0, 40.0, nij1), rng.uniform(3.0, 30.0, nij1)
    u0, v0, u1, v1 = la.shear_winds(rng, nij1, nlev, noise=0.0)
    ri, rj = la.advect(rig, rjg, u0, v0, u1, v1, 0.5, 1.0, 1000.0, 1000.0)
    d = (np.tile(rig, nlev) - ri).reshape(nlev, nij1)
    assert np.allclose(d[0], 18.0) and np.allclose(d[-1], 54.0)
    assert not la.bad_points(rig, rjg, ri, rj).any()
    u0[3] = np.nan
    u1[5] = 1.0e12
    ri, rj = la.advect(rig, rjg, u0, v0, u1, v1, 0.5, 1.0, 1000.0, 1000.0)
    assert np.flatnonzero(la.bad_points(rig, rjg, ri, rj)).tolist() == [3, 5]
