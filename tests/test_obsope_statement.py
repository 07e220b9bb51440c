"""Anchors of the numpy statement of the observation operator (tests/_obsope.py) that do not come from its author: the compiled
reference's com_gamma and com_distll_1, affine fields under the interpolation, the geometry of the radial velocity, published
coefficients of the three reflectivity methods, and the condition the GPU comparison rests on: no fixture row lies within 1e-6
(relative) of a comparison it took, the deliberate ties sitting where both sides are exact."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import _obsope as O
from _oracle import REF_SO

EPS = O.EPS


def ulps(a, b):
    return abs(a - b) / math.ulp(b)


@pytest.fixture(scope="module")
def ref():
    if not os.path.exists(REF_SO):
        pytest.skip("oracle/_ref not built (reference tree absent)")
    return C.CDLL(REF_SO)


def test_the_three_gamma_constants_are_the_compiled_references(ref):
    fn = getattr(ref, "_QMcommonPcom_gamma")
    fn.argtypes, fn.restype = [C.POINTER(C.c_double), C.POINTER(C.c_double)], None
    for x, mine in ((4.8, O.GAMMA_48), (4.25, O.GAMMA_425), (4.5, O.GAMMA_45)):
        xi, ga = C.c_double(x), C.c_double(0.0)
        fn(C.byref(xi), C.byref(ga))
        assert ulps(mine, ga.value) <= 4, (x, mine, ga.value)


def test_the_great_circle_distance_is_the_compiled_references(ref):
    fn = getattr(ref, "_QMcommonPcom_distll_1")
    fn.argtypes, fn.restype = [C.POINTER(C.c_double)] * 5, None
    rng = np.random.default_rng(5)
    for _ in range(100):
        alon, blon = rng.uniform(120.0, 150.0, size=2)
        alat, blat = rng.uniform(20.0, 50.0, size=2)
        a = [C.c_double(v) for v in (alon, alat, blon, blat)]
        d = C.c_double(0.0)
        fn(*[C.byref(v) for v in a], C.byref(d))
        assert ulps(O.com_distll_1(alon, alat, blon, blat), d.value) <= 4, (alon, alat, blon, blat)


def test_affine_fields_are_reproduced_by_the_interpolation():
    """200 seeded positions, integer coordinates, ri == 1.0 and ri == nlonh among them"""
    rng = np.random.default_rng(11)
    nj, ni, nk = 7, 9, 12
    a0, ak, ai, aj = 3.0, 0.7, -1.3, 2.9
    jj, ii, kk = np.meshgrid(np.arange(1, nj + 1), np.arange(1, ni + 1), np.arange(1, nk + 1), indexing="ij")
    var = a0 + ak * kk + ai * ii + aj * jj
    var2 = a0 + ai * ii[:, :, 0] + aj * jj[:, :, 0]
    pts = [(rng.uniform(1, nk), rng.uniform(1, ni), rng.uniform(1, nj)) for _ in range(180)]
    pts += [(float(rng.integers(2, nk + 1)), float(rng.integers(1, ni + 1)), float(rng.integers(1, nj + 1))) for _ in range(10)]
    pts += [(rng.uniform(1, nk), 1.0, rng.uniform(1, nj)) for _ in range(5)] + [(rng.uniform(1, nk), float(ni), 1.0) for _ in range(5)]
    assert len(pts) == 200
    for rk, ri, rj in pts:
        got, sabs = O.itpl_3d(var, rk, ri, rj)
        assert abs(got - (a0 + ak * rk + ai * ri + aj * rj)) <= 64 * EPS * sabs, (rk, ri, rj)
        got2, sabs2 = O.itpl_2d(var2, ri, rj)
        assert abs(got2 - (a0 + ai * ri + aj * rj)) <= 64 * EPS * sabs2
        col = O.itpl_2d_column(var, ri, rj)
        assert np.all(np.abs(col - (a0 + ak * np.arange(1, nk + 1) + ai * ri + aj * rj)) <= 64 * EPS * (sabs2 + ak * nk))


def test_a_zero_weight_corner_does_not_contribute():
    var = np.ones((4, 4, 4))
    var[0, :, :] = np.nan                          # j = 1 carries weight 0 for rj = 2.0
    var[:, :, 0] = np.nan                          # k = 1 likewise for rk = 2.0
    assert O.itpl_3d(var, 2.0, 2.5, 2.0)[0] == 1.0
    assert O.itpl_3d(var[1:], 2.0, 1.0, 1.0)[0] == 1.0       # ri == rj == 1.0: index 0 is never read


def test_radial_velocity_geometry_without_terminal_velocity():
    u, v, w = 7.0, -3.0, 1.5
    rlon, rlat, rz = 135.0, 35.0, 100.0
    for method in (1, 2, 3):
        # due east at the radar's height: 90 degrees up to the reference's ten-digit pi (rad2deg * (pi / 2) = 90 (1 + 2.9e-11))
        az, elev = O.radar_angles(rlon + 0.3, rlat, rz, rlon, rlat, rz)
        assert az == pytest.approx(90.0, abs=1e-8) and elev == 0.0
        vr = O.calc_ref_vr(method, False, 1e-4, 1e-5, 1e-5, u, v, w, 280.0, 8.0e4, az, elev)[1]
        assert vr == pytest.approx(u, abs=1e-9)
        az, elev = O.radar_angles(rlon, rlat + 0.3, rz, rlon, rlat, rz)
        assert az == 0.0 and elev == 0.0
        vr = O.calc_ref_vr(method, False, 1e-4, 1e-5, 1e-5, u, v, w, 280.0, 8.0e4, az, elev)[1]
        assert vr == pytest.approx(v, abs=1e-12)
        # straight above a point 0.2 degrees north of the radar: the closed form with the arc length re * 0.2 deg
        h = 5000.0
        az, elev = O.radar_angles(rlon, rlat + 0.2, rz + h, rlon, rlat, rz)
        dist = O.RE * 0.2 * O.DEG2RAD
        el = math.atan2(h, dist)
        want = v * math.cos(el) + w * math.sin(el)
        vr = O.calc_ref_vr(method, False, 1e-4, 1e-5, 1e-5, u, v, w, 280.0, 8.0e4, az, elev)[1]
        assert vr == pytest.approx(want, rel=1e-9)
        assert math.sin(elev * O.DEG2RAD) == pytest.approx(h / math.hypot(h, dist), rel=1e-9)


def test_method_1_is_sun_and_crooks_coefficient():
    t, p = 280.0, 8.0e4
    ro = p / (O.RD * t)
    q = 1.0e-3 / ro / 3.0
    ref = O.calc_ref_vr(1, True, q, q, q, 0.0, 0.0, 0.0, t, p, 0.0, 0.0)[0]
    assert abs(ref - 2.04e4) <= 0.005 * 2.04e4, ref


def test_method_3_rain_only_and_no_mixtures_without_a_partner():
    """rain alone: 2.53e4 (1000 rho qr)^1.84, the exponent as the reference holds it (a literal without a kind: single
    precision, widened)"""
    t, p, qr = 285.0, 9.0e4, 3.0e-4
    ro = p / (O.RD * t)
    ref, _, _, parts = O.calc_ref_vr(3, True, qr, 0.0, 0.0, 0.0, 0.0, 0.0, t, p, 0.0, 0.0)
    assert ref == 2.53e4 * (ro * qr * 1.0e3) ** float(np.float32(1.84))
    assert abs(ref / (2.53e4 * (1000.0 * ro * qr) ** 1.84) - 1.0) < 1e-6          # ... and the double-precision reading nearby
    assert parts["Fs"] == 0.0 and parts["Fg"] == 0.0
    parts = O.calc_ref_vr(3, True, qr, 2e-4, 0.0, 0.0, 0.0, 0.0, t, p, 0.0, 0.0)[3]
    assert parts["Fs"] > 0.0 and parts["Fg"] == 0.0 and parts["zmg"] == 0.0
    parts = O.calc_ref_vr(3, True, qr, 0.0, 2e-4, 0.0, 0.0, 0.0, t, p, 0.0, 0.0)[3]
    assert parts["Fg"] > 0.0 and parts["Fs"] == 0.0 and parts["zms"] == 0.0
    parts = O.calc_ref_vr(3, True, 0.0, 2e-4, 2e-4, 0.0, 0.0, 0.0, t, p, 0.0, 0.0)[3]
    assert parts["Fs"] == 0.0 and parts["Fg"] == 0.0


def test_method_2_snow_branch_switches_at_the_references_threshold():
    """t <= 273.16 with the literal as the reference holds it (single precision: 273.160003662109375)"""
    thr = float(np.float32(273.16))
    args = lambda t: (2, True, 0.0, 2.0e-4, 0.0, 0.0, 0.0, 0.0, t, 7.0e4, 0.0, 0.0)
    assert O.calc_ref_vr(*args(thr))[3]["snow"] == "cold"
    assert O.calc_ref_vr(*args(math.nextafter(thr, 1e9)))[3]["snow"] == "warm"
    assert O.calc_ref_vr(*args(273.16))[3]["snow"] == "cold"
    cold, warm = O.calc_ref_vr(*args(thr))[0], O.calc_ref_vr(*args(math.nextafter(thr, 1e9)))[0]
    assert abs(cold / warm - 1.0) > 0.1            # no continuity is expected there


@pytest.mark.parametrize("nlev", [8, 70])
def test_no_fixture_row_is_near_a_comparison(nlev):
    """Every (row, member) of the GPU fixtures, under every switch the GPU tests use, stays 1e-6 away from every comparison:
    no row has to be excluded from a GPU comparison."""
    case = O.make_case(nlev)
    assert 280 <= case["nrow"] <= 340
    configs = ([dict(method_ref_calc=m, use_terminal_velocity=tv, stggrd=s) for m in (1, 2, 3) for tv in (0, 1) for s in (0, 1)]
               if nlev == 8 else [dict(method_ref_calc=2, use_terminal_velocity=1, stggrd=0),
                                  dict(method_ref_calc=3, use_terminal_velocity=0, stggrd=1)])
    seen_qc, low, high = set(), 0, 0
    for kw in configs:
        st = O.statement(case, O.default_cfg(**kw))
        worst = np.unravel_index(np.argmin(st["dist"]), st["dist"].shape)
        assert st["dist"].min() >= 1e-6, (kw, worst, case["rows"][worst[0]], st["dist"].min())
        seen_qc |= set(np.unique(st["qc_m"]).tolist())
        low += int((st["kind"] == "lowref").sum())
        high += int((st["kind"] == "dbz").sum())
    assert {0, 10, 19, 20, 21, 90, 98} <= seen_qc
    assert low > 10 and high > 10                   # reflectivity on both sides of MIN_RADAR_REF
    tags = {r["tag"] for r in case["rows"]}
    assert {"conv", "radar", "ps", "ps-dz0", "unknown", "off", "outside", "vbound", "zmax", "on-radar", "terrain", "exact", "edge"} <= tags
