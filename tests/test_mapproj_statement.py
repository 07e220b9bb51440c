"""The statement of the map projection (tests/_mapproj.py) against itself, without a device: its float64 form against the
50-digit truth within the bounds, and the properties that make it the projection -- the base point, the scale factor 1 on both
parallels, rotc as the direction of north -- and the constant of the degree / radian conversions, pinned."""
import mpmath
import numpy as np
import pytest

import _mapproj as M

CONFIGS = list(M.configs())


@pytest.fixture(scope="module", params=CONFIGS)
def case(request):
    p = M.configs()[request.param]
    lon, lat = M.points(20261019, 200, south=request.param == "south")
    q, t = M.setup(p), M.mp_setup(p)
    return dict(name=request.param, p=p, q=q, t=t, lon=lon, lat=lat, truth=M.mp_phys2ij(t, lon, lat))


def test_the_golden_settings_are_the_three_configurations_and_the_southern_mirror():
    assert CONFIGS == ["BDA_d3_1km_9p_bf20", "2015summer_18km", "BDA_d3_100m_256p_bf40", "south"]
    first, south = M.configs()["BDA_d3_1km_9p_bf20"], M.configs()["south"]
    assert (first["basepoint_lon"], first["basepoint_lat"], first["lc_lat1"], first["lc_lat2"]) == (135.523, 34.823, 32.5, 37.5)
    assert (south["basepoint_lat"], south["lc_lat1"], south["lc_lat2"]) == (-34.823, -37.5, -32.5)
    assert M.setup(first)["h"] == 1.0 and M.setup(south)["h"] == -1.0
    assert abs(M.setup(first)["c"] - 0.57375861611964) < 1e-14


def test_the_two_forms_agree_within_the_bounds(case):
    got = M.phys2ij(case["q"], case["lon"], case["lat"])
    shares = M.check_rows(case["q"], case["p"], got, case["truth"], case["name"])
    assert np.all(got["k"] == 0) and set(shares) == {"ri", "rj", "rotc"}
    back = M.ij2phys(case["q"], got["ri"], got["rj"])
    M.check_phys(back, M.mp_ij2phys(case["t"], got["ri"], got["rj"]), case["name"])
    # the round trip in degrees: twice the bound
    assert np.abs(back["lon"] - case["lon"]).max() <= 2 * M.BOUND_DEG and np.abs(back["lat"] - case["lat"]).max() <= 2 * M.BOUND_DEG


def test_the_derived_constants_agree_with_the_truth(case):
    """c is a quotient of two differences of logarithms that lose a digit and a half to cancellation; what matters is what the
    constants do to a point, which the test above bounds.  Here: the constants themselves, to what _mapproj.bound_constants
    derives."""
    q, t = case["q"], case["t"]
    for k, b in M.bound_constants(case["p"], t).items():
        assert M.err(q[k], t[k]) <= b, k


def test_the_base_point_maps_to_its_coordinates(case):
    p, q, t = case["p"], case["q"], case["t"]
    with mpmath.workdps(M.DPS):
        D = mpmath.pi / 180
        x, y, r0, r1, rho, _ = M.mp_forward(t, M.mpf(p["basepoint_lon"]) * D, M.mpf(p["basepoint_lat"]) * D)
        assert abs(x - M.mpf(p["basepoint_x"])) < mpmath.mpf(10) ** -35 and abs(y - M.mpf(p["basepoint_y"])) < mpmath.mpf(10) ** -35
        assert r0 == 1 and r1 == 0
    # in float64 with the exact pi: x exactly, y to the two roundings of pole_y at the size of rho
    x, y, cs, sn, rho, _ = M.forward(q, q["lon0"], p["basepoint_lat"] * (np.pi / 180.0))
    assert x == p["basepoint_x"] and abs(y - p["basepoint_y"]) <= 4 * M.EPS * rho and (cs, sn) == (1.0, 0.0)


def test_the_scale_factor_is_one_on_both_parallels(case):
    """by central difference in the truth: |d(x, y)/d phi| / radius and |d(x, y)/d lam| / (radius cos phi)"""
    p, t = case["p"], case["t"]
    with mpmath.workdps(M.DPS):
        D, d = mpmath.pi / 180, mpmath.mpf(10) ** -15
        lam = M.mpf(p["basepoint_lon"] + 3.0) * D
        for lat in (p["lc_lat1"], p["lc_lat2"]):
            phi = M.mpf(lat) * D
            (xa, ya, *_), (xb, yb, *_) = M.mp_forward(t, lam, phi - d), M.mp_forward(t, lam, phi + d)
            assert abs(mpmath.hypot(xb - xa, yb - ya) / (2 * d * t["radius"]) - 1) < mpmath.mpf(10) ** -25, lat
            (xa, ya, *_), (xb, yb, *_) = M.mp_forward(t, lam - d, phi), M.mp_forward(t, lam + d, phi)
            assert abs(mpmath.hypot(xb - xa, yb - ya) / (2 * d * t["radius"] * mpmath.cos(phi)) - 1) < mpmath.mpf(10) ** -25, lat
        # ... and nowhere between them
        (xa, ya, *_), (xb, yb, *_) = (M.mp_forward(t, lam, M.mpf(0.5 * (p["lc_lat1"] + p["lc_lat2"])) * D + s * d) for s in (-1, 1))
        assert mpmath.hypot(xb - xa, yb - ya) / (2 * d * t["radius"]) < 1 - mpmath.mpf(10) ** -5


def test_rotc_is_the_direction_of_north(case):
    """alpha is the angle of north from +y: the unit vector of growing latitude in the map's frame is (sin alpha, cos alpha) =
    (rotc[1], rotc[0]), east is (cos alpha, -sin alpha), and a wind (u, v) in the map's frame has the eastward component
    u rotc[0] - v rotc[1], which is how the operator uses it.  By difference in the truth."""
    t = case["t"]
    with mpmath.workdps(M.DPS):
        d = mpmath.mpf(10) ** -15
        conv = M.mpf(M.PI_REF) / 180
        for lon, lat in zip(case["lon"][:5], case["lat"][:5]):
            lam, phi = M.mpf(lon) * conv, M.mpf(lat) * conv
            (xa, ya, r0, r1, *_), (xb, yb, *_) = M.mp_forward(t, lam, phi), M.mp_forward(t, lam, phi + d)
            n = mpmath.hypot(xb - xa, yb - ya)
            assert abs((xb - xa) / n - r1) < mpmath.mpf(10) ** -12 and abs((yb - ya) / n - r0) < mpmath.mpf(10) ** -12


def test_the_wrong_pi_in_the_conversion_is_far_outside_the_bound():
    """phys2ij's conversion with the exact pi in place of the reference's 10-digit one: more than 1000 bounds from the truth at
    135 E.  One constant in both places cannot pass."""
    p = M.configs()["BDA_d3_1km_9p_bf20"]
    q, t = M.setup(p), M.mp_setup(p)
    lon, lat = np.full(5, 135.0), np.linspace(30.0, 40.0, 5)
    truth = M.mp_phys2ij(t, lon, lat)
    right, wrong = M.phys2ij(q, lon, lat), M.phys2ij(q, lon, lat, pi_conv=np.pi)
    b = M.bound_ij(right["rho"], p)
    assert np.all(M.err(right["ri"], truth["ri"]) <= b)
    assert np.all(M.err(wrong["ri"], truth["ri"]) > 1000 * b)
    # ... and the other way round: a truth with the exact pi everywhere is as far from the statement
    other = M.mp_phys2ij(t, lon, lat, pi_conv=None)
    assert np.all(M.err(right["ri"], other["ri"]) > 1000 * b)


def test_the_undefined_inputs_follow_the_headers_decisions():
    p = M.configs()["BDA_d3_1km_9p_bf20"]
    q = M.setup(p)
    nan, inf = np.nan, np.inf
    got = M.phys2ij(q, [nan, 135.0, inf, -inf, 135.0, 135.0, 135.0 + 720.0], [35.0, nan, 35.0, 35.0, inf, -inf, 35.0])
    assert np.all(np.isnan(got["ri"])) and np.all(np.isnan(got["rj"])) and np.all(np.isnan(got["rotc"]))
    # one wrap, either way, is the same point to the conversion's rounding
    a, b = M.phys2ij(q, [135.0, 135.0], [35.0, 35.0]), M.phys2ij(q, [135.0 - 360.0, 135.0 + 360.0], [35.0, 35.0])
    assert list(b["k"]) == [1, -1] and np.abs(a["ri"] - b["ri"]).max() < 1e-5
    # the poles through the degree conversion: 4.5e-11 rad short of them
    pole = M.phys2ij(q, [135.0, 135.0], [90.0, -90.0])
    short = 90.0 * (np.pi - M.PI_REF) / 180.0             # (pi/2 - phi loses 6e-17 of 4.5e-11 to pi's own rounding: 1e-5 is wide)
    assert abs(pole["rho"][0] / (q["fact"] * q["radius"] * np.tan(0.5 * short) ** q["c"]) - 1.0) < 1e-5 and 1.0 < pole["rho"][0] < 100.0
    assert np.isfinite(pole["ri"][0]) and np.isfinite(pole["rj"][0])
    assert pole["rho"][1] > 1e12 and not (abs(pole["rj"][1]) < 1e9)
    beyond = M.phys2ij(q, [135.0, 135.0], [90.5, -90.5])
    assert np.all(np.isnan(beyond["ri"])) and np.all(np.isnan(beyond["rj"]))
    # the poles themselves, in radians
    x, y, cs, sn, rho, _ = M.forward(q, q["lon0"], np.array([0.5 * np.pi]))
    assert rho[0] < 1e-2 and np.isfinite(x[0]) and np.isfinite(y[0])
