"""The statement of include/letkf_amd_mapproj.h, twice: a numpy float64 form with exactly the header's order of operations,
vectorised, and the truth, an mpmath form at 50 digits whose derived constants are in high precision too.  Both take the same
double inputs; both carry the reference's 10-digit pi (common/common.f90:28) in the four degree / radian conversions and the
exact pi inside the projection.  No GPU, no library.

The bounds are the issue's: the forward result passes through about eight roundings (the conversion, the subtraction, tan, the
power, the product, sincos, the last product and sum), each at most one ulp relative to rho, the distance from the cone's pole;
16 * 2^-53 * rho gives plain libm a factor of 8."""
import functools
import json
import math
import os

import mpmath
import numpy as np

PI_REF = 3.1415926535                 # common/common.f90:28
RAD2DEG_REF = 180.0 / PI_REF          # :40
RADIUS = 6.37122e6
EPS = 2.0 ** -53
BOUND_ROTC = 8 * EPS                  # absolute
BOUND_DEG = 16 * EPS * 180.0          # degrees; the round trip ij2phys(phys2ij) gets twice that
DPS = 50
KEYS = ("basepoint_lon", "basepoint_lat", "basepoint_x", "basepoint_y", "lc_lat1", "lc_lat2", "cxg1", "cyg1", "dx", "dy")


def bound_ij(rho, p):
    """ri / rj against the truth, in grid units, for points at the distance rho (m) from the pole"""
    return 16 * EPS * rho / min(p["dx"], p["dy"])


@functools.lru_cache(None)
def configs():
    """{name: parameters} of the three configurations of tests/golden/mapproj_configs.json and `south`, the mirror of the first
    in the southern hemisphere"""
    raw = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "mapproj_configs.json")))
    out = {name: dict({k: float(c[k]) for k in KEYS}, radius=RADIUS, **{k: c[k] for k in ("imax", "jmax", "prc_num_x", "prc_num_y")})
           for name, c in raw.items() if not name.startswith("_")}
    first = out["BDA_d3_1km_9p_bf20"]
    out["south"] = dict(first, basepoint_lat=-first["basepoint_lat"], lc_lat1=-first["lc_lat2"], lc_lat2=-first["lc_lat1"])
    return out


def setup_args(p):
    """p as scale_letkf_amd.mapproj_setup takes it"""
    return dict({k: p[k] for k in KEYS}, radius=p["radius"])


# ---------------------------------------------------------------------------------------------------------------- float64
def setup(p):
    """the derived constants as doubles: each the real value rounded once (letkf_mapproj_setup works in the 64-bit significand of
    the x87 format for the same end -- the error of c is multiplied by dlam in every sincos(c dlam))"""
    t = mp_setup(p)
    return dict({k: float(t[k]) for k in ("lon0", "c", "fact", "radius", "pole_x", "pole_y", "cxg1", "cyg1", "dx", "dy")}, h=float(t["h"]))


def wrap_once(dl):
    """(dlam after one turn, the turns taken: -1, 0 or +1); what is still outside [-pi, pi] is NaN"""
    dl = np.asarray(dl, dtype=np.float64)
    k = np.where(dl > np.pi, -1, np.where(dl < -np.pi, 1, 0))
    with np.errstate(invalid="ignore"):
        out = np.where(k == -1, dl - 2.0 * np.pi, np.where(k == 1, dl + 2.0 * np.pi, dl))
        return np.where(np.abs(out) <= np.pi, out, np.nan), k


def forward(q, lam, phi):
    """(x, y, cos(c dlam), sin(c dlam), rho, turns) of points in radians"""
    lam, phi = np.asarray(lam, dtype=np.float64), np.asarray(phi, dtype=np.float64)
    with np.errstate(all="ignore"):
        dl, k = wrap_once(lam - q["lon0"])
        dl = np.where(np.abs(phi) <= np.pi, dl, np.nan)
        h = q["h"]
        rho = q["fact"] * q["radius"] * np.power(np.tan((0.5 * np.pi - h * phi) * 0.5), q["c"])
        a = q["c"] * dl
        sn, cs = np.sin(a), np.cos(a)
        return q["pole_x"] + rho * sn, q["pole_y"] - h * rho * cs, cs, sn, rho, k


def inverse(q, x, y):
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    h, rf = q["h"], q["radius"] * q["fact"]
    xx, yy = (x - q["pole_x"]) / rf, -h * (y - q["pole_y"]) / rf
    with np.errstate(all="ignore"):
        return q["lon0"] + np.arctan2(xx, yy) / q["c"], h * (0.5 * np.pi - 2.0 * np.arctan(np.power(np.hypot(xx, yy), 1.0 / q["c"])))


def phys2ij(q, lon, lat, pi_conv=PI_REF):
    """phys2ij and the rotation for rows in degrees: dict ri, rj, rotc [n, 2], rho, k.  pi_conv: the constant of the conversion
    (the reference's; the exact one makes the wrong-pi variant)"""
    lon, lat = np.asarray(lon, dtype=np.float64), np.asarray(lat, dtype=np.float64)
    with np.errstate(all="ignore"):
        x, y, cs, sn, rho, k = forward(q, lon * pi_conv / 180.0, lat * pi_conv / 180.0)
        return dict(ri=(x - q["cxg1"]) / q["dx"] + 1.0, rj=(y - q["cyg1"]) / q["dy"] + 1.0, rotc=np.stack([cs, -q["h"] * sn], axis=-1),
                    rho=rho, k=k)


def rotc_at(q, lon, lat):
    with np.errstate(all="ignore"):
        dl, _ = wrap_once(np.asarray(lon, dtype=np.float64) * PI_REF / 180.0 - q["lon0"])
        a = q["c"] * np.where(np.abs(lat) <= 180.0, dl, np.nan)
        return np.stack([np.cos(a), -q["h"] * np.sin(a)], axis=-1)


def xy2phys(q, x, y):
    lam, phi = inverse(q, x, y)
    lon, lat = lam * RAD2DEG_REF, phi * RAD2DEG_REF
    return dict(lon=lon, lat=lat, rotc=rotc_at(q, lon, lat))


def ij2phys(q, ri, rj):
    """ij2phys for rows: dict lon, lat (degrees), rotc [n, 2]"""
    ri, rj = np.asarray(ri, dtype=np.float64), np.asarray(rj, dtype=np.float64)
    return xy2phys(q, (ri - 1.0) * q["dx"] + q["cxg1"], (rj - 1.0) * q["dy"] + q["cyg1"])


def grid(q, nlon, nlat, ihalo, jhalo, cx1, cy1):
    """the loop of common_mpi_scale.f90:193-203: dict lon, lat [nlat, nlon], rotc [nlat, nlon, 2]"""
    ri = (np.arange(nlon) + 1 + ihalo).astype(np.float64)[None, :] * np.ones((nlat, 1))
    rj = (np.arange(nlat) + 1 + jhalo).astype(np.float64)[:, None] * np.ones((1, nlon))
    return xy2phys(q, (ri - 1.0) * q["dx"] + cx1, (rj - 1.0) * q["dy"] + cy1)


# ------------------------------------------------------------------------------------------------------------------ truth
def mpf(v):
    return mpmath.mpf(float(v))          # (a double is taken as the real number it is)


def mp_setup(p):
    with mpmath.workdps(DPS):
        pi, D = +mpmath.pi, mpmath.pi / 180
        h = 1 if p["lc_lat1"] + p["lc_lat2"] > 0.0 else -1
        psi1, psi2, psi0 = (pi / 2 - h * mpf(p[k]) * D for k in ("lc_lat1", "lc_lat2", "basepoint_lat"))
        c = (mpmath.log(mpmath.sin(psi1)) - mpmath.log(mpmath.sin(psi2))) / (mpmath.log(mpmath.tan(psi1 / 2)) - mpmath.log(mpmath.tan(psi2 / 2)))
        fact = mpmath.sin(psi1) / (c * mpmath.tan(psi1 / 2) ** c)
        return dict(h=h, lon0=mpf(p["basepoint_lon"]) * D, c=c, fact=fact, radius=mpf(p["radius"]), pole_x=mpf(p["basepoint_x"]),
                    pole_y=mpf(p["basepoint_y"]) + h * fact * mpf(p["radius"]) * mpmath.tan(psi0 / 2) ** c,
                    cxg1=mpf(p["cxg1"]), cyg1=mpf(p["cyg1"]), dx=mpf(p["dx"]), dy=mpf(p["dy"]))


def mp_forward(t, lam, phi, turns=None):
    """(x, y, rotc0, rotc1, rho, dlam before the turn) of one point in radians (mpf).  turns: the turn to take (from the float64
    form, for a row within rounding of the cut, where x and y jump); None: the truth's own"""
    pi = +mpmath.pi
    dl0 = lam - t["lon0"]
    k = turns if turns is not None else (-1 if dl0 > pi else 1 if dl0 < -pi else 0)
    dl = dl0 + 2 * pi * int(k)
    rho = t["fact"] * t["radius"] * mpmath.tan((pi / 2 - t["h"] * phi) / 2) ** t["c"]
    a = t["c"] * dl
    return (t["pole_x"] + rho * mpmath.sin(a), t["pole_y"] - t["h"] * rho * mpmath.cos(a), mpmath.cos(a), -t["h"] * mpmath.sin(a), rho, dl0)


def mp_phys2ij(t, lon, lat, turns=None, pi_conv=PI_REF):
    """the truth of phys2ij for rows of doubles in degrees: dict of object arrays ri, rj, rotc [n, 2], rho, dl0"""
    lon, lat = np.atleast_1d(np.asarray(lon, dtype=np.float64)), np.atleast_1d(np.asarray(lat, dtype=np.float64))
    out = dict(ri=[], rj=[], rotc=[], rho=[], dl0=[])
    with mpmath.workdps(DPS):
        conv = (+mpmath.pi if pi_conv is None else mpf(pi_conv)) / 180
        for n in range(lon.size):
            x, y, r0, r1, rho, dl0 = mp_forward(t, mpf(lon[n]) * conv, mpf(lat[n]) * conv, None if turns is None else turns[n])
            out["ri"].append((x - t["cxg1"]) / t["dx"] + 1), out["rj"].append((y - t["cyg1"]) / t["dy"] + 1)
            out["rotc"].append([r0, r1]), out["rho"].append(rho), out["dl0"].append(dl0)
    return {k: np.array(v, dtype=object) for k, v in out.items()}


def mp_xy2phys(t, x, y):
    pi = +mpmath.pi
    rf = t["radius"] * t["fact"]
    xx, yy = (x - t["pole_x"]) / rf, -t["h"] * (y - t["pole_y"]) / rf
    lam = t["lon0"] + mpmath.atan2(xx, yy) / t["c"]
    phi = t["h"] * (pi / 2 - 2 * mpmath.atan(mpmath.hypot(xx, yy) ** (1 / t["c"])))
    lon, lat = lam * 180 / mpf(PI_REF), phi * 180 / mpf(PI_REF)
    dl = lon * mpf(PI_REF) / 180 - t["lon0"]          # the rotation at the longitude returned (not near the cut here)
    a = t["c"] * dl
    return lon, lat, [mpmath.cos(a), -t["h"] * mpmath.sin(a)]


def mp_ij2phys(t, ri, rj, cx1=None, cy1=None):
    """the truth of ij2phys for rows of doubles (cx1 / cy1: a subdomain's GRID_CX(1) / GRID_CY(1) in place of cxg1 / cyg1): dict of
    object arrays lon, lat, rotc [n, 2]"""
    ri, rj = np.atleast_1d(np.asarray(ri, dtype=np.float64)), np.atleast_1d(np.asarray(rj, dtype=np.float64))
    out = dict(lon=[], lat=[], rotc=[])
    with mpmath.workdps(DPS):
        x1, y1 = (t["cxg1"] if cx1 is None else mpf(cx1)), (t["cyg1"] if cy1 is None else mpf(cy1))
        for n in range(ri.size):
            lon, lat, rotc = mp_xy2phys(t, (mpf(ri[n]) - 1) * t["dx"] + x1, (mpf(rj[n]) - 1) * t["dy"] + y1)
            out["lon"].append(lon), out["lat"].append(lat), out["rotc"].append(rotc)
    return {k: np.array(v, dtype=object) for k, v in out.items()}


def bound_constants(p, t):
    """{constant: absolute bound} for derived constants made with a 64-bit significand and rounded to double: the rounding, half
    an ulp, and as much again for what the wider format loses -- c = N / Dn is a quotient of two differences of logarithms, each
    logarithm with its own rounding and its argument's, 4 * 2^-63 per difference at most, so 4 * 2^-63 (1/|N| + 1/|Dn|) < 2^-56
    relative for parallels a degree apart or more; fact and the pole's offset inherit it twice and three times.  An ulp each;
    pole_y is a sum, rounded at its own size, of basepoint_y and an offset of the size of rho."""
    off = float(abs(t["pole_y"] - mpf(p["basepoint_y"])))
    return dict(lon0=2 * EPS * abs(float(t["lon0"])), c=2 * EPS * float(t["c"]), fact=2 * EPS * float(t["fact"]), pole_x=0.0,
                pole_y=2 * EPS * (abs(float(t["pole_y"])) + off))


def err(got, truth):
    """|got - truth| elementwise as float64, the difference taken at the truth's precision"""
    got, truth = np.asarray(got, dtype=np.float64), np.asarray(truth, dtype=object)
    assert got.shape == truth.shape, (got.shape, truth.shape)
    with mpmath.workdps(DPS):
        return np.array([float(abs(mpf(g) - t)) for g, t in zip(got.ravel(), truth.ravel())]).reshape(got.shape)


def check_rows(q, p, got, truth, what=""):
    """a phys2ij result (dict ri, rj and, where there, rotc) against the truth within the bounds; returns the maxima as shares of
    the bounds"""
    rho = np.array([float(r) for r in truth["rho"]])
    b = bound_ij(rho, p)
    shares = {}
    for k in ("ri", "rj"):
        e = err(got[k], truth[k])
        assert np.all(e <= b), (what, k, float(np.max(e / b)))
        shares[k] = float(np.max(e / b)) if e.size else 0.0
    if got.get("rotc") is not None:
        e = err(got["rotc"], truth["rotc"])
        assert np.all(e <= BOUND_ROTC), (what, "rotc", float(e.max() / BOUND_ROTC))
        shares["rotc"] = float(e.max() / BOUND_ROTC) if e.size else 0.0
    return shares


def check_phys(got, truth, what="", factor=1.0):
    """an ij2phys result (dict lon, lat, rotc where there) against the truth within the bound times factor"""
    shares = {}
    for k in ("lon", "lat"):
        e = err(got[k], truth[k])
        assert np.all(e <= factor * BOUND_DEG), (what, k, float(e.max() / BOUND_DEG))
        shares[k] = float(e.max() / BOUND_DEG) if e.size else 0.0
    if got.get("rotc") is not None:
        e = err(got["rotc"], truth["rotc"])
        assert np.all(e <= BOUND_ROTC), (what, "rotc", float(e.max() / BOUND_ROTC))
        shares["rotc"] = float(e.max() / BOUND_ROTC) if e.size else 0.0
    return shares


def points(seed, n, south=False):
    """n random points in 125..146 E, 25..45 N (S for the southern mirror), degrees"""
    rng = np.random.default_rng(seed)
    lon, lat = rng.uniform(125.0, 146.0, n), rng.uniform(25.0, 45.0, n)
    return lon, -lat if south else lat
