"""letkf_phys2ij_dev, letkf_ij2phys_dev and letkf_mapproj_grid_dev (include/letkf_amd_mapproj.h) against the truth of
tests/_mapproj.py, the 50-digit evaluation, within the issue's bounds:
  ri / rj      16 * 2^-53 * rho / min(dx, dy) grid units, rho the point's distance from the cone's pole
  rotc         8 * 2^-53 absolute
  lon / lat    16 * 2^-53 * 180 degrees; the round trip ij2phys(phys2ij) twice that
The truth costs 0.2 ms per row: every row up to 257 is compared with it, and of the long cases (70 001 rows; 524 545 rows, which
is above one pass of the grid-stride loop, 524 288 lanes) a strided sample, the first and last rows and the rows on both sides of
the pass -- while ALL their rows are compared with the float64 statement within twice the bound (each of the two is within one
bound of the truth).

Measured on an MI355X (worst error as a share of its bound, over all cases of this file): ri / rj 0.36, rotc 0.72, lon / lat
0.11, ij2phys' and the grid loop's rotc 0.43, the round trip 0.09 of twice the bound."""
import numpy as np
import pytest
import torch

import _mapproj as M

pytestmark = pytest.mark.gpu
NAMES = list(M.configs())
ROWS = (0, 1, 63, 64, 65, 257, 70001)
PASS = 524288                                   # lanes of one pass of the kernels' loop (letkf_mapproj.hip)
WORST = {}


@pytest.fixture(scope="module")
def env():
    from _gpu import ctx, pkg
    return pkg, ctx()


def make_cfg(pkg, name):
    p = M.configs()[name]
    return dict(name=name, p=p, q=M.setup(p), t=M.mp_setup(p), proj=pkg.mapproj_setup(**M.setup_args(p)))


@pytest.fixture(scope="module", params=NAMES)
def cfg(request, env):
    return make_cfg(env[0], request.param)


def dv(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()


def host(out):
    torch.cuda.synchronize()
    return [None if t is None else t.cpu().numpy() for t in out]


def note(kind, shares):
    for k, v in shares.items():
        WORST[(kind, k)] = max(WORST.get((kind, k), 0.0), v)
    print(kind, {k: round(v, 3) for k, v in shares.items()})


def sample(n):
    """the rows compared with the truth: all up to 600, else a stride, both ends and both sides of the loop's pass"""
    if n <= 600:
        return np.arange(n)
    picks = [np.arange(0, n, max(n // 200, 1)), np.arange(64), np.arange(n - 64, n)]
    if n > PASS:
        picks.append(np.arange(PASS - 32, PASS + 32))
    return np.unique(np.concatenate(picks))


def check_forward(cfg, lon, lat, ri, rj, rotc, turns=None, what=""):
    """device rows against the truth on sample(n) and against the statement on all rows"""
    n, p, q = lon.size, cfg["p"], cfg["q"]
    st = M.phys2ij(q, lon, lat)
    b = 2 * M.bound_ij(st["rho"], p)
    assert np.all(np.abs(ri - st["ri"]) <= b) and np.all(np.abs(rj - st["rj"]) <= b), what
    if rotc is not None:
        assert rotc.shape == (n, 2) and np.all(np.abs(rotc - st["rotc"]) <= 2 * M.BOUND_ROTC), what
    s = sample(n)
    truth = M.mp_phys2ij(cfg["t"], lon[s], lat[s], turns=None if turns is None else turns[s])
    note("phys2ij", M.check_rows(q, p, dict(ri=ri[s], rj=rj[s], rotc=None if rotc is None else rotc[s]), truth, what))
    return st


def forward_and_back(env, cfg, n, with_rotc):
    pkg, ctx = env
    lon, lat = M.points(1000 + n, n, south=cfg["name"] == "south")
    ri, rj, rotc = host(ctx.phys2ij(cfg["proj"], dv(lon), dv(lat), rotc=with_rotc))
    assert ri.shape == rj.shape == (n,) and (rotc is None) == (not with_rotc)
    if n == 0:
        return
    check_forward(cfg, lon, lat, ri, rj, rotc, what=f"{cfg['name']} n={n}")
    # ... and back, from the device's own ri / rj
    blon, blat, brotc = host(ctx.ij2phys(cfg["proj"], dv(ri), dv(rj), rotc=with_rotc))
    st = M.ij2phys(cfg["q"], ri, rj)
    assert np.all(np.abs(blon - st["lon"]) <= 2 * M.BOUND_DEG) and np.all(np.abs(blat - st["lat"]) <= 2 * M.BOUND_DEG)
    s = sample(n)
    truth = M.mp_ij2phys(cfg["t"], ri[s], rj[s])
    note("ij2phys", M.check_phys(dict(lon=blon[s], lat=blat[s], rotc=None if brotc is None else brotc[s]), truth))
    trip = max(np.abs(blon - lon).max(), np.abs(blat - lat).max()) / (2 * M.BOUND_DEG)
    note("roundtrip", dict(deg=float(trip)))
    assert trip <= 1.0


@pytest.mark.parametrize("n", ROWS)
@pytest.mark.parametrize("with_rotc", (True, False), ids=("rotc", "norotc"))
def test_phys2ij_and_back_within_the_bounds(env, cfg, n, with_rotc):
    forward_and_back(env, cfg, n, with_rotc)


def test_a_row_count_above_one_pass_of_the_loop(env):
    """524 545 rows: the second pass of the grid-stride loop, which does not depend on the projection's constants (one
    configuration)"""
    forward_and_back(env, make_cfg(env[0], NAMES[0]), PASS + 257, True)


def test_a_longitude_in_0_360_and_in_minus_180_180_is_the_same_point(env, cfg):
    """135 E as 135 and as -225, 150 W as 210 and as -150: the same point to the conversion's rounding, each within the bounds of
    its own truth (the turn is the truth's own: none of these is near the cut)"""
    pkg, ctx = env
    lon, lat = M.points(31, 65, south=cfg["name"] == "south")
    west = np.concatenate([lon, np.linspace(200.0, 230.0, 64)])                  # 160 W .. 130 W, far from the base point
    lat = np.concatenate([lat, lat[:64]])
    got = {}
    for tag, lo in (("0..360", west), ("-180..180", np.where(west > 180.0, west - 360.0, west)), ("minus", west - 360.0)):
        ri, rj, rotc = host(ctx.phys2ij(cfg["proj"], dv(lo), dv(lat)))
        st = check_forward(cfg, lo, lat, ri, rj, rotc, what=tag)
        got[tag] = (ri, rj, rotc, st["k"])
    assert set(got["minus"][3]) == {1} and set(got["0..360"][3][:65]) == {0}
    for a, b in (("0..360", "-180..180"), ("0..360", "minus")):
        # NOT the same point to rounding: the conversion turns 360 degrees into 2 * 3.1415926535 rad and the wrap takes 2 pi off,
        # so a longitude given one turn away lies 2 (pi - 3.1415926535) = 1.8e-10 rad from itself (a millimetre), times c < 1,
        # times rho, in grid units; beside it the rounding of the conversion at |lam| < 8, 2 * 2^-53 * 8 rad, and both bounds
        rho = M.phys2ij(cfg["q"], west, lat)["rho"]
        tol = (2 * (np.pi - M.PI_REF) + 16 * M.EPS) * rho / min(cfg["p"]["dx"], cfg["p"]["dy"]) + 2 * M.bound_ij(rho, cfg["p"])
        assert np.all(np.abs(got[a][0] - got[b][0]) <= tol) and np.all(np.abs(got[a][1] - got[b][1]) <= tol)


def test_the_cut_at_plus_and_minus_pi(env, cfg):
    """the 13 consecutive doubles of lon around each cut: their float64 dlam reaches +-pi to within its own spacing (lam has the
    spacing of a value in [4, 8), twice pi's: not every neighbour of pi is some row's dlam) and lies on both sides.  x and y jump
    at the cut, and a row within rounding of it may take either side: the truth is evaluated with the turn the float64 statement took, and the test asserts
    separately that this turn is right wherever the true dlam is further from the cut than the conversion's and the
    subtraction's rounding (4 * 2^-53 * 8 rad)."""
    pkg, ctx = env
    q, t = cfg["q"], cfg["t"]
    lons = []
    for sign in (1.0, -1.0):
        lon = (q["lon0"] + sign * np.pi) * 180.0 / M.PI_REF
        down = up = lon
        lons.append(lon)
        for _ in range(6):
            down, up = np.nextafter(down, -1000.0), np.nextafter(up, 1000.0)
            lons += [down, up]
    lon, lat = np.array(lons), np.full(len(lons), 35.0 * q["h"])
    st = M.phys2ij(q, lon, lat)
    assert set(st["k"]) == {-1, 0, 1}, st["k"]                                     # both sides of both cuts are there
    dl = np.abs(lon * M.PI_REF / 180.0 - q["lon0"])
    assert np.abs(dl - np.pi).min() <= 2 * np.spacing(np.pi) and (dl > np.pi).any() and (dl < np.pi).any()
    ri, rj, rotc = host(ctx.phys2ij(cfg["proj"], dv(lon), dv(lat)))
    assert np.all(np.isfinite(ri)) and np.all(np.isfinite(rotc))
    truth = M.mp_phys2ij(t, lon, lat, turns=st["k"])
    note("cut", M.check_rows(q, cfg["p"], dict(ri=ri, rj=rj, rotc=rotc), truth, "cut"))
    import mpmath
    with mpmath.workdps(M.DPS):
        for k, dl0 in zip(st["k"], truth["dl0"]):
            far = abs(abs(dl0) - mpmath.pi) > 4 * M.EPS * 8
            own = -1 if dl0 > mpmath.pi else 1 if dl0 < -mpmath.pi else 0
            assert not far or k == own, (k, float(dl0))


def test_special_rows(env, cfg):
    pkg, ctx = env
    p, q, h = cfg["p"], cfg["q"], cfg["q"]["h"]
    nan, inf = np.nan, np.inf
    blon, blat = p["basepoint_lon"], p["basepoint_lat"]
    lon = np.array([blon, blon, blon, nan, blon, inf, -inf, blon, blon, blon + 720.0, blon, blon])
    lat = np.array([blat, 90.0 * h, -90.0 * h, blat, nan, blat, blat, inf, -inf, blat, 90.5, -90.5])
    ri, rj, rotc = host(ctx.phys2ij(cfg["proj"], dv(lon), dv(lat)))
    # the base point: (basepoint_x, basepoint_y) but for the 10-digit pi of the conversion, within the bound of the truth
    truth = M.mp_phys2ij(cfg["t"], lon[:1], lat[:1])
    M.check_rows(q, p, dict(ri=ri[:1], rj=rj[:1], rotc=rotc[:1]), truth, "base point")
    rho0 = float(truth["rho"][0])
    off = 2.9e-11 * (abs(q["lon0"]) * q["c"] * rho0 + abs(blat) * np.pi / 180.0 * 2.0 * p["radius"]) + 1e-6      # metres
    assert abs((ri[0] - 1.0) * p["dx"] + p["cxg1"] - p["basepoint_x"]) < off and abs((rj[0] - 1.0) * p["dy"] + p["cyg1"] - p["basepoint_y"]) < off
    # the near pole, 4.5e-11 rad short of it through the conversion: finite, some metres from the pole's image
    px, py = (q["pole_x"] - p["cxg1"]) / p["dx"] + 1.0, (q["pole_y"] - p["cyg1"]) / p["dy"] + 1.0
    # (rho = fact * radius * tan(short / 2)^c; pi/2 - phi loses 6e-17 of 4.5e-11 to pi's own rounding, and the sum with the pole
    # rounds at the pole's size: 1e-5 relative and a micrometre are wide)
    short = 90.0 * (np.pi - M.PI_REF) / 180.0
    want = q["fact"] * q["radius"] * np.tan(0.5 * short) ** q["c"]
    assert np.isfinite(ri[1]) and np.isfinite(rj[1]) and 0.1 < want < 1000.0       # (0.27 m at c = 0.72, 180 m at c = 0.46)
    assert abs(np.hypot((ri[1] - px) * p["dx"], (rj[1] - py) * p["dy"]) - want) <= 1e-5 * want + 1e-6
    # the far pole: outside every domain
    assert not (abs(rj[2]) < 1e6) and not np.isnan(rotc[2]).any()
    # NaN, +-Inf, more than one wrap: NaN in ri, rj and rotc
    for n in range(3, 10):
        assert np.isnan(ri[n]) and np.isnan(rj[n]) and np.isnan(rotc[n]).all(), (n, lon[n], lat[n])
    # beyond a pole: NaN in ri / rj
    assert np.isnan(ri[10:]).all() and np.isnan(rj[10:]).all()
    # and the same bits as the statement wherever it gives NaN
    st = M.phys2ij(q, lon, lat)
    assert np.array_equal(np.isnan(st["ri"]), np.isnan(ri)) and np.array_equal(np.isnan(st["rotc"]), np.isnan(rotc))


def test_two_calls_give_equal_bits(env, cfg):
    pkg, ctx = env
    lon, lat = M.points(5, 70001, south=cfg["name"] == "south")
    a = host(ctx.phys2ij(cfg["proj"], dv(lon), dv(lat)))
    b = host(ctx.phys2ij(cfg["proj"], dv(lon), dv(lat)))
    for x, y in zip(a, b):
        assert np.array_equal(x.view(np.int64), y.view(np.int64))
    c = host(ctx.ij2phys(cfg["proj"], dv(a[0]), dv(a[1])))
    d = host(ctx.ij2phys(cfg["proj"], dv(a[0]), dv(a[1])))
    for x, y in zip(c, d):
        assert np.array_equal(x.view(np.int64), y.view(np.int64))
    # without rotc: the bits of ri / rj of the call with it
    e = host(ctx.phys2ij(cfg["proj"], dv(lon), dv(lat), rotc=False))
    assert np.array_equal(e[0].view(np.int64), a[0].view(np.int64)) and np.array_equal(e[1].view(np.int64), a[1].view(np.int64))


@pytest.mark.parametrize("i0,j0", [(0, 0), (6, 10)], ids=("first", "offset"))
def test_the_grid_loop_on_a_3_by_5_subdomain(env, cfg, i0, j0):
    """nlon = 3, nlat = 5, halos 2, as the subdomain whose first interior point is global (i0 + 1, j0 + 1): every output alone and
    all together, against the truth; then lon2d / lat2d back through letkf_phys2ij_dev"""
    pkg, ctx = env
    p, q, t = cfg["p"], cfg["q"], cfg["t"]
    nlon, nlat, ih, jh = 3, 5, 2, 2
    cx1, cy1 = p["cxg1"] + i0 * p["dx"], p["cyg1"] + j0 * p["dy"]            # GRID_CX(1) of the subdomain is GRID_CXG(1 + i0)
    every = ctx.mapproj_grid(cfg["proj"], nlon, nlat, ih, jh, cx1, cy1)
    lon2d, lat2d, rotc2d = host([every["lon"], every["lat"], every["rotc"]])
    assert lon2d.shape == lat2d.shape == (nlat, nlon) and rotc2d.shape == (nlat, nlon, 2)
    jj, ii = np.meshgrid(np.arange(nlat), np.arange(nlon), indexing="ij")
    ri, rj = (ii + 1 + ih).astype(np.float64).ravel(), (jj + 1 + jh).astype(np.float64).ravel()
    truth = M.mp_ij2phys(t, ri, rj, cx1=cx1, cy1=cy1)
    note("grid", M.check_phys(dict(lon=lon2d.ravel(), lat=lat2d.ravel(), rotc=rotc2d.reshape(-1, 2)), truth, "grid"))
    st = M.grid(q, nlon, nlat, ih, jh, cx1, cy1)
    assert np.all(np.abs(lon2d - st["lon"]) <= 2 * M.BOUND_DEG) and np.all(np.abs(rotc2d - st["rotc"]) <= 2 * M.BOUND_ROTC)
    for want in (("lon",), ("lat",), ("rotc",), ("lon", "rotc")):
        one = ctx.mapproj_grid(cfg["proj"], nlon, nlat, ih, jh, cx1, cy1, want=want)
        torch.cuda.synchronize()
        for k in ("lon", "lat", "rotc"):
            assert (one[k] is None) == (k not in want)
            if k in want:
                assert torch.equal(one[k].view(torch.int64), every[k].view(torch.int64)), (want, k)
    # back: the global grid coordinates i + IHALO + i0, j + JHALO + j0, within the round-trip bound carried to grid units:
    # 2 * 16 * 2^-53 * 180 degrees are 2 * 16 * 2^-53 * pi rad; d(lam) moves a point by rho c d(lam) < rho d(lam), d(phi) by
    # rho c d(phi) / sin(psi) < 1.5 rho d(phi) (c < 1, sin(psi) = cos(lat) > 0.7 below 45 degrees); plus phys2ij's own bound
    bri, brj, _ = host(ctx.phys2ij(cfg["proj"], every["lon"].reshape(-1), every["lat"].reshape(-1), rotc=False))
    rho = M.phys2ij(q, lon2d.ravel(), lat2d.ravel())["rho"]
    tol = 1.5 * 2 * 16 * M.EPS * np.pi * rho / min(p["dx"], p["dy"]) + M.bound_ij(rho, p)
    assert np.abs(lat2d).max() < 45.0
    assert np.all(np.abs(bri - (ri + i0)) <= tol) and np.all(np.abs(brj - (rj + j0)) <= tol), (np.abs(bri - ri - i0).max(), tol.min())


def test_the_host_helpers_agree_with_the_kernels_within_4_ulp(env, cfg):
    pkg, ctx = env
    lon, lat = M.points(77, 65, south=cfg["name"] == "south")
    ri, rj, rotc = host(ctx.phys2ij(cfg["proj"], dv(lon), dv(lat)))
    blon, blat, brotc = host(ctx.ij2phys(cfg["proj"], dv(ri), dv(rj)))
    rho = M.phys2ij(cfg["q"], lon, lat)["rho"]
    for n in range(lon.size):
        hri, hrj, hrotc = pkg.phys2ij_host(cfg["proj"], float(lon[n]), float(lat[n]), rotc=True)
        # ri is (x - cxg1) / dx + 1 with x = pole_x + rho sin: 4 ulp of the size it was computed at, rho
        ulp = np.spacing(rho[n]) / min(cfg["p"]["dx"], cfg["p"]["dy"])
        assert abs(hri - ri[n]) <= 4 * ulp and abs(hrj - rj[n]) <= 4 * ulp, (n, hri - ri[n], hrj - rj[n], ulp)
        assert abs(hrotc[0] - rotc[n, 0]) <= 4 * np.spacing(1.0) and abs(hrotc[1] - rotc[n, 1]) <= 4 * np.spacing(1.0)
        hlon, hlat, hr = pkg.ij2phys_host(cfg["proj"], float(ri[n]), float(rj[n]), rotc=True)
        # (phi is made as pi/2 - 2 atan(...): its roundings are those of values up to 90 degrees)
        assert abs(hlon - blon[n]) <= 4 * np.spacing(abs(blon[n])) and abs(hlat - blat[n]) <= 4 * np.spacing(90.0)
        assert abs(hr[0] - brotc[n, 0]) <= 4 * np.spacing(1.0) and abs(hr[1] - brotc[n, 1]) <= 4 * np.spacing(1.0)


def test_the_measured_maxima_stay_below_the_bounds():
    """(runs last: the worst shares of the bounds this file saw, printed for DESIGN.md section 19)"""
    print({f"{a}.{b}": round(v, 3) for (a, b), v in sorted(WORST.items())})
    assert WORST and max(WORST.values()) <= 1.0
