"""letkf_das_interp_window_dev (include/letkf_amd_interp_window.h): weight interpolation on the coarse lattice of the whole
domain, a call analysing a window of it.  The bar is bit equality: a tile handed the minimal array rectangle -- with every
input outside its owned rectangle that is not on a coarse column set to NaN -- gives, at its owned points, the bits of the
single-domain call (letkf_das_interp_dev on the whole arrays), and leaves every other output element at its fill value.
"Bitwise" is np.array_equal(..., equal_nan=True) on anal, rtps_infl_out and status.  The base case is the 7 x 5 x 3 grid of
tests/_interp.py; every call of a test takes the same search table."""
import importlib

import numpy as np
import pytest
import torch

import _interp as I

pytestmark = pytest.mark.gpu
RTPS = dict(relax_alpha_spread=0.95)
DET = dict(relax_alpha_spread=0.95, det_run=1)
ANAL_FILL, RTPS_FILL, STATUS_FILL, NOBS_FILL = -3.25, -5.5, -1, -7
XR, YR = ((0, 4), (4, 7)), ((0, 3), (3, 5))           # the uneven 2 x 2 tiles of the 7 x 5 grid: owned [p0, p1) x [q0, q1)
TILES = [(xr[0], xr[1], yr[0], yr[1]) for yr in YR for xr in XR]


def sharding():
    from _gpu import pkg  # noqa: F401  (loads the package)
    return importlib.import_module("scale_letkf_amd.sharding")


def rectangle(c, sx, sy, own):
    """the minimal array rectangle of the owned global rectangle (sharding.interp_window_rect), with the global lines lx, ly"""
    r = sharding().interp_window_rect(c["nx"], c["ny"], sx, sy, *own)
    r.update(lx=[i + r["gi0"] for i in r["lines_x"]], ly=[j + r["gj0"] for j in r["lines_y"]])
    return r


def cut(c, sx, sy, own, beta=None, rect=None, poison=True):
    """The arrays of one call: the rectangle cut out of the case, NaN at every input element outside the owned rectangle that
    is not on one of the call's coarse columns (coordinates, state, infl, beta)."""
    r = rect or rectangle(c, sx, sy, own)
    p0, p1, q0, q1 = own
    nx, ny, nlev, nv, NX, NY = r["nx"], r["ny"], c["nlev"], c["nv"], c["nx"], c["ny"]
    gi, gj = np.arange(r["gi0"], r["gi0"] + nx), np.arange(r["gj0"], r["gj0"] + ny)
    col = (gi[None, :] + NX * gj[:, None]).ravel()                                     # global column of array column
    gp = (col[None, :] + c["nij1"] * np.arange(nlev)[:, None]).ravel()                 # global point of array point
    owned_c = ((gi[None, :] >= p0) & (gi[None, :] < p1) & (gj[:, None] >= q0) & (gj[:, None] < q1)).ravel()
    coarse_c = (np.isin(gi, r["lx"])[None, :] & np.isin(gj, r["ly"])[:, None]).ravel()
    dead_c = ~owned_c & ~coarse_c if poison else np.zeros_like(owned_c)
    dead = np.tile(dead_c, nlev)
    a = dict(rig=c["rig"][col].copy(), rjg=c["rjg"][col].copy(), rlev=c["rlev"][gp].copy(), rz=c["rz"][gp].copy(),
             gues=c["gues"][:, :, gp].copy(), infl=c["infl"].reshape(nv, c["npts"])[:, gp].copy(),
             beta=None if beta is None else beta[gp].copy())
    a["rig"][dead_c] = a["rjg"][dead_c] = np.nan
    a["rlev"][dead] = a["rz"][dead] = np.nan
    a["gues"][:, :, dead] = np.nan
    a["infl"][:, dead] = np.nan
    if beta is not None:
        a["beta"][dead] = np.nan
    a.update(r, gp=gp, owned=np.tile(owned_c, nlev), dead=dead, npts=nx * ny * nlev, own=own)
    return a


def launch(c, a, sx, sy, cfg, window="own", mask=0, inplace=False, entry="window", ncoarse=None, **extra):
    """one call on the arrays `a`; dict(anal (nv, nens, npts), rtps (nv, npts), status, nobs, path, gues (after the call))"""
    from _gpu import ctx, dev
    from _search import device_struct
    cx = ctx()
    d = torch.device("cuda:0")
    t, keep = device_struct(c["tc"], d)
    k, nv, nens, npts = c["k"], c["nv"], c["nens"], a["npts"]
    gues = dev(a["gues"].reshape(-1))
    anal = gues if inplace else torch.full_like(gues, ANAL_FILL)
    status = torch.full((npts,), STATUS_FILL, dtype=torch.int32, device=d)
    rtps = torch.full((npts * nv,), RTPS_FILL, dtype=torch.float64, device=d)
    if ncoarse is None:
        ncoarse = len(a["lx"]) * len(a["ly"]) * c["nlev"]
    nobs = torch.full((ncoarse,), NOBS_FILL, dtype=torch.int32, device=d)
    out = dict(anal=anal, rtps=rtps, status=status, nobs=nobs)
    args = (k, nv, t, a["nx"], a["ny"], c["nlev"], sx, sy, dev(a["rig"]), dev(a["rjg"]), dev(a["rlev"]), dev(a["rz"]), dev(c["ensval"]),
            c["kld"], dev(c["dep"]), dev(a["infl"].reshape(-1)), gues, anal, 1, npts, npts * nens)
    kw = dict(nobs_coarse=nobs, beta=None if a["beta"] is None else dev(a["beta"]), status=status, rtps_infl_out=rtps, var_mask=mask,
              iv_q_last=min(10, nv - 1), **cfg, **extra)
    try:
        if entry == "window":
            cx.das_interp_window(*args, window=a["window"] if window == "own" else window, **kw)
        else:
            cx.das_interp(*args, **kw)
    finally:
        torch.cuda.synchronize()
        out = {n: v.cpu().numpy() for n, v in out.items()}
        out["anal"] = out["anal"].reshape(nv, nens, npts)
        out["rtps"] = out["rtps"].reshape(nv, npts)
        out["gues"] = gues.cpu().numpy().reshape(nv, nens, npts)
        launch.last = out
    out["path"] = cx.last_path()
    return out


def whole_arrays(c, beta=None):
    return cut(c, 1, 1, (0, c["nx"], 0, c["ny"]), beta=beta)


_whole = {}


def whole(c, sx, sy, cfg, beta=None, mask=0, inplace=False, tag=""):
    """letkf_das_interp_dev on the whole domain, once per setting"""
    key = (c["k"], c["nv"], sx, sy, tuple(sorted(cfg.items())), mask, inplace, tag)
    if key not in _whole:
        a = whole_arrays(c, beta)
        lx, ly = I.coarse_axis(c["nx"], sx), I.coarse_axis(c["ny"], sy)
        r = launch(c, a, sx, sy, cfg, mask=mask, inplace=inplace, entry="old", ncoarse=len(lx) * len(ly) * c["nlev"])
        assert "letkf_interp_apply_kernel" in r["path"], r["path"]
        for v in r.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _whole[key] = r
    return _whole[key]


def written_slots(c, cfg):
    return list(range(c["k"])) + ([c["k"] + 1] if cfg.get("det_run") else [])


def same_bits(c, cfg, w, t, a, mask=0, inplace=False, sx=None, sy=None):
    """the call's owned points hold the whole call's bits, everything else its fill value; nobs_coarse is the whole call's
    sub-block where sx, sy are given"""
    k, nv = c["k"], c["nv"]
    o, gp = a["owned"], a["gp"]
    slots = written_slots(c, cfg)
    other = [m for m in range(c["nens"]) if m not in slots]
    vs = [v for v in range(nv) if not mask or (mask >> v) & 1]
    nvs = [v for v in range(nv) if v not in vs]
    eq = lambda x, y: np.array_equal(x, y, equal_nan=True)
    assert o.sum() == (a["own"][1] - a["own"][0]) * (a["own"][3] - a["own"][2]) * c["nlev"]
    assert np.isfinite(t["anal"][vs][:, slots][:, :, o]).all()
    assert eq(t["anal"][vs][:, slots][:, :, o], w["anal"][vs][:, slots][:, :, gp[o]])
    assert eq(t["rtps"][vs][:, o], w["rtps"][vs][:, gp[o]])
    assert eq(t["status"][o], w["status"][gp[o]]) and (t["status"][o] == 0).all()
    assert (t["status"][~o] == STATUS_FILL).all()
    assert (t["rtps"][:, ~o] == RTPS_FILL).all() and (t["rtps"][nvs] == RTPS_FILL).all()
    if inplace:
        assert eq(t["anal"][:, :, ~o], a["gues"][:, :, ~o])            # the halo's state, NaN and coarse columns alike
        assert eq(t["anal"][:, other][:, :, o], a["gues"][:, other][:, :, o]) and eq(t["anal"][nvs], a["gues"][nvs])
    else:
        assert (t["anal"][:, :, ~o] == ANAL_FILL).all() and (t["anal"][:, other] == ANAL_FILL).all() and (t["anal"][nvs] == ANAL_FILL).all()
        assert eq(t["gues"], a["gues"])
    if sx is not None:
        Lx, Ly = list(I.coarse_axis(c["nx"], sx)), list(I.coarse_axis(c["ny"], sy))
        sub = w["nobs"].reshape(c["nlev"], len(Ly), len(Lx))[:, [Ly.index(l) for l in a["ly"]]][:, :, [Lx.index(l) for l in a["lx"]]]
        assert np.array_equal(t["nobs"], sub.ravel())


def tiles_same_bits(c, sx, sy, cfg, beta=None, mask=0, inplace=False, tiles=TILES, tag=""):
    w = whole(c, sx, sy, cfg, beta=beta, mask=mask, inplace=inplace, tag=tag)
    seen = np.zeros(c["npts"], int)
    for own in tiles:
        a = cut(c, sx, sy, own, beta=beta)
        t = launch(c, a, sx, sy, cfg, mask=mask, inplace=inplace)
        assert "letkf_interp_apply_kernel" in t["path"], t["path"]
        same_bits(c, cfg, w, t, a, mask=mask, inplace=inplace, sx=sx, sy=sy)
        seen[a["gp"][a["owned"]]] += 1
    return seen, w


# ---- a
@pytest.mark.parametrize("sx,sy", [(2, 2), (3, 2)])
def test_whole_domain_window_is_the_old_entry(sx, sy):
    c = I.tile_case(50)
    w = whole(c, sx, sy, DET)
    a = whole_arrays(c)
    a.update(lx=list(I.coarse_axis(c["nx"], sx)), ly=list(I.coarse_axis(c["ny"], sy)))
    for window in ((c["nx"], c["ny"], 0, 0, 0, 0, c["nx"], c["ny"]), None):
        t = launch(c, a, sx, sy, DET, window=window)
        for n in ("anal", "rtps", "status", "nobs"):
            assert np.array_equal(t[n], w[n], equal_nan=True), n
        assert t["path"] == w["path"]
    assert (w["nobs"] == 0).any() and (w["nobs"] > I.LIMITS[0]).any()


# ---- b (and g: same_bits compares nobs_coarse of every tile with the whole call's sub-block)
@pytest.mark.parametrize("sx,sy", [(2, 2), (3, 2), (4, 4), (8, 8)])
def test_uneven_tiles_stitch_to_the_whole_call_bit_for_bit(sx, sy):
    c = I.tile_case(50)
    if (sx, sy) == (8, 8):
        for own in TILES:                       # every tile needs both ends of both axes
            r = rectangle(c, sx, sy, own)
            assert r["lx"] == [0, 6] and r["ly"] == [0, 4] and (r["nx"], r["ny"]) == (7, 5)
    if (sx, sy) == (2, 2):                      # the minimal rectangles: one halo line where the cut is off the lattice
        assert [(r["gi0"], r["nx"], r["gj0"], r["ny"]) for r in (rectangle(c, 2, 2, own) for own in TILES)] == \
            [(0, 5, 0, 3), (4, 3, 0, 3), (0, 5, 2, 3), (4, 3, 2, 3)]
    seen, w = tiles_same_bits(c, sx, sy, DET)
    assert (seen == 1).all()                    # stitched: every point of the domain from exactly one tile


def test_poisoned_halo_is_really_poisoned():
    """the cut of the (2, 2) tiles sets something to NaN in three of four tiles, and only off the coarse columns"""
    c = I.tile_case(50)
    n = 0
    for own in TILES:
        a = cut(c, 2, 2, own)
        n += int(a["dead"].any())
        assert not np.isnan(a["gues"][:, :, a["owned"]]).any()
        assert np.isnan(a["gues"][:, :, a["dead"]]).all() and np.isnan(a["rz"][a["dead"]]).all()
    assert n >= 3


# ---- c
@pytest.mark.parametrize("name,own", [("point_0_0", (0, 1, 0, 1)), ("point_6_4", (6, 7, 4, 5)), ("point_3_2", (3, 4, 2, 3)),
                                      ("strip_i6", (6, 7, 0, 5)), ("strip_j3", (0, 7, 3, 4))])
def test_small_windows_equal_the_whole_call(name, own):
    c = I.tile_case(50)
    seen, w = tiles_same_bits(c, 2, 2, DET, tiles=[own])
    assert seen.sum() == (own[1] - own[0]) * (own[3] - own[2]) * c["nlev"]
    r = rectangle(c, 2, 2, own)
    want = dict(point_0_0=([0], [0]), point_6_4=([6], [4]), point_3_2=([2, 4], [2]), strip_i6=([6], [0, 2, 4]),
                strip_j3=([0, 2, 4, 6], [2, 4]))[name]
    assert (r["lx"], r["ly"]) == want


# ---- d
@pytest.mark.parametrize("k", [3, 63, 100, 128])
def test_ensemble_sizes_bitwise(k):
    """every NCT instantiation of the apply kernel and every solver route behind the coarse solves (one wave, two waves,
    staged): a coarse solve must not depend on its position in the batch or on the batch's longest list"""
    c = I.tile_case(k)
    seen, w = tiles_same_bits(c, 2, 2, DET)
    assert (seen == 1).all()
    route = "NW=1" if k <= 62 else "NW=2" if k <= 100 else "staged:"
    assert route in w["path"], w["path"]


# ---- e
def _beta(c):
    """zeros and tapers; coarse point (2, 2, level 1) of stride (2, 2) has beta = 0, its neighbours beta > 0"""
    rng = np.random.default_rng(3)
    b = np.ones(c["npts"])
    b[rng.integers(0, c["npts"], 12)] = 0.0
    b[rng.integers(0, c["npts"], 12)] = 0.37
    p = 2 + c["nx"] * 2 + c["nij1"] * 1
    b[[p - 1, p + 1, p - c["nx"], p + c["nx"]]] = [1.0, 0.6, 1.0, 0.8]
    b[p] = 0.0
    return b


def test_rules_q_update_top_q_clamp_and_beta():
    c = I.tile_case(50)
    cfg = dict(relax_alpha_spread=0.95, det_run=1, q_update_top=5.0e4, q_sprd_max=0.01)
    beta = _beta(c)
    top = c["gues"][4, c["k"]] < 5.0e4
    assert top.any() and not top.all()
    seen, w = tiles_same_bits(c, 2, 2, cfg, beta=beta, tag="beta")
    assert (seen == 1).all()
    free = whole(c, 2, 2, DET)
    assert not np.array_equal(free["anal"][5, :c["k"]], w["anal"][5, :c["k"]])
    assert (w["rtps"][:, beta == 0.0] == 1.0).all()


def test_rules_five_variables_and_a_class_mask():
    c = I.tile_case(20, nv=5)
    seen, w = tiles_same_bits(c, 2, 2, RTPS, mask=0b10110)
    assert (seen == 1).all()


def test_rules_in_place_leaves_the_halo_state_alone():
    c = I.tile_case(50)
    seen, w = tiles_same_bits(c, 2, 2, DET, inplace=True)
    assert (seen == 1).all()
    out_of_place = whole(c, 2, 2, DET)
    slots = written_slots(c, DET)
    assert np.array_equal(w["anal"][:, slots], out_of_place["anal"][:, slots])


# ---- f
def test_a_tile_against_the_numpy_statement():
    c = I.tile_case(50)
    """a tile of the (2, 2) stitching test, as run there (RTPS and det_run), against obs_local and letkf_core of the oracle and
    the blend and rules in numpy: the members and the deterministic member within 1e-10 max(|mean|, |x'|), rtps within 1e-10"""
    exp = I.expected(c, DET, 2, 2)
    own = TILES[3]
    a = cut(c, 2, 2, own)
    t = launch(c, a, 2, 2, DET)
    k, o, gp, x = c["k"], a["owned"], a["gp"], c["gues"]
    members = written_slots(c, DET)
    assert members == list(range(k)) + [k + 1] and (t["status"][o] == 0).all()
    for v in range(c["nv"]):
        scale = max(np.abs(x[v, k]).max(), np.abs(x[v, :k]).max())
        err = np.abs(t["anal"][v, members][:, o] - exp["anal"][v, members][:, gp[o]]).max()
        rerr = np.abs(t["rtps"][v, o] / exp["rtps"][v, gp[o]] - 1.0).max()
        print(f"v={v} err/scale={err / scale:.3e} rtps {rerr:.3e}")
        assert err <= 1e-10 * scale, (v, err / scale)
        assert rerr <= 1e-10, (v, rerr)


# ---- g
def test_nobs_coarse_is_the_whole_calls_sub_block():
    from _gpu import pkg
    c = I.tile_case(50)
    w = whole(c, 3, 2, DET)
    Lx, Ly = list(pkg.interp_coarse_axis(c["nx"], 3)), list(pkg.interp_coarse_axis(c["ny"], 2))
    full = w["nobs"].reshape(c["nlev"], len(Ly), len(Lx))
    assert np.array_equal(w["nobs"], I.expected(c, DET, 3, 2)["ncoarse"])
    for own in TILES:
        a = cut(c, 3, 2, own)
        win = a["window"]
        ax = pkg.interp_window_axis(c["nx"], 3, win[2], a["nx"], win[4], win[6]) + a["gi0"]
        ay = pkg.interp_window_axis(c["ny"], 2, win[3], a["ny"], win[5], win[7]) + a["gj0"]
        assert list(ax) == a["lx"] and list(ay) == a["ly"]
        t = launch(c, a, 3, 2, DET)
        sub = full[:, [Ly.index(j) for j in ay]][:, :, [Lx.index(i) for i in ax]]
        assert t["nobs"].size == len(ax) * len(ay) * c["nlev"] and np.array_equal(t["nobs"], sub.ravel())


# ---- h
OLD = ["infl_adaptive", "trans_out", "transm_out", "pa_out", "nsweep", "stride_0", "stride_9", "k_129", "npts"]
NEW = {"gnx_0": dict(gnx=0), "gny_0": dict(gny=0), "onx_0": dict(onx=0), "ony_0": dict(ony=0), "ony_negative": dict(ony=-2),
       "gi0_negative": dict(gi0=-1), "gj0_negative": dict(gj0=-1), "arrays_past_the_domain_x": dict(gi0=5),
       "arrays_past_the_domain_y": dict(gj0=3), "domain_smaller_than_arrays": dict(gnx=2), "oi0_negative": dict(oi0=-1),
       "oj0_negative": dict(oj0=-1), "owned_past_the_arrays_x": dict(onx=4), "owned_past_the_arrays_y": dict(oj0=2, ony=2)}
FIELDS = ("gnx", "gny", "gi0", "gj0", "oi0", "oj0", "onx", "ony")


def refused(c, a, sx, sy, window, extra, match="letkf_amd error -1:"):
    from _gpu import pkg
    launch.last = None
    with pytest.raises(pkg.LetkfError, match=match):
        launch(c, a, sx, sy, RTPS, window=window, **extra)
    r = launch.last
    assert (r["anal"] == ANAL_FILL).all() and (r["rtps"] == RTPS_FILL).all() and (r["status"] == STATUS_FILL).all()
    assert (r["nobs"] == NOBS_FILL).all()
    for v in extra.values():
        if torch.is_tensor(v):
            assert int(v.count_nonzero()) == 0


@pytest.mark.parametrize("what", OLD)
def test_refuses_what_the_old_entry_refuses(what):
    d = torch.device("cuda:0")
    c = I.tile_case(129, nlev=1) if what == "k_129" else I.tile_case(50)
    a = cut(c, 2, 2, TILES[3])
    buf = lambda n, dt=torch.float64: torch.zeros(n, dtype=dt, device=d)
    extra, sx, sy = {}, 2, 2
    if what == "infl_adaptive":
        extra = dict(infl_adaptive=True)
    elif what in ("trans_out", "pa_out"):
        extra = {what: buf(a["npts"] * c["k"] ** 2)}
    elif what == "transm_out":
        extra = {what: buf(a["npts"] * c["k"])}
    elif what == "nsweep":
        extra = dict(nsweep=buf(a["npts"], torch.int32))
    elif what == "stride_0":
        sx = 0
    elif what == "stride_9":
        sy = 9
    elif what == "npts":
        extra = dict(npts=a["npts"] - 1)
    refused(c, a, sx, sy, a["window"], extra)


@pytest.mark.parametrize("what", sorted(NEW))
def test_refuses_a_window_that_does_not_fit(what):
    """the tile [4, 7) x [3, 5) at stride (2, 2): arrays 3 x 3 at global (4, 2), owned from array index (0, 1), 3 x 2"""
    c = I.tile_case(50)
    a = cut(c, 2, 2, TILES[3])
    assert a["window"] == (7, 5, 4, 2, 0, 1, 3, 2)
    win = dict(zip(FIELDS, a["window"]))
    win.update(NEW[what])
    refused(c, a, 2, 2, tuple(win[f] for f in FIELDS), {}, match="letkf_amd error -1: window")


@pytest.mark.parametrize("axis,line", [("x", 4), ("x", 6), ("y", 2), ("y", 4)])
def test_refuses_when_a_needed_coarse_line_is_outside_the_arrays(axis, line):
    """owned global [5, 6) x [3, 4) at stride (2, 2) needs the lines x = 4, 6 and y = 2, 4; arrays that stop one short of one of
    them are refused with the axis and the global line in the message"""
    c = I.tile_case(50)
    gi0, gi1, gj0, gj1 = 4, 6, 2, 4                    # the minimal rectangle, inclusive
    if axis == "x":
        gi0, gi1 = (5, 6) if line == 4 else (4, 5)
    else:
        gj0, gj1 = (3, 4) if line == 2 else (2, 3)
    nx, ny = gi1 - gi0 + 1, gj1 - gj0 + 1
    rect = dict(gi0=gi0, gj0=gj0, nx=nx, ny=ny, lx=[4, 6], ly=[2, 4], window=(7, 5, gi0, gj0, 5 - gi0, 3 - gj0, 1, 1))
    a = cut(c, 2, 2, (5, 6, 3, 4), rect=rect, poison=False)
    refused(c, a, 2, 2, a["window"], {}, match=f"letkf_amd error -1: window: the needed coarse line {axis} = {line} ")
    good = cut(c, 2, 2, (5, 6, 3, 4))
    assert (good["gi0"], good["nx"], good["gj0"], good["ny"]) == (4, 3, 2, 3)


# ---- i: per-rank tables (the set_letkf_obs pipeline of tests/_tiles.py), every rank its own table and its own row order
NLON_G = NLAT_G = 24
RANK_K, RANK_NOBS, RANK_SEED = 20, 1500, 77
NGRD_CELL, NSCH, DX = (4, 2, 4), (2, 3, 1), 1000.0
ZLEV = np.array([800.0, 5000.0, 9500.0])
REACH = 2                                              # stride - 1 of the largest stride run here (3)
_worlds = {}


def rank_world(px, py):
    """the ranks' tables, built once per decomposition.  The extended subdomain of a rank covers NSCH mesh cells of NGRD_CELL
    grid cells; hori_loc is set so that the cut-off is that many grid cells less REACH, which a coarse column up to stride - 1
    columns outside the tile needs."""
    import _tiles
    from _obsprep import make_world
    if (px, py) not in _worlds:
        nlon, nlat = NLON_G // px, NLAT_G // py
        w = make_world(RANK_SEED, px=px, py=py, nlon=nlon, nlat=nlat, k=RANK_K, det_run=True, nobs=RANK_NOBS,
                       ngrd=tuple((nlon // s, nlat // s) for s in NGRD_CELL), ngrdsch=tuple((s, s) for s in NSCH))
        w["fix_ij_obsgrd"] = 0
        w["hori_loc"] = np.array([(s * cs - REACH) * DX / _tiles.DZF * 0.999 for s, cs in zip(NSCH, NGRD_CELL)])
        lev_glob = np.random.default_rng(RANK_SEED + 1).uniform(0.0, 12000.0, RANK_NOBS)
        _worlds[(px, py)] = (w, _tiles.rank_pipeline(w, lev_glob, DX))
    return _worlds[(px, py)]


def rank_analysis(px, py, sx, sy, x):
    """the whole 24 x 24 x 3 grid through px x py ranks, each with its own tables, the rectangle and window of
    sharding.interp_tile_window and NaN in the halo off the coarse columns.  (anal like x, {(lev, j, i): nobs_coarse})"""
    from _gpu import ctx, dev
    c, sh = ctx(), sharding()
    w, ranks = rank_world(px, py)
    k, nv, nens, nlev = RANK_K, x.shape[0], x.shape[1], len(ZLEV)
    anal = np.full_like(x, np.nan)
    nobs = {}
    nhalo = 0
    for rk, r in zip(w["ranks"], ranks):
        tw = sh.interp_tile_window(NLON_G, NLAT_G, px, py, rk["pi"], rk["pj"], sx, sy)
        gi0, gj0, nx, ny = tw["gi0"], tw["gj0"], tw["nx"], tw["ny"]
        _, _, _, _, oi0, oj0, onx, ony = tw["window"]
        assert (gi0 + oi0, gj0 + oj0, onx, ony) == (rk["pi"] * NLON_G // px, rk["pj"] * NLAT_G // py, NLON_G // px, NLAT_G // py)
        ii, jj = np.meshgrid(np.arange(nx), np.arange(ny))
        rig = (gi0 + ii.ravel() + 1 + w["ihalo"]).astype(np.float64)
        rjg = (gj0 + jj.ravel() + 1 + w["ihalo"]).astype(np.float64)
        nij, npts = nx * ny, nx * ny * nlev
        owned = ((ii >= oi0) & (ii < oi0 + onx) & (jj >= oj0) & (jj < oj0 + ony)).ravel()
        coarse = (np.isin(ii, tw["lines_x"]) & np.isin(jj, tw["lines_y"])).ravel()
        dead = np.tile(~owned & ~coarse, nlev)
        assert len(tw["halo"]) == (coarse & ~owned).sum() and (dead.any() or not tw["halo"])
        nhalo += len(tw["halo"])
        xs = np.ascontiguousarray(x[:, :, :, gj0:gj0 + ny, gi0:gi0 + nx]).reshape(nv, nens, npts)
        xs[:, :, dead] = np.nan
        rig[dead[:nij]] = rjg[dead[:nij]] = np.nan
        rz = np.repeat(ZLEV, nij)
        rz[dead] = np.nan
        gues = dev(xs.reshape(-1))
        an = torch.full_like(gues, ANAL_FILL)
        status = torch.full((npts,), STATUS_FILL, dtype=torch.int32, device="cuda")
        nc = torch.full((len(tw["lines_x"]) * len(tw["lines_y"]) * nlev,), NOBS_FILL, dtype=torch.int32, device="cuda")
        c.das_interp_window(k, nv, r["tables"], nx, ny, nlev, sx, sy, dev(rig), dev(rjg), dev(np.full(npts, 1.0e5)), dev(rz), r["ensval"],
                            w["kld"], r["dep"], torch.ones(npts * nv, dtype=torch.float64, device="cuda"), gues, an, 1, npts,
                            npts * nens, window=tw["window"], nobs_coarse=nc, det_run=True, status=status, relax_alpha_spread=0.95)
        torch.cuda.synchronize()
        st = status.cpu().numpy()
        o = np.tile(owned, nlev)
        assert (st[o] == 0).all() and (st[~o] == STATUS_FILL).all()
        got = an.cpu().numpy().reshape(nv, nens, nlev, ny, nx)
        assert (got.reshape(nv, nens, npts)[:, :, ~o] == ANAL_FILL).all()
        anal[:, :, :, gj0 + oj0:gj0 + oj0 + ony, gi0 + oi0:gi0 + oi0 + onx] = got[:, :, :, oj0:oj0 + ony, oi0:oi0 + onx]
        ncn = nc.cpu().numpy().reshape(nlev, len(tw["lines_y"]), len(tw["lines_x"]))
        for lev in range(nlev):
            for a, j in enumerate(tw["lines_y"]):
                for b, i in enumerate(tw["lines_x"]):
                    nobs.setdefault((lev, gj0 + j, gi0 + i), set()).add(int(ncn[lev, a, b]))
    assert (nhalo > 0) == (px * py > 1)          # the cuts of the 2 x 2 ranks are off the lattice: there are halo columns
    return anal, nobs


@pytest.mark.parametrize("sx,sy", [(2, 2), (3, 2)])
def test_ranks_with_their_own_tables_give_the_one_rank_analysis(sx, sy):
    from test_gpu_tiles import first_guess
    k = RANK_K
    x = first_guess(40 + k, 11, k, True, len(ZLEV), NLAT_G, NLON_G)
    a1, n1 = rank_analysis(1, 1, sx, sy, x)
    a2, n2 = rank_analysis(2, 2, sx, sy, x)
    # the same lattice, and every coarse point found with the same number of observations by every rank that solves it
    assert set(n2) == set(n1) and len(n1) == len(I.coarse_axis(NLON_G, sx)) * len(I.coarse_axis(NLAT_G, sy)) * len(ZLEV)
    assert n1 == n2 and all(len(v) == 1 for v in n2.values())
    assert np.mean([next(iter(v)) for v in n1.values()]) > 20
    members = list(range(k)) + [k + 1]
    assert np.isfinite(a2[:, members]).all()
    print("tiled == one rank bit for bit:", np.array_equal(a1[:, members], a2[:, members]))
    for v in range(x.shape[0]):
        scale = max(np.abs(x[v, k]).max(), np.abs(x[v, :k]).max())
        err = np.abs(a1[v, members] - a2[v, members]).max()
        print(f"v={v} err/scale={err / scale:.3e}")
        assert err <= 1e-10 * scale, (v, err, scale)
    assert np.abs(a1[0, :k] - (x[0, :k] + x[0, k:k + 1])).max() > 1e-3           # and the analysis did something
