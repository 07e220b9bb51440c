"""EFSO with localisation advection on the device (include/letkf_amd.h section 12): letkf_efso_locadv_dev against the numpy
restatement tests/_efso_locadv.py bit for bit; letkf_efso_search_dev bit for bit against letkf_obs_search_dev +
letkf_efso_points_dev at any list_bytes, within 1e-12 of tests/_efso.py on the oracle's obs_local lists at the advected
positions, bit for bit against letkf_efso_columns_dev where nothing moves; points advected out of the domain, argument
faults."""
import numpy as np
import pytest
import torch

import _efso
import _efso_locadv as la
from _search import build_case, device_struct, host_struct, oracle_csr

pytestmark = pytest.mark.gpu

DX = 1000.0


def _ctx():
    from _gpu import ctx
    return ctx()


def _d(a, dt=None):
    from _gpu import dev
    return dev(a, dt)


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def column_case(seed, nij1, nlev, max_nobs=(0, 0, 0, 0)):
    case = build_case(seed, npts=nij1, max_nobs=max_nobs)
    rng = np.random.default_rng(seed + 1000)
    rlev = rng.uniform(2.5e4, 1.0e5, nij1 * nlev)
    rz = rng.uniform(0.0, 12000.0, nij1 * nlev)
    return case, rlev, rz


def locadv(rig, rjg, nlev, u0, v0, u1, v1, rate, eft, dx=DX, dy=DX):
    ri, rj = _ctx().efso_locadv(_d(rig), _d(rjg), nlev, _d(u0), _d(v0), _d(u1), _d(v1), rate, eft, dx, dy)
    torch.cuda.synchronize()
    return ri.cpu().numpy(), rj.cpu().numpy()


def efso_inputs(k, nterm, term, npts, nobs, seed, kld=None):
    fcst, fcer, ya, _ = _efso.inputs(np.random.default_rng(seed), npts, k, len(term), nobs)
    kld = kld or k
    tab = np.full((nobs, kld), np.nan)
    tab[:, :k] = ya
    return fcst, fcer, ya, tab


def run_search(t, k, nterm, term, ri, rj, rlev, rz, tab, nobs, fcst, fcer, djdy0, var_mask=0, list_bytes=0):
    f, fs, e, es = _efso.ref_layout(fcst, fcer)
    dj = _d(np.ascontiguousarray(djdy0).ravel())
    _ctx().efso_search(k, len(term), term, nterm, t, _d(ri), _d(rj), _d(rlev), _d(rz), _d(tab.ravel()), tab.shape[1], nobs,
                       _d(f), *fs, _d(e), *es, dj, var_mask=var_mask, list_bytes=list_bytes)
    torch.cuda.synchronize()
    return dj.cpu().numpy().reshape(nobs, nterm)


def run_points(k, nterm, term, off, idx, rd, rl, tab, nobs, fcst, fcer, djdy0, var_mask=0):
    f, fs, e, es = _efso.ref_layout(fcst, fcer)
    dj = _d(np.ascontiguousarray(djdy0).ravel())
    _ctx().efso_points(k, len(term), term, nterm, off, idx, rd, rl, _d(tab.ravel()), tab.shape[1], nobs, _d(f), *fs, _d(e),
                       *es, dj, var_mask=var_mask)
    torch.cuda.synchronize()
    return dj.cpu().numpy().reshape(nobs, nterm)


# ---- letkf_efso_locadv_dev

@pytest.mark.parametrize("rate,eft,dy", [(0.5, 1.0, DX), (0.0, 6.0, DX), (-0.7, 3.0, 1500.0), (1.3, 0.25, 800.0)])
def test_locadv_bitwise_against_numpy(rate, eft, dy):
    rng = np.random.default_rng(3)
    nij1, nlev = 257, 13
    rig, rjg = rng.uniform(3.0, 240.0, nij1), rng.uniform(3.0, 240.0, nij1)
    u0, v0, u1, v1 = la.shear_winds(rng, nij1, nlev, u_bot=-25.0, u_top=35.0, v=-8.0, noise=6.0)   # winds of both signs
    assert (u0 < 0).any() and (u0 > 0).any() and (v1 < 0).any()
    ri, rj = locadv(rig, rjg, nlev, u0, v0, u1, v1, rate, eft, DX, dy)
    ei, ej = la.advect(rig, rjg, u0, v0, u1, v1, rate, eft, DX, dy)
    assert np.array_equal(_bits(ri), _bits(ei)) and np.array_equal(_bits(rj), _bits(ej))
    if rate == 0.0:
        assert np.array_equal(ri, np.tile(rig, nlev)) and np.array_equal(rj, np.tile(rjg, nlev))
    assert "efso_locadv_kernel" in _ctx().last_path()


def test_locadv_rejects_nan_wind_and_far_displacement():
    from _gpu import pkg
    rng = np.random.default_rng(4)
    nij1, nlev = 50, 4
    rig, rjg = rng.uniform(3.0, 40.0, nij1), rng.uniform(3.0, 30.0, nij1)
    winds = la.shear_winds(rng, nij1, nlev)
    ri, rj = locadv(rig, rjg, nlev, *winds, 0.5, 1.0)
    assert not la.bad_points(rig, rjg, ri, rj).any()
    for which, val in ((0, np.nan), (3, np.inf), (2, 3.0e6)):     # 3e6 m/s over 1 h at 1 km: 2.7e6 cells in i
        w = [x.copy() for x in winds]
        w[which][77] = val
        with pytest.raises(pkg.LetkfError, match="error -1"):
            locadv(rig, rjg, nlev, *w, 0.5, 1.0)
    # just inside the bound passes, just past it fails (2^20 cells = 0.5 * (u0 + u1) * 1800 m / 1000 m)
    w = [x.copy() for x in winds]
    w[0][5] = w[2][5] = 2.0 ** 20 / 1.8 * 0.999
    ri, rj = locadv(rig, rjg, nlev, *w, 0.5, 1.0)
    assert abs(ri[5] - rig[5]) < 2.0 ** 20
    w[0][5] = w[2][5] = 2.0 ** 20 / 1.8 * 1.001
    with pytest.raises(pkg.LetkfError, match="error -1"):
        locadv(rig, rjg, nlev, *w, 0.5, 1.0)


def test_locadv_invalid_arguments():
    from _gpu import pkg
    c = _ctx()
    z = _d(np.zeros(20))
    r = _d(np.ones(5))
    with pytest.raises(pkg.LetkfError, match="error -1"):
        c.efso_locadv(r, r, 4, z, None, z, z, 0.5, 1.0, DX, DX)
    with pytest.raises(pkg.LetkfError, match="error -1"):
        c.efso_locadv(r, r, 4, z, z, z, z, 0.5, 1.0, 0.0, DX)
    with pytest.raises(pkg.LetkfError, match="error -1"):
        c.efso_locadv(r, r, 4, z, z, z, z, np.nan, 1.0, DX, DX)
    with pytest.raises(pkg.LetkfError, match="error -1"):
        c.efso_locadv(r, r, 0, z, z, z, z, 0.5, 1.0, DX, DX)


# ---- letkf_efso_search_dev

@pytest.mark.parametrize("max_nobs", [(0, 0, 0, 0), (25, 25, 10, 5)])
def test_search_equals_obs_search_plus_points_at_any_list_bytes(max_nobs):
    """the route's bits are those of letkf_obs_search_dev + letkf_efso_points_dev on the same positions, for one run, a few
    runs and a run per point, and again on a repeated call"""
    nij1, nlev = 70, 5
    case, rlev, rz = column_case(21, nij1, nlev, max_nobs)
    t, keep = device_struct(case, "cuda")
    p = case["pts"]
    rng = np.random.default_rng(22)
    ri, rj = locadv(p["ri"], p["rj"], nlev, *la.shear_winds(rng, nij1, nlev), 0.5, 0.1)
    nobs, npts = case["nobs"], nij1 * nlev
    k, nterm, term = 20, 3, [0, 0, 1, 2, -1, 1]
    fcst, fcer, ya, tab = efso_inputs(k, nterm, term, npts, nobs, 23)
    c = _ctx()
    off, idx, rd, rl = c.obs_search(t, _d(ri), _d(rj), _d(rlev), _d(rz))
    z = np.zeros((nobs, nterm))
    ref = run_points(k, nterm, term, off, idx, rd, rl, tab, nobs, fcst, fcer, z)
    nnz = int(off[-1])
    assert nnz > 10 * npts
    per_entry = 20 + 8 * nterm + 20
    for lb in (0, nnz * per_entry // 7, 1, 0):
        got = run_search(t, k, nterm, term, ri, rj, rlev, rz, tab, nobs, fcst, fcer, z, list_bytes=lb)
        assert np.array_equal(_bits(got), _bits(ref)), lb
    assert "efso_pairs_kernel<3>" in c.last_path()
    assert ("radix select" in c.last_path()) == any(max_nobs)
    exp, scale = _efso.efso_loop(off.cpu().numpy(), idx.cpu().numpy(), rd.cpu().numpy(), rl.cpu().numpy(), ya, fcst, fcer,
                                 term, nterm)
    assert _efso.within(ref, exp, scale) < 1e-12


_ORACLE = {}


def advected_oracle_case():
    """one case for the k sweep: the columns advected by a shear of ~1.8 .. 5.4 cells, and the ORACLE's lists there"""
    if not _ORACLE:
        nij1, nlev = 60, 4
        case, rlev, rz = column_case(31, nij1, nlev)
        p, sc = case["pts"], case["scal"]
        rng = np.random.default_rng(32)
        # columns far enough from the west and south edges that every advected position stays inside the domain (the
        # oracle's obs_local reads the mesh at the search window as the reference does, without a clamp)
        p["ri"] = sc["i_org"] + rng.uniform(9.0, sc["nlon"] - 0.5, nij1)
        p["rj"] = sc["j_org"] + rng.uniform(3.0, sc["nlat"] - 0.5, nij1)
        winds = la.shear_winds(rng, nij1, nlev, noise=1.0)
        ri, rj = locadv(p["ri"], p["rj"], nlev, *winds, 0.5, 0.1)
        ei, ej = la.advect(p["ri"], p["rj"], *winds, 0.5, 0.1, DX, DX)
        assert np.array_equal(_bits(ri), _bits(ei)) and np.array_equal(_bits(rj), _bits(ej))
        assert (ri > sc["i_org"] + 0.5).all() and (ri < sc["i_org"] + sc["nlon"] - 0.5).all()
        assert (rj > sc["j_org"] + 0.5).all() and (rj < sc["j_org"] + sc["nlat"] - 0.5).all()
        moved = np.abs(ri - np.tile(p["ri"], nlev)).reshape(nlev, nij1).mean(axis=1)
        assert moved[0] > 1.0 and moved[-1] > 2.5 * moved[0]           # the levels move by different amounts
        h, keep = host_struct(case)
        off, idx, rd, rl, _ = oracle_csr(h, ri, rj, rlev, rz)
        _ORACLE.update(case=case, ri=ri, rj=rj, rlev=rlev, rz=rz, off=off, idx=idx, rd=rd, rl=rl)
    return _ORACLE


@pytest.mark.parametrize("k,nterm,term", [(3, 1, [0, -1, 0, 0, -1]), (20, 2, [1, 0, -1, 1, 0]), (50, 3, [2, -1, 1, 0, 0, 1]),
                                          (100, 4, [3, 2, 1, 0, -1, 3, 2]), (320, 3, [0, 1, 2, 0, 1, 2, -1])])
def test_advected_against_numpy_on_oracle_lists(k, nterm, term):
    """two variable classes accumulate into one djdy; the second class's localisation is its own varloc in the tables"""
    o = advected_oracle_case()
    case = o["case"]
    nobs = case["nobs"]
    npts = len(o["ri"])
    fcst, fcer, ya, tab = efso_inputs(k, nterm, term, npts, nobs, 40 + k, kld=k + 3)
    m1 = sum(1 << v for v in range(0, len(term), 2))
    m2 = sum(1 << v for v in range(1, len(term), 2))
    exp, s1 = _efso.efso_loop(o["off"], o["idx"], o["rd"], o["rl"], ya, fcst, fcer, term, nterm, var_mask=m1)
    exp, _ = _efso.efso_loop(o["off"], o["idx"], o["rd"], o["rl"], ya, fcst, fcer, term, nterm, var_mask=m2, djdy=exp)
    s2 = _efso.efso_loop(o["off"], o["idx"], o["rd"], o["rl"], ya, fcst, fcer, term, nterm, var_mask=m2)[1]
    t, keep = device_struct(case, "cuda")
    got = run_search(t, k, nterm, term, o["ri"], o["rj"], o["rlev"], o["rz"], tab, nobs, fcst, fcer, np.zeros((nobs, nterm)),
                     var_mask=m1)
    got = run_search(t, k, nterm, term, o["ri"], o["rj"], o["rlev"], o["rz"], tab, nobs, fcst, fcer, got, var_mask=m2)
    assert np.abs(exp).max() > 0
    assert _efso.within(got, exp, s1 + s2) < 1e-12
    assert np.isfinite(got).all()


@pytest.mark.parametrize("max_nobs", [(0, 0, 0, 0), (25, 25, 10, 5)])
def test_zero_displacement_equals_the_column_route(max_nobs):
    """rate 0: every point at its column's position.  No limit: the bits of letkf_efso_columns_dev; with limits (a
    different selection route) within 1e-12"""
    nij1, nlev = 80, 6
    case, rlev, rz = column_case(51, nij1, nlev, max_nobs)
    t, keep = device_struct(case, "cuda")
    p = case["pts"]
    ri, rj = locadv(p["ri"], p["rj"], nlev, *la.shear_winds(np.random.default_rng(52), nij1, nlev), 0.0, 1.0)
    assert np.array_equal(ri, np.tile(p["ri"], nlev))
    nobs, npts = case["nobs"], nij1 * nlev
    k, nterm, term = 16, 3, [0, 1, 2, 0, -1, 1]
    fcst, fcer, ya, tab = efso_inputs(k, nterm, term, npts, nobs, 53)
    z = np.zeros((nobs, nterm))
    got = run_search(t, k, nterm, term, ri, rj, rlev, rz, tab, nobs, fcst, fcer, z, list_bytes=npts * 400)
    f, fs, e, es = _efso.ref_layout(fcst, fcer)
    dj = torch.zeros(nobs * nterm, dtype=torch.float64, device="cuda")
    _ctx().efso_columns(k, len(term), term, nterm, t, nij1, nlev, _d(p["ri"]), _d(p["rj"]), _d(rlev), _d(rz),
                        _d(tab.ravel()), k, nobs, _d(f), *fs, _d(e), *es, dj)
    torch.cuda.synchronize()
    col = dj.cpu().numpy().reshape(nobs, nterm)
    if not any(max_nobs):
        assert np.array_equal(_bits(got), _bits(col))
    else:
        off, idx, rd, rl = (x.cpu().numpy() for x in _ctx().obs_search(t, _d(ri), _d(rj), _d(rlev), _d(rz)))
        _, scale = _efso.efso_loop(off, idx, rd, rl, ya, fcst, fcer, term, nterm)
        assert _efso.within(got, col, scale) < 1e-12


def test_points_advected_out_of_the_domain_and_unreached_rows():
    """a third of the columns blown 300 cells east, the others calm: the moved points find no observation and add
    nothing; rows no point reaches keep their prefilled bits.  (The oracle's obs_local reads the mesh at the search
    window without a clamp, as the reference does: it is asked about the points inside the domain only, the moved ones
    have empty lists by construction.)"""
    nij1, nlev = 60, 3
    case, rlev, rz = column_case(61, nij1, nlev)
    t, keep = device_struct(case, "cuda")
    p = case["pts"]
    u0, v0, u1, v1 = (np.zeros(nij1 * nlev) for _ in range(4))
    out = np.tile(np.arange(nij1) % 3 == 0, nlev)
    u0[out] = u1[out] = -300.0 / 0.18               # 0.5 * (u0 + u1) * c_i = -300 cells: 300 cells east
    ri, rj = locadv(p["ri"], p["rj"], nlev, u0, v0, u1, v1, 0.5, 0.1)
    assert (ri[out] > 300.0).all()
    nobs, npts = case["nobs"], nij1 * nlev
    c = _ctx()
    off = c.obs_search(t, _d(ri), _d(rj), _d(rlev), _d(rz))[0].cpu().numpy()
    cnt = np.diff(off)
    assert (cnt[out] == 0).all() and (cnt[~out] > 0).all()
    k, nterm, term = 12, 2, [0, 1, 1, 0, -1]
    fcst, fcer, ya, tab = efso_inputs(k, nterm, term, npts, nobs, 63)
    prefill = np.random.default_rng(64).standard_normal((nobs, nterm))
    got = run_search(t, k, nterm, term, ri, rj, rlev, rz, tab, nobs, fcst, fcer, prefill, list_bytes=1)
    h, hk = host_struct(case)
    i_off, o_idx, o_rd, o_rl, _ = oracle_csr(h, ri[~out], rj[~out], rlev[~out], rz[~out])
    o_cnt = np.zeros(npts, np.int64)
    o_cnt[~out] = np.diff(i_off)
    o_off = np.concatenate([[0], np.cumsum(o_cnt)])
    exp, scale = _efso.efso_loop(o_off, o_idx, o_rd, o_rl, ya, fcst, fcer, term, nterm, djdy=prefill)
    assert _efso.within(got, exp, scale) < 1e-12
    unreached = np.setdiff1d(np.arange(nobs), o_idx)
    assert len(unreached) > 20
    assert np.array_equal(_bits(got[unreached]), _bits(prefill[unreached]))


def test_search_invalid_arguments():
    from _gpu import pkg
    nij1, nlev = 30, 2
    case, rlev, rz = column_case(71, nij1, nlev)
    t, keep = device_struct(case, "cuda")
    p = case["pts"]
    nobs, npts = case["nobs"], nij1 * nlev
    ri, rj = _d(np.tile(p["ri"], nlev)), _d(np.tile(p["rj"], nlev))
    k, term = 8, [0, 1, 2]
    fcst, fcer, ya, tab = efso_inputs(k, 3, term, npts, nobs, 72)
    f, fs, e, es = _efso.ref_layout(fcst, fcer)
    g = dict(f=_d(f), e=_d(e), tab=_d(tab.ravel()), rlev=_d(rlev), rz=_d(rz))
    dj = torch.zeros(nobs * 4, dtype=torch.float64, device="cuda")

    def call(nterm=3, ri_=ri, rj_=rj, rlev_=g["rlev"], rz_=g["rz"], npts_=None):
        _ctx().efso_search(k, len(term), term, nterm, t, ri_, rj_, rlev_, rz_, g["tab"], k, nobs, g["f"], *fs, g["e"], *es,
                           dj, npts=npts_)

    for bad in (dict(ri_=None, npts_=npts), dict(rj_=None), dict(rlev_=None), dict(rz_=None), dict(npts_=npts - 1), dict(npts_=-1),
                dict(nterm=0), dict(nterm=5)):
        with pytest.raises(pkg.LetkfError, match="error -1"):
            call(**bad)
    torch.cuda.synchronize()
    assert float(dj.abs().max()) == 0.0
    call()                                            # the same arguments without the fault run
    torch.cuda.synchronize()
    assert float(dj.abs().max()) > 0.0
