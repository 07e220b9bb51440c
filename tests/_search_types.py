"""Search tables of any set of combined types on a 40 x 40 subdomain (make_case), and the six-type table that reaches every
branch of obs_local's per-type arithmetic (types_case): shared by tests/test_gpu_search_columns_fast.py and
tests/test_gpu_search_routes_types.py."""
import math

import numpy as np

from _search import DIST_ZERO_FAC

NLON = NLAT = 40
DX = 1000.0
I_ORG = J_ORG = 2.5


def make_case(types, groups, obs):
    """A _search.build_case-shaped dict for `types` = dict of per-type arrays (vmode, hori_loc, vert_loc, varloc) and
    obs[ic] = dict(ri, rj, lev, dat, err) in grid coordinates relative to the origin (mesh and ordering of
    letkf_obs.f90:655-976, as _search.build_case builds them)."""
    nctype = len(types["vmode"])
    hori_loc = np.asarray(types["hori_loc"], dtype=np.float64)
    ngrd_i, ngrd_j, nsch_i, nsch_j = (np.zeros(nctype, np.int32) for _ in range(4))
    for ic in range(nctype):
        spc = hori_loc[ic] * DIST_ZERO_FAC / 6.0
        ngrd_i[ic] = min(math.ceil(DX * NLON / spc), NLON)
        ngrd_j[ic] = min(math.ceil(DX * NLAT / spc), NLAT)
        nsch_i[ic] = math.ceil(hori_loc[ic] * DIST_ZERO_FAC / (DX * NLON / ngrd_i[ic]))
        nsch_j[ic] = math.ceil(hori_loc[ic] * DIST_ZERO_FAC / (DX * NLAT / ngrd_j[ic]))
    next_i, next_j = ngrd_i + 2 * nsch_i, ngrd_j + 2 * nsch_j
    cols = {k: [] for k in ("ri", "rj", "lev", "dat", "err")}
    ac_all, ac_off, rows = [], [], [0]
    for ic in range(nctype):
        o = {k: np.asarray(obs[ic][k], dtype=np.float64) for k in cols}
        n = o["ri"].size
        ri, rj = I_ORG + o["ri"], J_ORG + o["rj"]
        ogi = np.clip(np.ceil((ri - I_ORG) * ngrd_i[ic] / NLON).astype(np.int64) + nsch_i[ic], 1, next_i[ic])
        ogj = np.clip(np.ceil((rj - J_ORG) * ngrd_j[ic] / NLAT).astype(np.int64) + nsch_j[ic], 1, next_j[ic])
        order = np.lexsort((np.arange(n), ogi, ogj))
        cell = (ogj[order] - 1) * next_i[ic] + (ogi[order] - 1)
        cnt = np.bincount(cell, minlength=next_i[ic] * next_j[ic]).reshape(next_j[ic], next_i[ic])
        ac = np.zeros((next_j[ic], next_i[ic] + 1), dtype=np.int64)
        ac[:, 1:] = np.cumsum(cnt, axis=1)
        ac += rows[-1] + np.concatenate([[0], np.cumsum(cnt.sum(axis=1))[:-1]])[:, None]
        ac_off.append(sum(a.size for a in ac_all))
        ac_all.append(ac.reshape(-1).astype(np.int32))
        o["ri"], o["rj"] = ri, rj
        for k in cols:
            cols[k].append(o[k][order])
        rows.append(rows[-1] + n)
    arr = dict(group_start=np.cumsum([0] + [len(g) for g in groups]).astype(np.int32),
               group_member=np.array([ic for g in groups for ic in g], dtype=np.int32),
               vmode=np.asarray(types["vmode"], dtype=np.int32), hori_loc=hori_loc,
               vert_loc=np.asarray(types["vert_loc"], dtype=np.float64),
               varloc=np.asarray(types["varloc"], dtype=np.float64), max_nobs=np.zeros(nctype, np.int32),
               ngrd_i=ngrd_i, ngrd_j=ngrd_j, ngrdsch_i=nsch_i, ngrdsch_j=nsch_j, ngrdext_i=next_i.astype(np.int32),
               ngrdext_j=next_j.astype(np.int32), ac_off=np.array(ac_off, dtype=np.int64), ac_ext=np.concatenate(ac_all),
               ob_ri=np.concatenate(cols["ri"]), ob_rj=np.concatenate(cols["rj"]), ob_lev=np.concatenate(cols["lev"]),
               ob_dat=np.concatenate(cols["dat"]), ob_err=np.concatenate(cols["err"]))
    scal = dict(nctype=nctype, ngroup=len(groups), criterion=1, nlon=NLON, nlat=NLAT, dx=DX, dy=DX, i_org=I_ORG,
                j_org=J_ORG, rain_base=8.5e4)
    assert rows[-1] <= 4000
    return dict(arr=arr, scal=scal, ctype_rows=np.array(rows), nobs=rows[-1], groups=groups)


def types_case(rng, nobs, dense=None):
    """Six combined types: (0, 1) merged, height and ln(dat) localisation; 2 the rain-base mode; 3 without vertical
    localisation; 4 with varloc = 1e-300 (the counting pass must evaluate the weight); 5 with varloc < tiny (skipped).
    dense = (n, ci, cj, radius, lev_lo, lev_hi): n more rows of type 0 close together, within `radius` cells of (ci, cj)."""
    types = dict(vmode=[1, 2, 3, 0, 1, 1], hori_loc=[2500.0, 2000.0, 1500.0, 1800.0, 2200.0, 2500.0],
                 vert_loc=[2000.0, 0.3, 0.15, 0.0, 1500.0, 2000.0], varloc=[1.0, 0.7, 0.8, 0.5, 1e-300, 1e-310])
    obs = []
    for ic in range(6):
        n = nobs[ic]
        obs.append(dict(ri=rng.uniform(-3.0, NLON + 3.0, n), rj=rng.uniform(-3.0, NLAT + 3.0, n),
                        lev=rng.uniform(0.0, 12000.0, n), dat=rng.uniform(3.0e4, 1.03e5, n),
                        err=rng.choice([1.0, 3.0, 5.0], n)))
    if dense is not None:
        n, ci, cj, radius, lev_lo, lev_hi = dense
        rad, ang = radius * np.sqrt(rng.uniform(0.0, 1.0, n)), rng.uniform(0.0, 2.0 * np.pi, n)
        more = dict(ri=ci + rad * np.cos(ang), rj=cj + rad * np.sin(ang), lev=rng.uniform(lev_lo, lev_hi, n),
                    dat=rng.uniform(3.0e4, 1.03e5, n), err=rng.choice([1.0, 3.0, 5.0], n))
        obs[0] = {k: np.concatenate([obs[0][k], more[k]]) for k in more}
    return make_case(types, [[0, 1], [2], [3], [4], [5]], obs)
