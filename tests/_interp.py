"""Weight interpolation (include/letkf_amd_interp.h) stated without any of its code: a tile of nx x ny columns and nlev levels
with search tables (tests/_search.py build_case; observations in the merged radar group, which has a MAX_NOBS_PER_GRID, and in
upper-air T; none west of ri = i_org + 24, so the tile's west edge has points without any), the oracle's obs_local and
letkf_core at the coarse points, and the blend and the fine-point rules in numpy.  Pure numpy and the oracle."""
import functools

import numpy as np

import _oracle
from _search import build_case, host_struct, oracle_csr

LIMITS = (12, 12, 0, 0)


def coarse_axis(n, s):
    """{0, s, 2s, ...} united with {n - 1}"""
    idx = list(range(0, n, s))
    if idx[-1] != n - 1:
        idx.append(n - 1)
    return np.array(idx, dtype=np.int64)


@functools.lru_cache(maxsize=None)
def tile_case(k, nv=11, nx=7, ny=5, nlev=3, seed=5, dxs=5.5, dys=6.0):
    """columns dxs x dys grid lengths apart (build_case's domain is 40 x 32: a larger tile needs smaller spacings); with
    nv < 5 there is no pressure slot to fill, and no q_update_top for such a case"""
    rng = np.random.default_rng(seed + 1000 * k + nx)
    tc = build_case(seed, nlon=40, nlat=32, dx=1000.0, nobs_per_ctype=(180, 0, 120, 0), max_nobs=LIMITS, npts=1, obs_east_of=24.0)
    i_org, j_org = tc["scal"]["i_org"], tc["scal"]["j_org"]
    ii, jj = np.meshgrid(np.arange(nx), np.arange(ny), indexing="xy")          # column i + nx*j
    if nx > 1:
        rig = (i_org + 1.0 + dxs * ii).ravel() + rng.uniform(-0.2, 0.2, nx * ny)
    else:
        rig = np.full(nx * ny, i_org + 30.0) + rng.uniform(-0.2, 0.2, nx * ny)
    rjg = (j_org + 4.0 + dys * jj).ravel() + rng.uniform(-0.2, 0.2, nx * ny)
    nij1, npts = nx * ny, nx * ny * nlev
    zlev = np.linspace(500.0, 7000.0, nlev) if nlev > 1 else np.array([3000.0])
    rz = (zlev[:, None] + rng.uniform(-100.0, 100.0, (nlev, nij1))).ravel()
    rlev = 1.0e5 * np.exp(-rz / 7500.0)
    nobs, kld, nens = tc["nobs"], k + 1, k + 2
    ens = rng.standard_normal((nobs, kld))
    ens[:, :k] -= ens[:, :k].mean(axis=1, keepdims=True)
    dep = rng.standard_normal(nobs) * 1.5
    x = rng.standard_normal((nv, nens, npts))
    x[:, :k] *= np.array([2.0, 2.0, 2.0, 1.0, 50.0] + [1e-3] * max(nv - 5, 0))[:nv, None, None]
    x[:, :k] -= x[:, :k].mean(axis=1, keepdims=True)
    mean = rng.standard_normal((nv, npts)) * 5.0 + 50.0
    if nv > 5:
        mean[5:] = np.abs(mean[5:]) * 1e-3 + 1e-3
    if nv > 4:
        mean[4] = rlev
    x[:, k] = mean
    x[:, k + 1] = mean + rng.standard_normal((nv, npts)) * np.abs(x[:, 0]).max(axis=1, keepdims=True)
    infl = 1.07 * (1.0 + 0.05 * rng.uniform(size=npts * nv))
    h, keep = host_struct(tc)
    return dict(k=k, nv=nv, nx=nx, ny=ny, nlev=nlev, nij1=nij1, npts=npts, nens=nens, kld=kld, tc=tc, h=h, keep=keep,
                rig=rig, rjg=rjg, rlev=rlev, rz=rz, ensval=np.ascontiguousarray(ens), dep=dep, gues=np.ascontiguousarray(x),
                infl=infl, sp=1, sm=npts, sv=npts * nens)


def coarse_points(c, sx, sy):
    """(ix, iy, pts): fine point number of coarse point cx + ncx*cy + ncx*ncy*lev"""
    ix, iy = coarse_axis(c["nx"], sx), coarse_axis(c["ny"], sy)
    col = (ix[None, :] + c["nx"] * iy[:, None]).ravel()
    pts = (col[None, :] + c["nij1"] * np.arange(c["nlev"])[:, None]).ravel()
    return ix, iy, pts


_lists = {}


def coarse_lists(c, pts):
    """orc_obs_local at the given points, one search per point and case: {point: (idx, rdiag, rloc)}"""
    memo = _lists.setdefault(id(c), {})
    need = [int(p) for p in pts if int(p) not in memo]
    if need:
        q = np.array(need)
        col = q % c["nij1"]
        off, idx, rd, rl, tied = oracle_csr(c["h"], c["rig"][col], c["rjg"][col], c["rlev"][q], c["rz"][q])
        assert not tied.any()        # (a selection between equal keys: either choice would be the reference's)
        for n, p in enumerate(need):
            s = slice(off[n], off[n + 1])
            memo[p] = (idx[s].copy(), rd[s].copy(), rl[s].copy())
    return {int(p): memo[int(p)] for p in pts}


def solve_rho(c, cfg, p, mask):
    """solve_inflation (letkf_rules_dev.h): the slot of the first variable the point updates, 1 where it updates none"""
    k, nv, npts = c["k"], c["nv"], c["npts"]
    top = cfg.get("q_update_top", 0.0)
    qskip = top > 0.0 and c["gues"][4, k, p] < top
    for v in range(nv):
        if (mask >> v) & 1 and not (qskip and 5 <= v <= min(10, nv - 1)):
            return c["infl"][p + npts * v]
    return 1.0


_solves = {}


def coarse_solves(c, cfg, sx, sy, mask, ensval=None):
    """T, w-bar, w-bar_det of orc_letkf_core at the coarse points: {point: (T, wbar, wbard, n)}"""
    ix, iy, pts = coarse_points(c, sx, sy)
    lists = coarse_lists(c, pts)
    k = c["k"]
    det = bool(cfg.get("det_run", 0))
    ens = c["ensval"] if ensval is None else ensval
    out = {}
    for p in pts:
        p = int(p)
        idx, rd, rl = lists[p]
        n = len(idx)
        rho = solve_rho(c, cfg, p, mask)
        key = (id(c), p, float(rho), det) if ensval is None else None
        if key is not None and key in _solves:
            out[p] = _solves[key]
            continue
        n1 = max(n, 1)
        hd = np.zeros((n1, k))
        hd[:n] = ens[idx, :k]
        z = np.zeros(n1)
        pad = lambda a: np.concatenate([a, z[len(a):]])
        r = _oracle.letkf_core("oracle", k, n1, n, hd, pad(rd), pad(rl), pad(c["dep"][idx]), rho, want_transm=True, want_pao=False,
                               rdiag_wloc=True, infl_update=False, depd=pad(ens[idx, k]) if det else None,
                               want_transmd=det)
        res = (np.array(r["trans"]), r["transm"].copy(), r["transmd"].copy() if det else np.zeros(k), n)
        if key is not None:
            _solves[key] = res
        out[p] = res
    return out, (ix, iy, pts)


def corners_of(c, ix, iy, i, j, lev):
    """[(weight, coarse point)] of fine point (i, j, lev): the corners of non-zero weight"""
    ca = max(int(np.searchsorted(ix, i, side="right")) - 1, 0)
    cc = max(int(np.searchsorted(iy, j, side="right")) - 1, 0)
    a, b = int(ix[ca]), int(ix[min(ca + 1, len(ix) - 1)])
    cj, d = int(iy[cc]), int(iy[min(cc + 1, len(iy) - 1)])
    wx = (i - a) / (b - a) if b > a else 0.0
    wy = (j - cj) / (d - cj) if d > cj else 0.0
    out = []
    for w, (ci, cjj) in (((1.0 - wx) * (1.0 - wy), (a, cj)), (wx * (1.0 - wy), (b, cj)), ((1.0 - wx) * wy, (a, d)), (wx * wy, (b, d))):
        if w != 0.0:
            out.append((w, ci + c["nx"] * cjj + c["nij1"] * lev))
    return out


def expected(c, cfg, sx, sy, beta=None, mask=None):
    """The analysis of the interpolation route: anal (nv, nens, npts; NaN where nothing is written), rtps (nv, npts), n of the
    coarse points"""
    k, nv, nx, ny, nlev, npts = c["k"], c["nv"], c["nx"], c["ny"], c["nlev"], c["npts"]
    mask = (1 << nv) - 1 if not mask else mask
    sol, (ix, iy, pts) = coarse_solves(c, cfg, sx, sy, mask)
    x = c["gues"]
    anal = np.full_like(x, np.nan)
    rtps = np.full((nv, npts), np.nan)
    beta = np.ones(npts) if beta is None else beta
    alpha, spread = cfg.get("relax_alpha", 0.0), cfg.get("relax_alpha_spread", 0.0)
    top, qmax = cfg.get("q_update_top", 0.0), cfg.get("q_sprd_max", 0.0)
    rip = cfg.get("relax_to_inflated_prior", 0)
    qlast = min(10, nv - 1)
    km1 = k - 1.0
    det = bool(cfg.get("det_run", 0))
    for lev in range(nlev):
        for j in range(ny):
            for i in range(nx):
                p = i + nx * j + nx * ny * lev
                cw = corners_of(c, ix, iy, i, j, lev)
                T = sum(w * sol[q][0] for w, q in cw)
                wbar = sum(w * sol[q][1] for w, q in cw)
                wbard = sum(w * sol[q][2] for w, q in cw)
                qskip = top > 0.0 and x[4, k, p] < top
                b = beta[p]
                for v in range(nv):
                    if not (mask >> v) & 1:
                        continue
                    xp, xm, xd = x[v, :k, p], x[v, k, p], x[v, k + 1, p]
                    skipv = qskip and 5 <= v <= qlast
                    if b == 0.0 or skipv:
                        anal[v, :k, p] = xm + xp
                        anal[v, k + 1, p] = xd
                        rtps[v, p] = 1.0
                        continue
                    out = xp @ T                                  # anal(m) = sum_i x'(i) T(i, m)
                    parm = c["infl"][p + npts * v] if rip else 1.0
                    cf, cd = 1.0, 0.0
                    if alpha != 0.0:
                        cf, cd = 1.0 - alpha, alpha * np.sqrt(parm)
                    elif spread != 0.0:
                        var_g, var_a = xp @ xp, (out @ out) / km1
                        if var_g > 0.0 and var_a > 0.0:
                            cf = spread * np.sqrt(var_g * parm / (var_a * km1)) - spread + 1.0
                    val = xm + b * (cf * out + cd * xp + xp @ wbar) + (1.0 - b) * xp
                    if qmax > 0.0 and not qskip and v == 5:
                        q_mean = val.mean()
                        dq = val - q_mean
                        q_sprd = np.sqrt((dq @ dq) / km1) / q_mean
                        if q_sprd > qmax:
                            val = q_mean + dq * qmax / q_sprd
                    anal[v, :k, p] = val
                    anal[v, k + 1, p] = xd + (xp @ wbard) * b
                    rtps[v, p] = cf if (alpha == 0.0 and spread != 0.0) else 1.0
    if not det:
        anal[:, k + 1] = np.nan
    ncoarse = np.array([sol[int(p)][3] for p in pts], dtype=np.int32)
    return dict(anal=anal, rtps=rtps, ncoarse=ncoarse, ix=ix, iy=iy, pts=pts)
