"""das_letkf_obs (scale/letkf/letkf_tools.f90:933-1156) restated twice for the tests, on the synthetic tables of
tests/_search.py:
  (a) formula()  the reference's formula in numpy: T, w-bar (and Pa, the det weights) from _oracle.letkf_core (the compiled
                 reference where it was built, else the C restatement) on the oracle's obs_local lists at the targets'
                 coordinates, then RTPP / RTPS, beta and the q rules of the loop body (:457-513)
  (b) composed() the oracle's loop body orc_das_letkf_points on the two-variable pseudo-state: variable 0 the target
                 (members ensval, mean ob_dat - dep, det ob_dat - ensval[k]), variable 1 its pressure (Q_UPDATE_TOP)
Both return dict(ya [ntgt, k (+1)], mean [ntgt], table rows [ntgt, k (+1)], dep_a [ntgt], nobs [ntgt])."""
import numpy as np

import _oracle
from _search import host_struct, oracle_csr


def ctype_of_rows(case, rows):
    return np.searchsorted(case["ctype_rows"], rows, side="right") - 1


def interior_rows(case, ctypes):
    """rows of the given ctypes whose location lies inside the subdomain (the targets a rank takes, ObsTable.target_groups:
    the extended mesh then covers their whole cut-off, as obs_local requires)"""
    a, s = case["arr"], case["scal"]
    cr = case["ctype_rows"]
    rows = np.concatenate([np.arange(cr[c], cr[c + 1]) for c in ctypes]).astype(np.int64)
    di, dj = a["ob_ri"][rows] - s["i_org"], a["ob_rj"][rows] - s["j_org"]
    return rows[(di > 0.0) & (di <= s["nlon"]) & (dj > 0.0) & (dj <= s["nlat"])]


def coords(case, rows, rlev_tgt=None, rz_tgt=None):
    """(ri, rj, rlev, rz) of the targets: the vertical coordinate by the ctype's vmode, the other one from the caller"""
    a, s = case["arr"], case["scal"]
    vm = a["vmode"][ctype_of_rows(case, rows)]
    n = len(rows)
    rlev = np.array(rlev_tgt, dtype=np.float64) if rlev_tgt is not None else np.zeros(n)
    rz = np.array(rz_tgt, dtype=np.float64) if rz_tgt is not None else np.zeros(n)
    rlev = np.where(vm == 0, a["ob_lev"][rows], np.where(vm == 2, a["ob_dat"][rows], np.where(vm == 3, s["rain_base"], rlev)))
    rz = np.where(vm == 1, a["ob_lev"][rows], rz)
    return a["ob_ri"][rows], a["ob_rj"][rows], rlev, rz


def lists(case, rows, rlev_tgt=None, rz_tgt=None):
    h, keep = host_struct(case)
    ri, rj, rlev, rz = coords(case, rows, rlev_tgt, rz_tgt)
    off, idx, rd, rl, tied = oracle_csr(h, ri, rj, rlev, rz)
    return off, idx, rd, rl, rlev


def _q(p):
    tvar, qf, ql = p["tvar"], p.get("iv_q_first", 5), p.get("iv_q_last", 10)
    qtop = tvar >= 0 and qf <= tvar <= ql and p.get("q_update_top", 0.0) > 0
    qsprd = tvar >= 0 and tvar == qf and p.get("q_sprd_max", 0.0) > 0
    return qtop, qsprd


def _finish(case, rows, ya, k, det, nobs):
    dat = case["arr"]["ob_dat"][rows]
    mean = ya[:, :k].sum(axis=1) / k
    tab = ya[:, :k] - mean[:, None]
    if det:
        tab = np.concatenate([tab, (dat - ya[:, k])[:, None]], axis=1)
    return dict(ya=ya, mean=mean, table=tab, dep_a=dat - mean, nobs=nobs)


def formula(case, rows, ensval, dep, p, infl, beta=None, lst=None, which=None):
    """(a).  p: dict(k, tvar, det_run, relax_alpha, relax_alpha_spread, relax_to_inflated_prior, q_update_top, q_sprd_max,
    iv_q_first, iv_q_last); infl [ntgt]; beta [ntgt] or None."""
    k, det = p["k"], bool(p.get("det_run", False))
    which = which or ("ref" if _oracle.ref() is not None else "oracle")
    off, idx, rd, rl, rlev = lst if lst is not None else lists(case, rows)
    qtop, qsprd = _q(p)
    dat = case["arr"]["ob_dat"][rows]
    ya = np.zeros((len(rows), k + (1 if det else 0)))
    for t, j in enumerate(rows):
        x = ensval[j, :k]
        mean = dat[t] - dep[j]
        xdet = dat[t] - ensval[j, k] if det else 0.0
        b = 1.0 if beta is None else beta[t]
        rho = infl[t]
        if b == 0.0 or (qtop and rlev[t] < p["q_update_top"]):
            ya[t, :k] = mean + x
            if det:
                ya[t, k] = xdet
            continue
        e0, e1 = off[t], off[t + 1]
        n = int(e1 - e0)
        ii = idx[e0:e1]
        hdxb = np.zeros((max(n, 1), k))
        hdxb[:n] = ensval[ii, :k]
        pad = lambda v: np.concatenate([v, np.zeros(max(n, 1) - n)])
        c = _oracle.letkf_core(which, k, max(n, 1), n, hdxb, pad(rd[e0:e1]), pad(rl[e0:e1]), pad(dep[ii]), rho,
                               want_transm=True, want_pao=True, rdiag_wloc=True, infl_update=False,
                               depd=pad(ensval[ii, k]) if det else None, want_transmd=det)
        T = c["trans"]
        parm = rho if p.get("relax_to_inflated_prior", False) else 1.0
        if p.get("relax_alpha", 0.0) != 0.0:
            a = p["relax_alpha"]
            W = (1.0 - a) * T + a * np.sqrt(parm) * np.eye(k)
        elif p.get("relax_alpha_spread", 0.0) != 0.0:
            a = p["relax_alpha_spread"]
            var_g, var_a = x @ x, x @ c["pao"] @ x
            W = T * (a * np.sqrt(var_g * parm / (var_a * (k - 1))) - a + 1.0) if var_g > 0 and var_a > 0 else T
        else:
            W = T
        tot = (W + c["transm"][:, None]) * b + (1.0 - b) * np.eye(k)
        ya[t, :k] = mean + x @ tot
        if det:
            ya[t, k] = xdet + b * (x @ c["transmd"])
        if qsprd:
            qm = ya[t, :k].sum() / k
            qa = ya[t, :k] - qm
            qs = np.sqrt((qa @ qa) / (k - 1)) / qm
            if qs > p["q_sprd_max"]:
                ya[t, :k] = qm + qa * p["q_sprd_max"] / qs
    return _finish(case, rows, ya, k, det, np.diff(off))


def pseudo_state(case, rows, ensval, dep, k, det, rlev):
    """gues [2][k + 2][ntgt] flat (sp = 1, sm = ntgt, sv = ntgt (k + 2))"""
    n = len(rows)
    g = np.zeros((2, k + 2, n))
    dat = case["arr"]["ob_dat"][rows]
    g[0, :k] = ensval[rows, :k].T
    g[0, k] = dat - dep[rows]
    g[0, k + 1] = dat - ensval[rows, k] if det else 0.0
    g[1, k] = rlev
    g[1, k + 1] = rlev
    return g.ravel()


def composed(case, rows, ensval, dep, p, infl, beta=None, lst=None):
    """(b)"""
    k, det = p["k"], bool(p.get("det_run", False))
    off, idx, rd, rl, rlev = lst if lst is not None else lists(case, rows)
    qtop, qsprd = _q(p)
    tv = p["tvar"]
    qvar = tv >= 0 and p.get("iv_q_first", 5) <= tv <= p.get("iv_q_last", 10)
    n = len(rows)
    prm = _oracle.DasParams(k=k, nv=2, det_run=int(det), infl_adaptive=0,
                            relax_to_inflated_prior=int(bool(p.get("relax_to_inflated_prior", False))),
                            relax_alpha=p.get("relax_alpha", 0.0), relax_alpha_spread=p.get("relax_alpha_spread", 0.0),
                            q_update_top=p["q_update_top"] if qtop else 0.0, q_sprd_max=p["q_sprd_max"] if qsprd else 0.0,
                            iv_p=1, iv_q_first=0 if qvar else 2, iv_q_last=0 if qvar else 1, nthreads=1, var_mask=1)
    g = pseudo_state(case, rows, ensval, dep, k, det, rlev)
    r = _oracle.das_points(prm, off, idx, rd, rl, np.ascontiguousarray(ensval), dep,
                           None if beta is None else np.ascontiguousarray(beta, dtype=np.float64),
                           np.concatenate([infl, infl]), g, 1, n, n * (k + 2))
    assert r["rc"] == 0, r["rc"]
    an = r["anal"].reshape(2, k + 2, n)
    ya = an[0, :k].T.copy()
    if det:
        ya = np.concatenate([ya, an[0, k + 1][:, None]], axis=1)
    return _finish(case, rows, ya, k, det, np.diff(off))


def temperatures(case, seed=0):
    """ob_dat of the rows whose ctype does not read it for the vertical coordinate (vmode 0, 1) set to values of the size of
    a temperature, so that the analysis is judged at the size of its increments (ps rows keep their pressure)"""
    vm = case["arr"]["vmode"][ctype_of_rows(case, np.arange(case["nobs"]))]
    t = np.random.default_rng(seed).uniform(250.0, 300.0, case["nobs"])
    case["arr"]["ob_dat"] = np.where((vm == 0) | (vm == 1), t, case["arr"]["ob_dat"])
    return case


def table(case, k, kld, seed, spread=2.0):
    """obsda_sort's ensval [nobs, kld] (members: zero-mean perturbations; column k the det departure) and dep"""
    rng = np.random.default_rng(seed)
    nobs = case["nobs"]
    x = rng.standard_normal((nobs, k)) * spread
    x -= x.mean(axis=1, keepdims=True)
    ev = np.full((nobs, kld), np.nan)
    ev[:, :k] = x
    if kld > k:
        ev[:, k] = rng.standard_normal(nobs) * 1.5
    dep = rng.standard_normal(nobs) * 2.0
    return ev, dep


def relerr(got, exp, ref_level=None):
    """max-norm relative error; ref_level (e.g. ob_dat) is taken off both sides first, so that values near 1e5 are judged
    by their increments and spread, not by their size"""
    g, e = np.asarray(got, dtype=np.float64), np.asarray(exp, dtype=np.float64)
    if ref_level is not None:
        g, e = g - ref_level, e - ref_level
    s = np.abs(e).max()
    return float(np.abs(g - e).max() / (s if s > 0 else 1.0))
