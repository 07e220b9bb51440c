"""Numpy restatement of das_efso's loop (scale/letkf/letkf_tools.f90:1158-1302, commented out in the reference) for
SCALE's point layout, and the synthetic inputs the EFSO tests share.

    w_p(t, m)   = sum over v with term(v) = t of fcst[p, m, v] * fcer[p, v]                    ("work1")
    djdy[j, t] += sum over p with j in L_p of (rloc / rdiag)_{p,j} * sum_m ya[j, m] * w_p(t, m)
    obsense[j, t] = djdy[j, t] * dep[j]

djdy is [nobs][nterm] (the reference's djdy(nterm, nobstotal)); fcst [npts, k, nv], fcer [npts, nv], ya [nobs, k]."""
import numpy as np


def effective_terms(term_of_var, var_mask):
    te = np.array(term_of_var, dtype=np.int64)
    if var_mask:
        te = np.where([(var_mask >> v) & 1 for v in range(len(te))], te, -1)
    return te


def work1(fcst_p, fcer_p, te, nterm):
    """w_p [nterm, k]: variables in ascending order, as das_efso's loop over k = 1..nv3d"""
    w = np.zeros((nterm, fcst_p.shape[0]))
    for v, t in enumerate(te):
        if t >= 0:
            w[t] += fcst_p[:, v] * fcer_p[v]
    return w


def efso_loop(off, idx, rdiag, rloc, ya, fcst, fcer, term_of_var, nterm, var_mask=0, djdy=None):
    """Point by point, as das_efso: returns (djdy, scale) with scale[j, t] = sum of |terms| that entered djdy[j, t]."""
    te = effective_terms(term_of_var, var_mask)
    nobs = ya.shape[0]
    djdy = np.zeros((nobs, nterm)) if djdy is None else djdy.copy()
    scale = np.abs(djdy)
    for p in range(len(off) - 1):
        o0, o1 = off[p], off[p + 1]
        if o1 == o0:
            continue
        w = work1(fcst[p], fcer[p], te, nterm)
        j = idx[o0:o1]
        hr = ya[j] / rdiag[o0:o1, None] * rloc[o0:o1, None]          # hdxa_rinv: rho R^-1 Y^a
        np.add.at(djdy, j, hr @ w.T)
        np.add.at(scale, j, np.abs(hr) @ np.abs(w).T)
    return djdy, scale


def efso_dense(off, idx, rdiag, rloc, ya, fcst, fcer, term_of_var, nterm, var_mask=0):
    """The same as one matrix expression per term: djdy[:, t] = column sums of (rho o R^-1) o (W_t Y^a^T)."""
    te = effective_terms(term_of_var, var_mask)
    npts, nobs = len(off) - 1, ya.shape[0]
    rr = np.zeros((npts, nobs))
    pt = np.repeat(np.arange(npts), np.diff(off))
    rr[pt, idx] = rloc / rdiag
    out = np.zeros((nobs, nterm))
    for t in range(nterm):
        wt = np.einsum("pmv,pv->pm", fcst[:, :, te == t], fcer[:, te == t])
        out[:, t] = (rr * (wt @ ya.T)).sum(axis=0)
    return out


def inputs(rng, npts, k, nv, nobs):
    """fcst [npts, k, nv], fcer [npts, nv], ya [nobs, k], dep [nobs] of realistic magnitudes"""
    fcst = rng.standard_normal((npts, k, nv)) * rng.uniform(0.5, 2.0, nv)
    fcer = rng.standard_normal((npts, nv)) * 0.1
    ya = rng.standard_normal((nobs, k))
    dep = rng.standard_normal(nobs)
    return fcst, fcer, ya, dep


def ref_layout(fcst, fcer):
    """fcst3d(nij1*nlev, MEMBER, nv3d) / fcer3d(nij1*nlev, nv3d) flattened column-major: (p, m, v) at p + npts*m + npts*k*v"""
    npts, k, nv = fcst.shape
    return (np.ascontiguousarray(fcst.transpose(2, 1, 0)).ravel(), (1, npts, npts * k),
            np.ascontiguousarray(fcer.T).ravel(), (1, npts))


def within(got, exp, scale, tol=1e-12):
    """max of |got - exp| / sum|terms| over (j, t), rows with no terms compared exactly"""
    err = np.abs(got - exp)
    live = scale > 0
    assert np.all(err[~live] == 0), "an element without contributions changed"
    return float((err[live] / scale[live]).max()) if live.any() else 0.0
