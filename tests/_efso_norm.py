"""Numpy restatement of EFSO's two ends (include/letkf_amd.h section 13) and literal transcriptions of the reference's loops.

norm():      the fcer assembly of scale/letkf/efso.f90:100-117 and lnorm (scale/letkf/efso_tools.f90:52-156) in SCALE's
             frame, in the library's operation order, one IEEE operation at a time (as the device runs without fused
             multiply-adds), so the two agree bit for bit wherever the device's / and sqrt are correctly rounded.
lnorm_loops(): lnorm's loops as the reference writes them (member, level and variable loops, its IF / ELSE IF chain and
             its zeroing afterwards), given dp/ps -- the check that norm() is lnorm.
summary():   print_obsense's table (efso_tools.f90:232-253) by sorting; summary_loops() its loop row by row.

fcst is [npts, k, nv] (p = ij + nij1*lev), fcer [npts, nv]."""
import numpy as np

# SCALE's CONST_CPdry, CONST_LHV0 and lnorm's tref
CP, TREF, HVAP = 1004.64, 280.0, 2.501e6


def half_levels(pbar):
    """pbar [nlev, nij1] -> (dp [nlev, nij1], ps [nij1], p_top [nij1]) by the header's half-level rule (levels bottom first)"""
    nlev = pbar.shape[0]
    ph = np.empty((nlev + 1, pbar.shape[1]))
    ph[0] = pbar[0] + 0.5 * (pbar[0] - pbar[1])
    ph[1:nlev] = 0.5 * (pbar[:-1] + pbar[1:])
    ph[nlev] = np.maximum(0.0, pbar[nlev - 1] - 0.5 * (pbar[nlev - 2] - pbar[nlev - 1]))
    return ph[:-1] - ph[1:], ph[0], ph[nlev]


def dp_over_ps(pbar):
    """[nlev, nij1] dp/ps, and the columns the library rejects (dp <= 0, ps <= 0 or not finite)"""
    nlev = pbar.shape[0]
    if nlev == 1:
        return np.ones_like(pbar), np.zeros(pbar.shape[1], bool)
    dp, ps, _ = half_levels(pbar)
    with np.errstate(all="ignore"):
        r = dp / ps
        ok = (ps > 0) & np.isfinite(ps) & np.all((dp > 0) & np.isfinite(r), axis=0)
    return r, ~ok


def classes(nv, iv_u, iv_v, iv_t, iv_q):
    return np.array([1 if v in (iv_u, iv_v) else 2 if v == iv_t else 3 if v == iv_q else 0 for v in range(nv)])


def factors(sw, cls, cp=CP, tref=TREF, hvap=HVAP, wmoist=1.0):
    """[npts, nv]: the factor of every point and variable (lnorm's cptr * sigweight, qweight * sigweight)"""
    cptr = np.sqrt(cp / tref)
    qweight = np.sqrt(wmoist / (cp * tref)) * hvap
    f = np.zeros((sw.size, len(cls)))
    for v, c in enumerate(cls):
        f[:, v] = 0.0 if c == 0 else sw if c == 1 else cptr * sw if c == 2 else qweight * sw
    return f


def region(nij1, nlev, tar_minlev, tar_maxlev, lon=None, lat=None, box=(0.0, 360.0, -90.0, 90.0)):
    """[npts] bool: the target region"""
    lev = np.arange(nij1 * nlev) // nij1 + 1
    inr = (lev >= tar_minlev) & (lev <= tar_maxlev)
    if lon is not None:
        out = (lon < box[0]) | (lon > box[1]) | (lat < box[2]) | (lat > box[3])
        inr &= ~np.tile(out, nlev)
    return inr


def ens_mean(fcst):
    """[npts, nv]: sequential sum over members from 0, times 1/k"""
    k = fcst.shape[1]
    s = np.zeros((fcst.shape[0], fcst.shape[2]))
    for m in range(k):
        s = s + fcst[:, m, :]
    return s * (1.0 / k)


def norm(fcst, fcer, nij1, iv=(0, 1, 3, 5), iv_p=4, tar_lev=(1, 64), wlev=None, wg1=None, lon=None, lat=None,
         box=(0.0, 360.0, -90.0, 90.0), xf=None, xg=None, xa=None, cp=CP, tref=TREF, hvap=HVAP, wmoist=1.0):
    """-> (fcst_out, fcer_out, fmean, bad_columns); iv = (iv_u, iv_v, iv_t, iv_q), 0-based"""
    npts, k, nv = fcst.shape
    nlev = npts // nij1
    mean = ens_mean(fcst)
    bad = np.zeros(nij1, bool)
    if wlev is None:
        r, bad = dp_over_ps(mean[:, iv_p].reshape(nlev, nij1))
        wlev = r.ravel()
    with np.errstate(invalid="ignore"):
        sw = np.sqrt(wlev)
    if wg1 is not None:
        sw = sw * np.tile(wg1, nlev)
    f = factors(sw, classes(nv, *iv), cp, tref, hvap, wmoist)
    inr = region(nij1, nlev, tar_lev[0], tar_lev[1], lon, lat, box)
    if xf is not None:
        fcer = (0.5 * (xf + xg) - xa) / float(k - 1)
    # +0.0 outside the region and for variables without a factor; factor * value everywhere else
    live = inr[:, None] & (classes(nv, *iv)[None, :] != 0)
    fo = np.where(live[:, None, :], f[:, None, :] * (fcst - mean[:, None, :]), 0.0)
    eo = np.where(live, f * fcer, 0.0)
    return fo, eo, mean, bad


def lnorm_loops(fcst, fcer, nij1, dpps, iv=(0, 1, 3, 5), tar_lev=(1, 64), wg1=None, lon1=None, lat1=None,
                box=(0.0, 360.0, -90.0, 90.0), cp=CP, tref=TREF, hvap=HVAP, wmoist=1.0):
    """lnorm (efso_tools.f90:52-156) transcribed loop by loop for fcst3d(nij1, nlev, nbv, nv3d) / fcer3d(nij1, nlev, nv3d),
    given pdelta / ps (dpps [nlev, nij1]); nv2d = 0.  Returns (fcst, fcer) in norm()'s shapes."""
    npts, nbv, nv3d = fcst.shape
    nlev = npts // nij1
    f3 = fcst.reshape(nlev, nij1, nbv, nv3d).transpose(1, 0, 2, 3).copy()      # (i, k, m, v)
    e3 = fcer.reshape(nlev, nij1, nv3d).transpose(1, 0, 2).copy()
    wg = np.ones(nij1) if wg1 is None else wg1
    iv3d_u, iv3d_v, iv3d_t, iv3d_q = iv
    ensmn3d = np.zeros((nij1, nlev, nv3d))
    for i in range(nbv):
        ensmn3d[:, :, :] = ensmn3d[:, :, :] + f3[:, :, i, :]
    rinbv = 1.0 / float(nbv)
    ensmn3d[:, :, :] = ensmn3d[:, :, :] * rinbv
    for i in range(nbv):
        f3[:, :, i, :] = f3[:, :, i, :] - ensmn3d[:, :, :]
    sigweight = np.empty((nij1, nlev))
    for k in range(nlev):
        sigweight[:, k] = np.sqrt(dpps[k]) * wg[:]
    cptr = np.sqrt(cp / tref)
    qweight = np.sqrt(wmoist / (cp * tref)) * hvap
    for k in range(1, nlev + 1):
        kk = k - 1
        if k > tar_lev[1] or k < tar_lev[0]:
            f3[:, kk, :, :] = 0.0
            e3[:, kk, :] = 0.0
            continue
        for i in range(nv3d):
            if i == iv3d_u or i == iv3d_v:
                e3[:, kk, i] = sigweight[:, kk] * e3[:, kk, i]
                for j in range(nbv):
                    f3[:, kk, j, i] = sigweight[:, kk] * f3[:, kk, j, i]
            elif i == iv3d_t:
                e3[:, kk, i] = cptr * sigweight[:, kk] * e3[:, kk, i]
                for j in range(nbv):
                    f3[:, kk, j, i] = cptr * sigweight[:, kk] * f3[:, kk, j, i]
            elif i == iv3d_q:
                e3[:, kk, i] = qweight * sigweight[:, kk] * e3[:, kk, i]
                for j in range(nbv):
                    f3[:, kk, j, i] = qweight * sigweight[:, kk] * f3[:, kk, j, i]
            else:
                e3[:, kk, i] = 0.0
                f3[:, kk, :, i] = 0.0
    if lon1 is not None:
        for i in range(nij1):
            if lon1[i] < box[0] or lon1[i] > box[1] or lat1[i] < box[2] or lat1[i] > box[3]:
                e3[i, :, :] = 0.0
                f3[i, :, :, :] = 0.0
    return (f3.transpose(1, 0, 2, 3).reshape(npts, nbv, nv3d), e3.transpose(1, 0, 2).reshape(npts, nv3d))


def bins(elm, typ, lat, elem_uid, nobtype, latbound=20.0, qc=None):
    """[nobs] bin of every row, (region * (nobtype + 1) + typ - 1) * nid + element, -1 for a skipped row"""
    nid = len(elem_uid)
    out = np.full(len(elm), -1, np.int64)
    for n in range(len(elm)):
        if qc is not None and qc[n] != 0:
            continue
        hit = [u for u in range(nid) if elem_uid[u] == elm[n]]
        if not hit or typ[n] < 1 or typ[n] > nobtype + 1:
            continue
        reg = 0 if lat[n] > latbound else 2 if lat[n] < -latbound else 1
        out[n] = (reg * (nobtype + 1) + typ[n] - 1) * nid + hit[0]
    return out


def summary(obsense, elm, typ, lat, elem_uid, nobtype, latbound=20.0, qc=None):
    """(count [3, nobtype+1, nid], sum [nterm, 3, nobtype+1, nid], nneg): a stable sort by bin, one sequential sum per bin"""
    nobs, nterm = obsense.shape
    nid = len(elem_uid)
    nb = 3 * (nobtype + 1) * nid
    b = bins(elm, typ, lat, elem_uid, nobtype, latbound, qc)
    order = np.argsort(np.where(b < 0, nb, b), kind="stable")
    count = np.zeros(nb, np.int32)
    s = np.zeros((nterm, nb))
    neg = np.zeros((nterm, nb), np.int32)
    for n in order:
        if b[n] < 0:
            break
        count[b[n]] += 1
        for t in range(nterm):
            s[t, b[n]] = s[t, b[n]] + obsense[n, t]
            neg[t, b[n]] += obsense[n, t] < 0.0
    shape = (3, nobtype + 1, nid)
    return count.reshape(shape), s.reshape((nterm,) + shape), neg.reshape((nterm,) + shape)


def summary_loops(obsense, elm, typ, lat, elem_uid, nobtype, latbound=20.0, qc=None):
    """print_obsense:232-253 for every term, row by row: (nobs_sense, sumsense, rate) in the C order of summary()"""
    nobs, nterm = obsense.shape
    nid = len(elem_uid)
    uid_obs = {e: u + 1 for u, e in reversed(list(enumerate(elem_uid)))}     # the first match wins
    regnh, regtr, regsh = 1, 2, 3
    nobs_sense = np.zeros((nid, nobtype + 1, 3), np.int32, order="F")
    sumsense = np.zeros((nterm, nid, nobtype + 1, 3), order="F")
    rate = np.zeros((nterm, nid, nobtype + 1, 3), np.int32, order="F")
    for nob in range(nobs):
        if qc is not None and qc[nob] != 0:
            continue
        oid = uid_obs.get(int(elm[nob]), 0)
        if oid <= 0 or oid > nid:
            continue
        otype = int(typ[nob])
        if otype <= 0 or otype > nobtype + 1:
            continue
        if lat[nob] > latbound:
            ireg = regnh
        elif lat[nob] < -latbound:
            ireg = regsh
        else:
            ireg = regtr
        nobs_sense[oid - 1, otype - 1, ireg - 1] += 1
        for iterm in range(nterm):
            sumsense[iterm, oid - 1, otype - 1, ireg - 1] = sumsense[iterm, oid - 1, otype - 1, ireg - 1] + obsense[nob, iterm]
            if obsense[nob, iterm] < 0.0:
                rate[iterm, oid - 1, otype - 1, ireg - 1] += 1
    # (oid, otype, ireg) -> C order [ireg][otype][oid]
    return (np.ascontiguousarray(nobs_sense.transpose(2, 1, 0)), np.ascontiguousarray(sumsense.transpose(0, 3, 2, 1)),
            np.ascontiguousarray(rate.transpose(0, 3, 2, 1)))


def table_lines(count, ssum, nneg, nobs, obtypelist, obelmlist):
    """print_obsense's WRITEs (efso_tools.f90:255-287) for term 0, as Fortran formats them (none when nobs = 0)"""
    if nobs == 0:
        return []
    nreg, ntp, nid = count.shape
    charreg = ["NH", "TR", "SH"]
    lines = ["============================================", f" TOTAL NUMBER OF OBSERVATIONS:{nobs:10d}",
             "============================================", "              nobs     dJ(KE)       +rate[%]"]
    for otype in range(ntp):
        name = obtypelist[otype] if otype < ntp - 1 else "OTHERS"
        name = f"{name:<6.6s}"
        nobs_t = int(count[:, otype, :].sum())
        if nobs_t > 0:
            s_t = 0.0
            r_t = 0.0
            for ireg in range(nreg):              # Fortran SUM over (oid, ireg): oid fastest
                for oid in range(nid):
                    s_t = s_t + ssum[0, ireg, otype, oid]
                    r_t = r_t + float(nneg[0, ireg, otype, oid])
            rate_t = r_t / float(nobs_t) * 100.0
            lines.append("--------------------------------------------")
            lines.append(f"{name}  TOTAL {nobs_t:8d} {fortran_e12_5(s_t)} {rate_t:8.2f}")
        for ireg in range(nreg):
            for oid in range(nid):
                n = int(count[ireg, otype, oid])
                if n > 0:
                    rate_t = float(nneg[0, ireg, otype, oid]) / float(n) * 100.0
                    lines.append(f"{name} {charreg[ireg]} {obelmlist[oid]:<3.3s} {n:8d} {fortran_e12_5(ssum[0, ireg, otype, oid])} "
                                 f"{rate_t:8.2f}")
    lines.append("============================================")
    return lines


def fortran_e12_5(x):
    """Fortran's E12.5: [-]0.ddddd E+XX, right-aligned in 12 columns"""
    if x == 0.0:
        s = "0.00000E+00"
    else:
        m, e = f"{abs(x):.4e}".split("e")
        s = ("-" if x < 0 else "") + "0." + m.replace(".", "") + f"E{int(e) + 1:+03d}"
    return f"{s:>12s}"
