"""The Himawari-8 radiances of include/letkf_amd_h08.h restated in numpy, the seeded fixtures their tests share, and a STAND-IN
radiative transfer.

The restatement is the header's definition written out in its operation order: the record codec word by word, the selection as
a loop over the rows, itpl_2d / itpl_2d_column with the four products summed left to right (a corner of weight exactly 0 is
dropped, indexes are clamped), the unit conversions and cloud layers of RTTOV's profile structure one rounding at a time, the
zenith angle, and the weighting function's peak as the sequential loop of Trans_XtoY_H08.  Nothing here is taken from the library.

The stand-in (stand_in) is NOT a product: it is a smooth function of the profile arrays that gives every channel a transmittance
rising monotonically from the surface to the top with the peak of its vertical derivative inside the column, and all-sky / clear-
sky brightness temperatures that differ by the cloud column.  Tests and the Fortran driver use it where the host would call RTTOV.

Fields are v3 [nmem][NV3DD][nlath][nlonh][nlevh] and v2 [nmem][NV2DD][nlath][nlonh] doubles (the reference's layout per member:
level fastest), model level k at array level k + khalo."""
import functools

import numpy as np

NCH, ID_H08, TYP_H08, QC_BAD, QC_OUT, QC_OTYPE, UNDEF = 10, 8800, 23, 50, 98, 90, -9.99e33
NV3DD, NV2DD = 13, 9
V_T, V_P, V_Q, V_QC, V_QI, V_QS, V_QG = 3, 4, 5, 6, 8, 9, 10
V2_TOPO, V2_PS, V2_U10, V2_V10, V2_Q2M, V2_LSMASK, V2_SKINT = 0, 1, 3, 4, 6, 7, 8
D2R = 3.14159265358979 / 180.0
EPS = float(np.finfo(np.float64).eps)
REC = 4 + NCH + 2
PARAMS = dict(top_down=0, stggrd=0, rttov_units=0, reject_land=0, use_obs23=1, finish=0, member=1, ch_use=(1,) * NCH, ri_off=0.0,
              rj_off=0.0, rd=287.04, rv=461.46, q_ppmv=1.60771704e6, qmin=0.1e-10, minq=0.1, cfrac_cnst=0.1, sub_lon=140.7,
              r_pol=6356.7523e3, r_sat=42164.0e3, ell_tan=0.993305616, ell_ecc=0.00669438444, cldsky_thrs=-5.0, bris=-1.0e300,
              brie=1.0e300, brjs=-1.0e300, brje=1.0e300)


def params(**kw):
    p = dict(PARAMS)
    p.update(kw)
    return p


# ------------------------------------------------------------------------------------------------------------ the records
def nint32(x):
    """NINT of float32 values: half away from zero; NaN gives 0; saturating"""
    x = np.asarray(x, dtype=np.float32).astype(np.float64)
    with np.errstate(invalid="ignore"):
        r = np.trunc(x + np.copysign(0.5, x))
    r = np.where(np.isnan(x), 0.0, r)
    return np.clip(r, -2147483648.0, 2147483647.0).astype(np.int64).astype(np.int32)


def encode(cols, big_endian):
    """write_obs_H08: the file's bytes (uint8) from the columns, ten rows per profile"""
    nprof = cols["dat"].size // NCH
    w = np.zeros((nprof, REC), dtype=np.uint32)
    w[:, 0] = w[:, REC - 1] = 4 * (REC - 2)
    first = np.arange(nprof) * NCH
    with np.errstate(over="ignore", invalid="ignore"):
        for k, name in enumerate(("elm", "typ", "lon", "lat")):
            w[:, 1 + k] = cols[name][first].astype(np.float32).view(np.uint32)
        w[:, 5:5 + NCH] = cols["dat"].reshape(nprof, NCH).astype(np.float32).view(np.uint32)
    if big_endian:
        w = w.byteswap()
    return w.reshape(-1).view(np.uint8).copy()


def decode(image, obserr, big_endian):
    """read_obs_H08: (columns, number of records with a wrong marker) from the file's bytes"""
    w = np.frombuffer(np.ascontiguousarray(image).tobytes(), dtype=np.uint32).reshape(-1, REC)
    if big_endian:
        w = w.byteswap()
    nprof = w.shape[0]
    wk = w[:, 1:REC - 1].copy().view(np.float32)
    rep = lambda a: np.repeat(a, NCH)
    cols = dict(elm=rep(nint32(wk[:, 0])), typ=rep(nint32(wk[:, 1])), lon=rep(wk[:, 2].astype(np.float64)),
                lat=rep(wk[:, 3].astype(np.float64)), lev=np.tile(np.arange(NCH) + 7.0, nprof),
                dat=wk[:, 4:].astype(np.float64).reshape(-1), err=np.tile(np.asarray(obserr, dtype=np.float64), nprof),
                dif=np.zeros(nprof * NCH))
    nbad = int(((w[:, 0] != 4 * (REC - 2)) | (w[:, REC - 1] != 4 * (REC - 2))).sum())
    return cols, nbad


def file_cols(nprof, seed):
    """the columns of a file: elm 8800, typ 23, positions and brightness temperatures that need rounding to float32"""
    rng = np.random.default_rng(seed)
    lon, lat = 120.0 + 40.0 * rng.random(nprof), -40.0 + 80.0 * rng.random(nprof)
    dat = 200.0 + 90.0 * rng.random(nprof * NCH)
    return dict(elm=np.full(nprof * NCH, ID_H08, dtype=np.int32), typ=np.full(nprof * NCH, TYP_H08, dtype=np.int32),
                lon=np.repeat(lon, NCH), lat=np.repeat(lat, NCH), lev=np.tile(np.arange(NCH) + 7.0, nprof), dat=dat,
                err=np.tile(3.0 + 0.1 * np.arange(NCH), nprof), dif=np.zeros(nprof * NCH))


# ---------------------------------------------------------------------------------------------------------- the selection
def select(set_, idx, row0, nrows, h08_set, nprof_file):
    """(prof_list [nsel] ascending, slot_of_prof [nprof_file], nsel)"""
    named = np.zeros(nprof_file, dtype=bool)
    for r in range(row0, row0 + nrows):
        i1 = int(idx[r]) - 1
        if set_[r] == h08_set and 0 <= i1 < nprof_file * NCH:
            named[i1 // NCH] = True
    prof_list = np.flatnonzero(named).astype(np.int32)
    slot = np.full(nprof_file, -1, dtype=np.int32)
    slot[prof_list] = np.arange(prof_list.size, dtype=np.int32)
    return prof_list, slot, int(prof_list.size)


# ----------------------------------------------------------------------------------------------------------- the profiles
def split(r, n):
    """CEILING(r), the weight of the upper index and the two 0-based indexes clamped into the array"""
    c = int(np.ceil(r))
    return min(max(c - 2, 0), n - 1), min(max(c - 1, 0), n - 1), r - float(c - 1)


def term2(v, w1, w2):
    return v * w1 * w2 if (w1 != 0.0 and w2 != 0.0) else np.zeros_like(v)


def itpl(f, ri, rj):
    """itpl_2d / itpl_2d_column of f [nlath][nlonh][...]"""
    i0, i1, ai = split(ri, f.shape[1])
    j0, j1, aj = split(rj, f.shape[0])
    with np.errstate(all="ignore"):
        return term2(f[j0, i0], 1.0 - ai, 1.0 - aj) + term2(f[j0, i1], ai, 1.0 - aj) + term2(f[j1, i0], 1.0 - ai, aj) + \
            term2(f[j1, i1], ai, aj)


def zenith(lon, lat, p):
    """scale_H08_fwd.F90:551-572 with the argument of acos clamped; arrays or scalars"""
    with np.errstate(all="ignore"):
        rlat, rlon = lat * D2R, lon * D2R
        c_lat = np.arctan(p["ell_tan"] * np.tan(rlat))
        rl = p["r_pol"] / np.sqrt(1.0 - p["ell_ecc"] * np.cos(c_lat) * np.cos(c_lat))
        dl = rlon - p["sub_lon"] * D2R
        r1 = p["r_sat"] - rl * np.cos(c_lat) * np.cos(dl)
        r2 = -rl * np.cos(c_lat) * np.sin(dl)
        r3 = rl * np.sin(c_lat)
        rnps = np.sqrt(r1 * r1 + r2 * r2 + r3 * r3)
        r1ps, r2ps, r3ps = r1 * (-1.0), r2 * (-1.0), r3 * (-1.0)
        r1ep, r2ep, r3ep = r1 - p["r_sat"], r2, r3
        rnep = np.sqrt(r1ep * r1ep + r2ep * r2ep + r3ep * r3ep)
        z = r1ps * r1ep + r2ps * r2ep + r3ps * r3ep
        z = z / (rnps * rnep)
        z = np.fmax(-1.0, np.fmin(1.0, z))
        return np.arccos(z) / D2R


def zenith_mp(lon, lat, p, digits=50):
    """the same formula from the same double inputs and constants, evaluated with `digits` decimal digits"""
    import mpmath as mp
    with mp.workdps(digits):
        f = lambda x: mp.mpf(float(x))
        d2r = f(3.14159265358979) / 180
        rlat, rlon = f(lat) * d2r, f(lon) * d2r
        c = mp.atan(f(p["ell_tan"]) * mp.tan(rlat))
        rl = f(p["r_pol"]) / mp.sqrt(1 - f(p["ell_ecc"]) * mp.cos(c) ** 2)
        dl = rlon - f(p["sub_lon"]) * d2r
        r1, r2, r3 = f(p["r_sat"]) - rl * mp.cos(c) * mp.cos(dl), -rl * mp.cos(c) * mp.sin(dl), rl * mp.sin(c)
        e1 = r1 - f(p["r_sat"])
        z = (-r1 * e1 - r2 * r2 - r3 * r3) / (mp.sqrt(r1 * r1 + r2 * r2 + r3 * r3) * mp.sqrt(e1 * e1 + r2 * r2 + r3 * r3))
        return mp.acos(max(-1, min(1, z))) / d2r


def profiles(p, g, v3, v2, prof_list, ri, rj, lon, lat, rotc):
    """dict lev3 [nmem][nsel][5][nlev], sfc [nmem][nsel][8], pflag [nsel] and, under rttov_units, cloud [nmem][nsel][3][nlev-1]"""
    nmem, nlev, kh, nsel = v3.shape[0], g["nlev"], g["khalo"], len(prof_list)
    lev3, sfc = np.zeros((nmem, nsel, 5, nlev)), np.zeros((nmem, nsel, 8))
    cloud = np.zeros((nmem, nsel, 3, nlev - 1)) if p["rttov_units"] else None
    pflag = np.zeros(nsel, dtype=np.int32)
    order = slice(None, None, -1) if p["top_down"] else slice(None)
    repsb = 1.0 / (p["rd"] / p["rv"])
    nprof_file = p.get("nprof_file", len(ri))
    for s, fp in enumerate(prof_list):
        in_file = 0 <= fp < nprof_file                           # (a profile the file does not have is flagged, not read)
        ril, rjl = (ri[fp] - p["ri_off"], rj[fp] - p["rj_off"]) if in_file else (np.nan, np.nan)
        if not (ril >= 1.0 and ril <= float(g["nlonh"]) and rjl >= 1.0 and rjl <= float(g["nlath"])):
            pflag[s] = QC_OUT
            lev3[:, s], sfc[:, s] = UNDEF, UNDEF
            if cloud is not None:
                cloud[:, s] = UNDEF
            continue
        zen = float(zenith(lon[fp], lat[fp], p))
        for m in range(nmem):
            with np.errstate(all="ignore"):
                tsfc, qsfc = itpl(v2[m, V2_SKINT], ril, rjl), itpl(v2[m, V2_Q2M], ril, rjl)
                topo, lsm, ps = itpl(v2[m, V2_TOPO], ril, rjl), itpl(v2[m, V2_LSMASK], ril, rjl), itpl(v2[m, V2_PS], ril, rjl)
                if p["stggrd"] == 1:
                    u, v = itpl(v2[m, V2_U10], ril - 0.5, rjl), itpl(v2[m, V2_V10], ril, rjl - 0.5)
                else:
                    u, v = itpl(v2[m, V2_U10], ril, rjl), itpl(v2[m, V2_V10], ril, rjl)
                if rotc is not None:
                    u, v = u * rotc[fp, 0] - v * rotc[fp, 1], u * rotc[fp, 1] + v * rotc[fp, 0]
                col = lambda f: itpl(f[:, :, kh:kh + nlev], ril, rjl)
                prs, t, q, qc = col(v3[m, V_P]), col(v3[m, V_T]), col(v3[m, V_Q]), col(v3[m, V_QC])
                qice = col(v3[m, V_QI] + v3[m, V_QS] + v3[m, V_QG])
                if p["rttov_units"]:
                    tv = t * (1.0 + q * repsb) / (1.0 + q)
                    k2g = prs / (p["rd"] * tv) * 1000.0
                    liqc, icec = np.fmax(qc, 0.0) * k2g, np.fmax(qice, 0.0) * k2g
                    liq, ice = (liqc[:-1] + liqc[1:]) * 0.5, (icec[:-1] + icec[1:]) * 0.5
                    if p["cfrac_cnst"] <= 0.0:
                        cf = np.where((liq + ice) > p["minq"], 1.0, 0.0)
                    else:
                        cf = np.fmin((liq + ice) / p["cfrac_cnst"], 1.0)
                    cloud[m, s] = np.stack([liq[order], ice[order], cf[order]])
                    floor = p["qmin"] + p["qmin"] * 0.01
                    prs = prs * 0.01
                    q = q * p["q_ppmv"]
                    q = np.where(q < p["qmin"], floor, q)
                    qsfc = qsfc * p["q_ppmv"]
                    qsfc = floor if qsfc < p["qmin"] else qsfc
                    ps, topo = ps * 0.01, topo * 0.001                # (the mask stays as interpolated)
            lev3[m, s] = np.stack([prs[order], t[order], q[order], qc[order], qice[order]])
            sfc[m, s] = [tsfc, qsfc, ps, u, v, topo, lsm, zen]
    return dict(lev3=lev3, sfc=sfc, cloud=cloud, pflag=pflag)


# --------------------------------------------------------------------------------------------------------------- the rows
def peak(prs, tau):
    """the loop of common_obs_scale.f90:2918-2932 on model-order prs / tau [nlev]: (plev, the winning layer j)"""
    with np.errstate(all="ignore"):
        rdp = 1.0 / (prs[1] - prs[0])
        mx = abs((tau[1] - tau[0]) * rdp)
        plev, jwin = (prs[1] + prs[0]) * 0.5, 1
        for j in range(2, len(prs)):
            rdp = 1.0 / abs(prs[j] - prs[j - 1])
            w = (tau[j] - tau[j - 1]) * rdp
            if w > mx:
                mx, plev, jwin = w, (prs[j] + prs[j - 1]) * 0.5, j
    return plev, jwin


def weights(prs, tau):
    """every layer's weight [nlev-1] as the loop forms it"""
    with np.errstate(all="ignore"):
        w = (tau[1:] - tau[:-1]) * (1.0 / np.abs(prs[1:] - prs[:-1]))
        w[0] = abs((tau[1] - tau[0]) * (1.0 / (prs[1] - prs[0])))
    return w


def rows(p, row0, nrows, set_, idx, h08_set, slot_of_prof, nsel, nmem, m0, prof, btall, btclr, trans, rig, rjg, qc_replace, qc,
         ensval, lev, val2):
    """letkf_h08_rows_dev in place on qc [nrow], ensval [nrow][kld], lev, val2 [nrow]"""
    nlev, nprof_file = prof["lev3"].shape[3], len(slot_of_prof)
    order = slice(None, None, -1) if p["top_down"] else slice(None)
    for r in range(row0, row0 + nrows):
        i1 = int(idx[r]) - 1
        if set_[r] != h08_set or not (0 <= i1 < nprof_file * NCH):
            continue
        fp, c = i1 // NCH, i1 % NCH
        s = int(slot_of_prof[fp])
        if s < 0 or s >= nsel:
            continue
        if not p["use_obs23"]:
            qc[r] = QC_OTYPE if qc_replace else max(qc[r], QC_OTYPE)
            continue
        buffer = rig[fp] <= p["bris"] or rig[fp] >= p["brie"] or rjg[fp] <= p["brjs"] or rjg[fp] >= p["brje"]
        acc_lev, acc_v2, acc_qc = lev[r], val2[r], (0 if qc_replace else qc[r])
        for m in range(nmem):
            prs, tau = prof["lev3"][m, s, 0][order], trans[m, s, c][order]
            if p["rttov_units"]:
                prs = prs * 100.0
            plev, _ = peak(prs, tau)
            yobs = btall[m, s, c]
            if abs(btall[m, s, c] - btclr[m, s, c]) > p["cldsky_thrs"]:
                yobs = yobs * (-1.0)
            q = 0 if p["ch_use"][c] == 1 else QC_BAD
            if p["reject_land"] and prof["sfc"][m, s, 6] > 0.5:
                q = QC_BAD
            if q == 0 and buffer:
                q = QC_BAD
            q = max(q, int(prof["pflag"][s]))
            ensval[r, m0 + m] = yobs
            acc_lev, acc_v2, acc_qc = acc_lev + plev, acc_v2 + btclr[m, s, c], max(acc_qc, q)
        if p["finish"]:
            acc_lev, acc_v2 = acc_lev / float(p["member"]), acc_v2 / float(p["member"])
        lev[r], val2[r], qc[r] = acc_lev, acc_v2, acc_qc
    assert nlev >= 2


# ----------------------------------------------------------------------------------------------------------- the stand-in
def stand_in(prof, p):
    """(btall, btclr [nmem][nsel][NCH], trans [nmem][nsel][NCH][nlev]) from the profile arrays of `profiles`, in their level
    order.  tau_c(k) = exp(-(prs_k / pc_c)^2) with the pressure in Pa: it rises monotonically towards the top, and the peak of
    d tau / d p lies at pc_c / sqrt 2, inside the column for pc_c = 50 .. 86 kPa.  btclr is the surface's share plus the layers'
    temperatures weighted by their transmittance differences; btall subtracts a channel-dependent share of 1 - exp(-column of
    liquid + ice)."""
    lev3, sfc = prof["lev3"], prof["sfc"]
    nmem, nsel, _, nlev = lev3.shape
    prs = lev3[:, :, 0] * (100.0 if p["rttov_units"] else 1.0)
    if p["top_down"]:
        prs = prs[:, :, ::-1]
    t = lev3[:, :, 1, ::-1] if p["top_down"] else lev3[:, :, 1]
    cld = (lev3[:, :, 3] + lev3[:, :, 4]).sum(axis=2)                                   # kg/kg summed over the levels
    pc = 50.0e3 + 4.0e3 * np.arange(NCH)
    with np.errstate(all="ignore"):
        tau = np.exp(-(prs[:, :, None, :] / pc[None, None, :, None]) ** 2)              # model order
        dtau = tau[..., 1:] - tau[..., :-1]
        tmid = 0.5 * (t[..., 1:] + t[..., :-1])
        btclr = tau[..., 0] * sfc[:, :, 0, None] + (dtau * tmid[:, :, None, :]).sum(axis=3) + (1.0 - tau[..., -1]) * 210.0
        btall = btclr - (2.0 + 0.3 * np.arange(NCH))[None, None, :] * (1.0 - np.exp(-cld / CLOUD_SCALE))[:, :, None]
    trans = tau[..., ::-1] if p["top_down"] else tau
    return np.ascontiguousarray(btall), np.ascontiguousarray(btclr), np.ascontiguousarray(trans)


CLOUD_SCALE = 4.0e-3


# --------------------------------------------------------------------------------------------------------------- fixtures
def make_grid(nlev, khalo=2, nlon=12, nlat=10, ihalo=2, jhalo=2):
    return dict(nlev=nlev, khalo=khalo, nlon=nlon, nlat=nlat, ihalo=ihalo, jhalo=jhalo, nlevh=nlev + 2 * khalo,
                nlonh=nlon + 2 * ihalo, nlath=nlat + 2 * jhalo)


def make_fields(g, nmem, seed):
    """Smooth, physically ordered fields with a few per cent of seeded noise.  Cloud water and ice grow across the domain so that
    about half of the profiles are cloudy at cldsky_thrs = 1; the land mask is 1 on a corner block of cells; the variables the
    entries must not read (u, v, w, qr, rh, hgt, rain, t2m) are NaN."""
    rng = np.random.default_rng(seed)
    nk, ni, nj = g["nlevh"], g["nlonh"], g["nlath"]
    v3 = np.full((nmem, NV3DD, nj, ni, nk), np.nan)
    v2 = np.full((nmem, NV2DD, nj, ni), np.nan)
    jj, ii, kk = np.meshgrid(np.arange(nj), np.arange(ni), np.arange(nk), indexing="ij")
    for m in range(nmem):
        noise = lambda a: 1.0 + a * rng.uniform(-1.0, 1.0, size=(nj, ni, nk))
        topo = 150.0 + 20.0 * ii[:, :, 0] + 35.0 * jj[:, :, 0] + 10.0 * rng.uniform(-1, 1, size=(nj, ni))
        dz = 9000.0 / g["nlev"]
        z = topo[:, :, None] + (kk - g["khalo"] + 0.5) * dz * (1.0 + 0.02 * rng.uniform(-1, 1, size=(nj, ni, 1)))
        v3[m, V_P] = 1.0e5 * np.exp(-z / 8000.0) * (1.0 + 0.002 / g["nlev"] * rng.uniform(-1.0, 1.0, size=(nj, ni, nk)))
        v3[m, V_T] = (300.0 - 6.5e-3 * z) * noise(0.003)
        v3[m, V_Q] = 0.012 * np.exp(-z / 3000.0) * noise(0.05)
        amount = np.exp(0.45 * (ii + jj - 0.5 * (ni + nj))) / g["nlev"]
        v3[m, V_QC] = 2.0e-3 * amount * noise(0.2)
        v3[m, V_QI] = 1.0e-3 * amount * noise(0.2)
        v3[m, V_QS] = 0.6e-3 * amount * noise(0.2) * (ii > 2)
        v3[m, V_QG] = 0.4e-3 * amount * noise(0.2) * (jj > 1)
        v2[m, V2_TOPO] = topo
        v2[m, V2_PS] = 1.0e5 * np.exp(-topo / 8000.0) * (1.0 + 0.002 * rng.uniform(-1, 1, size=(nj, ni)))
        v2[m, V2_U10] = 5.0 + rng.uniform(-1, 1, size=(nj, ni))
        v2[m, V2_V10] = -3.0 + rng.uniform(-1, 1, size=(nj, ni))
        v2[m, V2_Q2M] = 0.01 * (1.0 + 0.1 * rng.uniform(-1, 1, size=(nj, ni)))
        v2[m, V2_LSMASK] = ((ii[:, :, 0] < 8) & (jj[:, :, 0] < 7)).astype(np.float64)
        v2[m, V2_SKINT] = 290.0 - 6.5e-3 * topo + rng.uniform(-1, 1, size=(nj, ni))
    return v3, v2


BUFFER = dict(bris=3.2, brie=13.9, brjs=3.0, brje=12.1)       # the buffer box of the fixtures, in global grid coordinates
N_EDGE = 6                                                     # the edge profiles at the head of a file, below


def make_case(nlev, nmem, seed, nprof=40):
    """Fields and a file of nprof profiles: the first N_EDGE are the edge cases (an integer coordinate, ri = 1.0, one outside the
    array, a NaN coordinate, the sub-satellite point, a cell whose q lies below qmin), the rest lie anywhere in the interior."""
    g = make_grid(nlev)
    v3, v2 = make_fields(g, nmem, seed)
    rng = np.random.default_rng(seed + 1)
    ri, rj = 2.6 + rng.uniform(0.0, 11.8, nprof), 2.6 + rng.uniform(0.0, 9.8, nprof)
    lon, lat = 100.0 + 80.0 * rng.random(nprof), -60.0 + 120.0 * rng.random(nprof)
    ri[0], rj[0] = 7.0, 5.0
    ri[1], rj[1] = 1.0, 4.3
    ri[2], rj[2] = 17.5, 4.0
    ri[3], rj[3] = np.nan, 6.2
    lon[4], lat[4] = PARAMS["sub_lon"], 0.0
    ri[5], rj[5] = 9.4, 8.7
    v3[:, V_Q, 7:9, 8:10, :] = 1.0e-19                         # the corners of profile 5: q * q_ppmv < qmin
    v2[:, V2_Q2M, 7:9, 8:10] = 1.0e-19
    ang = rng.uniform(-0.2, 0.2, nprof)
    rotc = np.stack([np.cos(ang), np.sin(ang)], axis=1)
    return dict(g=g, v3=v3, v2=v2, nmem=nmem, nprof=nprof, ri=ri, rj=rj, lon=lon, lat=lat, rotc=rotc)


def reference_strides(g):
    """element strides of v3[m, v, j, i, k] / v2[m, v, j, i] in C order: the reference's layout per member"""
    nk, ni, nj = g["nlevh"], g["nlonh"], g["nlath"]
    return dict(s3k=1, s3i=nk, s3j=nk * ni, s3v=nk * ni * nj, s3m=nk * ni * nj * NV3DD, s2i=1, s2j=ni, s2v=ni * nj,
                s2m=ni * nj * NV2DD)


def permuted(case, order3, order2):
    """v3 / v2 stored with their axes in another order: (array3, array2, strides).  order3 permutes 'mvjik', order2 'mvji'."""
    a3 = np.ascontiguousarray(np.transpose(case["v3"], ["mvjik".index(c) for c in order3]))
    a2 = np.ascontiguousarray(np.transpose(case["v2"], ["mvji".index(c) for c in order2]))
    es3 = {c: a3.strides[n] // 8 for n, c in enumerate(order3)}
    es2 = {c: a2.strides[n] // 8 for n, c in enumerate(order2)}
    return a3, a2, dict(s3k=es3["k"], s3i=es3["i"], s3j=es3["j"], s3v=es3["v"], s3m=es3["m"], s2i=es2["i"], s2j=es2["j"],
                        s2v=es2["v"], s2m=es2["m"])


def padded(case, canary):
    """v3 / v2 inside buffers of `canary` doubles with every stride larger than dense and a lead-in: (buffer3, buffer2, strides,
    offset3, offset2); element (m, v, j, i, k) lies at offset3 + the strides' sum"""
    v3, v2 = case["v3"], case["v2"]
    nm, nv3, nj, ni, nk = v3.shape
    s3 = dict(s3k=2, s3i=2 * nk + 1)
    s3["s3j"] = s3["s3i"] * ni + 3
    s3["s3v"] = s3["s3j"] * nj + 5
    s3["s3m"] = s3["s3v"] * nv3 + 7
    s2 = dict(s2i=3, s2j=3 * ni + 2)
    s2["s2v"] = s2["s2j"] * nj + 1
    s2["s2m"] = s2["s2v"] * v2.shape[1] + 4
    o3, o2 = 11, 5
    b3, b2 = canary(o3 + s3["s3m"] * nm + 13), canary(o2 + s2["s2m"] * nm + 9)
    m, v, j, i, k = np.ix_(np.arange(nm), np.arange(nv3), np.arange(nj), np.arange(ni), np.arange(nk))
    b3[o3 + m * s3["s3m"] + v * s3["s3v"] + j * s3["s3j"] + i * s3["s3i"] + k * s3["s3k"]] = v3
    m, v, j, i = np.ix_(np.arange(nm), np.arange(v2.shape[1]), np.arange(nj), np.arange(ni))
    b2[o2 + m * s2["s2m"] + v * s2["s2v"] + j * s2["s2j"] + i * s2["s2i"]] = v2
    return b3, b2, dict(s3, **s2), o3, o2


# the seeded fixtures tests/test_h08_statement.py pins and tests/test_gpu_h08.py runs: (nlev, nmem, seed).  (Forty profiles are a
# small sample: the seeds are ones under which the cloudy, land and buffer shares lie inside the statement test's bands.)
SIZES = [(2, 3, 113), (3, 1, 116), (63, 3, 119), (64, 17, 123), (65, 3, 137), (130, 1, 139), (3, 17, 147), (64, 1, 152)]


@functools.lru_cache(None)
def fixture(nlev, nmem, seed, top_down=0, rttov_units=0):
    """(case, params, prof_list (every profile of the file), the restatement's profiles, the stand-in's btall / btclr / trans)"""
    case = make_case(nlev, nmem, seed)
    p = params(top_down=top_down, rttov_units=rttov_units, nlev=nlev, nprof_file=case["nprof"])
    prof_list = np.arange(case["nprof"], dtype=np.int32)
    prof = profiles(p, case["g"], case["v3"], case["v2"], prof_list, case["ri"], case["rj"], case["lon"], case["lat"], case["rotc"])
    return case, p, prof_list, prof, stand_in(prof, p)


def tie_fixture(nlev, kind):
    """One member, one profile, exactly representable pressures (steps of -8192 Pa from 2^20) and transmittances (multiples of
    2^-10), every weight a multiple of 2^-23 computed without rounding.  kind "first": layers 1 and 2 tie for the maximum;
    "later": layers 2 and nlev - 1 tie above layer 1; "nan": the same with two NaN weights between them; "nan1": w1 is a NaN
    and a later layer has the largest weight (the first layer is kept).
    Returns (lev3 [1][1][5][nlev], trans [1][1][NCH][nlev], the winning layer j)."""
    assert nlev >= 6
    prs = 1048576.0 - 8192.0 * np.arange(nlev)
    step = np.ones(nlev - 1)                                    # step[j - 1]: layer j's rise of tau, in units of 2^-10
    if kind == "first":
        step[0], step[1], win = 4.0, 4.0, 1
    elif kind in ("later", "nan"):
        step[1], step[nlev - 2], win = 6.0, 6.0, 2
    else:
        step[nlev - 2], win = 9.0, 1
    tau = np.concatenate([[0.0], np.cumsum(step)]) / 1024.0
    lev3 = np.zeros((1, 1, 5, nlev))
    lev3[0, 0, 0] = prs
    trans = np.tile(tau, (1, 1, NCH, 1))
    if kind == "nan":
        trans[..., 3] = np.nan                                  # layers 3 and 4 have NaN weights; 2 and nlev - 1 still tie
    if kind == "nan1":
        trans[..., 0] = np.nan
    return lev3, trans, win
