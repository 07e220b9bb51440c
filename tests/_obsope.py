"""The observation operator in numpy / plain Python, written from scale/obs/obsope_tools.f90:454-507 and
scale/common/common_obs_scale.f90 (phys2ijk :999-1110, phys2ijkz :1116-1237, Trans_XtoY :264-338, Trans_XtoY_radar :342-493,
calc_ref_vr :626-990, prsadj :600-616, itpl_* :1295-1366) and common/common.f90 (com_distll_1 :401-424): the CPU statement the
device entry letkf_obsope_dev (include/letkf_amd_obsope.h) is compared with, the seeded fixtures, and the ctypes plumbing of a
device call.  tests/test_obsope_statement.py anchors the statement to things its author did not write.

Arrays are 0-based here: v3[m, v, j, i, k] and v2[m, v, j, i] in C order are the reference's (nlevh, nlonh, nlath, nv3dd) and
(nlonh, nlath, nv2dd) per member; coordinates ri, rj, rk stay 1-based as in the reference.  Real literals the reference
writes without a kind are single precision there: f32() widens them.
"""
import ctypes as C
import math

import numpy as np

EPS = float(np.finfo(np.float64).eps)


def f32(x):
    return float(np.float32(x))


PI, GG, RD, RV, RE, UNDEF = 3.1415926535, 9.81, 287.05, 461.50, 6371.3e3, -9.99e33     # common/common.f90:28-38
FVIRT, DEG2RAD, RAD2DEG = RV / RD - 1.0, PI / 180.0, 180.0 / PI
GAMMA_48, GAMMA_425, GAMMA_45 = math.gamma(4.8), math.gamma(4.25), math.gamma(4.5)    # com_gamma's three arguments in calc_ref_vr
ID_U, ID_V, ID_T, ID_TV, ID_Q, ID_RH, ID_PS, ID_RAIN = 2819, 2820, 3073, 3074, 3330, 3331, 14593, 19999
ID_REF, ID_REF_ZERO, ID_VR, ID_PRH = 4001, 4004, 4002, 4003
QC_PS_TER, QC_REF_LOW, QC_RADAR_VHI, QC_OUT_VHI, QC_OUT_VLO, QC_OTYPE, QC_OUT_H = 10, 11, 19, 20, 21, 90, 98
V_U, V_V, V_W, V_T, V_P, V_Q, V_QC, V_QR, V_QI, V_QS, V_QG, V_RH, V_HGT = range(13)     # iv3dd_* - 1
V2_TOPO, V2_PS, V2_RAIN, V2_U10, V2_V10, V2_T2M, V2_Q2M = range(7)                      # iv2dd_* - 1
NV3DD, NV2DD = 13, 7


class Branches:
    """The smallest relative distance to any comparison a (row, member) evaluation took.  An exact tie counts as distance 0
    unless the caller says both sides are exact by construction (integer ri, rj; a sum of exact zeros; direct inputs)."""

    def __init__(self):
        self.dist = math.inf

    def cmp(self, a, b, exact_ok=False):
        if a == b and exact_ok:
            return
        if not (math.isfinite(a) and math.isfinite(b)):
            return
        scale = max(abs(a), abs(b))
        self.dist = min(self.dist, abs(a - b) / scale if scale > 0.0 else 0.0)


def split(r):
    """CEILING(r) and the weight of that index (1-based)"""
    c = math.ceil(r)
    return c, r - float(c - 1)


def _clamp(idx1, n):
    """1-based index -> 0-based, inside the array (the one place the reference is undefined: weight exactly 0 on index 0)"""
    return min(max(idx1 - 1, 0), n - 1)


def itpl_3d(var, rk, ri, rj):
    """itpl_3d as its callers use it: var[j, i, k], the level is the first interpolation axis.  Returns (value, sum |w v|).
    Term order and the left-to-right products are the reference's; a weight of exactly 0 drops the term."""
    nj, ni, nk = var.shape
    k, ak = split(rk)
    i, ai = split(ri)
    j, aj = split(rj)
    s, sabs = 0.0, 0.0
    for jj, wj in ((j - 1, 1.0 - aj), (j, aj)):
        for ii, wi in ((i - 1, 1.0 - ai), (i, ai)):
            for kk, wk in ((k - 1, 1.0 - ak), (k, ak)):
                if wk == 0.0 or wi == 0.0 or wj == 0.0:
                    continue
                t = float(var[_clamp(jj, nj), _clamp(ii, ni), _clamp(kk, nk)]) * wk * wi * wj
                s += t
                sabs += abs(t)
    return s, sabs


def itpl_2d(var, ri, rj):
    """itpl_2d on var[j, i]; (value, sum |w v|)"""
    nj, ni = var.shape
    i, ai = split(ri)
    j, aj = split(rj)
    s, sabs = 0.0, 0.0
    for jj, ii, wi, wj in ((j - 1, i - 1, 1.0 - ai, 1.0 - aj), (j - 1, i, ai, 1.0 - aj), (j, i - 1, 1.0 - ai, aj), (j, i, ai, aj)):
        if wi == 0.0 or wj == 0.0:
            continue
        t = float(var[_clamp(jj, nj), _clamp(ii, ni)]) * wi * wj
        s += t
        sabs += abs(t)
    return s, sabs


def itpl_2d_column(var, ri, rj):
    """itpl_2d_column on var[j, i, :]: every level at once"""
    nj, ni, nk = var.shape
    i, ai = split(ri)
    j, aj = split(rj)
    out = np.zeros(nk)
    for jj, ii, wi, wj in ((j - 1, i - 1, 1.0 - ai, 1.0 - aj), (j - 1, i, ai, 1.0 - aj), (j, i - 1, 1.0 - ai, aj), (j, i, ai, aj)):
        if wi == 0.0 or wj == 0.0:
            continue
        out = out + var[_clamp(jj, nj), _clamp(ii, ni), :] * wi * wj
    return out


def corner_columns(var, ri, rj):
    nj, ni, _ = var.shape
    i, j = math.ceil(ri), math.ceil(rj)
    return [var[_clamp(jj, nj), _clamp(ii, ni), :] for jj in (j - 1, j) for ii in (i - 1, i)]


def vertical_index(field, radar, ri, rj, lev, g, br):
    """phys2ijk (pressure, radar False) / phys2ijkz (height, radar True) below the domain test: (rk, qc).  Levels are 0-based
    here, kb .. ktop the model levels; rk is the reference's 1-based coordinate."""
    kb, ktop = g["khalo"], g["khalo"] + g["nlev"] - 1
    ks = kb
    for col in corner_columns(field, ri, rj):
        k = kb
        while k <= ktop and not ((-300.0 < col[k] < 10000.0) if radar else (col[k] >= 0.0)):
            k += 1
        ks = max(ks, k)
    if ks > ktop:
        return UNDEF, QC_OUT_VLO
    with np.errstate(invalid="ignore", divide="ignore"):
        plev = itpl_2d_column(field if radar else np.log(field), ri, rj)
    tl = lev if radar else math.log(lev)
    exact = float(ri).is_integer() and float(rj).is_integer()
    br.cmp(tl, float(plev[ktop]), exact)
    if (tl > plev[ktop]) if radar else (tl < plev[ktop]):
        return UNDEF, QC_OUT_VHI
    br.cmp(tl, float(plev[ks]), exact)
    if (tl < plev[ks]) if radar else (tl > plev[ks]):
        return UNDEF, QC_OUT_VLO
    k = ks + 1
    while k <= ktop:
        br.cmp(float(plev[k]), tl, exact)
        if (plev[k] > tl) if radar else (plev[k] < tl):
            break
        k += 1
    if k > ktop:
        return float(ktop + 1), 0                  # on the top level itself (the reference: 0 / a halo difference)
    ak = (tl - float(plev[k - 1])) / (float(plev[k]) - float(plev[k - 1]))
    return float(k) + ak, 0                        # REAL(k' - 1) + ak with k' = k + 1


def com_distll_1(alon, alat, blon, blat):
    r180 = 1.0 / 180.0
    lon1, lon2, lat1, lat2 = alon * PI * r180, blon * PI * r180, alat * PI * r180, blat * PI * r180
    cosd = math.sin(lat1) * math.sin(lat2) + math.cos(lat1) * math.cos(lat2) * math.cos(lon2 - lon1)
    cosd = max(-1.0, min(1.0, cosd))
    return math.acos(cosd) * RE


def terminal_velocities(qr, qs, qg, ro, nor, nos, nog, ror, ros, rog, roo, rofactor_exp):
    a, b, c, d, cd = 2115.0, 0.8, 152.93, 0.25, 0.6
    rofactor = (roo / ro) ** rofactor_exp
    wr = ws = wg = 0.0
    if qr > 0.0:
        lr = (PI * ror * nor / (ro * qr)) ** 0.25
        wr = a * GAMMA_48 / (6.0 * (lr ** b))
        wr = 1.0e-2 * wr * rofactor
    if qs > 0.0:
        ls = (PI * ros * nos / (ro * qs)) ** 0.25
        ws = c * GAMMA_425 / (6.0 * (ls ** d))
        ws = 1.0e-2 * ws * rofactor
    if qg > 0.0:
        lg = (PI * rog * nog / (ro * qg)) ** 0.25
        wg = GAMMA_45 * (((4.0 * GG * 100.0 * rog) / (3.0 * cd * ro)) ** 0.5)
        wg = 1.0e-2 * wg / (6.0 * (lg ** 0.5))
    return wr, ws, wg


def calc_ref_vr(method, use_tv, qr, qs, qg, u, v, w, t, p, az, elev, br=None, zero=(False, False, False)):
    """calc_ref_vr: (ref [mm^6 m^-3], vr, wt, parts).  zero[n]: species n (r, s, g) is a sum of exact zeros."""
    br = br or Branches()
    zr = zs = zg = zms = zmg = ref = wt = 0.0
    ro = p / (RD * t)
    pip = PI ** 1.75
    parts = {}
    for q, z in zip((qr, qs, qg), zero):
        br.cmp(q, 0.0, z)
    if method == 1:
        nor, ror, cf, p0 = 8.0e6, 1000.0, 10.0e18 * 72, 1.0e5
        qt = qr + qs + qg
        br.cmp(qt, 0.0, all(zero))
        if qt > 0.0:
            ref = cf * ((ro * qt) ** 1.75)
            ref = ref / (pip * (nor ** 0.75) * (ror ** 1.75))
            a = (p0 / p) ** f32(0.4)
            wt = 5.40 * a * (qt ** 0.125)
    elif method == 2:
        nor, nos, nog, ror, ros, rog, roi, roo = 8.0e6, 3.0e6, 4.0e4, 1000.0, 100.0, 913.0, 917.0, 1.0
        ki2, kr2, cf = 0.176, 0.930, 1.0e18 * 720
        if qr > 0.0:
            zr = cf * ((ro * qr) ** 1.75)
            zr = zr / (pip * (nor ** 0.75) * (ror ** 1.75))
        if qs > 0.0:
            br.cmp(t, f32(273.16))
            if t <= f32(273.16):
                zs = cf * ki2 * (ros ** 0.25) * ((ro * qs) ** 1.75)
                zs = zs / (pip * kr2 * (nos ** 0.75) * (roi ** 2))
                parts["snow"] = "cold"
            else:
                zs = cf * ((ro * qs) ** 1.75)
                zs = zs / (pip * (nos ** 0.75) * (roi ** 1.75))
                parts["snow"] = "warm"
        if qg > 0.0:
            zg = (cf / (pip * (nog ** 0.75) * (rog ** 1.75))) ** f32(0.95)
            zg = zg * ((ro * qg) ** f32(1.6625))
        ref = zr + zs + zg
        if ref > 0.0:
            m = f32(1e-3)
            wr, ws, wg = terminal_velocities(qr, qs, qg, ro * m, nor * m, nos * m, nog * m, ror * m, ros * m, rog * m, roo * m, 0.25)
            wt = (wr * zr + ws * zs + wg * zg) / (zr + zs + zg)
    elif method == 3:
        maxf = 0.5
        fg = fs = fwg = fws = 0.0
        if qr > 0.0 and qg > 0.0:
            fg = maxf * (min(qr / qg, qg / qr)) ** (1.0 / 3.0)
            fwg = qr / (qr + qg)
        if qr > 0.0 and qs > 0.0:
            fs = maxf * (min(qr / qs, qs / qr)) ** (1.0 / 3.0)
            fws = qr / (qr + qs)
        qrp, qsp, qgp = (1.0 - fs - fg) * qr, (1.0 - fs) * qs, (1.0 - fg) * qg
        qms, qmg = fs * (qr + qs), fg * (qr + qg)
        # (Fs, Fg <= 0.5 and not both 0.5 unless qr = qs = qg: the primed species are > 0 exactly where their own is)
        br.cmp(qrp, 0.0, qr == 0.0 or zero[0])
        if qrp > 0.0:
            zr = 2.53e4 * (ro * qrp * 1.0e3) ** f32(1.84)
        if qsp > 0.0:
            zs = 3.48e3 * (ro * qsp * 1.0e3) ** f32(1.66)
        if qgp > 0.0:
            zg = 5.54e3 * (ro * qgp * 1.0e3) ** f32(1.70)
        if qms > 0.0:
            zms = (f32(0.00491) + f32(5.75) * fws - f32(5.588) * (fws ** 2)) * 1.0e5
            zms = zms * (ro * qms * 1.0e3) ** (f32(1.67) - f32(0.202) * fws + f32(0.398) * (fws ** 2))
        if qmg > 0.0:
            zmg = (f32(0.809) + f32(10.13) * fwg - f32(5.98) * (fwg ** 2)) * 1.0e5
            zmg = zmg * (ro * qmg * 1.0e3) ** (f32(1.48) + f32(0.0448) * fwg - f32(0.0313) * (fwg ** 2))
        ref = zr + zg + zs + zms + zmg
        parts.update(Fs=fs, Fg=fg, zr=zr, zs=zs, zg=zg, zms=zms, zmg=zmg)
        if ref > 0.0:
            wr, ws, wg = terminal_velocities(qr, qs, qg, 1.0e-3 * ro, 8.0e-2, 3.0e-2, 4.0e-4, 1.0, 0.1, 0.917, 0.001, 0.5)
            wt = (wr * zr + ws * zs + ws * zms + wg * zg + wg * zmg) / (zr + zs + zg + zms + zmg)
    else:
        raise ValueError("METHOD_REF_CALC must be 1..3")
    vr = u * math.cos(elev * DEG2RAD) * math.sin(az * DEG2RAD)
    vr = vr + v * math.cos(elev * DEG2RAD) * math.cos(az * DEG2RAD)
    vr = vr + ((w - wt) if use_tv else w) * math.sin(elev * DEG2RAD)
    return ref, vr, wt, parts


def radar_angles(lon, lat, lev, rlon, rlat, rz, br=None):
    """azimuth [0, 360) and elevation in degrees, Trans_XtoY_radar :408-425"""
    dlon, dlat = lon - rlon, lat - rlat
    az = RAD2DEG * math.atan2(dlon * math.cos(rlat * DEG2RAD), dlat)
    if br is not None:
        br.cmp(az, 0.0, dlon == 0.0)
    if az < 0.0:
        az = 360.0 + az
    elev = RAD2DEG * math.atan2(lev - rz, com_distll_1(lon, lat, rlon, rlat))
    return az, elev


def prsadj(p, dz, t, q):
    if dz != 0:
        tv = t * (1.0 + 0.608 * q)
        p = p * ((-5.0e-3 * dz + tv) / tv) ** (GG / (5.0e-3 * RD))
    return p


def operator(cfg, g, v3, v2, row, rotc=(1.0, 0.0)):
    """One (row, member): dict(val, qc (before the reduction), kind, tol, dist).  v3[v, j, i, k], v2[v, j, i] of the member.
    kind: 'zero' | 'undef' | 'lowref' (exact values), 'interp' | 'ps' | 'dbz' | 'vr' (tol = the derived bound)."""
    br = Branches()
    out = dict(val=0.0, qc=0, kind="zero", tol=0.0, dist=math.inf)

    def done(**kw):
        out.update(kw)
        out["dist"] = br.dist
        return out

    elm, lev = row["elm"], row["lev"]
    ril, rjl = row["ri"] - cfg["ri_off"], row["rj"] - cfg["rj_off"]
    if not cfg["use_obs"][row["typ"] - 1]:
        return done(qc=QC_OTYPE)
    radar = row["radar"]                                   # None: conventional; else (lon, lat, z) of the file's radar
    if radar is not None and lev > cfg["radar_zmax"]:
        return done(qc=QC_RADAR_VHI)
    if ril < 1.0 or ril > g["nlonh"] or rjl < 1.0 or rjl > g["nlath"]:
        return done(qc=QC_OUT_H)
    stg = cfg["stggrd"] == 1
    ulp = lambda x: 4.0 * EPS * abs(x)
    if radar is None:
        if elm > 9999:
            rk = lev
        else:
            rk, qc = vertical_index(v3[V_P], False, ril, rjl, lev, g, br)
            if qc:
                return done(qc=qc)
        if elm in (ID_U, ID_V):
            u, su = itpl_3d(v3[V_U], rk, ril - 0.5 if stg else ril, rjl)
            v, sv = itpl_3d(v3[V_V], rk, ril, rjl - 0.5 if stg else rjl)
            val = u * rotc[0] - v * rotc[1] if elm == ID_U else u * rotc[1] + v * rotc[0]
            a, b = (abs(rotc[0]), abs(rotc[1])) if elm == ID_U else (abs(rotc[1]), abs(rotc[0]))
            return done(val=val, kind="interp", tol=64.0 * EPS * (su * a + sv * b) + ulp(su * a + sv * b))
        if elm == ID_T:
            val, s = itpl_3d(v3[V_T], rk, ril, rjl)
            return done(val=val, kind="interp", tol=64.0 * EPS * s)
        if elm == ID_TV:
            t, st = itpl_3d(v3[V_T], rk, ril, rjl)
            q, sq = itpl_3d(v3[V_Q], rk, ril, rjl)
            val = t * (1.0 + FVIRT * q)
            return done(val=val, kind="interp", tol=64.0 * EPS * (st * (1.0 + FVIRT * abs(q)) + abs(t) * FVIRT * sq) + ulp(val))
        if elm == ID_Q:
            val, s = itpl_3d(v3[V_Q], rk, ril, rjl)
            return done(val=val, kind="interp", tol=64.0 * EPS * s)
        if elm == ID_RH:
            val, s = itpl_3d(v3[V_RH], rk, ril, rjl)
            return done(val=val, kind="interp", tol=64.0 * EPS * s)
        if elm == ID_PS:
            t, st = itpl_2d(v2[V2_T2M], ril, rjl)
            q, sq = itpl_2d(v2[V2_Q2M], ril, rjl)
            topo, sz = itpl_2d(v2[V2_TOPO], ril, rjl)
            ps, sp = itpl_2d(v2[V2_PS], ril, rjl)
            dz = rk - topo
            exact = float(ril).is_integer() and float(rjl).is_integer()
            br.cmp(rk, topo, exact)
            val = prsadj(ps, dz, t, q)
            br.cmp(abs(dz), cfg["ps_adjust_thres"])
            # the four interpolation bounds through prsadj's derivative, plus 64 ulp of the result
            gam, c = 5.0e-3, GG / (5.0e-3 * RD)
            tv = t * (1.0 + 0.608 * q)
            ratio = (-gam * dz + tv) / tv
            d_ps = ratio ** c
            d_topo = abs(ps) * c * ratio ** (c - 1.0) * gam / tv
            d_tv = abs(ps) * c * ratio ** (c - 1.0) * abs(gam * dz) / (tv * tv)
            e = 64.0 * EPS
            tol = (d_ps * e * sp + d_topo * e * sz + d_tv * ((1.0 + 0.608 * abs(q)) * e * st + 0.608 * abs(t) * e * sq)
                   + 64.0 * EPS * abs(val))
            return done(val=val, qc=QC_PS_TER if abs(dz) > cfg["ps_adjust_thres"] else 0, kind="ps", tol=tol)
        return done(val=UNDEF, qc=QC_OTYPE, kind="undef")
    rk, qc = vertical_index(v3[V_HGT], True, ril, rjl, lev, g, br)
    if qc:
        return done(qc=qc)
    ut, _ = itpl_3d(v3[V_U], rk, ril - 0.5 if stg else ril, rjl)
    vt, _ = itpl_3d(v3[V_V], rk, ril, rjl - 0.5 if stg else rjl)
    wr, _ = itpl_3d(v3[V_W], rk - 0.5 if stg else rk, ril, rjl)
    tr, _ = itpl_3d(v3[V_T], rk, ril, rjl)
    pr, _ = itpl_3d(v3[V_P], rk, ril, rjl)
    qrr, sr = itpl_3d(v3[V_QR], rk, ril, rjl)
    qsr, ss = itpl_3d(v3[V_QS], rk, ril, rjl)
    qgr, sg = itpl_3d(v3[V_QG], rk, ril, rjl)
    ur = ut * rotc[0] - vt * rotc[1]
    vr_ = ut * rotc[1] + vt * rotc[0]
    rlon, rlat, rz = radar
    if row["lon"] - rlon == 0.0 and row["lat"] - rlat == 0.0:
        return done(val=UNDEF, qc=QC_OUT_H, kind="undef")
    az, elev = radar_angles(row["lon"], row["lat"], lev, rlon, rlat, rz, br)
    ref, rv, wt, _ = calc_ref_vr(cfg["method_ref_calc"], cfg["use_terminal_velocity"], qrr, qsr, qgr, ur, vr_, wr, tr, pr, az, elev,
                                 br, (sr == 0.0, ss == 0.0, sg == 0.0))
    min_ref = 10.0 ** (cfg["min_radar_ref_dbz"] / 10.0)
    if elm in (ID_REF, ID_REF_ZERO, ID_VR):
        br.cmp(ref, min_ref)
    if elm in (ID_REF, ID_REF_ZERO):
        if ref < min_ref:
            return done(val=cfg["min_radar_ref_dbz"] + cfg["low_ref_shift"], kind="lowref")     # qc 11 -> 0
        return done(val=10.0 * math.log10(ref), kind="dbz", tol=1e-11)
    if elm == ID_VR:
        return done(val=rv, kind="vr", tol=1e-9 * (abs(ur) + abs(vr_) + abs(wr) + wt))
    return done(val=UNDEF, qc=QC_OTYPE, kind="undef")


# ---------------------------------------------------------------------------------------------------------------- fixtures
RADARS = np.array([[136.5, 35.9, 300.0], [135.0, 35.0, 50.0]])       # radar_meta rows: lon, lat, z
FILE_RADAR = np.array([-1, 1, 0], dtype=np.int32)                    # file 0 conventional, file 1 radar row 1, file 2 radar row 0
NOBTYPE = 24
TERRAIN_COLS = ((4, 2), (4, 3))                                      # 0-based (i, j) whose two lowest model levels are below ground


def default_cfg(**kw):
    use = np.ones(NOBTYPE, dtype=np.int32)
    use[2] = 0                                                       # report type 3 is switched off
    c = dict(method_ref_calc=2, use_terminal_velocity=1, stggrd=0, min_radar_ref_dbz=5.0, low_ref_shift=-5.0, radar_zmax=12000.0,
             ps_adjust_thres=100.0, ri_off=5.0, rj_off=0.0, use_obs=use)
    c.update(kw)
    return c


def make_grid(nlev, khalo=2, nlon=5, nlat=3, ihalo=2, jhalo=2):
    return dict(nlev=nlev, khalo=khalo, nlon=nlon, nlat=nlat, ihalo=ihalo, jhalo=jhalo, nlevh=nlev + 2 * khalo,
                nlonh=nlon + 2 * ihalo, nlath=nlat + 2 * jhalo)


def make_fields(g, nmem, seed):
    """Smooth, physically ordered fields (height ascending, pressure descending) with a few per cent of seeded noise; every
    hydrometeor is exactly 0 on part of the domain; TERRAIN_COLS have two model levels below ground (undef in every field)."""
    rng = np.random.default_rng(seed)
    nk, ni, nj = g["nlevh"], g["nlonh"], g["nlath"]
    v3 = np.zeros((nmem, NV3DD, nj, ni, nk))
    v2 = np.zeros((nmem, NV2DD, nj, ni))
    jj, ii, kk = np.meshgrid(np.arange(nj), np.arange(ni), np.arange(nk), indexing="ij")
    for m in range(nmem):
        noise = lambda a: 1.0 + a * rng.uniform(-1.0, 1.0, size=(nj, ni, nk))
        topo = 150.0 + 20.0 * ii[:, :, 0] + 35.0 * jj[:, :, 0] + 10.0 * rng.uniform(-1, 1, size=(nj, ni))
        dz = 9000.0 / g["nlev"]
        z = topo[:, :, None] + (kk - g["khalo"] + 0.5) * dz * (1.0 + 0.02 * rng.uniform(-1, 1, size=(nj, ni, 1)))
        v3[m, V_HGT] = z
        v3[m, V_P] = 1.0e5 * np.exp(-z / 8000.0) * noise(0.002)
        v3[m, V_T] = (300.0 - 6.5e-3 * z) * noise(0.003)
        v3[m, V_U] = (12.0 + 0.8 * ii - 0.5 * jj + 1.5e-3 * z) * noise(0.05)
        v3[m, V_V] = (-7.0 + 0.3 * ii + 0.9 * jj - 1.0e-3 * z) * noise(0.05)
        v3[m, V_W] = (0.5 + 0.05 * ii - 0.08 * jj + 1.0e-4 * z) * noise(0.1)
        v3[m, V_Q] = 0.012 * np.exp(-z / 3000.0) * noise(0.05)
        v3[m, V_RH] = (0.7 - 4.0e-5 * z) * noise(0.05)
        hyd = lambda a, b, c, d: np.exp(a + b * ii + c * jj + d * z / 1000.0) * noise(0.1)
        v3[m, V_QC] = hyd(-9.0, 0.1, 0.1, -0.1)
        v3[m, V_QR] = hyd(-13.5, 0.55, 0.35, -0.25) * (ii < 7)
        v3[m, V_QI] = hyd(-12.0, 0.1, 0.1, 0.2)
        v3[m, V_QS] = hyd(-15.0, 0.3, 0.6, 0.35) * (ii > 2)
        v3[m, V_QG] = hyd(-14.0, 0.5, 0.3, 0.1) * (jj > 1)
        for (i, j) in TERRAIN_COLS:
            v3[m, :, j, i, g["khalo"]:g["khalo"] + 2] = UNDEF
        v2[m, V2_TOPO] = topo
        v2[m, V2_PS] = 1.0e5 * np.exp(-topo / 8000.0) * (1.0 + 0.002 * rng.uniform(-1, 1, size=(nj, ni)))
        v2[m, V2_RAIN] = rng.uniform(0, 1, size=(nj, ni))
        v2[m, V2_U10] = 5.0 + rng.uniform(-1, 1, size=(nj, ni))
        v2[m, V2_V10] = -3.0 + rng.uniform(-1, 1, size=(nj, ni))
        v2[m, V2_T2M] = 288.0 - 6.5e-3 * topo + rng.uniform(-1, 1, size=(nj, ni))
        v2[m, V2_Q2M] = 0.01 * (1.0 + 0.1 * rng.uniform(-1, 1, size=(nj, ni)))
    return v3, v2


def _level_range(field, radar, ril, rjl, g):
    """(value at ks, value at the top) of the interpolated column, in the scan's variable (height, or log pressure), and ks"""
    kb, ktop = g["khalo"], g["khalo"] + g["nlev"] - 1
    ks = kb
    for col in corner_columns(field, ril, rjl):
        k = kb
        while k <= ktop and not ((-300.0 < col[k] < 10000.0) if radar else (col[k] >= 0.0)):
            k += 1
        ks = max(ks, k)
    with np.errstate(invalid="ignore", divide="ignore"):
        plev = itpl_2d_column(field if radar else np.log(field), ril, rjl)
    return float(plev[ks]), float(plev[ktop]), ks


SEEDS = {8: 7, 70: 9}       # seeds under which no row lies within 1e-6 of a comparison (tests/test_obsope_statement.py asserts it)


def make_case(nlev, nmem=3, seed=None):
    """Grid, fields and about 300 obsda rows covering what tests/test_gpu_obsope.py lists.  Levels are placed with member 0's
    columns; every member's own column then decides its qc."""
    seed = SEEDS.get(nlev, 7) if seed is None else seed
    g = make_grid(nlev)
    v3, v2 = make_fields(g, nmem, seed)
    rng = np.random.default_rng(seed + 1000)
    cfg = default_cfg()
    ro, rjo = cfg["ri_off"], cfg["rj_off"]
    rows = []

    def add(file, elm, ril, rjl, lev, typ=1, lon=None, lat=None, tag=""):
        rows.append(dict(file=file, elm=elm, typ=typ, lev=float(lev), ri=float(ril) + ro, rj=float(rjl) + rjo,
                         lon=137.0 + 0.07 * ril if lon is None else lon, lat=36.4 + 0.06 * rjl if lat is None else lat, tag=tag))

    def lev_at(file, ril, rjl, frac):
        radar = file > 0
        lo, hi, _ = _level_range(v3[0, V_HGT if radar else V_P], radar, ril, rjl, g)
        x = lo + frac * (hi - lo)
        return x if radar else math.exp(x)

    def pos(lo_i=1.05, hi_i=None, lo_j=1.05, hi_j=None):
        return (rng.uniform(lo_i, hi_i or g["nlonh"] - 0.05), rng.uniform(lo_j, hi_j or g["nlath"] - 0.05))

    # every element of both formats, at random positions and levels inside the members' common range
    for elm in (ID_U, ID_V, ID_T, ID_TV, ID_Q, ID_RH):
        for n in range(16):
            ri, rj = pos(1.6, None, 1.6, None)
            add(0, elm, ri, rj, lev_at(0, ri, rj, rng.uniform(0.08, 0.92)), typ=1 + n % 2, tag="conv")
    for elm in (ID_REF, ID_VR, ID_REF_ZERO):
        for n in range(48 if elm != ID_REF_ZERO else 12):
            ri, rj = pos(1.6, None, 1.6, None)
            add(1 + n % 2, elm, ri, rj, lev_at(1, ri, rj, rng.uniform(0.05, 0.9)), typ=22, tag="radar")
    # PS: station heights on both sides of PS_ADJUST_THRES, and one exactly on the model terrain at a grid point
    for n in range(16):
        ri, rj = pos()
        topo = itpl_2d(v2[0, V2_TOPO], ri, rj)[0]
        add(0, ID_PS, ri, rj, topo + (rng.uniform(-80, 80) if n % 2 else rng.uniform(120, 300) * (1 if n % 4 else -1)), tag="ps")
    add(0, ID_PS, 3.0, 4.0, v2[0, V2_TOPO, 3, 2], tag="ps-dz0")
    # elements the operator does not serve, and a switched-off report type
    add(0, 1234, 4.3, 3.2, lev_at(0, 4.3, 3.2, 0.5), tag="unknown")
    add(0, ID_RAIN, 4.3, 3.2, 0.0, tag="unknown")
    add(1, ID_U, 4.3, 3.2, lev_at(1, 4.3, 3.2, 0.5), tag="unknown")
    add(2, ID_PRH, 6.3, 2.2, lev_at(2, 6.3, 2.2, 0.4), tag="unknown")
    add(0, ID_T, 4.3, 3.2, lev_at(0, 4.3, 3.2, 0.5), typ=3, tag="off")
    add(1, ID_REF, 4.3, 3.2, lev_at(1, 4.3, 3.2, 0.5), typ=3, tag="off")
    # outside the domain on each side; too high and too low; above RADAR_ZMAX
    for file, elm in ((0, ID_T), (1, ID_REF)):
        for ri, rj in ((0.5, 3.0), (g["nlonh"] + 0.25, 3.0), (3.0, 0.75), (3.0, g["nlath"] + 0.5)):
            add(file, elm, ri, rj, lev_at(file, 3.0, 3.0, 0.5), typ=22 if file else 1, tag="outside")
        for frac in (1.15, -0.2):
            ri, rj = pos(1.6, None, 1.6, None)
            add(file, elm, ri, rj, lev_at(file, ri, rj, frac), typ=22 if file else 1, tag="vbound")
    add(1, ID_VR, 5.5, 3.5, 12000.5, typ=22, tag="zmax")
    add(2, ID_REF, 5.5, 3.5, 12500.0, typ=22, tag="zmax")
    # a target on the radar's own lon / lat
    add(1, ID_REF, 5.2, 3.3, lev_at(1, 5.2, 3.3, 0.3), typ=22, lon=RADARS[1, 0], lat=RADARS[1, 1], tag="on-radar")
    add(2, ID_VR, 5.2, 3.3, lev_at(2, 5.2, 3.3, 0.3), typ=22, lon=RADARS[0, 0], lat=RADARS[0, 1], tag="on-radar")
    # terrain: two of the four corner columns start two levels higher; rows just above and just below the lowest valid level
    for file, elm in ((0, ID_T), (0, ID_U), (1, ID_REF), (2, ID_VR)):
        for n in range(4):
            ri, rj = rng.uniform(4.1, 4.9), rng.uniform(3.1, 3.9)           # corners i = 4, 5 and j = 3, 4 (1-based)
            lo, hi, ks = _level_range(v3[0, V_HGT if file else V_P], file > 0, ri, rj, g)
            assert ks == g["khalo"] + 2
            d = (2e-3 * abs(lo)) if file else 2e-3
            x = lo + (d if (n % 2 == 0) == (file > 0) else -d)             # even n: inside the range
            add(file, elm, ri, rj, x if file else math.exp(x), typ=22 if file else 1, tag="terrain")
    # exact bounds on integer coordinates (the column interpolation is exact there), the terrain column among them
    for (i1, j1) in ((3, 2), (5, 3), (7, 5)):
        for file, elm in ((0, ID_Q), (1, ID_REF)):
            col = v3[0, V_HGT if file else V_P, j1 - 1, i1 - 1]
            kb = g["khalo"] + (2 if (i1 - 1, j1 - 1) in TERRAIN_COLS else 0)
            add(file, elm, float(i1), float(j1), col[kb], typ=22 if file else 1, tag="exact")
            add(file, elm, float(i1), float(j1), col[g["khalo"] + g["nlev"] - 1], typ=22 if file else 1, tag="exact")
    # ri on 1.0 and on nlonh, rj on 1.0 and on nlath
    for file, elm in ((0, ID_T), (0, ID_V), (1, ID_REF), (2, ID_VR), (0, ID_PS)):
        for ri, rj in ((1.0, 2.4), (float(g["nlonh"]), 4.7), (3.3, 1.0), (6.6, float(g["nlath"])), (1.0, 1.0),
                       (float(g["nlonh"]), float(g["nlath"]))):
            lev = itpl_2d(v2[0, V2_TOPO], ri, rj)[0] + 30.0 if elm == ID_PS else lev_at(file, ri, rj, 0.37)
            add(file, elm, ri, rj, lev, typ=22 if file else 1, tag="edge")
    nrow = len(rows)
    off = np.zeros(4, dtype=np.int64)
    files = {n: [] for n in ("elm", "typ", "lev", "ri", "rj", "lon", "lat")}
    set_, idx = np.zeros(nrow, dtype=np.int32), np.zeros(nrow, dtype=np.int32)
    order = rng.permutation(nrow)                                     # the obsda rows name the file rows in no particular order
    pos_in = {}
    for f in range(3):
        mine = [r for r in range(nrow) if rows[r]["file"] == f]
        off[f + 1] = off[f] + len(mine)
        for n, r in enumerate(mine):
            pos_in[r] = (f + 1, n + 1)
            for name in files:
                files[name].append(rows[r][name])
    obsda_rows = [rows[r] for r in order]
    for n, r in enumerate(order):
        set_[n], idx[n] = pos_in[r]
    for r in obsda_rows:
        r["radar"] = None if FILE_RADAR[r["file"]] < 0 else tuple(RADARS[FILE_RADAR[r["file"]]])
    ang = rng.uniform(-0.3, 0.3, size=nrow)
    rotc = np.stack([np.cos(ang), np.sin(ang)], axis=1)
    arr = dict(elm=np.array(files["elm"], dtype=np.int32), typ=np.array(files["typ"], dtype=np.int32),
               **{n: np.array(files[n], dtype=np.float64) for n in ("lev", "ri", "rj", "lon", "lat")})
    return dict(g=g, v3=v3, v2=v2, nmem=nmem, rows=obsda_rows, nrow=nrow, off=off, files=arr, set=set_, idx=idx, rotc=rotc)


_STATEMENT_CACHE = {}


def statement(case, cfg, rotc="case"):
    """The operator on every (row, member) of the case: dict of arrays val [nrow, nmem], qc_m [nrow, nmem], qc [nrow] (the
    maximum), tol, dist, kind.  Conventional rows do not depend on the radar switches: computed once per stggrd."""
    key_r = (id(case), cfg["method_ref_calc"], cfg["use_terminal_velocity"], cfg["stggrd"], rotc)
    key_c = (id(case), cfg["stggrd"], rotc)
    nrow, nmem = case["nrow"], case["nmem"]
    out = dict(val=np.zeros((nrow, nmem)), qc_m=np.zeros((nrow, nmem), dtype=np.int32), tol=np.zeros((nrow, nmem)),
               dist=np.full((nrow, nmem), np.inf), kind=np.empty((nrow, nmem), dtype=object))
    for n, row in enumerate(case["rows"]):
        key = (key_c if row["radar"] is None else key_r) + (n,)
        if key not in _STATEMENT_CACHE:
            rc = tuple(case["rotc"][n]) if rotc == "case" else (1.0, 0.0)
            _STATEMENT_CACHE[key] = [operator(cfg, case["g"], case["v3"][m], case["v2"][m], row, rc) for m in range(nmem)]
        for m, o in enumerate(_STATEMENT_CACHE[key]):
            out["val"][n, m], out["qc_m"][n, m], out["tol"][n, m], out["dist"][n, m], out["kind"][n, m] = (
                o["val"], o["qc"], o["tol"], o["dist"], o["kind"])
    out["qc"] = out["qc_m"].max(axis=1)
    return out


# ------------------------------------------------------------------------------------------------------- the device call
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


class DeviceCase:
    """The case's arrays on the device and the three structs of a call; keeps every host array the structs point to."""

    def __init__(self, pkg, case, cfg, dev, fields=None, strides=None, rotc="case", members=None):
        import torch
        self.pkg, self.case, self.dev = pkg, case, dev
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        g = case["g"]
        a3, a2 = fields if fields is not None else (case["v3"], case["v2"])
        if members is not None:                       # a slice of the members, in the reference layout
            a3, a2 = a3[members[0]:members[0] + members[1]], a2[members[0]:members[0] + members[1]]
        self.d3, self.d2 = t(a3), t(a2)
        self.d = {n: t(v) for n, v in case["files"].items()}
        self.set, self.idx = t(case["set"]), t(case["idx"])
        self.rotc = None if rotc is None else t(case["rotc"] if isinstance(rotc, str) else rotc)
        self.off = np.ascontiguousarray(case["off"], dtype=np.int64)
        self.file_radar = np.ascontiguousarray(case.get("file_radar", FILE_RADAR), dtype=np.int32)
        self.radars = np.ascontiguousarray(case.get("radars", RADARS), dtype=np.float64)
        self.use = np.ascontiguousarray(cfg["use_obs"], dtype=np.int32)
        f = pkg.ObsFileRows()
        f.nfile, f.off = len(self.off) - 1, self.off.ctypes.data_as(C.c_void_p)
        for n in ("elm", "typ", "lev", "ri", "rj", "dat", "err"):
            if n in self.d:
                setattr(f, n, C.c_void_p(self.d[n].data_ptr()))
        self.files = f
        p = pkg.ObsopeParams()
        p.lon, p.lat = C.c_void_p(self.d["lon"].data_ptr()), C.c_void_p(self.d["lat"].data_ptr())
        p.file_radar, p.radar_meta = self.file_radar.ctypes.data_as(C.c_void_p), self.radars.ctypes.data_as(C.c_void_p)
        p.rotc = None if self.rotc is None else C.c_void_p(self.rotc.data_ptr())
        p.use_obs, p.nobtype = self.use.ctypes.data_as(C.c_void_p), len(self.use)
        for n in ("method_ref_calc", "use_terminal_velocity", "stggrd", "min_radar_ref_dbz", "low_ref_shift", "radar_zmax",
                  "ps_adjust_thres", "ri_off", "rj_off"):
            setattr(p, n, cfg[n])
        self.params = p
        fl = pkg.ObsopeFields()
        for n in ("nlev", "nlon", "nlat", "khalo", "ihalo", "jhalo"):
            setattr(fl, n, g[n])
        fl.nv3dd, fl.nv2dd, fl.nmem, fl.m0 = NV3DD, NV2DD, (case["nmem"] if members is None else members[1]), 0
        fl.v3d, fl.v2d = C.c_void_p(self.d3.data_ptr()), C.c_void_p(self.d2.data_ptr())
        for n, v in (strides or reference_strides(g)).items():
            setattr(fl, n, v)
        self.fields = fl

    def run(self, ctx, kld=None, m0=0, row0=0, nrows=None, qc=None, ensval=None, canary=None):
        """One call; returns (ensval [nrow, kld], qc [nrow]) as numpy.  ensval starts as `canary` (default 0), qc as 0."""
        import torch
        nrow = self.case["nrow"]
        kld = kld or (m0 + self.fields.nmem)
        if ensval is None:
            ensval = torch.full((nrow, kld), 0.0 if canary is None else canary, dtype=torch.float64, device=self.dev)
        if qc is None:
            qc = torch.zeros(nrow, dtype=torch.int32, device=self.dev)
        self.fields.m0 = m0
        ctx.obsope(self.params, self.files, self.fields, self.set, self.idx, qc, ensval, kld, row0=row0, nrows=nrows)
        torch.cuda.synchronize()
        return ensval.cpu().numpy(), qc.cpu().numpy()


def compare(got_val, got_qc, st, members=None):
    """The tolerances of tests/test_gpu_obsope.py on every (row, member): list of failures (empty = pass)."""
    bad = []
    if not np.array_equal(got_qc, st["qc"] if members is None else st["qc_m"][:, members].max(axis=1)):
        bad.append(("qc", np.nonzero(got_qc != st["qc"])[0][:10].tolist()))
    cols = range(st["val"].shape[1]) if members is None else members
    for c, m in enumerate(cols):
        for n in range(st["val"].shape[0]):
            kind, want, got = st["kind"][n, m], st["val"][n, m], got_val[n, c]
            ok = got == want if kind in ("zero", "undef", "lowref") else abs(got - want) <= st["tol"][n, m]
            if not ok:
                bad.append((n, m, kind, float(got), float(want), float(st["tol"][n, m])))
    return bad
