"""The departure monitor in numpy / plain Python, written from scale/common/common_scale.f90:1292-1400 (state_to_history) with
:1434-1459 (scale_calc_z) and scale/common/common_obs_scale.f90:1467-1599 (the loop of monit_obs), :1851-1895 (monit_dep),
:1821-1837 (monit_type) and :1899-1948 (monit_print): the CPU statement the device entries of include/letkf_amd_monit.h are
compared with, the seeded fixtures, and the ctypes plumbing of a device call.  The operator itself is _obsope's, unchanged.
tests/test_monit_statement.py anchors the statement to things its author did not write.

Arrays are 0-based: a state is state[v, j, i, k] on the interior (the reference's v3dg(nlev,nlon,nlat,nv3d) read in C order),
the history fields are v3[v, j, i, k] / v2[v, j, i] with halos, as in _obsope.
"""
import ctypes as C
import math

import numpy as np

import _obsope as O

ELEM_UID = np.array([2819, 2820, 3073, 3074, 3330, 3331, 14593, 19999, 4001, 4004, 4002, 4003, 8800, 99991, 99992, 99993],
                    dtype=np.int32)                                                   # common_obs_scale.f90:74-77
OBELMLIST = ["  U", "  V", "  T", " Tv", "  Q", " RH", " PS", "PRC", "REF", "RE0", " Vr", "PRH", "H08", "TCX", "TCY", "TCP"]
ID_H08 = 8800
NSTATE = 11                                                                           # u v w t p q qc qr qi qs qg
WEST, EAST, SOUTH, NORTH = 1, 2, 4, 8


# ------------------------------------------------------------------------------------------------------ state_to_history
def state_to_history(state, topo, cz, ztop, g, edge_fill):
    """(v3, v2, w3, w2): the history fields of one state and the masks of what the call writes (the rest is NaN).
    state[v, j, i, k] with v >= 11 in iv3d_* order, topo[j, i], cz[k]."""
    nk, ni, nj, kh, ih, jh = g["nlev"], g["nlon"], g["nlat"], g["khalo"], g["ihalo"], g["jhalo"]
    a3 = np.zeros((O.NV3DD, nj, ni, nk))
    a3[:NSTATE] = state[:NSTATE]                                                      # :1316-1326
    a3[O.V_HGT] = ((ztop - topo) / ztop)[:, :, None] * cz[None, None, :] + topo[:, :, None]   # scale_calc_z :1452
    a2 = np.zeros((O.NV2DD, nj, ni))
    a2[O.V2_TOPO] = a3[O.V_HGT, :, :, 0]                                              # :1342
    for v2, v in ((O.V2_PS, O.V_P), (O.V2_U10, O.V_U), (O.V2_V10, O.V_V), (O.V2_T2M, O.V_T), (O.V2_Q2M, O.V_Q)):
        a2[v2] = state[v, :, :, 0]                                                    # :1345-1349
    a3 = np.concatenate([np.repeat(a3[..., :1], kh, axis=3), a3, np.repeat(a3[..., -1:], kh, axis=3)], axis=3)   # :1371-1379
    v3 = np.full((O.NV3DD, g["nlath"], g["nlonh"], g["nlevh"]), np.nan)
    v2 = np.full((O.NV2DD, g["nlath"], g["nlonh"]), np.nan)
    v3[:, jh:jh + nj, ih:ih + ni, :] = a3
    v2[:, jh:jh + nj, ih:ih + ni] = a2
    for je in range(g["nlath"]):                                                      # the lateral halo: the library's definition
        for ie in range(g["nlonh"]):
            need = ((WEST if ie < ih else 0) | (EAST if ie >= ih + ni else 0) | (SOUTH if je < jh else 0) |
                    (NORTH if je >= jh + nj else 0))
            if need == 0 or (need & ~edge_fill):
                continue
            ci, cj = min(max(ie, ih), ih + ni - 1), min(max(je, jh), jh + nj - 1)
            v3[:, je, ie, :] = v3[:, cj, ci, :]
            v2[:, je, ie] = v2[:, cj, ci]
    return v3, v2, ~np.isnan(v3), ~np.isnan(v2)


def make_state(g, seed, nv3d=NSTATE, perturb_of=None):
    """A smooth, physically ordered state in the manner of _obsope.make_fields: dict(state [nv3d, j, i, k], topo, cz, ztop).
    perturb_of: another such dict -- the result is that state changed by a few per cent (column-wise smooth in pressure, so
    that it stays monotonic; seeded noise elsewhere), on the same topo / cz / ztop."""
    rng = np.random.default_rng(seed)
    nk, ni, nj = g["nlev"], g["nlon"], g["nlat"]
    jj, ii, _ = np.meshgrid(np.arange(nj), np.arange(ni), np.arange(nk), indexing="ij")
    if perturb_of is not None:
        b = perturb_of
        s = b["state"].copy()
        col = 1.0 + 0.02 * np.sin(1.3 * ii + 0.7 * jj + 0.4)
        for v in range(s.shape[0]):
            s[v] = s[v] * (col if v == O.V_P else 1.0 + 0.03 * rng.uniform(-1.0, 1.0, size=(nj, ni, nk)))
        return dict(state=s, topo=b["topo"], cz=b["cz"], ztop=b["ztop"])
    noise = lambda a: 1.0 + a * rng.uniform(-1.0, 1.0, size=(nj, ni, nk))
    topo = 150.0 + 20.0 * ii[:, :, 0] + 35.0 * jj[:, :, 0] + 10.0 * rng.uniform(-1, 1, size=(nj, ni))
    dz = 9000.0 / nk
    cz = (np.arange(nk) + 0.5) * dz * (1.0 + 0.01 * rng.uniform(-1, 1, size=nk))
    ztop = 9000.0 * 1.07
    z = ((ztop - topo) / ztop)[:, :, None] * cz[None, None, :] + topo[:, :, None]
    s = np.zeros((nv3d, nj, ni, nk))
    s[O.V_P] = 1.0e5 * np.exp(-z / 8000.0) * noise(0.5e-3 if nk > 32 else 2e-3)
    s[O.V_T] = (300.0 - 6.5e-3 * z) * noise(0.003)
    s[O.V_U] = (12.0 + 0.8 * ii - 0.5 * jj + 1.5e-3 * z) * noise(0.05)
    s[O.V_V] = (-7.0 + 0.3 * ii + 0.9 * jj - 1.0e-3 * z) * noise(0.05)
    s[O.V_W] = (0.5 + 0.05 * ii - 0.08 * jj + 1.0e-4 * z) * noise(0.1)
    s[O.V_Q] = 0.012 * np.exp(-z / 3000.0) * noise(0.05)
    hyd = lambda a, b, c, d: np.exp(a + b * ii + c * jj + d * z / 1000.0) * noise(0.1)
    s[O.V_QC] = hyd(-9.0, 0.1, 0.1, -0.1)
    s[O.V_QR] = hyd(-12.5, 0.55, 0.35, -0.25) * (ii < ni - 1)
    s[O.V_QI] = hyd(-12.0, 0.1, 0.1, 0.2)
    s[O.V_QS] = hyd(-14.0, 0.3, 0.6, 0.35) * (ii > 0)
    s[O.V_QG] = hyd(-13.0, 0.5, 0.3, 0.1) * (jj > 0)
    for v in range(NSTATE, nv3d):
        s[v] = rng.uniform(1.0, 2.0, size=(nj, ni, nk))                               # a variable the call must not read
    return dict(state=s, topo=topo, cz=cz, ztop=ztop)


def history(st, g, edge_fill=15):
    """(v3 [1, 13, ...], v2 [1, 7, ...]) of a make_state dict: one member, as _obsope's cases carry them"""
    v3, v2, _, _ = state_to_history(st["state"], st["topo"], st["cz"], st["ztop"], g, edge_fill)
    return v3[None], v2[None]


# ------------------------------------------------------------------------------------------------------------- monit_obs
def default_mcfg(**kw):
    m = dict(departure_stat_radar=1, t_range=0.0, elem_uid=ELEM_UID, key=None)
    m.update(kw)
    return m


def monit_dep(elem_uid, elm, dep, qc):
    """monit_dep :1851-1895 in the reference's sequential order: (nobs, bias, rmse)"""
    nid = len(elem_uid)
    nobs, bias, rmse = np.zeros(nid, dtype=np.int32), np.zeros(nid), np.zeros(nid)
    uid = {int(e): n for n, e in enumerate(elem_uid)}
    for e, d, q in zip(elm, dep, qc):
        if q != 0:
            continue
        e = {O.ID_TV: O.ID_T, O.ID_REF_ZERO: O.ID_REF}.get(int(e), int(e))
        nobs[uid[e]] += 1
        bias[uid[e]] += d
        rmse[uid[e]] += d * d
    for i in range(nid):
        if nobs[i] == 0:
            bias[i] = rmse[i] = O.UNDEF
        else:
            bias[i] = bias[i] / nobs[i]
            rmse[i] = math.sqrt(rmse[i] / nobs[i])
    return nobs, bias, rmse


def _group(e):
    return {O.ID_TV: O.ID_T, O.ID_REF_ZERO: O.ID_REF}.get(int(e), int(e))


_ROW_CACHE = {}


def monit(cfg, mcfg, case, hist, step, rec):
    """monit_obs of one step on the history fields hist = (v3 [1, 13, ...], v2 [1, 7, ...]).  rec: None at step 1, the dict
    a step-1 call returned at step 2.  Returns dict(qc, dep, tol, dist, elm (this step's rows), rec (set, idx, qc, omb, oma),
    nobs, bias, rmse, bias_tol, rmse_tol)."""
    key = np.arange(case["nrow"]) if mcfg["key"] is None else np.asarray(mcfg["key"])
    nn = len(key)
    qc, dep, tol = np.zeros(nn, dtype=np.int32), np.full(nn, O.UNDEF), np.zeros(nn)
    dist, elm = np.full(nn, np.inf), np.zeros(nn, dtype=np.int32)
    tr = mcfg["t_range"]
    for n, r in enumerate(key):
        row = case["rows"][r]
        elm[n] = row["elm"]
        if tr > 0.0:
            dist[n] = abs(abs(row["dif"]) - tr) / max(abs(row["dif"]), tr)
        if tr > 0.0 and abs(row["dif"]) > tr:                                         # :1529-1530
            qc[n] = -1
            continue
        if row["radar"] is not None and not mcfg["departure_stat_radar"]:             # :1548
            qc[n] = O.QC_OTYPE
            continue
        ck = (id(case), id(hist[0]), cfg["method_ref_calc"], cfg["use_terminal_velocity"], cfg["stggrd"], int(r))
        if ck not in _ROW_CACHE:
            _ROW_CACHE[ck] = O.operator(cfg, case["g"], hist[0][0], hist[1][0], row, tuple(case["rotc"][r]))
        o = _ROW_CACHE[ck]
        qc[n], dist[n] = o["qc"], min(dist[n], o["dist"])
        if o["qc"] == 0:                                                              # :1567-1571
            dep[n] = row["dat"] - o["val"]
            tol[n] = o["tol"] + float(np.spacing(abs(dep[n])))
    if step == 1:
        new = dict(set=case["set"][key].copy(), idx=case["idx"][key].copy(), qc=qc.copy(), omb=dep.copy(), oma=None)
    else:
        new = dict(set=rec["set"], idx=rec["idx"], qc=np.where(rec["qc"] == 0, qc, rec["qc"]).astype(np.int32), omb=rec["omb"],
                   oma=dep.copy())                                                    # :1577-1580
    nobs, bias, rmse = monit_dep(mcfg["elem_uid"], elm, dep, qc)
    bias_tol, rmse_tol = np.zeros(len(nobs)), np.zeros(len(nobs))
    for i, e in enumerate(mcfg["elem_uid"]):
        m = (qc == 0) & np.array([_group(x) == int(e) for x in elm])
        if m.any():                                                                   # triangle inequality on the per-row bounds
            bias_tol[i] = tol[m].sum() / m.sum() + 1e-13 * np.abs(dep[m]).mean()
            rmse_tol[i] = math.sqrt((tol[m] ** 2).sum() / m.sum()) + 1e-13 * rmse[i]
    return dict(qc=qc, dep=dep, tol=tol, dist=dist, elm=elm, rec=new, nobs=nobs, bias=bias, rmse=rmse, bias_tol=bias_tol,
                rmse_tol=rmse_tol)


def monit_type(elem_uid, departure_stat_radar, departure_stat_h08):
    """:1821-1837"""
    on = {O.ID_U, O.ID_V, O.ID_T, O.ID_TV, O.ID_Q, O.ID_PS}
    if departure_stat_radar:
        on |= {O.ID_REF, O.ID_REF_ZERO, O.ID_VR}
    if departure_stat_h08:
        on.add(ID_H08)
    return np.array([1 if int(e) in on else 0 for e in elem_uid], dtype=np.int32)


def _es12_3(x):
    """Fortran's ES12.3"""
    s = f"{x:.3E}"
    mant, ex = s.split("E")
    return f"{mant}E{ex[0]}{int(ex[1:]):02d}".rjust(12)


def monit_print(nobs, bias, rmse, mtype, elem_uid=ELEM_UID, names=OBELMLIST):
    """monit_print :1899-1948: the seven lines it WRITEs"""
    cols = [i for i in range(len(elem_uid)) if mtype[i] and int(elem_uid[i]) not in (O.ID_TV, O.ID_REF_ZERO)]
    var = "".join(names[i].rjust(12) for i in cols)
    num = "".join(f"{int(nobs[i]):12d}" for i in cols)
    b = "".join(_es12_3(bias[i]) if nobs[i] > 0 else "N/A".rjust(12) for i in cols)
    r = "".join(_es12_3(rmse[i]) if nobs[i] > 0 else "N/A".rjust(12) for i in cols)
    rule = lambda ch: ch * 6 + (ch * 12) * len(cols)
    return [rule("="), " " * 6 + var, rule("-"), "BIAS  " + b, "RMSE  " + r, "NUMBER" + num, rule("=")]


# ---------------------------------------------------------------------------------------------------------------- fixtures
SEEDS = {8: 21, 70: 23}     # seeds under which no row lies within 1e-6 of a comparison (tests/test_monit_statement.py asserts it)
T_RANGE = 1800.0            # the DEPARTURE_STAT_T_RANGE the fixture's dif is drawn around


def make_case(nlev, seed=None):
    """Grid, two states (guess, analysis), their histories (edge_fill = 15) and about 200 file rows in three files (one
    conventional, two radar) with dat and dif, every row in the owned range."""
    seed = SEEDS.get(nlev, 21) if seed is None else seed
    g = O.make_grid(nlev)
    gues = make_state(g, seed)
    anal = make_state(g, seed + 500, perturb_of=gues)
    hg, ha = history(gues, g), history(anal, g)
    rng = np.random.default_rng(seed + 1000)
    cfg = O.default_cfg(stggrd=1)
    ro, rjo = cfg["ri_off"], cfg["rj_off"]
    ih, jh, ni, nj = g["ihalo"], g["jhalo"], g["nlon"], g["nlat"]
    ilo, ihi, jlo, jhi = ih + 0.5, ih + ni + 0.5, jh + 0.5, jh + nj + 0.5            # the owned range [lo, hi)
    rows = []

    def add(file, elm, ril, rjl, lev, typ=None, lon=None, lat=None, tag=""):
        assert ilo <= ril < ihi and jlo <= rjl < jhi, (ril, rjl)
        rows.append(dict(file=file, elm=elm, typ=(22 if file else 1) if typ is None else typ, lev=float(lev), ri=float(ril) + ro,
                         rj=float(rjl) + rjo, lon=137.0 + 0.07 * ril if lon is None else lon,
                         lat=36.4 + 0.06 * rjl if lat is None else lat, tag=tag))

    def rng_of(h, file, ril, rjl):
        return O._level_range(h[0][0, O.V_HGT if file else O.V_P], file > 0, ril, rjl, g)

    def lev_at(file, ril, rjl, frac, h=hg):
        lo, hi, _ = rng_of(h, file, ril, rjl)
        x = lo + frac * (hi - lo)
        return x if file else math.exp(x)

    def pos(a=None, b=None, c=None, d=None):
        return (rng.uniform(ilo + 0.02 if a is None else a, ihi - 0.02 if b is None else b),
                rng.uniform(jlo + 0.02 if c is None else c, jhi - 0.02 if d is None else d))

    # every element of both formats inside both states' range
    for elm in (O.ID_U, O.ID_V, O.ID_T, O.ID_TV, O.ID_Q, O.ID_RH):
        for n in range(10):
            ri, rj = pos()
            add(0, elm, ri, rj, lev_at(0, ri, rj, rng.uniform(0.1, 0.9)), typ=1 + n % 2, tag="conv")
    for elm, cnt in ((O.ID_REF, 24), (O.ID_VR, 24), (O.ID_REF_ZERO, 8)):
        for n in range(cnt):
            ri, rj = pos()
            add(1 + n % 2, elm, ri, rj, lev_at(1, ri, rj, rng.uniform(0.06, 0.9)), tag="radar")
    # the lateral halo: at least four rows per side whose interpolation reads a halo column, in both formats
    for n in range(5):
        for (a, b, c, d) in ((ilo, ih + 1.0, None, None), (ih + ni + 0.02, ihi - 0.02, None, None), (None, None, jlo, jh + 1.0),
                             (None, None, jh + nj + 0.02, jhi - 0.02)):
            ri, rj = pos(a, b, c, d)
            file, elm = ((0, O.ID_T), (0, O.ID_Q), (1, O.ID_REF), (2, O.ID_VR), (0, O.ID_PS))[n]
            lev = O.itpl_2d(hg[1][0, O.V2_TOPO], ri, rj)[0] + 20.0 if elm == O.ID_PS else lev_at(file, ri, rj, rng.uniform(0.2, 0.8))
            add(file, elm, ri, rj, lev, tag="halo")
    # U / V rows whose staggered read alone reaches the west / south halo
    for n in range(4):
        ri, rj = pos(ih + 1.02, ih + 1.48)
        add(0, O.ID_U, ri, rj, lev_at(0, ri, rj, rng.uniform(0.2, 0.8)), tag="stagger")
        ri, rj = pos(None, None, jh + 1.02, jh + 1.48)
        add(0, O.ID_V, ri, rj, lev_at(0, ri, rj, rng.uniform(0.2, 0.8)), tag="stagger")
        ri, rj = pos(ih + 1.02, ih + 1.48)
        add(1 + n % 2, O.ID_VR, ri, rj, lev_at(1, ri, rj, rng.uniform(0.2, 0.8)), tag="stagger")
    # PS on both sides of PS_ADJUST_THRES
    for n in range(12):
        ri, rj = pos()
        topo = O.itpl_2d(hg[1][0, O.V2_TOPO], ri, rj)[0]
        add(0, O.ID_PS, ri, rj, topo + (rng.uniform(-80, 80) if n % 2 else rng.uniform(120, 300) * (1 if n % 4 else -1)), tag="ps")
    # too high and too low in both states; unknown elements
    for file, elm in ((0, O.ID_T), (1, O.ID_REF), (2, O.ID_VR)):
        for frac in (1.2, -0.25, 1.1, -0.15):
            ri, rj = pos()
            add(file, elm, ri, rj, lev_at(file, ri, rj, frac), tag="vbound")
    for file, elm in ((0, 1234), (0, O.ID_RAIN), (1, O.ID_U), (2, O.ID_PRH), (0, ID_H08)):
        ri, rj = pos()
        add(file, elm, ri, rj, 0.0 if elm == O.ID_RAIN else lev_at(file, ri, rj, 0.5), tag="unknown")
    # between the two states' tops (pressure): good in one state, too high in the other -- both ways round
    for n in range(12):
        ri, rj = pos()
        top_g, top_a = rng_of(hg, 0, ri, rj)[1], rng_of(ha, 0, ri, rj)[1]
        add(0, (O.ID_T, O.ID_Q, O.ID_U)[n % 3], ri, rj, math.exp(0.5 * (top_g + top_a)), tag="flip")
    nrow = len(rows)
    # dat: near the guess's H(x) where there is one; dif: a fifth of the rows beyond T_RANGE
    for r in rows:
        r["radar"] = None if O.FILE_RADAR[r["file"]] < 0 else tuple(O.RADARS[O.FILE_RADAR[r["file"]]])
    ang = rng.uniform(-0.3, 0.3, size=nrow)
    for r in rows:
        o = O.operator(cfg, g, hg[0][0], hg[1][0], r, (1.0, 0.0))
        base = o["val"] if o["kind"] not in ("zero", "undef") else 1.0
        r["dat"] = float(base + rng.normal() * max(0.02 * abs(base), 1e-4 if r["elm"] == O.ID_Q else 0.5))
        r["dif"] = float(rng.choice([-1.0, 1.0]) * (rng.uniform(2000.0, 3000.0) if rng.uniform() < 0.2 else rng.uniform(0.0, 1500.0)))
    off = np.zeros(4, dtype=np.int64)
    names = ("elm", "typ", "lev", "ri", "rj", "lon", "lat", "dat", "dif")
    files = {n: [] for n in names}
    set_, idx = np.zeros(nrow, dtype=np.int32), np.zeros(nrow, dtype=np.int32)
    order = rng.permutation(nrow)                                     # the obsda rows name the file rows in no particular order
    pos_in = {}
    for f in range(3):
        mine = [r for r in range(nrow) if rows[r]["file"] == f]
        off[f + 1] = off[f] + len(mine)
        for n, r in enumerate(mine):
            pos_in[r] = (f + 1, n + 1)
            for name in names:
                files[name].append(rows[r][name])
    obsda_rows = [rows[r] for r in order]
    for n, r in enumerate(order):
        set_[n], idx[n] = pos_in[r]
    rotc = np.stack([np.cos(ang), np.sin(ang)], axis=1)
    arr = dict(elm=np.array(files["elm"], dtype=np.int32), typ=np.array(files["typ"], dtype=np.int32),
               **{n: np.array(files[n], dtype=np.float64) for n in names[2:]})
    return dict(g=g, gues=gues, anal=anal, hist=(hg, ha), v3=hg[0], v2=hg[1], nmem=1, rows=obsda_rows, nrow=nrow, off=off,
                files=arr, set=set_, idx=idx, rotc=rotc, cfg=cfg)


_CASES = {}


def case(nlev):
    if nlev not in _CASES:
        _CASES[nlev] = make_case(nlev)
    return _CASES[nlev]


# ------------------------------------------------------------------------------------------------------- the device calls
def hist_layout(pkg, g, strides=None):
    """letkf_obsope_fields for one member on grid g (reference strides by default), without the pointers"""
    fl = pkg.ObsopeFields()
    for n in ("nlev", "nlon", "nlat", "khalo", "ihalo", "jhalo"):
        setattr(fl, n, g[n])
    fl.nv3dd, fl.nv2dd, fl.nmem, fl.m0 = O.NV3DD, O.NV2DD, 1, 0
    for n, v in (strides or O.reference_strides(g)).items():
        setattr(fl, n, v)
    return fl


class DeviceState:
    """A make_state dict on the device in one of the two layouts, and its letkf_hist_state"""

    def __init__(self, pkg, st, dev, layout="point", edge_fill=15):
        import torch
        s = st["state"]
        nv, nj, ni, nk = s.shape
        if layout == "point":                          # gues3d(ij, lev, v): point-fastest
            a = np.ascontiguousarray(np.transpose(s, (0, 3, 1, 2)))                  # [v, k, j, i]
            si, sj, sl, sv = 1, ni, ni * nj, ni * nj * nk
        else:                                          # v3dg(nlev, nlon, nlat, nv3d): level-fastest
            a = np.ascontiguousarray(s)                                              # [v, j, i, k]
            si, sj, sl, sv = nk, nk * ni, 1, nk * ni * nj
        self.x = torch.from_numpy(a).to(dev)
        self.topo = torch.from_numpy(np.ascontiguousarray(st["topo"])).to(dev)
        self.cz = np.ascontiguousarray(st["cz"], dtype=np.float64)
        h = pkg.HistState()
        h.nv3d, h.edge_fill, h.x = nv, edge_fill, C.c_void_p(self.x.data_ptr())
        h.si, h.sj, h.sl, h.sv = si, sj, sl, sv
        h.topo, h.cz, h.ztop = C.c_void_p(self.topo.data_ptr()), self.cz.ctypes.data_as(C.c_void_p), st["ztop"]
        self.hs = h


def monit_structs(pkg, dc, mcfg, step, nn, dev, rec=None, canary=None):
    """(MonitParams, Obsdep, record tensors dict, kept host arrays) for a call on the _obsope.DeviceCase dc"""
    import torch
    ids = np.ascontiguousarray(mcfg["elem_uid"], dtype=np.int32)
    mp = pkg.MonitParams()
    mp.step, mp.departure_stat_radar, mp.nid, mp.reserved0 = step, int(mcfg["departure_stat_radar"]), len(ids), 0
    mp.elem_uid, mp.t_range = ids.ctypes.data_as(C.c_void_p), mcfg["t_range"]
    mp.dif = C.c_void_p(dc.d["dif"].data_ptr()) if "dif" in dc.d else None
    if rec is None:
        ci, cd = (0, 0.0) if canary is None else canary
        rec = dict(set=torch.full((max(nn, 1),), ci, dtype=torch.int32, device=dev), idx=torch.full((max(nn, 1),), ci, dtype=torch.int32, device=dev),
                   qc=torch.full((max(nn, 1),), ci, dtype=torch.int32, device=dev),
                   omb=torch.full((max(nn, 1),), cd, dtype=torch.float64, device=dev),
                   oma=torch.full((max(nn, 1),), cd, dtype=torch.float64, device=dev))
    od = pkg.Obsdep()
    for n in ("set", "idx", "qc", "omb", "oma"):
        setattr(od, n, C.c_void_p(rec[n].data_ptr()))
    return mp, od, rec, ids


def run_monit(pkg, ctx, dc, mcfg, step, dev, rec=None, canary=None):
    """One letkf_monit_obs_dev call on dc's fields: dict(rec (numpy), nobs, bias, rmse, rec_t (the tensors, for step 2))"""
    import torch
    key = mcfg["key"]
    nn = dc.case["nrow"] if key is None else len(key)
    key_t = None if key is None else torch.from_numpy(np.ascontiguousarray(key, dtype=np.int32)).to(dev)
    mp, od, rec_t, ids = monit_structs(pkg, dc, mcfg, step, nn, dev, rec, canary)
    nobs, bias, rmse = ctx.monit_obs(mp, dc.params, dc.files, dc.fields, dc.set, dc.idx, od, key=key_t, nn=nn)
    torch.cuda.synchronize()
    return dict(rec={n: t.cpu().numpy()[:nn] for n, t in rec_t.items()}, rec_t=rec_t, nobs=nobs.cpu().numpy(),
                bias=bias.cpu().numpy(), rmse=rmse.cpu().numpy())


def compare(got, st, step):
    """The tolerances of tests/test_gpu_monit.py: list of failures (empty = pass)"""
    bad = []
    want = st["rec"]
    for n in ("set", "idx", "qc"):
        if not np.array_equal(got["rec"][n], want[n]):
            bad.append((n, np.nonzero(got["rec"][n] != want[n])[0][:10].tolist()))
    g_dep, w_dep = (got["rec"]["omb"], want["omb"]) if step == 1 else (got["rec"]["oma"], want["oma"])
    for n in range(len(w_dep)):
        ok = g_dep[n] == w_dep[n] if st["qc"][n] != 0 else abs(g_dep[n] - w_dep[n]) <= st["tol"][n]
        if not ok:
            bad.append((n, int(st["qc"][n]), float(g_dep[n]), float(w_dep[n]), float(st["tol"][n])))
    if step == 2 and not np.array_equal(got["rec"]["omb"], want["omb"]):
        bad.append(("omb changed",))
    if not np.array_equal(got["nobs"], st["nobs"]):
        bad.append(("nobs", got["nobs"].tolist(), st["nobs"].tolist()))
    for i in range(len(st["nobs"])):
        if st["nobs"][i] == 0:
            if got["bias"][i] != O.UNDEF or got["rmse"][i] != O.UNDEF:
                bad.append(("undef", i))
        else:
            if abs(got["bias"][i] - st["bias"][i]) > st["bias_tol"][i]:
                bad.append(("bias", i, float(got["bias"][i]), float(st["bias"][i]), float(st["bias_tol"][i])))
            if abs(got["rmse"][i] - st["rmse"][i]) > st["rmse_tol"][i]:
                bad.append(("rmse", i, float(got["rmse"][i]), float(st["rmse"][i]), float(st["rmse_tol"][i])))
    return bad
