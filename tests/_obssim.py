"""obssim_cal in numpy / plain Python, written from scale/obs/obsope_tools.f90:1090-1146 (the loop nest) and :1184-1204 (the record
order of write_grd_mpi): the CPU statement the device entry letkf_obssim_dev (include/letkf_amd_obssim.h) is compared with, the
seeded fixtures, and the ctypes plumbing of a device call.  The point operators Trans_XtoY (common_obs_scale.f90:264-338) and
Trans_XtoY_radar (:342-493) are composed of the pieces of tests/_obsope.py -- itpl_3d, itpl_2d, radar_angles, calc_ref_vr,
prsadj, Branches -- and carry that file's tolerances (the docstring of tests/test_gpu_obsope.py derives them).
tests/test_obssim_statement.py anchors the statement to _obsope.operator, which it does not share its control flow with.

Arrays are 0-based: v3[s, v, j, i, k] and v2[s, v, j, i] with halo as in _obsope; lon, lat [nlat, nlon] and rotc [nlat, nlon, 2]
over the interior; outputs val3[s, n, j, i, k] and val2[s, n, j, i].  Coordinates ri, rj, rk stay 1-based as in the reference.
"""
import ctypes as C
import math

import numpy as np

from _obsope import (EPS, FVIRT, GG, ID_PRH, ID_PS, ID_Q, ID_REF, ID_REF_ZERO, ID_RH, ID_T, ID_TV, ID_U, ID_V, ID_VR, NV2DD, NV3DD,
                     QC_OTYPE, QC_OUT_H, QC_PS_TER, RD, TERRAIN_COLS, UNDEF, V2_PS, V2_Q2M, V2_T2M, V2_TOPO, V_HGT, V_P, V_Q, V_QG,
                     V_QR, V_QS, V_RH, V_T, V_U, V_V, V_W, Branches, calc_ref_vr, itpl_2d, itpl_3d, make_fields, make_grid, prsadj,
                     radar_angles, reference_strides)

RADAR_IDS = (ID_REF, ID_REF_ZERO, ID_VR, ID_PRH)
EXACT_KINDS = ("pass", "undef", "lowref")
RADAR = (136.5, 35.9, 300.0)                       # OBSSIM_RADAR_LON / _LAT / _Z
ON_RADAR = (1, 1)                                  # interior (j, i) of the column placed exactly on the radar, where the grid has it


def default_cfg(**kw):
    c = dict(method_ref_calc=2, use_terminal_velocity=1, stggrd=0, min_radar_ref_dbz=5.0, low_ref_shift=-5.0, ps_adjust_thres=100.0)
    c.update(kw)
    return c


def trans_xtoy(cfg, v3, v2, elm, ri, rj, rk, rotc, br):
    """Trans_XtoY: dict(val, qc, kind, tol).  kind 'pass': an interpolation that reduces to one term of weight 1 (exact)."""
    stg = cfg["stggrd"] == 1
    ulp = lambda x: 4.0 * EPS * abs(x)
    out = lambda **kw: kw
    if elm in (ID_U, ID_V):
        u, su = itpl_3d(v3[V_U], rk, ri - 0.5 if stg else ri, rj)
        v, sv = itpl_3d(v3[V_V], rk, ri, rj - 0.5 if stg else rj)
        val = u * rotc[0] - v * rotc[1] if elm == ID_U else u * rotc[1] + v * rotc[0]
        a, b = (abs(rotc[0]), abs(rotc[1])) if elm == ID_U else (abs(rotc[1]), abs(rotc[0]))
        plain = not stg and rotc == (1.0, 0.0)
        return out(val=val, qc=0, kind="pass" if plain else "interp", tol=64.0 * EPS * (su * a + sv * b) + ulp(su * a + sv * b))
    if elm in (ID_T, ID_Q, ID_RH):
        val, s = itpl_3d(v3[{ID_T: V_T, ID_Q: V_Q, ID_RH: V_RH}[elm]], rk, ri, rj)
        return out(val=val, qc=0, kind="pass", tol=64.0 * EPS * s)
    if elm == ID_TV:
        t, st = itpl_3d(v3[V_T], rk, ri, rj)
        q, sq = itpl_3d(v3[V_Q], rk, ri, rj)
        val = t * (1.0 + FVIRT * q)
        return out(val=val, qc=0, kind="interp", tol=64.0 * EPS * (st * (1.0 + FVIRT * abs(q)) + abs(t) * FVIRT * sq) + ulp(val))
    if elm == ID_PS:
        t, st = itpl_2d(v2[V2_T2M], ri, rj)
        q, sq = itpl_2d(v2[V2_Q2M], ri, rj)
        topo, sz = itpl_2d(v2[V2_TOPO], ri, rj)
        ps, sp = itpl_2d(v2[V2_PS], ri, rj)
        dz = rk - topo                                              # a level index minus metres: the reference's own
        br.cmp(rk, topo, True)
        val = prsadj(ps, dz, t, q)
        br.cmp(abs(dz), cfg["ps_adjust_thres"])
        gam, c = 5.0e-3, GG / (5.0e-3 * RD)
        tv = t * (1.0 + 0.608 * q)
        ratio = (-gam * dz + tv) / tv
        d_ps = ratio ** c
        d_topo = abs(ps) * c * ratio ** (c - 1.0) * gam / tv
        d_tv = abs(ps) * c * ratio ** (c - 1.0) * abs(gam * dz) / (tv * tv)
        e = 64.0 * EPS
        tol = (d_ps * e * sp + d_topo * e * sz + d_tv * ((1.0 + 0.608 * abs(q)) * e * st + 0.608 * abs(t) * e * sq)
               + 64.0 * EPS * abs(val))
        return out(val=val, qc=QC_PS_TER if abs(dz) > cfg["ps_adjust_thres"] else 0, kind="ps", tol=tol)
    return out(val=UNDEF, qc=QC_OTYPE, kind="undef", tol=0.0)


def trans_xtoy_radar(cfg, v3, elm, radar, ri, rj, rk, lon, lat, lev, rotc, br):
    """Trans_XtoY_radar with obssim_cal's `if (tmpqc == iqc_ref_low) tmpqc = iqc_good` applied: dict(val, qc, kind, tol)"""
    stg = cfg["stggrd"] == 1
    out = lambda **kw: kw
    ut, _ = itpl_3d(v3[V_U], rk, ri - 0.5 if stg else ri, rj)
    vt, _ = itpl_3d(v3[V_V], rk, ri, rj - 0.5 if stg else rj)
    wr, _ = itpl_3d(v3[V_W], rk - 0.5 if stg else rk, ri, rj)
    tr, _ = itpl_3d(v3[V_T], rk, ri, rj)
    pr, _ = itpl_3d(v3[V_P], rk, ri, rj)
    qrr, sr = itpl_3d(v3[V_QR], rk, ri, rj)
    qsr, ss = itpl_3d(v3[V_QS], rk, ri, rj)
    qgr, sg = itpl_3d(v3[V_QG], rk, ri, rj)
    ur = ut * rotc[0] - vt * rotc[1]
    vr_ = ut * rotc[1] + vt * rotc[0]
    rlon, rlat, rz = radar
    if lon - rlon == 0.0 and lat - rlat == 0.0:
        return out(val=UNDEF, qc=QC_OUT_H, kind="undef", tol=0.0)
    az, elev = radar_angles(lon, lat, lev, rlon, rlat, rz, br)
    ref, rv, wt, _ = calc_ref_vr(cfg["method_ref_calc"], cfg["use_terminal_velocity"], qrr, qsr, qgr, ur, vr_, wr, tr, pr, az, elev,
                                 br, (sr == 0.0, ss == 0.0, sg == 0.0))
    min_ref = 10.0 ** (cfg["min_radar_ref_dbz"] / 10.0)
    if elm in (ID_REF, ID_REF_ZERO, ID_VR):
        br.cmp(ref, min_ref)
    if elm in (ID_REF, ID_REF_ZERO):
        if ref < min_ref:
            return out(val=cfg["min_radar_ref_dbz"] + cfg["low_ref_shift"], qc=0, kind="lowref", tol=0.0)      # qc 11 -> 0
        return out(val=10.0 * math.log10(ref), qc=0, kind="dbz", tol=1e-11)
    if elm == ID_VR:
        return out(val=rv, qc=0, kind="vr", tol=1e-9 * (abs(ur) + abs(vr_) + abs(wr) + wt))
    return out(val=UNDEF, qc=QC_OTYPE, kind="undef", tol=0.0)


def statement(case, cfg, vars3, vars2, round_single=False, rotc=True, states=None):
    """obsope_tools.f90:1090-1146 over every state: dict of val3 [ns, n3, nlat, nlon, nlev], kind3, tol3, terrain3 (radar values
    computed from below-ground numbers), val2 [ns, n2, nlat, nlon], kind2, tol2 and dist (the closest comparison taken)."""
    g = case["g"]
    nlev, nlon, nlat, kh, ih, jh = g["nlev"], g["nlon"], g["nlat"], g["khalo"], g["ihalo"], g["jhalo"]
    states = range(case["v3"].shape[0]) if states is None else states
    ns, n3, n2 = len(states), len(vars3), len(vars2)
    o = dict(val3=np.zeros((ns, n3, nlat, nlon, nlev)), tol3=np.zeros((ns, n3, nlat, nlon, nlev)),
             kind3=np.empty((ns, n3, nlat, nlon, nlev), dtype=object), terrain3=np.zeros((ns, n3, nlat, nlon, nlev), dtype=bool),
             val2=np.zeros((ns, n2, nlat, nlon)), tol2=np.zeros((ns, n2, nlat, nlon)), kind2=np.empty((ns, n2, nlat, nlon), dtype=object))
    br = Branches()
    undef = float(np.float32(UNDEF)) if round_single else UNDEF
    store = lambda r: (float(np.float32(r["val"])) if round_single else r["val"]) if r["qc"] == 0 else undef
    for si, s in enumerate(states):
        v3, v2 = case["v3"][s], case["v2"][s]
        for j in range(nlat):
            rj = float(j + 1 + jh)
            for i in range(nlon):
                ri = float(i + 1 + ih)
                lon, lat = float(case["lon"][j, i]), float(case["lat"][j, i])
                rc = (float(case["rotc"][j, i, 0]), float(case["rotc"][j, i, 1])) if rotc else (1.0, 0.0)
                for k in range(nlev):
                    rk = float(k + 1 + kh)
                    for n, elm in enumerate(vars3):
                        if elm in RADAR_IDS:
                            lev = float(v3[V_HGT, j + jh, i + ih, k + kh])
                            r = trans_xtoy_radar(cfg, v3, elm, case["radar"], ri, rj, rk, lon, lat, lev, rc, br)
                            o["terrain3"][si, n, j, i, k] = lev == UNDEF
                        else:
                            r = trans_xtoy(cfg, v3, v2, elm, ri, rj, rk, rc, br)
                        o["val3"][si, n, j, i, k], o["tol3"][si, n, j, i, k] = store(r), r["tol"]
                        o["kind3"][si, n, j, i, k] = r["kind"] if r["qc"] == 0 else "undef"
                    if k == 0:
                        for n, elm in enumerate(vars2):
                            r = trans_xtoy(cfg, v3, v2, elm, ri, rj, rk, rc, br)
                            o["val2"][si, n, j, i], o["tol2"][si, n, j, i] = store(r), r["tol"]
                            o["kind2"][si, n, j, i] = r["kind"] if r["qc"] == 0 else "undef"
    o["dist"] = br.dist
    return o


def rec_index(s, r, j, i, nrec, nlat, nlon):
    return ((s * nrec + r) * nlat + j) * nlon + i


def records(val3, val2):
    """write_grd_mpi's records of one subdomain as float32 [ns, nrec, nlat, nlon] (x fastest), by the index formula"""
    ns, n3, nlat, nlon, nlev = val3.shape
    n2 = val2.shape[1]
    rec = np.zeros((ns, n3 * nlev + n2, nlat, nlon), dtype=np.float32)
    with np.errstate(over="ignore"):                 # (what the physics makes of below-ground numbers may leave single precision)
        for n in range(n3):
            for k in range(nlev):
                rec[:, n * nlev + k] = val3[:, n, :, :, k].astype(np.float32)
        for n in range(n2):
            rec[:, n3 * nlev + n] = val2[:, n].astype(np.float32)
    return rec


# ---------------------------------------------------------------------------------------------------------------- fixtures
# name: (nlev, nlon, nlat, khalo, ihalo, jhalo, seed).  Under these seeds no point lies within 1e-6 of a comparison the statement
# takes (tests/test_obssim_statement.py asserts it).
GRIDS = {
    "8x5x3": (8, 5, 3, 2, 2, 2, 7),             # the operator's fixture sizes: partial waves ...
    "70x5x3": (70, 5, 3, 2, 2, 2, 9),           # ... a row of 350 lanes, more than 64 levels
    "64x4x2": (64, 4, 2, 2, 2, 2, 11),          # every wave exactly full
    "1x1x1": (1, 1, 1, 2, 2, 2, 13),
    "8x5x3-nohalo": (8, 5, 3, 1, 0, 0, 15),     # the clamped edge reads under stggrd = 1
}
NSTATE = 2
VARS3 = (ID_REF, ID_VR, ID_U, ID_V, ID_T, ID_TV, ID_Q, ID_RH, ID_REF_ZERO, ID_PRH, ID_PS)
VARS2 = (ID_PS, ID_T, ID_U, ID_REF, ID_Q)
_CASES = {}


def make_case(name):
    """Grid, NSTATE states of make_fields, the interior's lon / lat (one column exactly on the radar), seeded rotc."""
    if name in _CASES:
        return _CASES[name]
    nlev, nlon, nlat, kh, ih, jh, seed = GRIDS[name]
    if jh == 0:      # make_fields names its terrain columns up to row 3: build one halo row more and cut it off again
        gb = make_grid(nlev, khalo=kh, nlon=nlon, nlat=nlat, ihalo=ih, jhalo=1)
        v3, v2 = make_fields(gb, NSTATE, seed)
        v3, v2 = np.ascontiguousarray(v3[:, :, 1:-1]), np.ascontiguousarray(v2[:, :, 1:-1])
        terrain = [(i, j - 1) for (i, j) in TERRAIN_COLS]
    else:
        v3, v2 = make_fields(make_grid(nlev, khalo=kh, nlon=nlon, nlat=nlat, ihalo=ih, jhalo=jh), NSTATE, seed)
        terrain = list(TERRAIN_COLS)
    g = make_grid(nlev, khalo=kh, nlon=nlon, nlat=nlat, ihalo=ih, jhalo=jh)
    jj, ii = np.meshgrid(np.arange(nlat), np.arange(nlon), indexing="ij")
    lon = 137.0 + 0.07 * (ii + 1.0 + ih)
    lat = 36.4 + 0.06 * (jj + 1.0 + jh)
    on_radar = ON_RADAR if (nlat > ON_RADAR[0] and nlon > ON_RADAR[1]) else None
    if on_radar:
        lon[on_radar], lat[on_radar] = RADAR[0], RADAR[1]
    ang = np.random.default_rng(seed + 2000).uniform(-0.3, 0.3, size=(nlat, nlon))
    rotc = np.stack([np.cos(ang), np.sin(ang)], axis=2)
    # interior terrain points: (j, i) interior indices of the columns whose two lowest model levels are below ground
    tcols = [(j - jh, i - ih) for (i, j) in terrain if 0 <= j - jh < nlat and 0 <= i - ih < nlon]
    case = dict(g=g, v3=v3, v2=v2, lon=lon, lat=lat, rotc=rotc, radar=RADAR, on_radar=on_radar, terrain_cols=tcols,
                nterrain=len(tcols) * min(2, nlev), name=name)
    _CASES[name] = case
    return case


_STATEMENTS = {}


def cached_statement(name, cfg, vars3=VARS3, vars2=VARS2, rotc=True):
    key = (name, tuple(sorted(cfg.items())), tuple(vars3), tuple(vars2), rotc)
    if key not in _STATEMENTS:
        _STATEMENTS[key] = statement(make_case(name), cfg, vars3, vars2, rotc=rotc)
    return _STATEMENTS[key]


# ------------------------------------------------------------------------------------------------------- the device call
class DeviceCase:
    """The case's arrays on the device and the two structs of a call; keeps what the structs point to."""

    def __init__(self, pkg, case, cfg, vars3, vars2, dev, rotc=True, fields=None, strides=None, states=None, round_single=0):
        import torch
        self.pkg, self.case, self.dev = pkg, case, dev
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        g = case["g"]
        a3, a2 = fields if fields is not None else (case["v3"], case["v2"])
        if states is not None:
            a3, a2 = a3[states[0]:states[0] + states[1]], a2[states[0]:states[0] + states[1]]
        self.ns = NSTATE if states is None else states[1]
        self.d3, self.d2, self.lon, self.lat = t(a3), t(a2), t(case["lon"]), t(case["lat"])
        self.rotc = t(case["rotc"]) if rotc else None
        p = pkg.ObssimParams()
        p.nvar3, p.nvar2 = len(vars3), len(vars2)
        for n, e in enumerate(vars3[:16]):
            p.vars3[n] = e
        for n, e in enumerate(vars2[:16]):
            p.vars2[n] = e
        p.radar_lon, p.radar_lat, p.radar_z = case["radar"]
        p.lon, p.lat = C.c_void_p(self.lon.data_ptr()), C.c_void_p(self.lat.data_ptr())
        p.rotc = None if self.rotc is None else C.c_void_p(self.rotc.data_ptr())
        for n in ("method_ref_calc", "use_terminal_velocity", "stggrd", "min_radar_ref_dbz", "low_ref_shift", "ps_adjust_thres"):
            setattr(p, n, cfg[n])
        p.round_single = round_single
        self.params = p
        fl = pkg.ObsopeFields()
        for n in ("nlev", "nlon", "nlat", "khalo", "ihalo", "jhalo"):
            setattr(fl, n, g[n])
        fl.nv3dd, fl.nv2dd, fl.nmem, fl.m0 = NV3DD, NV2DD, self.ns, 0
        fl.v3d, fl.v2d = C.c_void_p(self.d3.data_ptr()), C.c_void_p(self.d2.data_ptr())
        for n, v in (strides or reference_strides(g)).items():
            setattr(fl, n, v)
        self.fields = fl
        self.n3, self.n2 = len(vars3), len(vars2)

    def outputs(self, want=("v3", "v2", "rec"), canary=-777.0):
        import torch
        g = self.case["g"]
        shape = dict(v3=(self.ns, self.n3, g["nlat"], g["nlon"], g["nlev"]), v2=(self.ns, self.n2, g["nlat"], g["nlon"]),
                     rec=(self.ns, self.n3 * g["nlev"] + self.n2, g["nlat"], g["nlon"]))
        return {n: (torch.full(shape[n], canary, dtype=torch.float32 if n == "rec" else torch.float64, device=self.dev)
                    if n in want else None) for n in ("v3", "v2", "rec")}

    def run(self, ctx, want=("v3", "v2", "rec")):
        """One call; returns dict of numpy arrays (None where not asked for)."""
        import torch
        out = self.outputs(want)
        ctx.obssim(self.params, self.fields, out["v3"], out["v2"], out["rec"])
        torch.cuda.synchronize()
        return {n: (None if v is None else v.cpu().numpy()) for n, v in out.items()}


def compare(got3, got2, st, exclude_terrain=True):
    """The statement's tolerances on every value: (failures, worst error / tolerance per kind, excluded count)."""
    bad, worst, excluded = [], {}, 0
    for got, val, tol, kind, terr in ((got3, st["val3"], st["tol3"], st["kind3"], st["terrain3"]),
                                      (got2, st["val2"], st["tol2"], st["kind2"], None)):
        if got is None:
            continue
        for ix in np.ndindex(val.shape):
            kd = kind[ix]
            if terr is not None and terr[ix] and exclude_terrain:
                excluded += 1
                continue
            g_, w_ = float(got[ix]), float(val[ix])
            if kd in EXACT_KINDS:
                ok = g_ == w_ or (g_ != g_ and w_ != w_)
                ratio = 0.0 if ok else math.inf
            else:
                err = abs(g_ - w_)
                ok = err <= tol[ix]
                ratio = err / tol[ix] if tol[ix] > 0.0 else (0.0 if err == 0.0 else math.inf)
            worst[kd] = max(worst.get(kd, 0.0), ratio)
            if not ok:
                bad.append((ix, kd, g_, w_, float(tol[ix])))
    return bad, worst, excluded
