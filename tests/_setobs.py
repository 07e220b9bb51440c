"""set_letkf_obs behind one call (include/letkf_amd.h section 9): synthetic observation files + obsda for a world of
subdomains, and the reference answer -- tests/native/setobs_oracle.c (pre-processing, ctype tables, mesh sizes, count
tables) composed with the oracle's departure, bucket sort and extended-subdomain plan (oracle/letkf_oracle.c) and plain
numpy indexing for the gathers."""
import ctypes as C
import os
import subprocess

import numpy as np

import _oracle
from _obsprep import HaloLayout, Mesh, QcParams, fill, qc_params

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "setobs_oracle.c")
SO = os.path.join(HERE, "native", "libsetobs_oracle.so")
NID_OBS, NOBTYPE = 16, 24
ELEM_UID = [2819, 2820, 3073, 3074, 3330, 3331, 14593, 19999, 4001, 4004, 4002, 4003, 8800, 99991, 99992, 99993]
UID = {e: i + 1 for i, e in enumerate(ELEM_UID)}
UNDEF = -9.99e33

_lib = None


def lib():
    global _lib
    if _lib is None:
        if (not os.path.exists(SO)) or os.path.getmtime(SO) < os.path.getmtime(SRC):
            subprocess.check_call(["gcc", "-O2", "-fPIC", "-shared", "-std=c11", "-Wall", "-o", SO, SRC, "-lm"])
        _lib = C.CDLL(SO)
        _lib.orc_obs_preprocess.restype = C.c_int
        _lib.orc_ctype_tables.restype = C.c_int
    return _lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def namelist(**over):
    """Per-report-type namelist values: type 1 ADPUPA the default mesh (hori_loc-derived), type 8 ADPSFC an explicit
    OBS_SORT_GRID_SPACING, type 22 PHARAD a MAX_NOBS_PER_GRID with OBS_MIN_SPACING, type 23 H08IRB the default."""
    hl = np.full(NOBTYPE, 3000.0)
    hl[[0, 7, 21, 22]] = [4000.0, 5000.0, 2500.0, 3500.0]
    vl = np.full(NOBTYPE, 0.4)
    vl[21] = 3000.0
    spc = np.zeros(NOBTYPE)
    spc[7] = 3000.0
    mx = np.zeros(NOBTYPE, np.int32)
    mx[21] = 40
    ms = np.full(NOBTYPE, 300.0)
    d = dict(hori_local=hl, vert_local=vl, obs_sort_grid_spacing=spc, max_nobs_per_grid=mx, obs_min_spacing=ms,
             min_radar_ref_dbz=5.0, low_ref_shift=-1.0, use_obserr_radar_ref=1, obserr_radar_ref=5.0,
             use_obserr_radar_vr=1, obserr_radar_vr=3.0, hori_local_radar_obsnoref=2000.0, hori_local_radar_vr=2200.0,
             vert_local_radar_vr=2500.0, dx=1000.0, dy=1000.0, rain_base=85000.0, criterion=1)
    d.update(over)
    return d


def make_world(seed, px=1, py=1, nlon=12, nlat=12, k=10, det_run=True, nfile_rows=(3000, 1500), h08=False, ihalo=2,
               qc_reject=0.1):
    """Two observation files over a (px*nlon) x (py*nlat) domain.  File 1 (radar, type 22): raw reflectivities in mW
    units (below MIN_RADAR_REF, >= 1e10, negative, ordinary), rows already typed 4004, radial velocities.  File 2: upper-air u
    (type 1), surface pressure (type 8), upper-air T (type 1) that no obsda row references, and -- h08 -- Himawari-8 IR
    (type 23).  Rank r = (r % px, r // px) holds the referenced rows inside its subdomain as obsda rows."""
    rng = np.random.default_rng(seed)
    files = []
    n1, n2 = nfile_rows
    gx, gy = px * nlon, py * nlat
    kind1 = rng.choice(3, n1, p=[0.6, 0.1, 0.3])
    elm1 = np.array([4001, 4004, 4002], np.int32)[kind1]
    raw = 10.0 ** rng.uniform(-0.5, 5.0, n1)
    pick = rng.random(n1)
    raw[pick < 0.05] = -rng.uniform(0.0, 5.0, (pick < 0.05).sum())
    raw[(pick >= 0.05) & (pick < 0.08)] = rng.uniform(1.0e10, 1.0e12, ((pick >= 0.05) & (pick < 0.08)).sum())
    raw[(pick >= 0.08) & (pick < 0.09)] = 1.0e10                      # the bound itself: undef
    dat1 = np.where(elm1 == 4002, rng.normal(0.0, 6.0, n1), raw)
    files.append(dict(elm=elm1, typ=np.full(n1, 22, np.int32), lev=rng.uniform(500.0, 12000.0, n1), dat=dat1,
                      err=rng.choice([2.0, 4.0], n1)))
    choices = [2819, 14593, 3073] + ([8800] if h08 else [])
    kind2 = rng.integers(0, len(choices), n2)
    elm2 = np.array(choices, np.int32)[kind2]
    typ2 = np.array([1, 8, 1, 23][:len(choices)], np.int32)[kind2]
    lev2 = np.where(elm2 == 8800, rng.integers(7, 17, n2).astype(np.float64), rng.uniform(20000.0, 95000.0, n2))
    dat2 = np.where(elm2 == 14593, rng.normal(1.0e5, 300.0, n2),
                    np.where(elm2 == 8800, 250.0 + 20.0 * rng.standard_normal(n2), rng.normal(0.0, 5.0, n2)))
    files.append(dict(elm=elm2, typ=typ2, lev=lev2, dat=dat2, err=np.where(elm2 == 14593, 100.0, 1.5)))
    for f in files:
        n = len(f["elm"])
        f["ri"] = ihalo + 0.5 + rng.uniform(0.0, gx, n)
        f["rj"] = ihalo + 0.5 + rng.uniform(0.0, gy, n)
    off = np.array([0, n1, n1 + n2], np.int64)
    flat = {key: np.concatenate([f[key] for f in files]) for key in ("elm", "typ", "lev", "dat", "err", "ri", "rj")}
    flat["elm"] = flat["elm"].astype(np.int32)
    flat["typ"] = flat["typ"].astype(np.int32)
    kld = k + (1 if det_run else 0)
    ranks = []
    for r in range(px * py):
        pi, pj = r % px, r // px
        inside = ((flat["ri"] - ihalo - 0.5 > pi * nlon) & (flat["ri"] - ihalo - 0.5 <= (pi + 1) * nlon) &
                  (flat["rj"] - ihalo - 0.5 > pj * nlat) & (flat["rj"] - ihalo - 0.5 <= (pj + 1) * nlat))
        rows = np.nonzero(inside & (flat["elm"] != 3073))[0]
        rng.shuffle(rows)
        set_ = (np.searchsorted(off, rows, side="right")).astype(np.int32)
        idx = (rows - off[set_ - 1] + 1).astype(np.int32)
        n = len(rows)
        e = flat["elm"][rows]
        base = np.where(np.isin(e, (4001, 4004)), rng.uniform(0.0, 40.0, n),
                        np.where(e == 14593, 1.0e5, np.where(e == 8800, 250.0, 0.0)))
        ens = base[:, None] + rng.normal(0.0, 3.0, (n, kld))
        if h08:
            cloudy = (e == 8800)[:, None] & (rng.random((n, kld)) < 0.3)
            ens = np.where(cloudy, -ens, ens)
        ens[rng.random(n) < 0.05] += 15.0
        qc = np.where(rng.random(n) < qc_reject, rng.choice([10, 20, 21], n), 0).astype(np.int32)
        olev = np.where(e == 8800, rng.uniform(5000.0, 90000.0, n), 0.0)
        val2 = np.where(e == 8800, 255.0 + 10.0 * rng.standard_normal(n), 0.0)
        ranks.append(dict(rank=r, pi=pi, pj=pj, set=set_, idx=idx, ensval=np.ascontiguousarray(ens), qc=qc, lev=olev,
                          val2=val2))
    return dict(px=px, py=py, nlon=nlon, nlat=nlat, ihalo=ihalo, k=k, kld=kld, det_run=det_run, h08=h08, off=off,
                files=flat, ranks=ranks)


def qc_of(w, **over):
    d = dict(h08=int(w["h08"]), h08_min_cld_member=2, h08_limit_lev=20000.0, gross_error_h08=4.0, h08_bt_min=180.0)
    d.update(over)
    return qc_params(QcParams, w["k"], w["det_run"], **d)


def oracle_local(w, rk, nml):
    """The local half for one rank (w["fix_ij_obsgrd"], default 0: letkf_mesh.fix_ij_obsgrd of the sort).  Returns dict(files
    (pre-processed), ctype tables, mesh dims, rows, val, qc, ensval, tot, n_cell, key, send)."""
    L, O = lib(), _oracle.oracle()
    O.orc_obs_mesh_sort.restype = C.c_int64
    f = {key: v.copy() for key, v in w["files"].items()}
    nrows = len(f["elm"])
    use = np.zeros(NID_OBS * NOBTYPE, np.int32)
    rc = L.orc_obs_preprocess(C.c_int64(nrows), _p(f["elm"]), _p(f["typ"]), _p(f["dat"]), _p(f["err"]), C.c_int32(NOBTYPE),
                              C.c_double(nml["min_radar_ref_dbz"]), C.c_double(nml["low_ref_shift"]),
                              C.c_int32(nml["use_obserr_radar_ref"]), C.c_double(nml["obserr_radar_ref"]),
                              C.c_int32(nml["use_obserr_radar_vr"]), C.c_double(nml["obserr_radar_vr"]), _p(use))
    assert rc == 0
    cap = NID_OBS * NOBTYPE
    t = dict(elm_ctype=np.zeros(cap, np.int32), elm_u_ctype=np.zeros(cap, np.int32), typ_ctype=np.zeros(cap, np.int32),
             hori_loc_ctype=np.zeros(cap), vert_loc_ctype=np.zeros(cap), ctype_elmtyp=np.zeros(cap, np.int32))
    hl = np.ascontiguousarray(nml["hori_local"], np.float64)
    vl = np.ascontiguousarray(nml["vert_local"], np.float64)
    nc = L.orc_ctype_tables(C.c_int32(NOBTYPE), _p(use), _p(hl), _p(vl), C.c_double(nml["hori_local_radar_obsnoref"]),
                            C.c_double(nml["hori_local_radar_vr"]), C.c_double(nml["vert_local_radar_vr"]),
                            _p(t["elm_ctype"]), _p(t["elm_u_ctype"]), _p(t["typ_ctype"]), _p(t["hori_loc_ctype"]),
                            _p(t["vert_loc_ctype"]), _p(t["ctype_elmtyp"]))
    for key in ("elm_ctype", "elm_u_ctype", "typ_ctype", "hori_loc_ctype", "vert_loc_ctype"):
        t[key] = t[key][:nc].copy()
    t["ctype_elmtyp"] = t["ctype_elmtyp"].reshape(NOBTYPE, NID_OBS)
    dims = oracle_mesh_dims(t["typ_ctype"], t["hori_loc_ctype"], nml, w["nlon"], w["nlat"])
    # row gather: obs(set)%...(idx)
    r = w["off"][rk["set"] - 1] + rk["idx"] - 1
    rows = {key: f[key][r].copy() for key in ("elm", "typ", "dat", "err", "ri", "rj", "lev")}
    uid = np.array([UID[int(e)] for e in rows["elm"]], np.int32) if len(r) else np.zeros(0, np.int32)
    rows["ctype"] = (t["ctype_elmtyp"][rows["typ"] - 1, uid - 1] - 1).astype(np.int32) if len(r) else np.zeros(0, np.int32)
    n = len(r)
    ens = rk["ensval"].copy()
    val = np.zeros(max(n, 1))
    qc = rk["qc"].copy()
    lev, v2 = rk["lev"].copy(), rk["val2"].copy()
    prm = qc_of(w)
    prm.h08_lev = lev.ctypes.data
    prm.h08_val2 = v2.ctypes.data if w["h08"] else None
    O.orc_obs_departure(C.byref(prm), C.c_int64(n), _p(rows["elm"]), _p(rows["dat"]), _p(rows["err"]), _p(ens),
                        C.c_int64(w["kld"]), _p(val), _p(qc))
    tot = np.zeros(max(2 * nc, 1), np.int32)
    L.orc_obs_counts(C.c_int64(n), C.c_int32(nc), _p(rows["ctype"]), _p(qc), _p(tot))
    ncell = int((dims["ngrd_i"].astype(np.int64) * dims["ngrd_j"]).sum())
    n_cell = np.zeros(max(ncell, 1), np.int32)
    key = np.zeros(max(n, 1), np.int32)
    m = fill(Mesh, nctype=nc, nlon=w["nlon"], nlat=w["nlat"], ihalo=w["ihalo"], jhalo=w["ihalo"], rank_i=rk["pi"],
             rank_j=rk["pj"], fix_ij_obsgrd=int(w.get("fix_ij_obsgrd", 0)), ngrd_i=dims["ngrd_i"].ctypes.data, ngrd_j=dims["ngrd_j"].ctypes.data)
    ns = O.orc_obs_mesh_sort(C.byref(m), C.c_int64(n), _p(rows["ctype"]), _p(rows["ri"]), _p(rows["rj"]), _p(qc),
                             _p(n_cell), _p(key)) if n else 0
    key = key[:ns]
    kld = w["kld"]
    send = np.zeros((ns, kld + 4))
    send[:, :kld] = ens[key]
    send[:, kld] = val[key]
    send[:, kld + 1] = rk["lev"][key] if w["h08"] else 0.0
    send[:, kld + 2] = rk["set"][key]
    send[:, kld + 3] = rk["idx"][key]
    return dict(files=f, nctype=nc, tables=t, dims=dims, rows=rows, val=val[:n], qc=qc, ensval=ens, val2=v2,
                tot=tot[:2 * nc].reshape(nc, 2), n_cell=n_cell[:ncell], key=key, send=send, ncell=ncell)


def oracle_mesh_dims(typ_ctype, hori_loc_ctype, nml, nlon, nlat):
    nc = len(typ_ctype)
    o = {key: np.zeros(max(nc, 1), np.int32) for key in ("ngrd_i", "ngrd_j", "ngrdsch_i", "ngrdsch_j", "ngrdext_i", "ngrdext_j")}
    o["grdspc_i"], o["grdspc_j"] = np.zeros(max(nc, 1)), np.zeros(max(nc, 1))
    ty = np.ascontiguousarray(typ_ctype, np.int32)
    hl = np.ascontiguousarray(hori_loc_ctype, np.float64)
    sp = np.ascontiguousarray(nml["obs_sort_grid_spacing"], np.float64)
    mx = np.ascontiguousarray(nml["max_nobs_per_grid"], np.int32)
    ms = np.ascontiguousarray(nml["obs_min_spacing"], np.float64)
    lib().orc_obs_mesh_dims(C.c_int32(nc), _p(ty), _p(hl), _p(sp), _p(mx), _p(ms), C.c_double(nml["dx"]),
                            C.c_double(nml["dy"]), C.c_int32(nlon), C.c_int32(nlat), _p(o["ngrd_i"]), _p(o["ngrd_j"]),
                            _p(o["grdspc_i"]), _p(o["grdspc_j"]), _p(o["ngrdsch_i"]), _p(o["ngrdsch_j"]),
                            _p(o["ngrdext_i"]), _p(o["ngrdext_j"]))
    return {key: v[:nc].copy() for key, v in o.items()}


def oracle_finish(w, me, locs):
    """The finish half for rank `me` from every rank's oracle_local: the plan and the obsda_sort columns."""
    O = _oracle.oracle()
    O.orc_obs_halo_plan.restype = C.c_int64
    lo = locs[me]
    d = lo["dims"]
    nc = lo["nctype"]
    n_all = np.ascontiguousarray(np.stack([x["n_cell"] for x in locs]), np.int32)
    recv = np.concatenate([x["send"] for x in locs]) if locs else np.zeros((0, w["kld"] + 4))
    nacx = int(((d["ngrdext_i"] + 1).astype(np.int64) * d["ngrdext_j"]).sum())
    ac_ext = np.zeros(max(nacx, 1), np.int32)
    src_row = np.zeros(max(len(recv), 1), np.int32)
    if nc:
        lay = fill(HaloLayout, nctype=nc, nprocs=w["px"] * w["py"], prc_num_x=w["px"], myrank=me,
                   ngrd_i=d["ngrd_i"].ctypes.data, ngrd_j=d["ngrd_j"].ctypes.data, ngrdsch_i=d["ngrdsch_i"].ctypes.data,
                   ngrdsch_j=d["ngrdsch_j"].ctypes.data)
        nt = O.orc_obs_halo_plan(C.byref(lay), _p(n_all), _p(ac_ext), _p(src_row), C.c_int64(len(recv)))
    else:
        nt = 0
    src = src_row[:nt]
    kld = w["kld"]
    rows = recv[src]
    f = lo["files"]
    r = w["off"][rows[:, kld + 2].astype(np.int64) - 1] + rows[:, kld + 3].astype(np.int64) - 1
    ob_lev = f["lev"][r].copy()
    if w["h08"]:
        h = f["typ"][r] == 23
        ob_lev[h] = rows[h, kld + 1]
    tot_g = sum(x["tot"] for x in locs)
    return dict(ac_ext=ac_ext[:nacx], src_row=src, nobstotal=nt, ensval=rows[:, :kld].copy(), val=rows[:, kld].copy(),
                qc=np.zeros(nt, np.int32), ob_ri=f["ri"][r], ob_rj=f["rj"][r], ob_lev=ob_lev, ob_dat=f["dat"][r],
                ob_err=f["err"][r], tot_g=tot_g, ac_off=np.concatenate(
                    [[0], np.cumsum((d["ngrdext_i"] + 1).astype(np.int64) * d["ngrdext_j"])])[:nc])


def setobs_params(cls, w, nml, myrank=0):
    keep = [np.ascontiguousarray(nml[key], dt) for key, dt in
            (("hori_local", np.float64), ("vert_local", np.float64), ("obs_sort_grid_spacing", np.float64),
             ("obs_min_spacing", np.float64), ("max_nobs_per_grid", np.int32))]
    p = fill(cls, nobtype=NOBTYPE, use_obserr_radar_ref=nml["use_obserr_radar_ref"],
             use_obserr_radar_vr=nml["use_obserr_radar_vr"], nlon=w["nlon"], nlat=w["nlat"], ihalo=w["ihalo"],
             jhalo=w["ihalo"], nprocs=w["px"] * w["py"], prc_num_x=w["px"], myrank=myrank,
             fix_ij_obsgrd=int(w.get("fix_ij_obsgrd", 0)),
             criterion=nml["criterion"], min_radar_ref_dbz=nml["min_radar_ref_dbz"], low_ref_shift=nml["low_ref_shift"],
             obserr_radar_ref=nml["obserr_radar_ref"], obserr_radar_vr=nml["obserr_radar_vr"],
             hori_local_radar_obsnoref=nml["hori_local_radar_obsnoref"], hori_local_radar_vr=nml["hori_local_radar_vr"],
             vert_local_radar_vr=nml["vert_local_radar_vr"], dx=nml["dx"], dy=nml["dy"], rain_base=nml["rain_base"],
             hori_local=keep[0].ctypes.data, vert_local=keep[1].ctypes.data, obs_sort_grid_spacing=keep[2].ctypes.data,
             obs_min_spacing=keep[3].ctypes.data, max_nobs_per_grid=keep[4].ctypes.data, ctype_merge=None)
    return p, keep
