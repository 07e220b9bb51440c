"""The analysis step of PROGRAM letkf (scale/letkf/letkf.f90:142 -> 196 -> 207) driven from Fortran:
scale-letkf_amd/fortran/letkf_analysis_driver.f90 runs set_letkf_obs_amd (letkf_obs_amd.f90, the table stays on the device) ->
das_letkf_amd on the device table -> the analysis mean, and then the host-table das_letkf_amd on the same tables downloaded.
CPU: the module and the driver compile and link.  GPU: a multi-level domain with a radar group under a limit (reflectivity,
zero reflectivity, radial velocity, type 22), upper-air u and surface pressure -- the observation table equals the oracle's
composition (tests/_setobs.py), the local-observation count per point and the analysis equal the oracle's das_letkf, the
departure statistics equal orc_monit_dep, and the two das_letkf_amd specifics agree bit for bit."""
import ctypes as C
import os
import struct
import subprocess
import tempfile

import numpy as np
import pytest

import _oracle
from __graft_entry__ import PKG_DIR, load_package
from _search import SearchTables
from _setobs import ELEM_UID, make_world, namelist, oracle_finish, oracle_local

FDIR = os.path.join(PKG_DIR, "fortran")
DRIVER = os.path.join(FDIR, "build", "letkf_analysis_driver")
HAVE_FC = os.path.exists("/opt/rocm/bin/amdflang")


def build_fortran():
    load_package().build()
    subprocess.check_call(["make", "-C", FDIR], stdout=subprocess.DEVNULL)


@pytest.mark.skipif(not HAVE_FC, reason="amdflang not present")
def test_set_letkf_obs_amd_and_driver_compile_and_link():
    build_fortran()
    assert os.path.exists(DRIVER)
    src = open(os.path.join(FDIR, "letkf_obs_amd.f90")).read()
    assert "SUBROUTINE set_letkf_obs_amd(" in src and "letkf_set_obs_dev" in src and "letkf_monit_dep_dev" in src
    tools = open(os.path.join(FDIR, "letkf_tools_amd.f90")).read()
    assert "INTERFACE das_letkf_amd" in tools and "TYPE :: letkf_obs_tables_dev" in tools


def _p(a, t):
    return a.ctypes.data_as(C.POINTER(t))


@pytest.mark.gpu
@pytest.mark.skipif(not HAVE_FC, reason="amdflang not present")
@pytest.mark.parametrize("k,det", [(10, 0), (20, 1)])
def test_analysis_step_from_fortran(k, det):
    build_fortran()
    nml = namelist()
    nlon = nlat = 12
    nlev, nv, ihalo, dx = 3, 11, 2, nml["dx"]
    w = make_world(500 + k, k=k, det_run=bool(det), nfile_rows=(2500, 1200), nlon=nlon, nlat=nlat, ihalo=ihalo)
    rk = w["ranks"][0]
    o = oracle_local(w, rk, nml)
    of = oracle_finish(w, 0, [o])
    nc, nt, kld = o["nctype"], of["nobstotal"], w["kld"]
    nij1, npts, nens = nlon * nlat, nlon * nlat * nlev, k + 1 + det
    rng = np.random.default_rng(k)
    ii, jj = np.meshgrid(np.arange(nlon), np.arange(nlat))
    rig, rjg = ii.ravel() + 1.0 + ihalo, jj.ravel() + 1.0 + ihalo
    zlev = np.array([500.0, 3000.0, 8000.0])
    hgt = zlev[:, None] + rng.uniform(-50.0, 50.0, (nlev, nij1))
    full = rng.normal(1.0, 1.0, (nv, nens, npts))
    full[4] = (1.0e5 * np.exp(-hgt / 7500.0)).ravel()[None, :] + rng.normal(0.0, 40.0, (nens, npts))
    full[5:] = np.abs(full[5:]) * 1e-3 + 1e-3
    g = full.reshape(-1).copy()
    lib = _oracle.oracle()
    lib.orc_ensmean(C.c_int(k), C.c_int(nv), C.c_int64(npts), _p(g, C.c_double), C.c_int64(1), C.c_int64(npts),
                    C.c_int64(npts * nens))
    full_in = g.copy()
    lib.orc_to_perturbations(C.c_int(k), C.c_int(nv), C.c_int64(npts), _p(g, C.c_double), C.c_int64(1), C.c_int64(npts),
                             C.c_int64(npts * nens))
    var_local = np.ones((nv, 9))
    infl_mul, rtps = 1.05, 0.9

    # ---- the oracle's das_letkf on the oracle's tables: obs_local for every point + the loop body (one variable class)
    t, d = o["tables"], o["dims"]
    vm = np.array([2 if e == 14593 else 3 if e == 19999 else 1 if ty == 22 else 0
                   for e, ty in zip(t["elm_ctype"], t["typ_ctype"])], np.int32)
    arrs = dict(group_start=np.arange(nc + 1, dtype=np.int32), group_member=np.arange(nc, dtype=np.int32), vmode=vm,
                hori_loc=t["hori_loc_ctype"], vert_loc=t["vert_loc_ctype"], varloc=np.ones(nc),
                max_nobs=nml["max_nobs_per_grid"][t["typ_ctype"] - 1].astype(np.int32), ngrd_i=d["ngrd_i"],
                ngrd_j=d["ngrd_j"], ngrdsch_i=d["ngrdsch_i"], ngrdsch_j=d["ngrdsch_j"], ngrdext_i=d["ngrdext_i"],
                ngrdext_j=d["ngrdext_j"], ac_off=of["ac_off"].astype(np.int64), ac_ext=of["ac_ext"], ob_ri=of["ob_ri"],
                ob_rj=of["ob_rj"], ob_lev=of["ob_lev"], ob_dat=of["ob_dat"], ob_err=of["ob_err"])
    th = SearchTables()
    keep = []
    for key, v in arrs.items():
        a = np.ascontiguousarray(v)
        keep.append(a)
        setattr(th, key, a.ctypes.data)
    for key, v in dict(nctype=nc, ngroup=nc, criterion=nml["criterion"], nlon=nlon, nlat=nlat, limit_hint=2, dx=dx, dy=dx,
                       i_org=ihalo + 0.5, j_org=ihalo + 0.5, rain_base=nml["rain_base"]).items():
        setattr(th, key, v)
    lib.orc_obs_local.restype = C.c_int
    gm = g.reshape(nv, nens, npts)
    cap = 8000
    idx, rd, rl, ds = np.zeros(cap, np.int32), np.zeros(cap), np.zeros(cap), np.zeros(cap)
    off, li, lrd, lrl = [0], [], [], []
    for p in range(npts):
        n = lib.orc_obs_local(C.byref(th), C.c_double(rig[p % nij1]), C.c_double(rjg[p % nij1]), C.c_double(gm[4, k, p]),
                              C.c_double(hgt.ravel()[p]), C.c_int(cap), _p(idx, C.c_int32), _p(rd, C.c_double),
                              _p(rl, C.c_double), _p(ds, C.c_double))
        assert n >= 0
        li.append(idx[:n].copy()); lrd.append(rd[:n].copy()); lrl.append(rl[:n].copy())
        off.append(off[-1] + n)
    counts = np.diff(off)
    assert (counts > 0).mean() > 0.5
    ens = np.ascontiguousarray(of["ensval"])
    prm = _oracle.DasParams(k=k, nv=nv, det_run=det, infl_adaptive=0, relax_to_inflated_prior=0, relax_alpha=0.0,
                            relax_alpha_spread=rtps, q_update_top=0.0, q_sprd_max=0.0, iv_p=4, iv_q_first=5, iv_q_last=10,
                            nthreads=4, var_mask=0)
    lib.orc_relax_beta.restype = C.c_double
    from test_fortran_das import OrcBeta
    bp = OrcBeta(0, 99.0e3, max(nml["vert_local"][21], nml["vert_local_radar_vr"]), 0.0, dx, dx, ihalo, ihalo, nlon, nlat)
    beta = np.array([lib.orc_relax_beta(C.byref(bp), C.c_double(rig[p % nij1]), C.c_double(rjg[p % nij1]),
                                        C.c_double(hgt.ravel()[p])) for p in range(npts)])
    ref = _oracle.das_points(prm, np.array(off), np.concatenate(li) if off[-1] else np.zeros(0, np.int32),
                             np.concatenate(lrd) if off[-1] else np.zeros(0), np.concatenate(lrl) if off[-1] else np.zeros(0),
                             ens, np.ascontiguousarray(of["val"]), beta, np.full(npts * nv, infl_mul), g, 1, npts, npts * nens)
    assert ref["rc"] == 0
    want = ref["anal"].reshape(nv, nens, npts)
    # departure statistics of the local rows (letkf_obs.f90:639-646)
    nid = len(ELEM_UID)
    mn, mb, mr = np.zeros(nid, np.int32), np.zeros(nid), np.zeros(nid)
    eu = np.array(ELEM_UID, np.int32)
    rows_elm = np.ascontiguousarray(o["rows"]["elm"], np.int32)
    lib.orc_monit_dep(C.c_int(nid), _p(eu, C.c_int32), C.c_int64(len(rows_elm)), _p(rows_elm, C.c_int32),
                      _p(np.ascontiguousarray(o["val"]), C.c_double), _p(o["qc"], C.c_int32), _p(mn, C.c_int32),
                      _p(mb, C.c_double), _p(mr, C.c_double))

    # ---- the Fortran host
    f = w["files"]
    qp = dict(member=k, det_run=det, use_radar_ref=1, use_radar_vr=1, min_radar_ref_member=3, min_radar_ref_member_obsref=2,
              h08=0, h08_min_cld_member=2)
    qd = [15.0, 5.0, 4.0, 3.0, 2.5, 5.0, 5.0, 5.0, 5.0, 20000.0, 4.0, 180.0]
    with tempfile.TemporaryDirectory() as tmp:
        fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
        with open(fin, "wb") as fh:
            wr = lambda a, dt: fh.write(np.ascontiguousarray(a, dtype=dt).tobytes())
            fh.write(struct.pack("<16i", k, det, nlon, nlat, nlev, nv, ihalo, len(w["off"]) - 1, len(f["elm"]),
                                 len(rk["qc"]), kld, 0, nml["use_obserr_radar_ref"], nml["use_obserr_radar_vr"],
                                 nml["criterion"], 1))
            fh.write(struct.pack("<11d", dx, nml["min_radar_ref_dbz"], nml["low_ref_shift"], nml["obserr_radar_ref"],
                                 nml["obserr_radar_vr"], nml["hori_local_radar_obsnoref"], nml["hori_local_radar_vr"],
                                 nml["vert_local_radar_vr"], nml["rain_base"], rtps, infl_mul))
            for key in ("hori_local", "vert_local", "obs_sort_grid_spacing", "obs_min_spacing"):
                wr(nml[key], "<f8")
            wr(nml["max_nobs_per_grid"], "<i4")
            fh.write(struct.pack("<8i", *qp.values()))
            fh.write(struct.pack("<12d", *qd))
            wr(w["off"], "<i8")
            wr(f["elm"], "<i4"); wr(f["typ"], "<i4")
            for key in ("lev", "dat", "err", "ri", "rj"):
                wr(f[key], "<f8")
            wr(rk["set"], "<i4"); wr(rk["idx"], "<i4"); wr(rk["qc"], "<i4")
            wr(rk["ensval"], "<f8"); wr(rk["lev"], "<f8"); wr(rk["val2"], "<f8")
            wr(var_local.T, "<f8")
            wr(rig, "<f8"); wr(rjg, "<f8"); wr(hgt, "<f8"); wr(full_in, "<f8")
        r = subprocess.run([DRIVER, fin, fout], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        raw = open(fout, "rb").read()
    assert "OBSERVATIONAL DEPARTURE STATISTICS" in r.stdout and "OBSERVATION COUNTS" in r.stdout
    pos = 0

    def take(dt, n):
        nonlocal pos
        a = np.frombuffer(raw, dtype=dt, count=n, offset=pos)
        pos += a.nbytes
        return a
    assert take("<i4", 1)[0] == nt
    g_mn = take("<i4", nid)
    g_mb, g_mr = take("<f8", nid), take("<f8", nid)
    nst = nv * nens * npts
    a_dev = take("<f8", nst).reshape(nv, nens, npts)
    a_host = take("<f8", nst).reshape(nv, nens, npts)
    np_dev, np_host = take("<i4", npts), take("<i4", npts)
    g_ens = take("<f8", kld * nt).reshape(nt, kld)
    cols = {key: take("<f8", nt) for key in ("val", "ob_ri", "ob_rj", "ob_lev", "ob_dat", "ob_err")}
    g_qc = take("<i4", len(rk["qc"]))
    g_dat = take("<f8", len(f["dat"]))
    # set_letkf_obs_amd: the table, the QC flags and the pre-processed files equal the oracle's composition
    assert np.array_equal(g_qc, o["qc"]) and np.array_equal(g_dat, o["files"]["dat"])
    assert np.array_equal(g_ens, of["ensval"])
    for key in cols:
        assert np.array_equal(cols[key], of[key]), key
    # departure statistics
    assert np.array_equal(g_mn, mn)
    has = mn > 0
    assert np.allclose(g_mb[has], mb[has], rtol=1e-13, atol=1e-13) and np.allclose(g_mr[has], mr[has], rtol=1e-13, atol=0)
    assert np.array_equal(g_mb[~has], mb[~has])
    # das_letkf_amd on the device table = the host-table specific, bit for bit
    assert np.array_equal(a_dev, a_host) and np.array_equal(np_dev, np_host)
    # ... and the oracle's das_letkf: the same local observations at every point, the analysis within 1e-10
    assert np.array_equal(np_dev, counts)
    members = list(range(k)) + ([k + 1] if det else [])
    for v in range(nv):
        scale = max(np.abs(gm[v, k]).max(), np.abs(gm[v, :k]).max())
        assert np.abs(a_dev[v, members] - want[v, members]).max() <= 1e-10 * scale, v
