"""das_letkf_obs from a Fortran host on the device: scale-letkf_amd/fortran/letkf_tools_amd.f90 `das_letkf_obs_amd`
(das_letkf_obs, scale/letkf/letkf_tools.f90:933-1156; one letkf_das_obs_dev call per target variable, varloc set and
restored around them), called by fortran/obsanal_driver.f90 on a set_letkf_obs table, against Context.das_obs over the
ObsTable.target_groups() of the same table: the same bits."""
import ctypes as C
import os
import struct
import subprocess
import tempfile

import numpy as np
import pytest

from __graft_entry__ import PKG_DIR, load_package

FDIR = os.path.join(PKG_DIR, "fortran")
DRIVER = os.path.join(FDIR, "build", "obsanal_driver")
HAVE_FC = os.path.exists("/opt/rocm/bin/amdflang")


def build_fortran():
    load_package().build()
    subprocess.check_call(["make", "-C", FDIR], stdout=subprocess.DEVNULL)


@pytest.mark.skipif(not HAVE_FC, reason="amdflang not present")
def test_das_letkf_obs_amd_compiles_and_links():
    build_fortran()
    assert os.path.exists(DRIVER)


def _host(ptr, dtype, n):
    """n elements of a library-owned device array, copied to the host"""
    import torch
    t = torch.empty(max(n, 1), dtype=dtype, device="cuda")
    if n:
        hip = C.CDLL("libamdhip64.so")
        assert hip.hipMemcpy(C.c_void_p(t.data_ptr()), C.c_void_p(ptr), C.c_size_t(n * t.element_size()), C.c_int(3)) == 0
    return t[:n].cpu().numpy()


@pytest.mark.gpu
@pytest.mark.skipif(not HAVE_FC, reason="amdflang not present")
@pytest.mark.parametrize("rtps,q", [(0.9, False), (0.0, True)])
def test_das_letkf_obs_amd_equals_das_obs_over_target_groups(rtps, q):
    import torch
    from _gpu import ctx, dev
    from _setobs import make_world, namelist
    from test_gpu_setobs import run_local
    build_fortran()
    w = make_world(31, k=10, det_run=True, nfile_rows=(4000, 2000))
    g = run_local(w, w["ranks"][0], namelist(), both=True)
    tab = g["tab"]
    h, dl = tab.host(), tab.download()
    t = tab.search_tables()
    nc, ng = t.nctype, t.ngroup
    nobs, kld, k = int(h["nobstotal"]), int(h["kld"]), w["k"]
    i32, i64, f64 = torch.int32, torch.int64, torch.float64
    gs = _host(t.group_start, i32, ng + 1)
    arr = dict(group_start=gs, group_member=_host(t.group_member, i32, int(gs[-1])))
    for name in ("vmode", "max_nobs", "ngrd_i", "ngrd_j", "ngrdsch_i", "ngrdsch_j", "ngrdext_i", "ngrdext_j"):
        arr[name] = _host(getattr(t, name), i32, nc)
    for name in ("hori_loc", "vert_loc", "varloc"):
        arr[name] = _host(getattr(t, name), f64, nc)
    arr["ac_off"] = _host(t.ac_off, i64, nc)
    arr["ac_ext"] = dl["ac_ext"]
    for name in ("ob_ri", "ob_rj", "ob_lev", "ob_dat", "ob_err"):
        arr[name] = _host(getattr(t, name), f64, nobs)
    varloc0 = arr["varloc"].copy()
    rng = np.random.default_rng(7)
    var_local = rng.uniform(0.3, 1.0, (11, 9))
    uid = (np.arange(nc) % 9 + 1).astype(np.int32)           # column of var_local per ctype, 1-based
    groups = tab.target_groups()
    assert len(groups) >= 2
    rows = np.concatenate([groups[tv] for tv in sorted(groups)])
    ac = dl["ac_ext"].astype(np.int64)
    ctype_of = np.full(nobs, -1)
    for c in range(nc):
        lo, hi = ac[arr["ac_off"][c]], ac[arr["ac_off"][c] + (int(arr["ngrdext_i"][c]) + 1) * int(arr["ngrdext_j"][c]) - 1]
        ctype_of[lo:hi] = c
    elm = h["elm_ctype"][ctype_of[rows]].astype(np.int32)
    rlev = 3.0e4 + 50.0 * (rows % 1000)
    rz = 500.0 + 7.0 * (rows % 1000)
    infl = 1.0 + 0.001 * (rows % 300)
    tab0 = rng.standard_normal((nobs, kld))
    prm = dict(relax_alpha_spread=rtps, q_update_top=4.0e4 if q else 0.0, q_sprd_max=0.01 if q else -1.0, infl_mul=1.0)
    # ---- the Python side: one das_obs per group, varloc set per target variable
    c = ctx()
    ens, dep = dev(dl["ensval"]), dev(dl["val"])
    yt = dev(tab0)
    exp = {}
    for tv in sorted(groups):
        sel = np.nonzero(np.isin(rows, groups[tv]))[0]
        r = rows[sel]
        tab.set_varloc(np.array([var_local[tv, uid[ic] - 1] if tv >= 0 else 1.0 for ic in range(nc)]))
        ya = torch.empty((len(r), k + 1), dtype=f64, device="cuda")
        ym = torch.empty(len(r), dtype=f64, device="cuda")
        da = torch.empty(len(r), dtype=f64, device="cuda")
        c.das_obs(k, tv, tab.search_tables(), ens, kld, dep, nobs, ya, tgt_row=dev(r.astype(np.int32)), ya_mean=ym, ya_table=yt,
                  dep_a=da, rlev_tgt=dev(rlev[sel]), rz_tgt=dev(rz[sel]), infl=dev(infl[sel]), det_run=True, **prm)
        torch.cuda.synchronize()
        exp[tv] = (sel, ya.cpu().numpy(), ym.cpu().numpy(), da.cpu().numpy())
    tab.set_varloc(varloc0)
    ya_e = np.zeros((len(rows), k + 1))
    ym_e, da_e = np.zeros(len(rows)), np.zeros(len(rows))
    for sel, ya, ym, da in exp.values():
        ya_e[sel], ym_e[sel], da_e[sel] = ya, ym, da
    yt_e = yt.cpu().numpy()
    # ---- the Fortran side
    ntgt = len(rows)
    with tempfile.TemporaryDirectory() as d:
        fin, fout = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
        with open(fin, "wb") as fh:
            hdr = [nc, ng, t.criterion, t.nlon, t.nlat, k, 1, kld, nobs, arr["ac_ext"].size, arr["group_member"].size, ntgt, 11,
                   0, 0, 0]
            fh.write(struct.pack("<16i", *hdr))
            fh.write(struct.pack("<10d", t.dx, t.dy, t.i_org, t.j_org, t.rain_base, prm["infl_mul"], 0.0,
                                 prm["relax_alpha_spread"], prm["q_update_top"], prm["q_sprd_max"]))
            wr = lambda a, dt: fh.write(np.ascontiguousarray(a, dtype=dt).tobytes())
            for a in (arr["group_start"], arr["group_member"], arr["vmode"], arr["max_nobs"], arr["ngrd_i"], arr["ngrd_j"],
                      arr["ngrdsch_i"], arr["ngrdsch_j"], arr["ngrdext_i"], arr["ngrdext_j"], uid):
                wr(a, "<i4")
            wr(arr["ac_off"], "<i8")
            wr(arr["ac_ext"], "<i4")
            for a in (arr["hori_loc"], arr["vert_loc"], varloc0, arr["ob_ri"], arr["ob_rj"], arr["ob_lev"], arr["ob_dat"],
                      arr["ob_err"], dl["ensval"], dl["val"], tab0):
                wr(a, "<f8")
            wr(rows + 1, "<i4")
            wr(elm, "<i4")
            for a in (rlev, rz, infl, var_local.T):                 # var_local(nv3d, 9), column-major
                wr(a, "<f8")
        r = subprocess.run([DRIVER, fin, fout], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        raw = np.fromfile(fout, dtype="<f8")
    n1 = ntgt * (k + 1)
    assert raw.size == n1 + 2 * ntgt + nobs * kld
    ya_f = raw[:n1].reshape(ntgt, k + 1)                            # ya(member + 1, ntgt), column-major
    ym_f, da_f = raw[n1:n1 + ntgt], raw[n1 + ntgt:n1 + 2 * ntgt]
    yt_f = raw[n1 + 2 * ntgt:].reshape(nobs, kld)
    assert np.isfinite(ya_f).all() and np.abs(da_f).max() > 0
    for got, want in ((ya_f, ya_e), (ym_f, ym_e), (da_f, da_e), (yt_f, yt_e)):
        assert np.array_equal(got.view(np.int64), want.view(np.int64))
    # (one rank: every row lies in the interior, so every row is a target; untouched rows: tests/test_gpu_obsanal.py)
    assert np.array_equal(np.sort(rows), np.arange(nobs))
    assert not np.array_equal(yt_f, tab0)
