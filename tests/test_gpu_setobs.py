"""GPU parity of set_letkf_obs behind one call (include/letkf_amd.h section 9) against the oracle's composition
(tests/_setobs.py): pre-processed files, ctype tables, mesh sizes, qc, departures, count tables, n_cell, key, ac_ext and
every obsda_sort column bit-identical -- except that a reflectivity converted by 10 log10 on the device may differ from libm
in the last bits: that dat and the departures derived from it agree within 2 ulp of the dat."""
import numpy as np
import pytest
import torch

from _setobs import make_world, namelist, oracle_finish, oracle_local, qc_of, setobs_params

pytestmark = pytest.mark.gpu


def run_local(w, rk, nml, me=0, both=False):
    from _gpu import ctx, dev, pkg
    c = ctx()
    f = w["files"]
    d = {k: dev(v) for k, v in f.items()}
    off = np.ascontiguousarray(w["off"], np.int64)
    files = pkg.ObsFileRows(nfile=len(off) - 1, off=off.ctypes.data, elm=d["elm"].data_ptr(), typ=d["typ"].data_ptr(),
                            lev=d["lev"].data_ptr(), dat=d["dat"].data_ptr(), err=d["err"].data_ptr(), ri=d["ri"].data_ptr(),
                            rj=d["rj"].data_ptr())
    p, keep = setobs_params(pkg.SetObsParams, w, nml, me)
    lev, v2 = dev(rk["lev"]), dev(rk["val2"])
    q = qc_of(w)
    q.h08_lev = lev.data_ptr()
    q.h08_val2 = v2.data_ptr() if w["h08"] else None
    ens, qc = dev(rk["ensval"]), dev(rk["qc"])
    s, i = dev(rk["set"]), dev(rk["idx"])
    fn = c.set_obs if both else c.set_obs_local
    tab = fn(p, q, files, s, i, qc, ens, w["kld"], keep=(keep, d, off, lev, v2, ens, qc, s, i, files))
    torch.cuda.synchronize()
    return dict(tab=tab, files=d, qc=qc, ensval=ens, val2=v2)


def _np(info_ptr, dtype, n):
    """copy n elements of a library-owned device array to the host"""
    import ctypes as C
    from _gpu import pkg  # noqa: F401
    t = torch.empty(max(n, 1), dtype=dtype, device="cuda")
    if n:
        hip = C.CDLL("libamdhip64.so")
        assert hip.hipMemcpy(C.c_void_p(t.data_ptr()), C.c_void_p(info_ptr), C.c_size_t(n * t.element_size()), C.c_int(3)) == 0
    return t[:n].cpu().numpy()


def assert_dat_close(got, exp, conv, what):
    """bit-identical outside `conv`; within 2 ulp of the converted dat on `conv` rows"""
    assert np.array_equal(got[~conv], exp[~conv]), what
    tol = 2.0 * np.spacing(np.abs(exp[conv]))
    assert np.all(np.abs(got[conv] - exp[conv]) <= tol), what


def check_local(w, g, o):
    f0 = w["files"]
    conv_file = (f0["elm"] == 4001) & (o["files"]["elm"] == 4001) & (o["files"]["dat"] != -9.99e33)
    assert np.array_equal(g["files"]["elm"].cpu().numpy(), o["files"]["elm"])
    assert np.array_equal(g["files"]["err"].cpu().numpy(), o["files"]["err"])
    gd = g["files"]["dat"].cpu().numpy()
    assert_dat_close(gd, o["files"]["dat"], conv_file, "pre-processed dat")
    h = g["tab"].host()
    for k in ("elm_ctype", "elm_u_ctype", "typ_ctype", "hori_loc_ctype", "vert_loc_ctype", "ctype_elmtyp"):
        assert np.array_equal(h[k], o["tables"][k]), k
    for k in ("ngrd_i", "ngrd_j", "ngrdsch_i", "ngrdsch_j", "ngrdext_i", "ngrdext_j", "grdspc_i", "grdspc_j"):
        assert np.array_equal(h[k], o["dims"][k]), k
    assert np.array_equal(g["qc"].cpu().numpy(), o["qc"])
    assert np.array_equal(h["tot_sub"], o["tot"])
    i = g["tab"].info()
    n = len(o["qc"])
    r = w["off"][w_rows(w, g)[0] - 1] + w_rows(w, g)[1] - 1 if n else np.zeros(0, np.int64)
    conv_row = conv_file[r] if n else np.zeros(0, bool)
    good = o["qc"] == 0
    assert_dat_close(_np(i.val, torch.float64, n)[good], o["val"][good], conv_row[good], "val")
    ge = g["ensval"].cpu().numpy()
    K = w["k"]
    assert np.array_equal(ge[:, :K], o["ensval"][:, :K])
    if w["det_run"]:
        assert_dat_close(ge[:, K], o["ensval"][:, K], conv_row & good, "det departure")
    assert np.array_equal(_np(i.n_cell, torch.int32, i.ncell), o["n_cell"])
    assert np.array_equal(_np(i.key, torch.int32, i.nsorted), o["key"])
    if w["h08"]:
        assert np.array_equal(g["val2"].cpu().numpy(), o["val2"])
    return conv_file, int((gd[conv_file] != o["files"]["dat"][conv_file]).sum()), int(conv_file.sum())


def w_rows(w, g):
    return g["_set"], g["_idx"]


def check_finish(w, tab, of, conv_file):
    d = tab.download()
    h = tab.host()
    assert d["ac_ext"].size == of["ac_ext"].size and np.array_equal(d["ac_ext"], of["ac_ext"])
    assert np.array_equal(h["ac_off"], of["ac_off"])
    assert np.array_equal(h["tot_g"], of["tot_g"])
    nt = of["nobstotal"]
    assert tab.info().nobstotal == nt
    K = w["k"]
    conv = of["conv"]
    for k in ("ob_ri", "ob_rj", "ob_lev", "ob_err", "qc"):
        assert np.array_equal(d[k], of[k]), k
    assert_dat_close(d["ob_dat"], of["ob_dat"], conv, "ob_dat")
    assert_dat_close(d["val"], of["val"], conv, "val_sort")
    assert np.array_equal(d["ensval"][:, :K], of["ensval"][:, :K])
    if w["det_run"]:
        assert_dat_close(d["ensval"][:, K], of["ensval"][:, K], conv, "ensval det")


def finish_conv(w, locs, me, conv_file):
    of = oracle_finish(w, me, locs)
    recv = np.concatenate([x["send"] for x in locs])
    rows = recv[of["src_row"]]
    r = w["off"][rows[:, w["kld"] + 2].astype(np.int64) - 1] + rows[:, w["kld"] + 3].astype(np.int64) - 1
    of["conv"] = conv_file[r]
    return of


@pytest.mark.parametrize("k,det_run,h08", [(3, False, False), (10, True, False), (50, False, True), (100, True, False),
                                           (10, False, True), (50, True, False)])
def test_set_obs_one_rank_matches_oracle(k, det_run, h08):
    nml = namelist()
    w = make_world(100 + k, k=k, det_run=det_run, h08=h08)
    rk = w["ranks"][0]
    o = oracle_local(w, rk, nml)
    g = run_local(w, rk, nml, both=True)
    g["_set"], g["_idx"] = rk["set"], rk["idx"]
    conv_file, ndiff, nconv = check_local(w, g, o)
    print(f"device log10: {ndiff} of {nconv} converted reflectivities differ from libm")
    of = finish_conv(w, [o], 0, conv_file)
    check_finish(w, g["tab"], of, conv_file)
    assert of["nobstotal"] > 0.25 * len(rk["qc"])
    g["tab"].close()


def test_empty_obsda_all_rejected_and_unreferenced_ctype():
    from _gpu import pkg
    nml = namelist()
    w = make_world(7, k=10)
    rk = w["ranks"][0]
    for variant in ("empty", "rejected"):
        r = dict(rk)
        if variant == "empty":
            for key in ("set", "idx", "qc", "lev", "val2"):
                r[key] = rk[key][:0].copy()
            r["ensval"] = np.zeros((0, w["kld"]))
        else:
            r["qc"] = np.full_like(rk["qc"], 21)
        o = oracle_local(w, r, nml)
        g = run_local(w, r, nml, both=True)
        g["_set"], g["_idx"] = r["set"], r["idx"]
        conv_file, _, _ = check_local(w, g, o)
        h = g["tab"].host()
        assert h["nobstotal"] == 0 and h["nsorted"] == 0
        # the ctype of T (3073), present in a file, referenced by no row: counted, zero rows
        ic = list(h["elm_ctype"]).index(3073)
        assert h["tot_sub"][ic, 0] == 0
        of = finish_conv(w, [o], 0, conv_file)
        check_finish(w, g["tab"], of, conv_file)
        g["tab"].close()
    with pytest.raises(pkg.LetkfError):            # a row outside the files is refused, not read
        r = dict(rk)
        r["idx"] = rk["idx"].copy()
        r["idx"][0] = 10 ** 6
        run_local(w, r, nml, both=True)


def test_two_by_two_world():
    """each rank runs the local half, a concatenation stands in for the exchange, each rank runs the finish half"""
    from _gpu import ctx, dev
    c = ctx()
    nml = namelist()
    w = make_world(21, px=2, py=2, k=12, det_run=True, nfile_rows=(6000, 3000))
    locs = [oracle_local(w, rk, nml) for rk in w["ranks"]]
    gs = []
    for me, rk in enumerate(w["ranks"]):
        g = run_local(w, rk, nml, me=me)
        g["_set"], g["_idx"] = rk["set"], rk["idx"]
        conv_file, _, _ = check_local(w, g, locs[me])
        gs.append(g)
    infos = [g["tab"].info() for g in gs]
    n_all = torch.stack([dev(_np(i.n_cell, torch.int32, i.ncell)) for i in infos]).contiguous()
    recv = torch.cat([dev(_np(i.sendbuf, torch.float64, i.nsorted * i.ld_send)).view(-1, i.ld_send) for i in infos]).contiguous()
    tot_g = dev(sum(g["tab"].host()["tot_sub"] for g in gs).astype(np.int32).ravel())
    for me, g in enumerate(gs):
        c.set_obs_finish(g["tab"], n_all, recv, tot_g=tot_g)
        torch.cuda.synchronize()
        of = finish_conv(w, locs, me, conv_file)
        check_finish(w, g["tab"], of, conv_file)
    for g in gs:
        g["tab"].close()


def test_handle_tables_drive_das_columns():
    """the handle's letkf_search_tables feed letkf_das_columns_dev: the analysis equals, bit for bit, the same call on tables
    the oracle built and uploaded"""
    from _gpu import ctx, dev, pkg
    c = ctx()
    nml = namelist()
    w = make_world(31, k=10, det_run=False, nfile_rows=(4000, 2000))
    rk = w["ranks"][0]
    o = oracle_local(w, rk, nml)
    of = oracle_finish(w, 0, [o])
    g = run_local(w, rk, nml, both=True)
    t_h = g["tab"].search_tables()
    t = o["tables"]
    d = o["dims"]
    nc = o["nctype"]
    vm = np.array([2 if e == 14593 else 3 if e == 19999 else 1 if ty == 22 else 0
                   for e, ty in zip(t["elm_ctype"], t["typ_ctype"])], np.int32)
    arrs = dict(group_start=np.arange(nc + 1, dtype=np.int32), group_member=np.arange(nc, dtype=np.int32), vmode=vm,
                hori_loc=t["hori_loc_ctype"], vert_loc=t["vert_loc_ctype"], varloc=np.ones(nc),
                max_nobs=nml["max_nobs_per_grid"][t["typ_ctype"] - 1].astype(np.int32), ngrd_i=d["ngrd_i"],
                ngrd_j=d["ngrd_j"], ngrdsch_i=d["ngrdsch_i"], ngrdsch_j=d["ngrdsch_j"], ngrdext_i=d["ngrdext_i"],
                ngrdext_j=d["ngrdext_j"], ac_off=of["ac_off"].astype(np.int64), ac_ext=of["ac_ext"], ob_ri=of["ob_ri"],
                ob_rj=of["ob_rj"], ob_lev=of["ob_lev"], ob_dat=g["tab"].download()["ob_dat"], ob_err=of["ob_err"])
    t_o = pkg.SearchTables()
    keep = []
    for key, v in arrs.items():
        a = dev(np.ascontiguousarray(v))
        keep.append(a)
        setattr(t_o, key, a.data_ptr())
    # the scalars from the world and the namelist (ij_obsgrd_ext, letkf_obs.f90:1221: rank 0 of one rank)
    scal = dict(nctype=nc, ngroup=nc, criterion=nml["criterion"], nlon=w["nlon"], nlat=w["nlat"],
                limit_hint=2 if (arrs["max_nobs"] > 0).any() else 1, dx=nml["dx"], dy=nml["dy"], i_org=w["ihalo"] + 0.5,
                j_org=w["ihalo"] + 0.5, rain_base=nml["rain_base"])
    for key, v in scal.items():
        setattr(t_o, key, v)
        assert getattr(t_h, key) == v, key
    dl = g["tab"].download()
    k, nv, nlev = w["k"], 11, 3
    nens = k + 1
    nij1 = w["nlon"] * w["nlat"]
    npts = nij1 * nlev
    rng = np.random.default_rng(3)
    gi, gj = np.meshgrid(np.arange(w["nlon"]), np.arange(w["nlat"]), indexing="xy")
    rig = dev(w["ihalo"] + 1.0 + gi.ravel().astype(np.float64))
    rjg = dev(w["ihalo"] + 1.0 + gj.ravel().astype(np.float64))
    rlev = dev(np.repeat([90000.0, 60000.0, 30000.0], nij1))
    rz = dev(np.repeat([1000.0, 4000.0, 9000.0], nij1))
    sv, sm, sp = 1, nv, nens * nv
    gues = dev(rng.normal(0.0, 1.0, npts * sp))
    c.ens_mean(k, nv, npts, gues, sp, sm, sv)
    c.to_perturbations(k, nv, npts, gues, sp, sm, sv)
    ens, dep = dev(dl["ensval"]), dev(dl["val"])
    out = []
    for tabs in (t_h, t_o):
        anal = torch.zeros_like(gues)
        infl = torch.ones(npts * nv, dtype=torch.float64, device="cuda")
        st = torch.zeros(npts, dtype=torch.int32, device="cuda")
        nob = torch.zeros(npts, dtype=torch.int32, device="cuda")
        c.das_columns(k, nv, tabs, nij1, nlev, rig, rjg, rlev, rz, ens, w["kld"], dep, infl, gues, anal, sp, sm, sv,
                      nobs_out=nob, status=st, relax_alpha_spread=0.95)
        torch.cuda.synchronize()
        out.append((anal.cpu().numpy(), nob.cpu().numpy(), st.cpu().numpy()))
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])
    assert out[0][1].sum() > 0 and np.abs(out[0][2]).max() == 0
    g["tab"].close()
