"""A Himawari-8 file from its bytes to the analysis' table, on the 12 x 10 x 4 domain of tests/test_gpu_obsope_chain.py:
Context.h08_decode -> Context.phys2ij -> Context.obsope (all rows; the H08 rows are not its own) -> Context.h08_select ->
Context.h08_profiles -> the stand-in of tests/_h08.py where the host calls RTTOV -> Context.h08_rows -> Context.set_obs with
letkf_qc_params.h08 = 1, h08_lev and h08_val2.  The used channel's rows reach the table with the departures, the levels and the
clear-sky values of the restatement; without h08_rows they keep the operator's code and never reach the table, as before."""
import ctypes as C

import numpy as np
import pytest
import torch

import _h08 as H
import _mapproj as M
import _obsope as O
from _setobs import namelist, qc_of, setobs_params

pytestmark = pytest.mark.gpu
K, NLEV, NPROF, USED = 4, 4, 40, 3
CONFIG = "BDA_d3_1km_9p_bf20"


def test_a_himawari_file_reaches_the_table():
    from _gpu import ctx, dev, pkg
    from test_gpu_h08 import fields_of, params_of
    c, device = ctx(), torch.device("cuda:0")
    g = H.make_grid(NLEV)
    v3, v2 = H.make_fields(g, K, 21)
    mp = M.configs()[CONFIG]
    proj = pkg.mapproj_setup(**M.setup_args(mp))
    rng = np.random.default_rng(5)
    where = M.ij2phys(M.setup(mp), 2.6 + rng.uniform(0.0, 11.8, NPROF), 2.6 + rng.uniform(0.0, 9.8, NPROF))
    obserr = np.full(H.NCH, 3.0)
    use = tuple(int(ch == USED) for ch in range(H.NCH))
    p = H.params(nlev=NLEV, nprof_file=NPROF, top_down=1, rttov_units=1, reject_land=1, finish=1, member=K, ch_use=use, cldsky_thrs=1.0,
                 **H.BUFFER)
    n = NPROF * H.NCH
    off = np.array([0, n], dtype=np.int64)
    set_h, idx_h = np.ones(n, dtype=np.int32), np.arange(1, n + 1, dtype=np.int32)

    def image_of(dat):
        cols = dict(elm=np.full(n, H.ID_H08, dtype=np.int32), typ=np.full(n, H.TYP_H08, dtype=np.int32), lon=np.repeat(where["lon"], H.NCH),
                    lat=np.repeat(where["lat"], H.NCH), dat=dat)
        return torch.from_numpy(H.encode(cols, False)).cuda()

    def chain(image, with_rows):
        assert pkg.h08_count(image.numel()) == NPROF
        cols = c.h08_decode(image, obserr, check=True)                                   # 1. read_obs_H08
        assert cols["nbad"] == 0
        ri, rj, rotc = c.phys2ij(proj, cols["lon"], cols["lat"])                        # 2. phys2ij
        files = pkg.ObsFileRows()                                                       # 3. the operator for all members
        files.nfile, files.off = 1, off.ctypes.data_as(C.c_void_p)
        for name, t in (("elm", cols["elm"]), ("typ", cols["typ"]), ("lev", cols["lev"]), ("dat", cols["dat"]), ("err", cols["err"]),
                        ("ri", ri), ("rj", rj)):
            setattr(files, name, C.c_void_p(t.data_ptr()))
        set_, idx = dev(set_h), dev(idx_h)
        cfg = O.default_cfg(ri_off=0.0, rj_off=0.0, use_obs=np.ones(O.NOBTYPE, dtype=np.int32))
        case = dict(g=g, v3=v3, v2=v2, nmem=K, nrow=n, off=off, set=set_h, idx=idx_h, files=dict(lon=np.zeros(n), lat=np.zeros(n)),
                    rotc=np.zeros((n, 2)), file_radar=np.array([-1], dtype=np.int32))
        dc = O.DeviceCase(pkg, case, cfg, device)                                       # (the fields on the device, the operator's parameters)
        f = fields_of(pkg, g, K, dc.d3, dc.d2, H.reference_strides(g))                  # (nine 2-D variables: lsmask, skint)
        dc.params.lon, dc.params.lat = C.c_void_p(cols["lon"].data_ptr()), C.c_void_p(cols["lat"].data_ptr())
        dc.params.rotc = C.c_void_p(rotc.data_ptr())
        ens = torch.zeros((n, K), dtype=torch.float64, device=device)
        qc = torch.zeros(n, dtype=torch.int32, device=device)
        c.obsope(dc.params, files, f, set_, idx, qc, ens, K)
        torch.cuda.synchronize()
        assert (qc.cpu().numpy() != 0).all()                                            # today's behaviour, and it stays
        lev, val2 = torch.zeros(n, dtype=torch.float64, device=device), torch.zeros(n, dtype=torch.float64, device=device)
        rip, rjp = ri[::H.NCH].contiguous(), rj[::H.NCH].contiguous()                   # per file profile: its first row's
        lonp, latp, rotp = cols["lon"][::H.NCH].contiguous(), cols["lat"][::H.NCH].contiguous(), rotc[::H.NCH].contiguous()
        got = None
        if with_rows:
            pl, slot, nsel = c.h08_select(set_, idx, 1, NPROF)                          # 4. select, profiles, RTTOV's stand-in, rows
            assert nsel == NPROF
            ps = params_of(pkg, p)
            prof = c.h08_profiles(ps, f, nsel, pl, rip, rjp, lonp, latp, rotp)
            torch.cuda.synchronize()
            host = {k: (None if t is None else t.cpu().numpy()) for k, t in prof.items()}
            rt = H.stand_in(host, p)                                                    # (the host's part: download, RTTOV, upload)
            c.h08_rows(ps, set_, idx, 1, slot, nsel, prof, dev(rt[0]), dev(rt[1]), dev(rt[2]), rip, rjp, qc, ens, K, lev, val2)
            torch.cuda.synchronize()
            got = dict(prof=host, rt=rt, qc=qc.cpu().numpy(), ens=ens.cpu().numpy(), lev=lev.cpu().numpy(), val2=val2.cpu().numpy())
        w = dict(nlon=12, nlat=10, ihalo=2, px=1, py=1, k=K, kld=K, det_run=False, h08=True)
        sp, keep = setobs_params(pkg.SetObsParams, w, namelist())
        qp = qc_of(w)
        qp.h08_lev, qp.h08_val2 = lev.data_ptr(), val2.data_ptr()
        tab = c.set_obs(sp, qp, files, set_, idx, qc, ens, K, keep=(keep, dc, f, lev, val2, qc, ens, cols, ri, rj, rotc, off))   # 5. set_letkf_obs
        torch.cuda.synchronize()
        return tab, got, (rip.cpu().numpy(), rjp.cpu().numpy(), lonp.cpu().numpy(), latp.cpu().numpy(), rotp.cpu().numpy()), val2.cpu().numpy()

    # the positions as the file holds them, and from them the restatement of the whole operator
    _, _, (ri, rj, lon, lat, rotc), _ = chain(image_of(np.full(n, 250.0)), False)
    assert np.all((ri > 2.5) & (ri < 14.5) & (rj > 2.5) & (rj < 12.5))
    prof_list = np.arange(NPROF, dtype=np.int32)
    want_prof = H.profiles(p, g, v3, v2, prof_list, ri, rj, lon, lat, rotc)
    rt = H.stand_in(want_prof, p)
    state = (np.full(n, 90, dtype=np.int32), np.zeros((n, K)), np.zeros(n), np.zeros(n))
    qc_w, ens_w, lev_w, val2_w = (a.copy() for a in state)
    H.rows(p, 0, n, set_h, idx_h, 1, prof_list, NPROF, K, 0, want_prof, *rt, ri, rj, True, qc_w, ens_w, lev_w, val2_w)
    good = np.flatnonzero(qc_w == 0)
    assert 10 <= good.size < NPROF and np.all(good % H.NCH == USED)                      # land and buffer profiles are out
    assert set(np.unique(qc_w)) == {0, 50}
    # the observations: the members' mean brightness temperature plus noise well inside the gross-error bound
    dat = np.full(n, 250.0)
    dat[good] = np.abs(ens_w[good]).mean(axis=1) + rng.uniform(-1.0, 1.0, good.size)
    dat = dat.astype(np.float32).astype(np.float64)

    tab, got, _, ca = chain(image_of(dat), True)
    from test_gpu_h08 import same
    assert np.array_equal(got["qc"], qc_w) and same(got["ens"], ens_w) and same(got["lev"], lev_w) and same(got["val2"], val2_w)
    hd, dd = tab.host(), tab.download()
    assert hd["nobs"] == n and hd["nobstotal"] == good.size
    assert (dd["qc"] == 0).all()
    key = {(ri[r // H.NCH], rj[r // H.NCH]): r for r in good}
    rows = np.array([key[(a, b)] for a, b in zip(dd["ob_ri"], dd["ob_rj"])])
    assert sorted(rows.tolist()) == good.tolist()
    assert np.array_equal(dd["ob_lev"], lev_w[rows]) and np.all(lev_w[rows] >= 20000.0)  # localised with the weighting function's peak
    assert np.array_equal(dd["ob_dat"], dat[rows]) and np.all(dd["ob_err"] == 3.0)
    bt = np.abs(ens_w[rows])                                                             # the sign (cloudy) is restored before the mean
    mean = bt.mean(axis=1)
    tol = 8 * H.EPS * bt.max()
    assert np.all(np.abs(dd["val"] - (dat[rows] - mean)) <= tol) and np.all(np.abs(dd["val"]) <= 1.0 + tol)
    assert np.all(np.abs(dd["ensval"] - (bt - mean[:, None])) <= tol)
    want_ca = (np.abs(mean - val2_w[rows]) + np.abs(dat[rows] - val2_w[rows])) * 0.5     # letkf_obs.f90:480-487 on the clear-sky mean
    assert np.all(np.abs(ca[rows] - want_ca) <= tol)
    assert (ens_w[rows] < 0.0).any() and (ens_w[rows] > 0.0).any()                       # both skies among the rows that arrive
    # without the rows entry: the operator's code on every row, nothing for the analysis
    tab0 = chain(image_of(dat), False)[0]
    assert tab0.host()["nobstotal"] == 0
