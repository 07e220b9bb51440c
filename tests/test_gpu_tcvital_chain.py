"""A TC vitals report from the file to the analysis' table, on the 12 x 10 x 4 domain of tests/test_gpu_obsope_chain.py:
Context.obs_decode (lon / lat to x / y in metres, OBSERR_TCX/TCY/TCP) -> Context.phys2ij -> Context.obsope (the three rows get
qc 90) -> Context.tcvital_rows / tcvital_search / tcvital_fill -> Context.set_obs.  The three rows survive QC with the departures
the restatement of tests/_tcvital.py gives; without the fill they stay at qc 90 and never reach the table, as before."""
import ctypes as C

import numpy as np
import pytest
import torch

import _mapproj as M
import _obsfile as F
import _obsope as O
import _tcvital as T
from _setobs import namelist, qc_of, setobs_params

pytestmark = pytest.mark.gpu
K = 4
CONFIG = "BDA_d3_1km_9p_bf20"
TYP_TCVITL = 24


def test_a_tc_vitals_report_reaches_the_table():
    from _gpu import ctx, dev, pkg
    c, device = ctx(), torch.device("cuda:0")
    g = O.make_grid(4, khalo=2, nlon=12, nlat=10, ihalo=2, jhalo=2)
    v3, v2 = O.make_fields(g, K, 21)
    assert T.FIXTURES["chain"] == (12, 10, 2, 2, K, 31)                                  # (tests/test_tcvital_statement.py pins its gaps)
    low, ci, cj = T.low_fixture(*T.FIXTURES["chain"])
    for iv in (T.IV_TOPO, T.IV_PS, T.IV_T2M, T.IV_Q2M):
        v2[:, iv] = low[:, iv]
    # the file: an older TCX row of another time, then the report; lon / lat of a point near the members' lows
    mp = M.configs()[CONFIG]
    q = M.setup(mp)
    where = M.ij2phys(q, np.array([6.3]), np.array([5.4]))
    lon, lat = float(np.float32(where["lon"][0])), float(np.float32(where["lat"][0]))
    tp = dict(dx=mp["dx"], dy=mp["dy"], cxg1=mp["cxg1"], cyg1=mp["cyg1"], i_off=0, j_off=0, tc_search_dis=200.0e3)
    rec = np.array([[T.ID_TCX, lon, lat, 1000.0, 0.0, 0.0, TYP_TCVITL, 3.0],
                    [T.ID_TCX, lon, lat, 1000.0, 0.0, 0.0, TYP_TCVITL, 0.0],
                    [T.ID_TCY, lon, lat, 1000.0, 0.0, 0.0, TYP_TCVITL, 0.0],
                    [T.ID_TCP, lon, lat, 1000.0, 985.0, 0.0, TYP_TCVITL, 0.0]], dtype=np.float32)
    n = len(rec)
    image = torch.from_numpy(np.frombuffer(F.frame(rec), dtype=np.uint8).copy()).cuda()
    proj = pkg.mapproj_setup(**M.setup_args(mp))

    def chain(with_fill):
        cols = c.obs_decode(image, F.CONV, proj=proj)                                   # 1. read_obs
        ri, rj, rotc = c.phys2ij(proj, cols["lon"], cols["lat"])                        # 2. phys2ij
        # 3. the operator for all members: the TC rows are not its own
        off = np.array([0, n], dtype=np.int64)
        files = pkg.ObsFileRows()
        files.nfile, files.off = 1, off.ctypes.data_as(C.c_void_p)
        for name, t in (("elm", cols["elm"]), ("typ", cols["typ"]), ("lev", cols["lev"]), ("dat", cols["dat"]), ("err", cols["err"]),
                        ("ri", ri), ("rj", rj)):
            setattr(files, name, C.c_void_p(t.data_ptr()))
        set_ = torch.ones(n, dtype=torch.int32, device=device)
        idx = torch.arange(1, n + 1, dtype=torch.int32, device=device)
        cfg = O.default_cfg(ri_off=0.0, rj_off=0.0, use_obs=np.ones(O.NOBTYPE, dtype=np.int32))
        case = dict(g=g, v3=v3, v2=v2, nmem=K, nrow=n, off=off, set=np.ones(n, dtype=np.int32), idx=np.arange(1, n + 1, dtype=np.int32),
                    files=dict(lon=np.zeros(n), lat=np.zeros(n)), rotc=np.zeros((n, 2)), file_radar=np.array([-1], dtype=np.int32))
        dc = O.DeviceCase(pkg, case, cfg, device)                                       # (the fields and the operator's parameters)
        dc.params.lon, dc.params.lat = C.c_void_p(cols["lon"].data_ptr()), C.c_void_p(cols["lat"].data_ptr())
        dc.params.rotc = C.c_void_p(rotc.data_ptr())
        ens = torch.zeros((n, K), dtype=torch.float64, device=device)
        qc = torch.zeros(n, dtype=torch.int32, device=device)
        c.obsope(dc.params, files, dc.fields, set_, idx, qc, ens, K)
        torch.cuda.synchronize()
        assert qc.cpu().numpy().tolist() == [90] * n                                    # today's behaviour, and it stays
        cand = None
        if with_fill:
            rows, valid = c.tcvital_rows(cols["elm"], cols["dif"], -0.5, 0.5)           # 4. rows, search, fill
            assert rows.tolist() == [2, 3, 4] and valid
            tps = pkg.TcvitalParams()
            for k, val in tp.items():
                setattr(tps, k, val)
            r = int(rows[0]) - 1
            cand = c.tcvital_search(tps, dc.fields, ri[r:r + 1], rj[r:r + 1])           # (the centre stays on the device)
            c.tcvital_fill(cand[None], rows - 1, qc, ens, K, qc_replace=True)           # (obsda row = file row here)
        w = dict(nlon=12, nlat=10, ihalo=2, px=1, py=1, k=K, kld=K, det_run=False, h08=False)
        p, keep = setobs_params(pkg.SetObsParams, w, namelist())
        qp = qc_of(w)
        zeros = dev(np.zeros(n))
        qp.h08_lev, qp.h08_val2 = zeros.data_ptr(), None
        ens_in = ens.clone()
        tab = c.set_obs(p, qp, files, set_, idx, qc, ens, K, keep=(keep, dc, zeros, qc, ens, cols, ri, rj, rotc, off))   # 5. set_letkf_obs
        torch.cuda.synchronize()
        return tab, cols, ri, rj, ens_in, cand

    tab, cols, ri, rj, ens_in, cand = chain(True)
    ri_h, rj_h = ri.cpu().numpy(), rj.cpu().numpy()
    assert abs(ri_h[1] - 6.3) < 0.05 and abs(rj_h[1] - 5.4) < 0.05                      # (the file holds lon / lat in single precision)
    want = T.search(v2, 12, 10, 2, 2, tp, ri_h[1], rj_h[1])
    got = cand.cpu().numpy()
    assert np.array_equal(got[:, :2].view(np.int64), want[:, :2].view(np.int64))
    assert (np.abs(got[:, 2] - want[:, 2]) <= 64 * T.EPS * want[:, 2]).all()
    hd, dd = tab.host(), tab.download()
    assert hd["nobstotal"] == 3 and hd["nobs"] == 4
    assert (dd["qc"] == 0).all()
    dat = cols["dat"].cpu().numpy()
    assert dat[3] == float(np.float32(985.0) * np.float32(100.0)) and cols["err"].cpu().numpy()[1:].tolist() == [50.0e3, 50.0e3, 5.0e2]
    # the table's rows are the report's three, each with the departure obs - mean of the restatement's values
    order = [int(np.flatnonzero(dat[1:] == x)[0]) for x in dd["ob_dat"]]
    assert sorted(order) == [0, 1, 2]
    for row, comp in enumerate(order):
        dep = dat[1 + comp] - want[:, comp].mean()
        tol = 64 * T.EPS * np.abs(want[:, comp]).max() + 8 * T.EPS * max(abs(dat[1 + comp]), np.abs(want[:, comp]).max())
        assert abs(dd["val"][row] - dep) <= tol, (comp, dd["val"][row], dep)
        assert np.all(np.abs(dd["ensval"][row] - (want[:, comp] - want[:, comp].mean())) <= tol), comp
    assert abs(dd["val"][order.index(2)]) < 2500.0 and np.abs(dd["val"]).max() < 250.0e3    # inside GROSS_ERROR_TCP / TCX / TCY
    # without the fill: qc 90 on all four, nothing for the analysis
    tab0 = chain(False)[0]
    assert tab0.host()["nobstotal"] == 0
