"""Context.obsope -> Context.set_obs -> Context.state_to_history -> Context.monit_obs on the 12 x 10 x 4 domain of
tests/test_gpu_obsope_chain.py: the monitor runs over the rows the table's key names (info.key / info.nsorted), on the files as
set_obs pre-processed them (reflectivities in dBZ, elements rewritten), with the history fields built on the device from a mean
state.  Compared with the statement on the same rows, dat and elm read back after the pre-processing."""
import ctypes as C

import numpy as np
import pytest
import torch

import _monit as M
import _obsope as O
from _setobs import namelist, qc_of, setobs_params
from test_gpu_obsope_chain import K, chain_case, observed

pytestmark = pytest.mark.gpu
STATE_SEED = 61      # under it no row of the chain's fixture lies within 1e-6 of a comparison (asserted below)


def test_the_monitor_runs_on_the_tables_key_and_the_preprocessed_files():
    from _gpu import ctx, dev, pkg
    c, device = ctx(), torch.device("cuda:0")
    case = chain_case()
    g = case["g"]
    cfg = O.default_cfg(method_ref_calc=2, ri_off=0.0, rj_off=0.0, use_obs=np.ones(O.NOBTYPE, dtype=np.int32), min_radar_ref_dbz=5.0,
                        low_ref_shift=-1.0)
    dat, err = observed(case, O.statement(case, cfg), np.random.default_rng(3))
    dc = O.DeviceCase(pkg, dict(case, files=dict(case["files"], dat=dat.copy(), err=err.copy())), cfg, device)
    # 1. the operator on the K members, 2. set_letkf_obs (pre-processes the files in place)
    ens_d = torch.zeros((case["nrow"], K), dtype=torch.float64, device=device)
    qc_d = torch.zeros(case["nrow"], dtype=torch.int32, device=device)
    c.obsope(dc.params, dc.files, dc.fields, dc.set, dc.idx, qc_d, ens_d, K)
    w = dict(nlon=12, nlat=10, ihalo=2, px=1, py=1, k=K, kld=K, det_run=False, h08=False)
    p, keep = setobs_params(pkg.SetObsParams, w, namelist())
    q = qc_of(w)
    zeros = dev(np.zeros(case["nrow"]))
    q.h08_lev, q.h08_val2 = zeros.data_ptr(), None
    tab = c.set_obs(p, q, dc.files, dc.set, dc.idx, qc_d, ens_d, K, keep=(keep, dc, zeros, qc_d, ens_d))
    info = tab.info()
    nn = int(info.nsorted)
    assert nn > 100
    # the key on the host: identity gathered through it
    ident, key_t = dev(np.arange(case["nrow"], dtype=np.int32)), torch.zeros(nn, dtype=torch.int32, device=device)
    assert pkg.lib().letkf_obs_gather_i32_dev(c._c, nn, C.c_void_p(info.key), C.c_void_p(ident.data_ptr()), C.c_void_p(key_t.data_ptr())) == 0
    torch.cuda.synchronize()
    key = key_t.cpu().numpy()
    back = {n: dc.d[n].cpu().numpy() for n in ("elm", "typ", "lev", "ri", "rj", "dat")}
    assert not np.array_equal(back["dat"], dat)                                   # (reflectivities are dBZ now)
    # 3. the monitor on a mean state's history, built on the device
    st = M.make_state(g, STATE_SEED)
    ds = M.DeviceState(pkg, st, device)
    fl = M.hist_layout(pkg, g)
    d3 = torch.full((O.NV3DD * g["nlath"] * g["nlonh"] * g["nlevh"],), np.nan, dtype=torch.float64, device=device)
    d2 = torch.full((O.NV2DD * g["nlath"] * g["nlonh"],), np.nan, dtype=torch.float64, device=device)
    fl.v3d, fl.v2d = C.c_void_p(d3.data_ptr()), C.c_void_p(d2.data_ptr())
    c.state_to_history(ds.hs, fl, d3, d2)
    dc.params.stggrd = 1
    mcfg = M.default_mcfg(key=key)
    mp, od, rec_t, ids = M.monit_structs(pkg, dc, mcfg, 1, nn, device)
    nobs, bias, rmse = c.monit_obs(mp, dc.params, dc.files, fl, dc.set, dc.idx, od, key=int(info.key), nn=nn)
    torch.cuda.synchronize()
    got = dict(rec={n: t.cpu().numpy()[:nn] for n, t in rec_t.items()}, nobs=nobs.cpu().numpy(), bias=bias.cpu().numpy(),
               rmse=rmse.cpu().numpy())
    # the statement on the same rows, the files as read back
    rows = []
    for n, r in enumerate(case["rows"]):
        fr = int(case["off"][case["set"][n] - 1] + case["idx"][n] - 1)
        rows.append(dict(r, dif=0.0, **{name: back[name][fr].item() for name in back}))
    scase = dict(case, rows=rows)
    want = M.monit(dict(cfg, stggrd=1), mcfg, scase, M.history(st, g), 1, None)
    assert want["dist"].min() >= 1e-6, want["dist"].min()
    # U T REF Vr are counted; the stations' heights belong to the members' terrain, far from this state's first level: qc 10
    assert (want["qc"] == 0).sum() > 80 and want["nobs"][[0, 2, 8, 10]].all() and (want["qc"] == O.QC_PS_TER).any()
    assert M.compare(got, want, 1) == []
