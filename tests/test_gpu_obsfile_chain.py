"""The two-program workflow through the record codec, on the 12 x 10 x 4 domain of tests/test_gpu_obsope_chain.py:
Context.obsope -> one obsda file image per member and one for the mean (Context.obsda_encode) -> Context.obsda_assemble ->
Context.set_obs, then Context.monit_obs -> Context.obsdep_encode.  The assembled ensval is float64(float32(operator's ensval))
bit for bit -- the files hold single precision --, set / idx / qc are the operator's, set_obs builds a table from the result, and
the departure file is the statement's (tests/_obsfile.py) of the monitor's outputs and the files as set_obs left them."""
import ctypes as C

import numpy as np
import pytest
import torch

import _monit as M
import _obsfile as F
import _obsope as O
from _setobs import namelist, qc_of, setobs_params
from test_gpu_obsope_chain import K, chain_case, observed

pytestmark = pytest.mark.gpu
STATE_SEED = 61      # tests/test_gpu_monit_chain.py's


def test_operator_files_assemble_set_obs_and_the_departure_file():
    from _gpu import ctx, dev, pkg
    c, device = ctx(), torch.device("cuda:0")
    case = chain_case()
    g, nrow = case["g"], case["nrow"]
    cfg = O.default_cfg(method_ref_calc=2, ri_off=0.0, rj_off=0.0, use_obs=np.ones(O.NOBTYPE, dtype=np.int32), min_radar_ref_dbz=5.0,
                        low_ref_shift=-1.0)
    dat, err = observed(case, O.statement(case, cfg), np.random.default_rng(3))
    files = dict(case["files"], dat=dat.copy(), err=err.copy(), dif=np.zeros(nrow))
    dc = O.DeviceCase(pkg, dict(case, files=files), cfg, device)
    # 1. obsope: the operator, then write_obs_da per member and for the mean
    ens_d = torch.zeros((nrow, K), dtype=torch.float64, device=device)
    qc_d = torch.zeros(nrow, dtype=torch.int32, device=device)
    c.obsope(dc.params, dc.files, dc.fields, dc.set, dc.idx, qc_d, ens_d, K)
    mean_d = ens_d.mean(dim=1)
    images = [c.obsda_encode(dc.set, dc.idx, qc_d, ensval=ens_d, col=m) for m in range(K)]
    images.append(c.obsda_encode(dc.set, dc.idx, qc_d, val=mean_d, col=-1))
    torch.cuda.synchronize()
    ens_h, qc_h = ens_d.cpu().numpy(), qc_d.cpu().numpy()
    for m in range(K):
        assert images[m].cpu().numpy().tobytes() == F.frame(F.encode_obsda(case["set"], case["idx"], ens_h[:, m], qc_h))
    # 2. letkf: the files assembled, the mean's into the last column
    res = c.obsda_assemble(images, nrow, K + 1, col=np.arange(K + 1), check=True)
    torch.cuda.synchronize()
    assert (res["nbad"], res["ninconsistent"]) == (0, 0)
    got = res["ensval"].cpu().numpy()
    assert F.same_bits(got[:, :K], ens_h.astype(np.float32).astype(np.float64))
    assert F.same_bits(got[:, K], mean_d.cpu().numpy().astype(np.float32).astype(np.float64))
    assert np.array_equal(res["set"].cpu().numpy(), case["set"]) and np.array_equal(res["idx"].cpu().numpy(), case["idx"])
    assert np.array_equal(res["qc"].cpu().numpy(), qc_h) and (qc_h == 0).sum() > 150
    # 3. set_letkf_obs accepts what the members' files gave
    mem = c.obsda_assemble(images[:K], nrow, K)
    w = dict(nlon=12, nlat=10, ihalo=2, px=1, py=1, k=K, kld=K, det_run=False, h08=False)
    p, keep = setobs_params(pkg.SetObsParams, w, namelist())
    q = qc_of(w)
    zeros = dev(np.zeros(nrow))
    q.h08_lev, q.h08_val2 = zeros.data_ptr(), None
    tab = c.set_obs(p, q, dc.files, mem["set"], mem["idx"], mem["qc"], mem["ensval"], K, keep=(keep, dc, zeros, mem))
    info = tab.info()
    nn = int(info.nsorted)
    assert nn > 100 and int(info.nobs) == nrow
    # 4. the monitor on a mean state's history, then write_obs_dep
    ident, key_t = dev(np.arange(nrow, dtype=np.int32)), torch.zeros(nn, dtype=torch.int32, device=device)
    assert pkg.lib().letkf_obs_gather_i32_dev(c._c, nn, C.c_void_p(info.key), C.c_void_p(ident.data_ptr()), C.c_void_p(key_t.data_ptr())) == 0
    torch.cuda.synchronize()
    st = M.make_state(g, STATE_SEED)
    ds = M.DeviceState(pkg, st, device)
    fl = M.hist_layout(pkg, g)
    d3 = torch.full((O.NV3DD * g["nlath"] * g["nlonh"] * g["nlevh"],), np.nan, dtype=torch.float64, device=device)
    d2 = torch.full((O.NV2DD * g["nlath"] * g["nlonh"],), np.nan, dtype=torch.float64, device=device)
    fl.v3d, fl.v2d = C.c_void_p(d3.data_ptr()), C.c_void_p(d2.data_ptr())
    c.state_to_history(ds.hs, fl, d3, d2)
    dc.params.stggrd = 1
    mp, od, rec_t, ids = M.monit_structs(pkg, dc, M.default_mcfg(key=key_t.cpu().numpy()), 1, nn, device)
    c.monit_obs(mp, dc.params, dc.files, fl, mem["set"], mem["idx"], od, key=int(info.key), nn=nn)
    rows = pkg.obsfile_rows(case["off"], {k: dc.d[k] for k in F.COLUMNS})
    rec = {k: t[:nn].contiguous() for k, t in rec_t.items()}
    image = c.obsdep_encode(rec["set"], rec["idx"], rec["qc"], rec["omb"], rec["oma"], rows)
    torch.cuda.synchronize()
    back = {k: dc.d[k].cpu().numpy() for k in F.COLUMNS}
    assert not np.array_equal(back["dat"], dat)                                   # (set_obs made the reflectivities dBZ)
    h = {k: t.cpu().numpy() for k, t in rec.items()}
    want = F.encode_dep(h["set"], h["idx"], h["qc"], h["omb"], h["oma"], case["off"], back)
    assert len(want) == nn and (h["qc"] == 0).sum() > 80
    assert image.cpu().numpy().tobytes() == F.frame(want)
