"""Context.obsope -> Context.set_obs on a 12 x 10 x 4 domain: the chain that replaces CALL obsope_cal and CALL set_letkf_obs.
The table built from the device operator's ensval / qc is compared with the one built, by the same set_obs, from the numpy
statement's ensval / qc: the QC flags, counts, keys and the sorted metadata bit for bit, ensval (perturbations) and the
departures within the operator's tolerances (tests/test_gpu_obsope.py) carried through the mean: a perturbation differs by at
most its own row's tolerance plus the mean's, i.e. twice the largest tolerance of the row, plus 8 ulp of the values."""
import numpy as np
import pytest
import torch

import _obsope as O
from _setobs import namelist, qc_of, setobs_params

pytestmark = pytest.mark.gpu
K = 4


def chain_case(seed=21):
    g = O.make_grid(4, khalo=2, nlon=12, nlat=10, ihalo=2, jhalo=2)
    v3, v2 = O.make_fields(g, K, seed)
    rng = np.random.default_rng(seed + 1)
    radars = np.array([[135.0, 35.0, 50.0]])
    rows = []
    for file, elm, typ, n in ((0, O.ID_REF, 22, 60), (0, O.ID_VR, 22, 40), (1, O.ID_U, 1, 30), (1, O.ID_T, 1, 30), (1, O.ID_PS, 8, 20)):
        for _ in range(n):
            ri, rj = 2.6 + rng.uniform(0.0, 11.8), 2.6 + rng.uniform(0.0, 9.8)
            if elm == O.ID_PS:
                lev = O.itpl_2d(v2[0, O.V2_TOPO], ri, rj)[0] + rng.uniform(-60.0, 60.0)
            else:
                lo, hi, _ = O._level_range(v3[0, O.V_HGT if file == 0 else O.V_P], file == 0, ri, rj, g)
                x = lo + rng.uniform(0.1, 0.9) * (hi - lo)
                lev = x if file == 0 else float(np.exp(x))
            rows.append(dict(file=file, elm=elm, typ=typ, lev=float(lev), ri=ri, rj=rj, lon=135.4 + 0.01 * ri, lat=35.3 + 0.01 * rj,
                             radar=tuple(radars[0]) if file == 0 else None, tag="chain"))
    nrow = len(rows)
    n0 = sum(r["file"] == 0 for r in rows)
    off = np.array([0, n0, nrow], dtype=np.int64)
    files = {n: np.array([r[n] for r in rows], dtype=np.int32 if n in ("elm", "typ") else np.float64)
             for n in ("elm", "typ", "lev", "ri", "rj", "lon", "lat")}
    order = rng.permutation(nrow)
    set_ = np.array([rows[r]["file"] + 1 for r in order], dtype=np.int32)
    idx = np.array([r + 1 - off[rows[r]["file"]] for r in order], dtype=np.int32)
    case = dict(g=g, v3=v3, v2=v2, nmem=K, rows=[rows[r] for r in order], nrow=nrow, off=off, files=files, set=set_, idx=idx,
                rotc=np.tile(np.array([1.0, 0.0]), (nrow, 1)), file_radar=np.array([0, -1], dtype=np.int32), radars=radars,
                order=order)
    return case


def observed(case, st, rng):
    """dat / err of the files: the statement's ensemble mean plus noise (reflectivity as raw mm^6 m^-3, as the files hold it)"""
    mean = st["val"].mean(axis=1)
    dat, err = np.zeros(case["nrow"]), np.zeros(case["nrow"])
    for n, fr in enumerate(case["order"]):
        elm = case["rows"][n]["elm"]
        sig = {O.ID_REF: 2.0, O.ID_VR: 1.0, O.ID_U: 1.0, O.ID_T: 0.5, O.ID_PS: 50.0}[elm]
        y = mean[n] + sig * rng.standard_normal()
        dat[fr], err[fr] = (10.0 ** (y / 10.0) if elm == O.ID_REF else y), 2.0 * sig
    return dat, err


def test_operator_then_set_obs_builds_the_statements_table():
    from _gpu import ctx, dev, pkg
    c = ctx()
    case = chain_case()
    cfg = O.default_cfg(method_ref_calc=2, ri_off=0.0, rj_off=0.0, use_obs=np.ones(O.NOBTYPE, dtype=np.int32), min_radar_ref_dbz=5.0,
                        low_ref_shift=-1.0)
    st = O.statement(case, cfg)
    assert st["dist"].min() >= 1e-6
    assert (st["qc"] == 0).sum() > 150
    dat, err = observed(case, st, np.random.default_rng(3))
    w = dict(nlon=12, nlat=10, ihalo=2, px=1, py=1, k=K, kld=K, det_run=False, h08=False)
    nml = namelist()

    def table(ensval, qc):
        """set_obs on fresh copies of the files (it pre-processes them in place)"""
        files = dict(case["files"], dat=dat.copy(), err=err.copy())
        dc = O.DeviceCase(pkg, dict(case, files=files), cfg, torch.device("cuda:0"))
        p, keep = setobs_params(pkg.SetObsParams, w, nml)
        q = qc_of(w)
        zeros = dev(np.zeros(case["nrow"]))
        q.h08_lev, q.h08_val2 = zeros.data_ptr(), None
        tab = c.set_obs(p, q, dc.files, dc.set, dc.idx, qc, ensval, K, keep=(keep, dc, zeros, qc, ensval))
        torch.cuda.synchronize()
        return tab

    # the chain on the device: the operator reads the files before set_obs pre-processes them
    files = dict(case["files"], dat=dat.copy(), err=err.copy())
    dc = O.DeviceCase(pkg, dict(case, files=files), cfg, torch.device("cuda:0"))
    ens_d = torch.zeros((case["nrow"], K), dtype=torch.float64, device="cuda")
    qc_d = torch.zeros(case["nrow"], dtype=torch.int32, device="cuda")
    c.obsope(dc.params, dc.files, dc.fields, dc.set, dc.idx, qc_d, ens_d, K)
    torch.cuda.synchronize()
    assert O.compare(ens_d.cpu().numpy(), qc_d.cpu().numpy(), st) == []
    tab_d = table(ens_d, qc_d)
    tab_s = table(dev(st["val"]), dev(st["qc"].astype(np.int32)))

    hd, hs = tab_d.host(), tab_s.host()
    for name in ("nctype", "nobs", "nsorted", "ncell", "nacx", "nobstotal", "kld"):
        assert hd[name] == hs[name], name
    for name in ("elm_ctype", "typ_ctype", "ngrd_i", "ngrd_j", "tot_sub", "tot_g", "ctype_elmtyp"):
        assert np.array_equal(hd[name], hs[name]), name
    assert hd["nobstotal"] > 100
    dd, ds = tab_d.download(), tab_s.download()
    for name in ("qc", "ob_ri", "ob_rj", "ob_lev", "ob_dat", "ob_err", "ac_ext"):
        assert np.array_equal(dd[name], ds[name]), name
    # the sorted rows are the same obsda rows in the same order: find each one's tolerance through its coordinates
    key = {(r["ri"], r["rj"], r["lev"]): n for n, r in enumerate(case["rows"])}
    rows = np.array([key[(a, b, l)] for a, b, l in zip(dd["ob_ri"], dd["ob_rj"], dd["ob_lev"])])
    tol = 2.0 * st["tol"][rows].max(axis=1) + 8.0 * O.EPS * np.abs(st["val"][rows]).max(axis=1)
    assert np.all(np.abs(dd["ensval"] - ds["ensval"]) <= tol[:, None])
    assert np.all(np.abs(dd["val"] - ds["val"]) <= tol + 8.0 * O.EPS * np.abs(ds["ob_dat"]))
