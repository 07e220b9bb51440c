"""letkf_das_columns_nobs_dev and nobs_fields_amd (scale-letkf_amd/fortran/letkf_nobsout_amd.f90) from a Fortran host: the driver
builds with its goal; on a device it reads the domain of tests/test_gpu_nobsout.py, runs the two entries and writes the
diagnostics, work3dn, the eleven fields and the analysis -- the diagnostics and the analysis bitwise what the Python binding's
call on the same inputs gives, work3dn and the fields bitwise the numpy statement (tests/_nobsout.py) of those diagnostics."""
import os
import subprocess

import numpy as np
import pytest

import _nobsout as N
from __graft_entry__ import PKG_DIR, load_package

FDIR = os.path.join(PKG_DIR, "fortran")
DRIVER = os.path.join(FDIR, "build", "nobsout_driver")
HAVE_FC = os.path.exists("/opt/rocm/bin/amdflang")
NOBTYPE = 24


@pytest.mark.skipif(not HAVE_FC, reason="amdflang not present")
def test_the_goal_builds_the_driver():
    load_package().build()
    subprocess.check_call(["make", "-C", FDIR, "nobsout"], stdout=subprocess.DEVNULL)
    assert os.access(DRIVER, os.X_OK)
    dyn = subprocess.check_output(["readelf", "-d", DRIVER], text=True)
    assert "[libletkf_amd_nobsout.so]" in dyn and "[libletkf_amd.so]" in dyn


def write_case(path, k, nens, case, rig, rjg, rlev, rz, beta, ens, dep, infl, gues, nij1, nlev, nv, elm_u, typ, list_bytes, alpha):
    a, s = case["arr"], case["scal"]
    nobs = int(case["ctype_rows"][-1])
    with open(path, "wb") as f:
        np.array([k, nv, nij1, nlev, nobs, k, s["nctype"], s["ngroup"], s["criterion"], s["nlon"], s["nlat"], NOBTYPE], dtype=np.int32).tofile(f)
        np.array([list_bytes, a["ac_ext"].size], dtype=np.int64).tofile(f)
        np.array([s["dx"], s["dy"], s["i_org"], s["j_org"], s["rain_base"], alpha]).tofile(f)
        for n in ("group_start", "group_member", "vmode", "max_nobs", "ngrd_i", "ngrd_j", "ngrdsch_i", "ngrdsch_j", "ngrdext_i", "ngrdext_j"):
            np.ascontiguousarray(a[n], dtype=np.int32).tofile(f)
        np.array(elm_u, dtype=np.int32).tofile(f)
        np.array(typ, dtype=np.int32).tofile(f)
        for n in ("hori_loc", "vert_loc", "varloc"):
            np.ascontiguousarray(a[n], dtype=np.float64).tofile(f)
        np.ascontiguousarray(a["ac_off"], dtype=np.int64).tofile(f)
        np.ascontiguousarray(a["ac_ext"], dtype=np.int32).tofile(f)
        for x in (a["ob_ri"], a["ob_rj"], a["ob_lev"], a["ob_dat"], a["ob_err"], rig, rjg, rlev, rz, ens, dep, beta, infl):
            np.ascontiguousarray(x, dtype=np.float64).tofile(f)
        # gues (npts, nens, nv) in Fortran order is [v][m][p] in C order: the Python state's own layout
        np.ascontiguousarray(gues, dtype=np.float64).tofile(f)


@pytest.mark.gpu
@pytest.mark.skipif(not HAVE_FC, reason="amdflang not present")
def test_fortran_driver_gives_the_python_calls_bits_and_the_statements_fields(tmp_path):
    import torch
    from test_gpu_nobsout import ELM_U, NIJ1, NLEV, NPTS, NV, TYP, Setup, domain, state, three_slabs
    load_package().build()
    subprocess.check_call(["make", "-C", FDIR, "nobsout"], stdout=subprocess.DEVNULL)
    k = 10
    s = Setup(k, 1, True)
    lb = three_slabs(s.search()[0])
    case, rig, rjg, rlev, rz, beta = domain(1, True)
    ens, dep, gues, nens = state(k)
    infl = np.full(NPTS * NV, 1.03)
    fin, fout = str(tmp_path / "case.bin"), str(tmp_path / "out.bin")
    write_case(fin, k, nens, case, rig, rjg, rlev, rz, beta, ens, dep, infl, gues, NIJ1, NLEV, NV, ELM_U, TYP, lb, 0.95)
    r = subprocess.run([DRIVER, fin, fout], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    raw = np.fromfile(fout, dtype=np.uint8)
    at = 0

    def take(count, dtype):
        nonlocal at
        a = raw[at:at + count * np.dtype(dtype).itemsize].view(dtype)
        at += a.nbytes
        return a

    nobs_out, nct = take(NPTS, np.int32), take(NPTS * 4, np.int32).reshape(NPTS, 4)
    cut = take(NPTS * 4, np.float64).reshape(NPTS, 4)
    w3n, w3 = take(NPTS * (NOBTYPE + 6), np.float64).reshape(NPTS, NOBTYPE + 6), take(NPTS * 11, np.float64).reshape(11, NPTS)
    anal = take(NV * nens * NPTS, np.float64)
    assert at == raw.size
    # the same call through the Python binding (no adaptive inflation in the driver)
    from test_gpu_nobsout import Run
    p = Run(k, nens).diag()
    a, kw = s.args(p, lb)
    kw.update(infl_adaptive=False, rtps_infl_out=None, nobs_ctype=p.nobs_ctype, cutd_ctype=p.cutd_ctype)
    p.anal.fill_(0.0)
    s.c.das_columns_nobs(*a, **kw)
    torch.cuda.synchronize()
    assert np.array_equal(nobs_out, p.nobs_out.cpu().numpy()) and np.array_equal(nct, p.nobs_ctype.view(NPTS, 4).cpu().numpy())
    assert np.array_equal(cut.view(np.int64), p.cutd_ctype.view(NPTS, 4).cpu().numpy().view(np.int64))
    assert np.array_equal(anal.view(np.int64), p.anal.cpu().numpy().view(np.int64))
    want = N.work3dn(nct, cut, ELM_U, TYP, nobtype=NOBTYPE)
    assert np.array_equal(w3n.view(np.int64), want.view(np.int64))
    assert np.array_equal(w3.view(np.int64), np.ascontiguousarray(N.fields(want).T).view(np.int64))
    assert nct.sum() > 1000 and (nct.sum(axis=1) == nobs_out).all()
