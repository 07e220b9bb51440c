"""The three entries of include/letkf_amd_tcvital.h from a Fortran host (scale-letkf_amd/fortran/letkf_tcvital_amd.f90): the driver
builds with its goal; on a device it reads the main fixture of tests/_tcvital.py and a file's decoded columns, runs rows, search and
fill, and writes what they gave -- bit for bit what the Python binding's calls on the same inputs give."""
import os
import subprocess

import numpy as np
import pytest

import _tcvital as T
from __graft_entry__ import PKG_DIR, load_package

FDIR = os.path.join(PKG_DIR, "fortran")
DRIVER = os.path.join(FDIR, "build", "tcvital_driver")
HAVE_FC = os.path.exists("/opt/rocm/bin/amdflang")


@pytest.mark.skipif(not HAVE_FC, reason="amdflang not present")
def test_the_goal_builds_the_driver():
    load_package().build()
    subprocess.check_call(["make", "-C", FDIR, "tcvital"], stdout=subprocess.DEVNULL)
    assert os.access(DRIVER, os.X_OK)
    dyn = subprocess.check_output(["readelf", "-d", DRIVER], text=True)
    assert "[libletkf_amd_tcvital.so]" in dyn and "[libletkf_amd.so]" in dyn


@pytest.mark.gpu
@pytest.mark.skipif(not HAVE_FC, reason="amdflang not present")
def test_fortran_driver_gives_the_python_calls_bits(tmp_path):
    import torch
    from test_gpu_tcvital import bits, dev, fields_of, params_of
    from _gpu import ctx, pkg
    load_package().build()
    subprocess.check_call(["make", "-C", FDIR, "tcvital"], stdout=subprocess.DEVNULL)
    nlon, nlat, ih, jh, nmem, seed = T.FIXTURES["main"]
    v, ci, cj = T.low_fixture(nlon, nlat, ih, jh, nmem, seed)
    p = T.params(i_off=0, j_off=0)
    m0, kld, n = 1, 6, 40
    rng = np.random.default_rng(7)
    elm = rng.choice(np.array([2819, 3073, 14593], dtype=np.int32), n)
    dif = rng.uniform(-1.0, 1.0, n).round(2)
    for row, e in ((3, T.ID_TCX), (20, T.ID_TCX), (21, T.ID_TCY), (22, T.ID_TCP)):
        elm[row], dif[row] = e, 0.25
    qc = np.where(np.isin(elm, (T.ID_TCX, T.ID_TCY, T.ID_TCP)), 90, 0).astype(np.int32)
    ens = rng.standard_normal((n, kld))
    fin, fout = str(tmp_path / "case.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        np.array([nlon, nlat, ih, jh, nmem, m0, kld, n, p["i_off"], p["j_off"], 1], dtype=np.int32).tofile(f)
        np.array([p["dx"], p["dy"], p["cxg1"], p["cyg1"], p["tc_search_dis"], 0.0, 0.5, ci[0], cj[0]]).tofile(f)
        v.tofile(f)                                                                # (nlonh, nlath, 7, nmem) in Fortran order
        elm.tofile(f)
        dif.tofile(f)
        qc.tofile(f)
        ens.tofile(f)                                                              # (kld, n) in Fortran order
    r = subprocess.run([DRIVER, fin, fout], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    raw = np.fromfile(fout, dtype=np.uint8)
    at = 0

    def take(count, dtype):
        nonlocal at
        a = raw[at:at + count * np.dtype(dtype).itemsize].view(dtype)
        at += a.nbytes
        return a

    rows, valid, cand = take(3, np.int64), take(1, np.int32), take(3 * nmem, np.float64).reshape(nmem, 3)
    qc_f, ens_f = take(n, np.int32), take(n * kld, np.float64).reshape(n, kld)
    assert at == raw.size
    # the same calls through the Python binding
    c = ctx()
    got_rows, got_valid = c.tcvital_rows(dev(elm), dev(dif), 0.0, 0.5)
    centre = dev(np.array([ci[0], cj[0]]))
    vd = dev(v)
    got_cand = c.tcvital_search(params_of(pkg, p), fields_of(pkg, vd, nlon, nlat, ih, jh, nmem), centre[0:1], centre[1:2])
    qc_d, ens_d = dev(qc), dev(ens)
    c.tcvital_fill(got_cand[None], got_rows - 1, qc_d, ens_d, kld, m0=m0, qc_replace=True)
    torch.cuda.synchronize()
    assert rows.tolist() == got_rows.tolist() == [21, 22, 23] and valid[0] == 1 and got_valid
    assert np.array_equal(bits(cand), bits(got_cand.cpu().numpy())) and (cand[:, 2] < T.CAP).all()
    assert np.array_equal(qc_f, qc_d.cpu().numpy()) and qc_f[[3, 20, 21, 22]].tolist() == [90, 0, 0, 0]
    assert np.array_equal(bits(ens_f), bits(ens_d.cpu().numpy())) and np.array_equal(ens_f[20, m0:m0 + nmem], cand[:, 0])
