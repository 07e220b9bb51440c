"""obsope_amd (scale-letkf_amd/fortran/letkf_obsope_amd.f90) from a Fortran host: the driver program reads the chain case of
tests/test_gpu_obsope_chain.py, uploads it, calls obsope_amd and writes ensval / qc back -- bitwise what the Python binding's call
on the same inputs gives -- and then hands them to set_letkf_obs_amd, whose table holds the rows the Python chain's holds."""
import os
import subprocess

import numpy as np
import pytest

import _obsope as O
from __graft_entry__ import PKG_DIR, load_package

FDIR = os.path.join(PKG_DIR, "fortran")
DRIVER = os.path.join(FDIR, "build", "obsope_driver")
HAVE_FC = os.path.exists("/opt/rocm/bin/amdflang")


def write_case(path, case, cfg, dat, err, with_setobs):
    g = case["g"]
    with open(path, "wb") as f:
        np.array([g["nlev"], g["nlon"], g["nlat"], g["khalo"], g["ihalo"], g["jhalo"], case["nmem"], len(case["off"]) - 1,
                  case["off"][-1], case["nrow"], O.NOBTYPE, cfg["method_ref_calc"], cfg["use_terminal_velocity"], cfg["stggrd"],
                  len(case["radars"]), with_setobs], dtype=np.int32).tofile(f)
        np.array([cfg[n] for n in ("min_radar_ref_dbz", "low_ref_shift", "radar_zmax", "ps_adjust_thres", "ri_off", "rj_off")]).tofile(f)
        np.ascontiguousarray(case["off"], dtype=np.int64).tofile(f)
        np.ascontiguousarray(case["file_radar"], dtype=np.int32).tofile(f)
        np.ascontiguousarray(case["radars"], dtype=np.float64).tofile(f)
        np.ascontiguousarray(cfg["use_obs"], dtype=np.int32).tofile(f)
        for n in ("elm", "typ"):
            np.ascontiguousarray(case["files"][n], dtype=np.int32).tofile(f)
        for a in (case["files"]["lev"], case["files"]["ri"], case["files"]["rj"], case["files"]["lon"], case["files"]["lat"], dat, err):
            np.ascontiguousarray(a, dtype=np.float64).tofile(f)
        np.ascontiguousarray(case["set"], dtype=np.int32).tofile(f)
        np.ascontiguousarray(case["idx"], dtype=np.int32).tofile(f)
        np.ascontiguousarray(case["rotc"], dtype=np.float64).tofile(f)
        np.ascontiguousarray(case["v3"]).tofile(f)            # [m, v, j, i, k] in C order = (nlevh, nlonh, nlath, 13, nmem)
        np.ascontiguousarray(case["v2"]).tofile(f)


@pytest.mark.gpu
@pytest.mark.skipif(not HAVE_FC, reason="amdflang not present")
def test_fortran_driver_gives_the_bits_of_the_python_call(tmp_path):
    import torch
    from _gpu import ctx, pkg
    from test_gpu_obsope_chain import K, chain_case, observed
    load_package().build()
    subprocess.check_call(["make", "-C", FDIR], stdout=subprocess.DEVNULL)
    case = chain_case()
    cfg = O.default_cfg(method_ref_calc=3, ri_off=0.0, rj_off=0.0, use_obs=np.ones(O.NOBTYPE, dtype=np.int32), low_ref_shift=-1.0)
    st = O.statement(case, cfg)
    dat, err = observed(case, st, np.random.default_rng(3))
    fin, fout = str(tmp_path / "case.bin"), str(tmp_path / "out.bin")
    write_case(fin, case, cfg, dat, err, 1)
    r = subprocess.run([DRIVER, fin, fout], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    nrow = case["nrow"]
    raw = np.fromfile(fout, dtype=np.uint8)
    ens = raw[:8 * K * nrow].view(np.float64).reshape(nrow, K)
    qc = raw[8 * K * nrow:8 * K * nrow + 4 * nrow].view(np.int32)
    nobstotal = int(raw[8 * K * nrow + 4 * nrow:].view(np.int32)[0])
    want, want_qc = O.DeviceCase(pkg, case, cfg, torch.device("cuda:0")).run(ctx())
    assert np.array_equal(ens.view(np.int64), np.ascontiguousarray(want).view(np.int64))
    assert np.array_equal(qc, want_qc)
    assert 100 < nobstotal <= int((want_qc == 0).sum())
