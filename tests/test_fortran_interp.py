"""das_letkf_interp_amd (scale-letkf_amd/fortran/letkf_interp_amd.f90) from a Fortran host: the driver program reads the base
grid of tests/_interp.py, makes one call at stride (2, 2) and writes the analysis back -- bitwise what the Python binding's call
on the same inputs gives."""
import os
import subprocess

import numpy as np
import pytest

import _interp as I
from __graft_entry__ import PKG_DIR, load_package
from _search import ARRAY_FIELDS

FDIR = os.path.join(PKG_DIR, "fortran")
DRIVER = os.path.join(FDIR, "build", "interp_driver")
HAVE_FC = os.path.exists("/opt/rocm/bin/amdflang")


def write_case(path, c, sx, sy, spread, det):
    tc = c["tc"]
    s = tc["scal"]
    with open(path, "wb") as f:
        np.array([c["k"], c["nv"], c["nx"], c["ny"], c["nlev"], sx, sy, tc["nobs"], c["kld"], det], dtype=np.int32).tofile(f)
        np.array([spread]).tofile(f)
        np.array([s["nctype"], s["ngroup"], s["criterion"], s["nlon"], s["nlat"], 0], dtype=np.int32).tofile(f)
        np.array([s["dx"], s["dy"], s["i_org"], s["j_org"], s["rain_base"]]).tofile(f)
        for name in ARRAY_FIELDS:                           # (the struct's order)
            a = np.ascontiguousarray(tc["arr"][name])
            np.array([a.nbytes], dtype=np.int64).tofile(f)
            a.tofile(f)
        for a in (c["rig"], c["rjg"], c["rlev"], c["rz"], c["ensval"], c["dep"], c["infl"], c["gues"]):
            np.ascontiguousarray(a, dtype=np.float64).tofile(f)


@pytest.mark.gpu
@pytest.mark.skipif(not HAVE_FC, reason="amdflang not present")
def test_fortran_driver_gives_the_bits_of_the_python_call(tmp_path):
    from test_gpu_interp import call
    load_package().build()
    subprocess.check_call(["make", "-C", FDIR], stdout=subprocess.DEVNULL)
    c = I.tile_case(50)
    cfg = dict(relax_alpha_spread=0.95, det_run=1)
    fin, fout = str(tmp_path / "case.bin"), str(tmp_path / "anal.bin")
    write_case(fin, c, 2, 2, 0.95, 1)
    r = subprocess.run([DRIVER, fin, fout], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    k, nv, nens, npts = c["k"], c["nv"], c["nens"], c["npts"]
    got = np.fromfile(fout).reshape(nv, nens, npts)
    want = call(c, 2, 2, cfg, want_nobs=False)[0]
    members = list(range(k)) + [k + 1]
    assert np.isfinite(got[:, members]).all()
    assert np.array_equal(got[:, members], want[:, members])
