"""das_letkf_interp_window_amd (scale-letkf_amd/fortran/letkf_interp_window_amd.f90) from a Fortran host: the driver program
reads the arrays of one tile of the base grid of tests/_interp.py -- the tile [4, 7) x [3, 5) at stride (2, 2) in its minimal
rectangle, NaN wherever the call may not read --, makes one call and writes the analysis array back: bitwise what
Context.das_interp_window gives on the same inputs, the fill value included where the call does not own the point."""
import os
import subprocess

import numpy as np
import pytest

import _interp as I
from __graft_entry__ import PKG_DIR, load_package
from _search import ARRAY_FIELDS

FDIR = os.path.join(PKG_DIR, "fortran")
DRIVER = os.path.join(FDIR, "build", "interp_window_driver")
HAVE_FC = os.path.exists("/opt/rocm/bin/amdflang")


def write_case(path, c, a, sx, sy, spread, det):
    tc = c["tc"]
    s = tc["scal"]
    with open(path, "wb") as f:
        np.array([c["k"], c["nv"], a["nx"], a["ny"], c["nlev"], sx, sy, tc["nobs"], c["kld"], det], dtype=np.int32).tofile(f)
        np.array(a["window"], dtype=np.int32).tofile(f)
        np.array([spread]).tofile(f)
        np.array([s["nctype"], s["ngroup"], s["criterion"], s["nlon"], s["nlat"], 0], dtype=np.int32).tofile(f)
        np.array([s["dx"], s["dy"], s["i_org"], s["j_org"], s["rain_base"]]).tofile(f)
        for name in ARRAY_FIELDS:                           # (the struct's order)
            arr = np.ascontiguousarray(tc["arr"][name])
            np.array([arr.nbytes], dtype=np.int64).tofile(f)
            arr.tofile(f)
        for arr in (a["rig"], a["rjg"], a["rlev"], a["rz"], c["ensval"], c["dep"], a["infl"], a["gues"]):
            np.ascontiguousarray(arr, dtype=np.float64).tofile(f)


@pytest.mark.gpu
@pytest.mark.skipif(not HAVE_FC, reason="amdflang not present")
def test_fortran_driver_gives_the_bits_of_the_python_call(tmp_path):
    from test_gpu_interp_window import ANAL_FILL, DET, TILES, cut, launch
    load_package().build()
    subprocess.check_call(["make", "-C", FDIR], stdout=subprocess.DEVNULL)
    c = I.tile_case(50)
    a = cut(c, 2, 2, TILES[3])
    assert a["dead"].any() and np.isnan(a["gues"]).any()
    fin, fout = str(tmp_path / "case.bin"), str(tmp_path / "anal.bin")
    write_case(fin, c, a, 2, 2, 0.95, 1)
    r = subprocess.run([DRIVER, fin, fout], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    got = np.fromfile(fout).reshape(c["nv"], c["nens"], a["npts"])
    want = launch(c, a, 2, 2, DET)["anal"]
    o = a["owned"]
    members = list(range(c["k"])) + [c["k"] + 1]
    assert np.isfinite(got[:, members][:, :, o]).all() and (got[:, :, ~o] == ANAL_FILL).all()
    assert np.array_equal(got, want)
