"""obssim_cal_amd (scale-letkf_amd/fortran/letkf_obssim_amd.f90) from a Fortran host: the driver program runs the `restart` branch
of PROGRAM obssim on one subdomain -- state_to_history_amd, obssim_cal_amd with stggrd = 1, download -- and writes the
direct-access GrADS file record by record.  Read back with numpy, the file is `rec` of the Python calls bit for bit."""
import os
import subprocess

import numpy as np
import pytest

import _monit as M
import _obsope as O
import _obssim as S
from __graft_entry__ import PKG_DIR, load_package

FDIR = os.path.join(PKG_DIR, "fortran")
DRIVER = os.path.join(FDIR, "build", "obssim_driver")
HAVE_FC = os.path.exists("/opt/rocm/bin/amdflang")
VARS3 = (O.ID_REF, O.ID_VR, O.ID_U, O.ID_V, O.ID_T, O.ID_Q)
VARS2 = (O.ID_T, O.ID_PS)


def write_case(path, g, st, cfg, base, edge_fill):
    pad = lambda v: list(v) + [0] * (16 - len(v))
    with open(path, "wb") as out:
        np.array([g["nlev"], g["nlon"], g["nlat"], g["khalo"], g["ihalo"], g["jhalo"], st["state"].shape[0], edge_fill,
                  cfg["method_ref_calc"], cfg["use_terminal_velocity"], len(VARS3), len(VARS2), 1, 0, 0, 0], dtype=np.int32).tofile(out)
        np.array(pad(VARS3) + pad(VARS2), dtype=np.int32).tofile(out)
        np.array(list(S.RADAR) + [cfg["min_radar_ref_dbz"], cfg["low_ref_shift"], cfg["ps_adjust_thres"], st["ztop"], 0.0]).tofile(out)
        np.ascontiguousarray(st["cz"], dtype=np.float64).tofile(out)
        np.ascontiguousarray(st["topo"], dtype=np.float64).tofile(out)
        np.ascontiguousarray(np.transpose(st["state"], (0, 3, 1, 2))).tofile(out)      # [v, k, j, i] = (nlon, nlat, nlev, nv3d)
        for n in ("lon", "lat", "rotc"):
            np.ascontiguousarray(base[n], dtype=np.float64).tofile(out)


@pytest.mark.gpu
@pytest.mark.skipif(not HAVE_FC, reason="amdflang not present")
def test_the_drivers_grads_file_is_rec_of_the_python_calls(tmp_path):
    import ctypes as C
    import torch
    from _gpu import ctx, pkg
    load_package().build()
    subprocess.check_call(["make", "-C", FDIR], stdout=subprocess.DEVNULL)
    g = O.make_grid(8)
    st = M.make_state(g, M.SEEDS[8])
    base = S.make_case("8x5x3")
    cfg = S.default_cfg(method_ref_calc=3, stggrd=1, ps_adjust_thres=1.0e4)
    fin, fout = str(tmp_path / "case.bin"), str(tmp_path / "sim.grd")
    write_case(fin, g, st, cfg, base, 15)
    r = subprocess.run([DRIVER, fin, fout], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    # the Python calls on the same inputs
    c, dev = ctx(), torch.device("cuda:0")
    v3, v2 = M.history(st, g)
    case = dict(g=g, v3=v3, v2=v2, lon=base["lon"], lat=base["lat"], rotc=base["rotc"], radar=S.RADAR)
    fl = M.hist_layout(pkg, g)
    d3 = torch.full((O.NV3DD * g["nlath"] * g["nlonh"] * g["nlevh"],), np.nan, dtype=torch.float64, device=dev)
    d2 = torch.full((O.NV2DD * g["nlath"] * g["nlonh"],), np.nan, dtype=torch.float64, device=dev)
    fl.v3d, fl.v2d = C.c_void_p(d3.data_ptr()), C.c_void_p(d2.data_ptr())
    c.state_to_history(M.DeviceState(pkg, st, dev).hs, fl, d3, d2)
    dc = S.DeviceCase(pkg, case, cfg, VARS3, VARS2, dev, states=(0, 1), round_single=1)
    out = dc.outputs(("rec",))
    c.obssim(dc.params, fl, None, None, out["rec"])
    torch.cuda.synchronize()
    want = out["rec"].cpu().numpy()
    nrec = len(VARS3) * g["nlev"] + len(VARS2)
    got = np.fromfile(fout, dtype=np.float32)
    assert got.size == nrec * g["nlat"] * g["nlon"]
    assert np.array_equal(got.view(np.int32), want.ravel().view(np.int32))
    assert (want != np.float32(O.UNDEF)).sum() > 0.9 * want.size and (want == np.float32(O.UNDEF)).any()
