"""state_to_history_amd / monit_obs_amd / monit_print_amd (scale-letkf_amd/fortran/letkf_monit_amd.f90) from a Fortran host:
the driver program reads the fixture of tests/_monit.py, runs step 1 on the guess state and step 2 on the analysis state
through a key, and writes the records and statistics after each step -- bitwise what the Python calls on the same inputs
give -- and prints monit_print's two tables, character for character what the Python restatement of its format gives."""
import os
import subprocess

import numpy as np
import pytest

import _monit as M
import _obsope as O
from __graft_entry__ import PKG_DIR, load_package

FDIR = os.path.join(PKG_DIR, "fortran")
DRIVER = os.path.join(FDIR, "build", "monit_driver")
HAVE_FC = os.path.exists("/opt/rocm/bin/amdflang")


def write_case(path, case, cfg, mcfg, edge_fill):
    g, f = case["g"], case["files"]
    key = mcfg["key"]
    with open(path, "wb") as out:
        np.array([g["nlev"], g["nlon"], g["nlat"], g["khalo"], g["ihalo"], g["jhalo"], len(case["off"]) - 1, case["off"][-1],
                  case["nrow"], O.NOBTYPE, cfg["method_ref_calc"], cfg["use_terminal_velocity"], cfg["stggrd"], len(O.RADARS),
                  case["gues"]["state"].shape[0], edge_fill, mcfg["departure_stat_radar"], -1 if key is None else len(key), 0, 0],
                 dtype=np.int32).tofile(out)
        np.array([cfg[n] for n in ("min_radar_ref_dbz", "low_ref_shift", "radar_zmax", "ps_adjust_thres", "ri_off", "rj_off")] +
                 [mcfg["t_range"], case["gues"]["ztop"]]).tofile(out)
        np.ascontiguousarray(case["off"], dtype=np.int64).tofile(out)
        np.ascontiguousarray(O.FILE_RADAR, dtype=np.int32).tofile(out)
        np.ascontiguousarray(O.RADARS, dtype=np.float64).tofile(out)
        np.ascontiguousarray(cfg["use_obs"], dtype=np.int32).tofile(out)
        for n in ("elm", "typ"):
            np.ascontiguousarray(f[n], dtype=np.int32).tofile(out)
        for n in ("lev", "ri", "rj", "lon", "lat", "dat", "dif"):
            np.ascontiguousarray(f[n], dtype=np.float64).tofile(out)
        np.ascontiguousarray(case["set"], dtype=np.int32).tofile(out)
        np.ascontiguousarray(case["idx"], dtype=np.int32).tofile(out)
        np.ascontiguousarray(case["rotc"], dtype=np.float64).tofile(out)
        if key is not None:
            np.ascontiguousarray(key, dtype=np.int32).tofile(out)
        np.ascontiguousarray(case["gues"]["cz"], dtype=np.float64).tofile(out)
        np.ascontiguousarray(case["gues"]["topo"], dtype=np.float64).tofile(out)
        for st in (case["gues"], case["anal"]):                # [v, k, j, i] in C order = (nlon, nlat, nlev, nv3d)
            np.ascontiguousarray(np.transpose(st["state"], (0, 3, 1, 2))).tofile(out)


@pytest.mark.gpu
@pytest.mark.skipif(not HAVE_FC, reason="amdflang not present")
def test_fortran_driver_gives_the_bits_and_the_tables_of_the_python_calls(tmp_path):
    import torch
    from _gpu import ctx, pkg
    load_package().build()
    subprocess.check_call(["make", "-C", FDIR], stdout=subprocess.DEVNULL)
    case = M.case(8)
    cfg, dev = case["cfg"], torch.device("cuda:0")
    key = np.random.default_rng(4).permutation(case["nrow"])[:150].astype(np.int32)
    mcfg = M.default_mcfg(key=key, t_range=M.T_RANGE)
    fin, fout = str(tmp_path / "case.bin"), str(tmp_path / "out.bin")
    write_case(fin, case, cfg, mcfg, 15)
    r = subprocess.run([DRIVER, fin, fout], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    # the Python calls: both histories built on the device, step 1 then step 2 on the same records
    c = ctx()
    dc = O.DeviceCase(pkg, dict(case, v3=np.zeros_like(case["hist"][0][0]), v2=np.zeros_like(case["hist"][0][1])), cfg, dev)
    want, rec = [], None
    for step, st in ((1, case["gues"]), (2, case["anal"])):
        c.state_to_history(M.DeviceState(pkg, st, dev).hs, dc.fields, dc.d3, dc.d2)
        w = M.run_monit(pkg, c, dc, mcfg, step, dev, rec=rec)
        rec = w["rec_t"]
        want.append(w)
    nn, raw, o = len(key), np.fromfile(fout, dtype=np.uint8), 0
    for step, w in enumerate(want, 1):
        for name, dt in (("set", np.int32), ("idx", np.int32), ("qc", np.int32), ("omb", np.float64), ("oma", np.float64)):
            nb = nn * np.dtype(dt).itemsize
            got = raw[o:o + nb].view(dt)
            o += nb
            if not (step == 1 and name == "oma"):                    # (step 1 does not write oma)
                assert np.array_equal(got.view(np.uint8), np.ascontiguousarray(w["rec"][name]).view(np.uint8)), (step, name)
        for name, dt in (("nobs", np.int32), ("bias", np.float64), ("rmse", np.float64)):
            nb = 16 * np.dtype(dt).itemsize
            assert np.array_equal(raw[o:o + nb], np.ascontiguousarray(w[name]).view(np.uint8)), (step, name)
            o += nb
    assert o == raw.size
    mtype = pkg.monit_type(M.ELEM_UID, mcfg["departure_stat_radar"], False)
    lines = sum((M.monit_print(w["nobs"], w["bias"], w["rmse"], mtype) for w in want), [])
    assert r.stdout.splitlines() == lines, (r.stdout, lines)
    assert sum(w["nobs"].sum() for w in want) > 100
