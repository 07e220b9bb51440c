"""rand_create_amd / obsmake_slot_amd / obsmake_noise_amd (scale-letkf_amd/fortran/letkf_obsmake_amd.f90) from a Fortran host:
the driver program reads the fixture of tests/_obsmake.py with two time slots on two nature-run states, zeroes dat, runs
both slots and then the noise with a fixed seed, and writes the counts, dat before the noise, dat and err after it --
bitwise what the Python calls on the same inputs give."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import _obsmake as M
import _obsope as O
from __graft_entry__ import PKG_DIR, load_package

FDIR = os.path.join(PKG_DIR, "fortran")
DRIVER = os.path.join(FDIR, "build", "obsmake_driver")
HAVE_FC = os.path.exists("/opt/rocm/bin/amdflang")
SEED, TINT = 4242, 600.0


def write_case(path, case, cfg, dif, own, err, outside_undef, nslot):
    g, f = case["g"], case["files"]
    with open(path, "wb") as out:
        np.array([g["nlev"], g["nlon"], g["nlat"], g["khalo"], g["ihalo"], g["jhalo"], len(case["off"]) - 1, case["off"][-1],
                  O.NOBTYPE, cfg["method_ref_calc"], cfg["use_terminal_velocity"], cfg["stggrd"], len(O.RADARS), nslot, outside_undef,
                  SEED, 1, 0, 0, 0], dtype=np.int32).tofile(out)
        np.array([cfg[n] for n in ("min_radar_ref_dbz", "low_ref_shift", "radar_zmax", "ps_adjust_thres", "ri_off", "rj_off")] +
                 [M.LB, TINT]).tofile(out)
        np.array([M.ERR[n] for n in ("obserr_u", "obserr_v", "obserr_t", "obserr_q", "obserr_rh", "obserr_ps", "obserr_radar_ref",
                                     "obserr_radar_vr")]).tofile(out)
        np.ascontiguousarray(case["off"], dtype=np.int64).tofile(out)
        np.ascontiguousarray(O.FILE_RADAR, dtype=np.int32).tofile(out)
        np.ascontiguousarray(O.RADARS, dtype=np.float64).tofile(out)
        np.ascontiguousarray(cfg["use_obs"], dtype=np.int32).tofile(out)
        for n in ("elm", "typ"):
            np.ascontiguousarray(f[n], dtype=np.int32).tofile(out)
        for a in (f["lev"], f["ri"], f["rj"], f["lon"], f["lat"], err, dif, M.rotc_by_file_row(case)):
            np.ascontiguousarray(a, dtype=np.float64).tofile(out)
        np.ascontiguousarray(own, dtype=np.int32).tofile(out)
        for m in range(nslot):                           # v3[m, v, j, i, k] in C order = (nlevh, nlonh, nlath, nv3dd) in Fortran's
            np.ascontiguousarray(case["v3"][m]).tofile(out)
            np.ascontiguousarray(case["v2"][m]).tofile(out)


@pytest.mark.gpu
@pytest.mark.skipif(not HAVE_FC, reason="amdflang not present")
def test_fortran_driver_gives_the_bits_of_the_python_calls(tmp_path):
    import torch
    from _gpu import ctx, pkg
    load_package().build()
    subprocess.check_call(["make", "-C", FDIR], stdout=subprocess.DEVNULL)
    case, cfg, dev = O.make_case(8), M.cfg_of(stggrd=1), torch.device("cuda:0")
    n = case["nrow"]
    dif, own = M.slot_inputs(case, 3)
    dif = np.where(np.random.default_rng(8).uniform(size=n) < 0.5, dif, dif + TINT)
    err0 = np.random.default_rng(2).uniform(0.5, 2.0, size=n)
    err0[::17] = M.UNDEF
    fin, fout = str(tmp_path / "case.bin"), str(tmp_path / "out.bin")
    write_case(fin, case, cfg, dif, own, err0, 1, 2)
    r = subprocess.run([DRIVER, fin, fout], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    # the Python calls
    c = ctx()
    dat, counts = np.zeros(n), []
    for m in range(2):
        lb = M.LB + m * TINT
        dc = M.device_case(pkg, case, cfg, dev, m, dat, err=err0)
        dat, cnt = M.run_slot(pkg, c, dc, dif, own, lb, lb + TINT, 1)
        counts.append(cnt)
    before = dat.copy()
    rand = pkg.Rand(SEED)
    c.obsmake_noise(M.err_struct(pkg), dc.files, rand)
    torch.cuda.synchronize()
    after, err = dc.d["dat"].cpu().numpy(), dc.d["err"].cpu().numpy()
    raw, o = np.fromfile(fout, dtype=np.uint8), 0
    for name, want in (("counts", np.concatenate(counts).astype(np.int64)), ("dat before", before), ("dat after", after), ("err", err)):
        nb = want.nbytes
        assert np.array_equal(raw[o:o + nb], np.ascontiguousarray(want).view(np.uint8)), name
        o += nb
    assert o == raw.size
    assert counts[0][1] > 40 and counts[1][1] > 40 and (after != before).sum() > 100 and (before == M.UNDEF).any()
