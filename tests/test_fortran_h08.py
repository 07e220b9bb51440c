"""The entries of include/letkf_amd_h08.h from a Fortran host (scale-letkf_amd/fortran/letkf_h08_amd.f90): the driver builds with
its goal; on a device it (1) checks the record framing against amdflang's own sequential unformatted I/O, as the obsfile driver
does for the other formats -- every line it prints must say PASS -- and (2) runs a case through select, profiles, its stand-in
for the radiative transfer and rows, whose outputs are held to the numpy restatement bit for bit (the zenith angle within the
bound of tests/test_gpu_h08.py; the rows from the driver's own stand-in arrays)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import _h08 as H
from __graft_entry__ import PKG_DIR, load_package

FDIR = os.path.join(PKG_DIR, "fortran")
DRIVER = os.path.join(FDIR, "build", "h08_driver")
HAVE_FC = os.path.exists("/opt/rocm/bin/amdflang")
CHECKS = {"h08_count", "h08_decode", "h08_encode", "h08_case"}


@pytest.mark.skipif(not HAVE_FC, reason="amdflang not present")
def test_the_goal_builds_the_driver():
    load_package().build()
    subprocess.check_call(["make", "-C", FDIR, "h08"], stdout=subprocess.DEVNULL)
    assert os.access(DRIVER, os.X_OK)
    dyn = subprocess.check_output(["readelf", "-d", DRIVER], text=True)
    assert "[libletkf_amd_h08.so]" in dyn and "[libletkf_amd.so]" in dyn


@pytest.mark.gpu
@pytest.mark.skipif(not HAVE_FC, reason="amdflang not present")
def test_fortran_driver_checks_the_framing_and_gives_the_restatements_bits(tmp_path):
    from test_gpu_h08 import H08_SET, check_profiles, check_rows, obsda_rows, want_rows
    pkg = load_package()
    pkg.build()
    subprocess.check_call(["make", "-C", FDIR, "h08"], stdout=subprocess.DEVNULL)
    nlev, nmem, seed = 65, 3, 137
    case = H.make_case(nlev, nmem, seed)
    g, nprof = case["g"], case["nprof"]
    p = H.params(nlev=nlev, nprof_file=nprof, top_down=1, rttov_units=1, stggrd=1, cldsky_thrs=1.0, reject_land=1, finish=1, member=nmem,
                 ch_use=(1, 1, 0, 1, 1, 1, 1, 2, 1, 1), **H.BUFFER)
    set_, idx = obsda_rows(nprof, seed, "shuffled")
    nrow, kld, m0 = set_.size, nmem + 1, 1
    rng = np.random.default_rng(2)
    start = (np.full(nrow, 90, dtype=np.int32), rng.standard_normal((nrow, kld)), np.zeros(nrow), np.zeros(nrow))
    fin, fout = str(tmp_path / "case.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        np.array([nlev, g["khalo"], g["nlon"], g["nlat"], g["ihalo"], g["jhalo"], nmem, nprof, nrow, kld, m0, H08_SET], dtype=np.int32).tofile(f)
        f.write(bytes(pkg.h08_params(**p)))
        case["v3"].tofile(f)                                       # (nlevh, nlonh, nlath, 13, nmem) in Fortran order
        case["v2"].tofile(f)
        for k in ("ri", "rj", "lon", "lat", "rotc"):
            case[k].tofile(f)
        for a in (set_, idx) + start:
            a.tofile(f)
    r = subprocess.run([DRIVER, str(tmp_path), fin, fout], capture_output=True, text=True, timeout=120)
    lines = [l.split() for l in r.stdout.splitlines() if l.strip()]
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    assert all(l[0] == "PASS" for l in lines) and {l[1] for l in lines} == CHECKS, r.stdout
    assert os.path.getsize(tmp_path / "h08.dat") == os.path.getsize(tmp_path / "h08_dev.dat") == 64 * 130
    own, devs = (np.fromfile(tmp_path / n, dtype=np.uint8).reshape(130, 64) for n in ("h08.dat", "h08_dev.dat"))
    assert np.array_equal(np.delete(own, 6, axis=0), np.delete(devs, 6, axis=0)) and not np.array_equal(own[6], devs[6])   # (record 7: NINT)

    raw = np.fromfile(fout, dtype=np.uint8)
    at = 0

    def take(count, dtype, shape=None):
        nonlocal at
        a = raw[at:at + count * np.dtype(dtype).itemsize].view(dtype)
        at += a.nbytes
        return a if shape is None else a.reshape(shape)

    nsel = int(take(1, np.int64)[0])
    pl, slot = take(nprof, np.int32), take(nprof, np.int32)
    got = dict(lev3=take(nmem * nsel * 5 * nlev, np.float64, (nmem, nsel, 5, nlev)), sfc=take(nmem * nsel * 8, np.float64, (nmem, nsel, 8)),
               pflag=take(nsel, np.int32), cloud=None)
    rt = tuple(take(nmem * nsel * H.NCH * k, np.float64, (nmem, nsel, H.NCH) + ((nlev,) if k > 1 else ())) for k in (1, 1, nlev))
    rows = (take(nrow, np.int32), take(nrow * kld, np.float64, (nrow, kld)), take(nrow, np.float64), take(nrow, np.float64))
    assert at == raw.size
    wl, ws, wn = H.select(set_, idx, 0, nrow, H08_SET, nprof)
    assert nsel == wn and np.array_equal(pl[:nsel], wl) and np.all(pl[nsel:] == -1) and np.array_equal(slot, ws)
    want = H.profiles(p, g, case["v3"], case["v2"], wl, case["ri"], case["rj"], case["lon"], case["lat"], case["rotc"])
    check_profiles(got, dict(want, cloud=None))
    for a in rt:
        assert np.all(np.isfinite(a[:, want["pflag"] == 0]))
    assert np.all(np.diff(rt[2][:, want["pflag"] == 0], axis=-1) < 0.0)                 # top down: tau falls towards the surface
    check_rows(rows, want_rows(p, set_, idx, ws, nsel, nmem, got, rt, case["ri"], case["rj"], kld, m0=m0, state=start))
    assert (rows[0] == 0).sum() > 50 and (rows[1][:, 0] == start[1][:, 0]).all()
