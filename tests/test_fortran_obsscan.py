"""obsscan_amd and obsope_slot_amd (scale-letkf_amd/fortran/letkf_obsscan_amd.f90) from a Fortran host: the driver program reads
the case of tests/test_gpu_obsscan_chain.py, uploads it, scans, runs the operator subdomain by subdomain and slot by slot and
writes the tables, the lists and ensval / qc back -- the tables and lists bitwise the numpy statement's, ensval / qc bitwise what
the Python binding's calls on the same inputs give -- and then hands them to set_letkf_obs_amd."""
import os
import subprocess

import numpy as np
import pytest

import _obsope as O
import _obsscan as S
from __graft_entry__ import PKG_DIR, load_package

FDIR = os.path.join(PKG_DIR, "fortran")
DRIVER = os.path.join(FDIR, "build", "obsscan_driver")
HAVE_FC = os.path.exists("/opt/rocm/bin/amdflang")


def write_case(path, case, scan_in, cfg, subs, dat, err, nlist, with_setobs):
    g = subs[0][2]
    nlon, nlat, ihalo, jhalo, px, py = scan_in["layout"]
    s0, s1, base, tint = scan_in["slots"]
    nfile = len(case["off"]) - 1
    with open(path, "wb") as f:
        np.array([g["nlev"], nlon, nlat, g["khalo"], ihalo, jhalo, case["nmem"], nfile, case["off"][-1], nlist, O.NOBTYPE,
                  cfg["method_ref_calc"], cfg["use_terminal_velocity"], cfg["stggrd"], len(case["radars"]), with_setobs,
                  px, py, s0, s1, base], dtype=np.int32).tofile(f)
        np.array([cfg[n] for n in ("min_radar_ref_dbz", "low_ref_shift", "radar_zmax", "ps_adjust_thres")] + [tint]).tofile(f)
        np.ascontiguousarray(case["off"], dtype=np.int64).tofile(f)
        np.ascontiguousarray(case["file_radar"], dtype=np.int32).tofile(f)
        np.ones(nfile, dtype=np.int32).tofile(f)
        np.ascontiguousarray(case["radars"], dtype=np.float64).tofile(f)
        np.ascontiguousarray(cfg["use_obs"], dtype=np.int32).tofile(f)
        for n in ("elm", "typ"):
            np.ascontiguousarray(case["files"][n], dtype=np.int32).tofile(f)
        for a in (case["files"]["lev"], case["files"]["ri"], case["files"]["rj"], case["files"]["lon"], case["files"]["lat"], dat, err,
                  scan_in["dif"]):
            np.ascontiguousarray(a, dtype=np.float64).tofile(f)
        for v3, _, _, _ in subs:                              # [m, v, j, i, k] in C order = (nlevh, nlonh, nlath, 13, nmem) each
            np.ascontiguousarray(v3).tofile(f)
        for _, v2, _, _ in subs:
            np.ascontiguousarray(v2).tofile(f)


@pytest.mark.gpu
@pytest.mark.skipif(not HAVE_FC, reason="amdflang not present")
def test_fortran_driver_gives_the_statements_lists_and_the_bits_of_the_python_calls(tmp_path):
    import torch
    from _gpu import ctx, dev, pkg
    from test_gpu_obsscan_chain import K, PX, SLOTS, config, device_case, scan_chain_case, subdomain
    load_package().build()
    subprocess.check_call(["make", "-C", FDIR, "obsscan"], stdout=subprocess.DEVNULL)
    case, scan_in, st = scan_chain_case()
    nlist = len(st["set"])
    subs = [subdomain(case, ip) for ip in range(PX)]
    from test_gpu_obsope_chain import observed
    dat, err = observed(case, O.statement(case, config(0.0)), np.random.default_rng(3))   # observations near the members' mean
    fin, fout = str(tmp_path / "case.bin"), str(tmp_path / "out.bin")
    write_case(fin, case, scan_in, config(0.0), subs, dat, err, nlist, 1)
    r = subprocess.run([DRIVER, fin, fout], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)

    raw = np.fromfile(fout, dtype=np.uint8)
    at = 0

    def take(count, dtype):
        nonlocal at
        a = raw[at:at + count * np.dtype(dtype).itemsize].view(dtype)
        at += a.nbytes
        return a

    nb = SLOTS[1] - SLOTS[0] + 3
    got = dict(bsn=take(PX * nb, np.int32).reshape(PX, nb), bsna=take(PX * (nb + 1), np.int32).reshape(PX, nb + 1),
               set=take(nlist, np.int32), idx=take(nlist, np.int32))
    qc = take(nlist, np.int32)
    ens = take(nlist * K, np.float64).reshape(nlist, K)
    nobstotal = int(take(1, np.int32)[0])
    S.assert_same_bits(got, st, ["bsn", "bsna", "set", "idx"])

    # the same calls through the Python binding (ensval starts at 0 in the driver)
    c, d = ctx(), torch.device("cuda:0")
    dcs = [device_case(pkg, case, st, ip, d) for ip in range(PX)]
    scan = c.obsscan(dcs[0].files, dev(scan_in["dif"]), scan_in["layout"], SLOTS)
    want = torch.zeros((nlist, K), dtype=torch.float64, device=d)
    for ip in range(PX):
        for islot in range(SLOTS[0], SLOTS[1] + 1):
            c.obsope_slot(scan, SLOTS[0], ip, islot, dcs[ip].params, dcs[ip].files, dcs[ip].fields, want, K)
    torch.cuda.synchronize()
    assert np.array_equal(ens.view(np.int64), want.cpu().numpy().view(np.int64))
    want_qc = scan["qc"].cpu().numpy()
    assert np.array_equal(qc, want_qc)
    assert (qc == S.IQC_TIME).sum() >= 10 and (qc == S.IQC_OUT_H).sum() >= 5
    assert 0 < nobstotal <= int((want_qc == 0).sum())
