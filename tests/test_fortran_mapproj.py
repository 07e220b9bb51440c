"""mapproj_setup_amd and phys2ij_amd (scale-letkf_amd/fortran/letkf_mapproj_amd.f90) from a Fortran host: the driver program reads
a small file's lon / lat / dif, projects its rows on the device, hands ri / rj to obsscan_amd there and writes everything back --
ri, rj and rotc the bits of the Python binding's call, the tables and lists bitwise the numpy statement of the scan on them."""
import os
import subprocess

import numpy as np
import pytest

import _mapproj as M
import _obsscan as S
from __graft_entry__ import PKG_DIR, load_package

FDIR = os.path.join(PKG_DIR, "fortran")
DRIVER = os.path.join(FDIR, "build", "mapproj_driver")
HAVE_FC = os.path.exists("/opt/rocm/bin/amdflang")
NAME = "BDA_d3_1km_9p_bf20"


@pytest.mark.gpu
@pytest.mark.skipif(not HAVE_FC, reason="amdflang not present")
def test_fortran_driver_projects_and_scans(tmp_path):
    import torch
    from _gpu import ctx, dev, pkg
    load_package().build()
    subprocess.check_call(["make", "-C", FDIR, "mapproj"], stdout=subprocess.DEVNULL)
    p = M.configs()[NAME]
    q = M.setup(p)
    layout = (p["imax"], p["jmax"], 2, 2, p["prc_num_x"], p["prc_num_y"])
    slots = (1, 3, 2, 600.0)
    rng = np.random.default_rng(12)
    n = 300
    # rows over the whole 180 km domain and a margin outside it
    back = M.ij2phys(q, rng.uniform(-10.0, 195.0, n), rng.uniform(-10.0, 195.0, n))
    lon, lat, dif = back["lon"], back["lat"], rng.uniform(-1100.0, 1100.0, n)
    fin, fout = str(tmp_path / "case.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        np.array([n, *layout, slots[0], slots[1], slots[2]], dtype=np.int32).tofile(f)
        np.array([p[k] for k in M.KEYS] + [slots[3]]).tofile(f)
        for a in (lon, lat, dif):
            np.ascontiguousarray(a, dtype=np.float64).tofile(f)
    r = subprocess.run([DRIVER, fin, fout], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    assert r.stdout.count("bsna") == layout[4] * layout[5]

    raw = np.fromfile(fout, dtype=np.uint8)
    at = 0

    def take(count, dtype):
        nonlocal at
        a = raw[at:at + count * np.dtype(dtype).itemsize].view(dtype)
        at += a.nbytes
        return a

    nprocs, nb = layout[4] * layout[5], slots[1] - slots[0] + 3
    ri, rj, rotc = take(n, np.float64), take(n, np.float64), take(2 * n, np.float64).reshape(n, 2)
    got = dict(bsn=take(nprocs * nb, np.int32).reshape(nprocs, nb), bsna=take(nprocs * (nb + 1), np.int32).reshape(nprocs, nb + 1),
               set=take(n, np.int32), idx=take(n, np.int32), qc=take(n, np.int32))
    assert at == raw.size

    c = ctx()
    want = c.phys2ij(pkg.mapproj_setup(**M.setup_args(p)), dev(lon), dev(lat))
    torch.cuda.synchronize()
    for a, b in zip((ri, rj, rotc), want):
        assert np.array_equal(a.view(np.int64), b.cpu().numpy().view(np.int64))
    st = M.phys2ij(q, lon, lat)
    assert np.all(np.abs(ri - st["ri"]) <= 2 * M.bound_ij(st["rho"], p)) and np.all(np.abs(rotc - st["rotc"]) <= 2 * M.BOUND_ROTC)
    scan = S.scan(dict(off=np.array([0, n], dtype=np.int64), ri=ri, rj=rj, dif=dif, layout=layout, slots=slots, run=None))
    S.assert_same_bits(got, scan, ["bsn", "bsna", "set", "idx", "qc"])
    assert (got["qc"] == S.IQC_OUT_H).sum() >= 5 and (got["qc"] == 0).sum() >= 50 and (got["bsn"].sum(axis=1) > 0).sum() >= 5
