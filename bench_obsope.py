#!/usr/bin/env python3
"""The observation operator (letkf_obsope_dev, include/letkf_amd_obsope.h) on C2's grid and observation lattice
(bench_workload.py: 240 x 240 x 60, lattice spacing 2900 m) at k = 50 members: ms per call for METHOD_REF_CALC 2 and 3, (row,
member) pairs per second, and the algorithmic bytes of DESIGN.md section 12's ledger divided by the time.  Every lattice point is
one radar row, reflectivity and radial velocity alternating; the fields are synthetic (stretched levels over flat terrain, a
standard-atmosphere column, hydrometeors spanning both sides of MIN_RADAR_REF) with a few per cent of noise per member.
Not the contract bench (bench.py).

  bench_obsope.py [WORKLOAD] [--k 50] [--reps 5] [--out FILE]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
from __graft_entry__ import load_package  # noqa: E402
import bench_workload as bw                # noqa: E402

NV3DD, NV2DD, KHALO, IHALO = 13, 7, 2, 2
U, V, W, T, P, Q, QC, QR, QI, QS, QG, RH, HGT = range(13)


def fields(cfg, k, dev, seed):
    """v3 [m, v, j, i, k], v2 [m, v, j, i] on the device, the reference's layout per member"""
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    nk, ni, nj = cfg["nz"] + 2 * KHALO, cfg["nx"] + 2 * IHALO, cfg["ny"] + 2 * IHALO
    zl = bw.level_heights(cfg["nz"], cfg["ztop"])
    dz0, dz1 = zl[1] - zl[0], zl[-1] - zl[-2]
    z = np.concatenate([zl[0] - dz0 * np.arange(KHALO, 0, -1), zl, zl[-1] + dz1 * np.arange(1, KHALO + 1)])
    z = torch.from_numpy(z).to(dev)[None, None, :].expand(nj, ni, nk)
    x = torch.arange(ni, device=dev, dtype=torch.float64)[None, :, None] / ni
    y = torch.arange(nj, device=dev, dtype=torch.float64)[:, None, None] / nj
    v3 = torch.empty((k, NV3DD, nj, ni, nk), dtype=torch.float64, device=dev)
    v2 = torch.empty((k, NV2DD, nj, ni), dtype=torch.float64, device=dev)
    noise = lambda a: 1.0 + a * (2.0 * torch.rand((nj, ni, nk), dtype=torch.float64, device=dev, generator=g) - 1.0)
    for m in range(k):
        v3[m, HGT] = z
        v3[m, P] = 1.0e5 * torch.exp(-z / 8000.0) * noise(0.002)
        v3[m, T] = (300.0 - 6.5e-3 * torch.clamp(z, max=11000.0)) * noise(0.003)
        v3[m, U] = (10.0 + 8.0 * x - 5.0 * y + 1.0e-3 * z) * noise(0.05)
        v3[m, V] = (-6.0 + 3.0 * x + 9.0 * y - 0.5e-3 * z) * noise(0.05)
        v3[m, W] = (0.5 + x - y) * noise(0.1)
        v3[m, Q] = 0.012 * torch.exp(-z / 3000.0) * noise(0.05)
        v3[m, RH] = torch.clamp(0.7 - 4.0e-5 * z, min=0.05) * noise(0.05)
        v3[m, QC] = 1.0e-4 * torch.exp(-z / 4000.0) * noise(0.1)
        v3[m, QR] = torch.exp(-14.0 + 7.0 * x + 3.0 * y - 0.25e-3 * z) * noise(0.1)
        v3[m, QI] = 1.0e-5 * noise(0.1)
        v3[m, QS] = torch.exp(-15.0 + 4.0 * x + 5.0 * y + 0.2e-3 * torch.clamp(z, max=9000.0)) * noise(0.1) * (x > 0.2)
        v3[m, QG] = torch.exp(-14.0 + 6.0 * x + 2.0 * y) * noise(0.1) * (y > 0.3)
        v2[m] = 0.0
        v2[m, 1], v2[m, 5], v2[m, 6] = 1.0e5, 288.0, 0.01
    return v3, v2


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("workload", nargs="?", default="C2")
    ap.add_argument("--k", type=int, default=50)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    pkg = load_package()
    pkg.build()
    dev = torch.device("cuda:0")
    ctx = pkg.Context(0, torch.cuda.current_stream().cuda_stream)
    cfg = bw.CONFIGS[args.workload]
    k, nlev = args.k, cfg["nz"]
    v3, v2 = fields(cfg, k, dev, cfg["seed"])
    ox, oy, oz, _, _ = bw.lattice(cfg, dev)
    oz = oz[(oz > bw.level_heights(nlev, cfg["ztop"])[0] + 1.0) & (oz < cfg["ztop"] - 1.0)]
    zz, yy, xx = torch.meshgrid(oz, oy, ox, indexing="ij")
    xx, yy, zz = xx.reshape(-1), yy.reshape(-1), zz.reshape(-1)
    nrow = xx.numel()
    ri, rj = IHALO + 0.5 + xx / cfg["dx"], IHALO + 0.5 + yy / cfg["dx"]
    cx, cy = 0.5 * cfg["nx"] * cfg["dx"], 0.5 * cfg["ny"] * cfg["dx"]
    lon, lat = 135.0 + (xx - cx) / 91.0e3, 35.0 + (yy - cy) / 111.0e3
    elm = torch.where(torch.arange(nrow, device=dev) % 2 == 0, 4001, 4002).to(torch.int32)
    typ = torch.full((nrow,), 22, dtype=torch.int32, device=dev)
    set_ = torch.ones(nrow, dtype=torch.int32, device=dev)
    idx = torch.arange(1, nrow + 1, dtype=torch.int32, device=dev)
    off = np.array([0, nrow], dtype=np.int64)
    file_radar, radars = np.array([0], dtype=np.int32), np.array([[135.0, 35.0, 50.0]])
    use = np.ones(24, dtype=np.int32)
    p = lambda t: C.c_void_p(t.data_ptr())
    files = pkg.ObsFileRows(nfile=1, off=off.ctypes.data, elm=p(elm), typ=p(typ), lev=p(zz), ri=p(ri), rj=p(rj))
    prm = pkg.ObsopeParams(lon=p(lon), lat=p(lat), file_radar=file_radar.ctypes.data, radar_meta=radars.ctypes.data, rotc=None,
                           use_obs=use.ctypes.data, nobtype=24, method_ref_calc=2, use_terminal_velocity=1, stggrd=0,
                           min_radar_ref_dbz=5.0, low_ref_shift=-5.0, radar_zmax=99.0e3, ps_adjust_thres=100.0, ri_off=0.0, rj_off=0.0)
    nk, ni, nj = nlev + 2 * KHALO, cfg["nx"] + 2 * IHALO, cfg["ny"] + 2 * IHALO
    fl = pkg.ObsopeFields(nlev=nlev, nlon=cfg["nx"], nlat=cfg["ny"], khalo=KHALO, ihalo=IHALO, jhalo=IHALO, nv3dd=NV3DD, nv2dd=NV2DD,
                          nmem=k, m0=0, v3d=p(v3), s3k=1, s3i=nk, s3j=nk * ni, s3v=nk * ni * nj, s3m=nk * ni * nj * NV3DD,
                          v2d=p(v2), s2i=1, s2j=ni, s2v=ni * nj, s2m=ni * nj * NV2DD)
    ens = torch.zeros((nrow, k), dtype=torch.float64, device=dev)
    qc = torch.zeros(nrow, dtype=torch.int32, device=dev)
    ledger = 4 * nlev * 8 + 4 * 12 * 16                  # bytes per (row, member)
    res = dict(workload=args.workload, k=k, nlev=nlev, nx=cfg["nx"], ny=cfg["ny"], rows=nrow, row_members=nrow * k, reps=args.reps,
               ledger_bytes_per_row_member=ledger, fields_gb=round(v3.numel() * 8 / 2 ** 30, 2),
               library=os.path.basename(pkg.LIB_PATH), device=torch.cuda.get_device_name(0), methods={})
    for method in (2, 3):
        prm.method_ref_calc = method
        qc.zero_()
        ms = sorted(timed(lambda: ctx.obsope(prm, files, fl, set_, idx, qc, ens, k), args.reps))
        med = ms[len(ms) // 2]
        res["methods"][str(method)] = dict(ms=round(med, 3), min=round(ms[0], 3), max=round(ms[-1], 3),
                                           row_members_per_s=round(nrow * k / (med * 1e-3)),
                                           ledger_gb_per_s=round(ledger * nrow * k / (med * 1e-3) / 1e9, 1),
                                           qc_nonzero=int((qc != 0).sum()), finite=bool(torch.isfinite(ens).all()),
                                           ref_pairs_below_min_ref=int((ens[::2] == 0.0).sum()))
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
