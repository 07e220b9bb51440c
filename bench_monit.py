#!/usr/bin/env python3
"""The departure monitor (letkf_state_to_history_dev and letkf_monit_obs_dev, include/letkf_amd_monit.h) on C2's grid and
observation lattice (bench_workload.py: 240 x 240 x 60, lattice spacing 2900 m): ms per call of each, the median of --reps
calls after a warm-up, and for state_to_history the algorithmic bytes of DESIGN.md section 13's ledger divided by the time.
The state is synthetic (stretched levels over gentle terrain, a standard-atmosphere column, hydrometeors spanning both sides of
MIN_RADAR_REF) in the point-fastest layout das_letkf_amd keeps; every lattice point is one radar row, reflectivity and radial
velocity alternating.  Not the contract bench (bench.py).

  bench_monit.py [WORKLOAD] [--reps 5] [--out FILE]
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

NV3D, NV3DD, NV2DD, KHALO, IHALO = 11, 13, 7, 2, 2
U, V, W, T, P, Q, QC, QR, QI, QS, QG = range(11)
ELEM_UID = np.array([2819, 2820, 3073, 3074, 3330, 3331, 14593, 19999, 4001, 4004, 4002, 4003, 8800, 99991, 99992, 99993], dtype=np.int32)


def state(cfg, dev, seed):
    """x [v, k, j, i] (point-fastest), topo [j, i] on the device, cz [k] on the host"""
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    nk, ni, nj = cfg["nz"], cfg["nx"], cfg["ny"]
    cz = np.ascontiguousarray(bw.level_heights(nk, cfg["ztop"]), dtype=np.float64)
    xx = torch.arange(ni, device=dev, dtype=torch.float64)[None, None, :] / ni
    yy = torch.arange(nj, device=dev, dtype=torch.float64)[None, :, None] / nj
    topo = (40.0 + 30.0 * xx[0] + 20.0 * yy[0]).expand(nj, ni).contiguous()
    z = (cfg["ztop"] - topo)[None] / cfg["ztop"] * torch.from_numpy(cz).to(dev)[:, None, None] + topo[None]
    noise = lambda a: 1.0 + a * (2.0 * torch.rand((nk, nj, ni), dtype=torch.float64, device=dev, generator=g) - 1.0)
    x = torch.empty((NV3D, nk, nj, ni), dtype=torch.float64, device=dev)
    x[P] = 1.0e5 * torch.exp(-z / 8000.0) * noise(0.002)
    x[T] = (300.0 - 6.5e-3 * torch.clamp(z, max=11000.0)) * noise(0.003)
    x[U] = (10.0 + 8.0 * xx - 5.0 * yy + 1.0e-3 * z) * noise(0.05)
    x[V] = (-6.0 + 3.0 * xx + 9.0 * yy - 0.5e-3 * z) * noise(0.05)
    x[W] = (0.5 + xx - yy) * noise(0.1)
    x[Q] = 0.012 * torch.exp(-z / 3000.0) * noise(0.05)
    x[QC] = 1.0e-4 * torch.exp(-z / 4000.0) * noise(0.1)
    x[QR] = torch.exp(-14.0 + 7.0 * xx + 3.0 * yy - 0.25e-3 * z) * noise(0.1)
    x[QI] = 1.0e-5 * noise(0.1)
    x[QS] = torch.exp(-15.0 + 4.0 * xx + 5.0 * yy + 0.2e-3 * torch.clamp(z, max=9000.0)) * noise(0.1) * (xx > 0.2)
    x[QG] = torch.exp(-14.0 + 6.0 * xx + 2.0 * yy) * noise(0.1) * (yy > 0.3)
    return x, topo, cz


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
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    pkg = load_package()
    pkg.build()
    dev = torch.device("cuda:0")
    ctx = pkg.Context(0, torch.cuda.current_stream().cuda_stream)
    cfg = bw.CONFIGS[args.workload]
    nlev, nx, ny = cfg["nz"], cfg["nx"], cfg["ny"]
    x, topo, cz = state(cfg, dev, cfg["seed"])
    p = lambda t: C.c_void_p(t.data_ptr())
    nk, ni, nj = nlev + 2 * KHALO, nx + 2 * IHALO, ny + 2 * IHALO
    v3 = torch.zeros((NV3DD, nj, ni, nk), dtype=torch.float64, device=dev)
    v2 = torch.zeros((NV2DD, nj, ni), dtype=torch.float64, device=dev)
    hs = pkg.HistState(nv3d=NV3D, edge_fill=15, x=p(x), si=1, sj=nx, sl=nx * ny, sv=nx * ny * nlev, topo=p(topo), cz=cz.ctypes.data,
                       ztop=float(cfg["ztop"]))
    fl = pkg.ObsopeFields(nlev=nlev, nlon=nx, nlat=ny, khalo=KHALO, ihalo=IHALO, jhalo=IHALO, nv3dd=NV3DD, nv2dd=NV2DD, nmem=1, m0=0,
                          v3d=p(v3), s3k=1, s3i=nk, s3j=nk * ni, s3v=nk * ni * nj, s3m=nk * ni * nj * NV3DD,
                          v2d=p(v2), s2i=1, s2j=ni, s2v=ni * nj, s2m=ni * nj * NV2DD)
    # the rows: C2's lattice, every point a radar row
    ox, oy, oz, _, _ = bw.lattice(cfg, dev)
    oz = oz[(oz > cz[0] + 100.0) & (oz < cfg["ztop"] - 1.0)]
    zz, yy, xx = torch.meshgrid(oz, oy, ox, indexing="ij")
    xx, yy, zz = xx.reshape(-1).contiguous(), yy.reshape(-1).contiguous(), zz.reshape(-1).contiguous()
    nrow = xx.numel()
    ri, rj = IHALO + 0.5 + xx / cfg["dx"], IHALO + 0.5 + yy / cfg["dx"]
    cx, cy = 0.5 * nx * cfg["dx"], 0.5 * ny * cfg["dx"]
    lon, lat = 135.0 + (xx - cx) / 91.0e3, 35.0 + (yy - cy) / 111.0e3
    elm = torch.where(torch.arange(nrow, device=dev) % 2 == 0, 4001, 4002).to(torch.int32)
    typ = torch.full((nrow,), 22, dtype=torch.int32, device=dev)
    dat = torch.where(elm == 4001, 12.0, 3.0).to(torch.float64)
    set_ = torch.ones(nrow, dtype=torch.int32, device=dev)
    idx = torch.arange(1, nrow + 1, dtype=torch.int32, device=dev)
    key = torch.flip(torch.arange(nrow, dtype=torch.int32, device=dev), dims=[0]).contiguous()
    off = np.array([0, nrow], dtype=np.int64)
    file_radar, radars = np.array([0], dtype=np.int32), np.array([[135.0, 35.0, 50.0]])
    use = np.ones(24, dtype=np.int32)
    files = pkg.ObsFileRows(nfile=1, off=off.ctypes.data, elm=p(elm), typ=p(typ), lev=p(zz), dat=p(dat), ri=p(ri), rj=p(rj))
    prm = pkg.ObsopeParams(lon=p(lon), lat=p(lat), file_radar=file_radar.ctypes.data, radar_meta=radars.ctypes.data, rotc=None,
                           use_obs=use.ctypes.data, nobtype=24, method_ref_calc=2, use_terminal_velocity=1, stggrd=1,
                           min_radar_ref_dbz=5.0, low_ref_shift=-5.0, radar_zmax=99.0e3, ps_adjust_thres=100.0, ri_off=0.0, rj_off=0.0)
    mp = pkg.MonitParams(step=1, departure_stat_radar=1, nid=len(ELEM_UID), reserved0=0, elem_uid=ELEM_UID.ctypes.data, t_range=0.0,
                         dif=None)
    rec_t = [torch.zeros(nrow, dtype=torch.int32, device=dev) for _ in range(3)] + [torch.zeros(nrow, dtype=torch.float64, device=dev)
                                                                                     for _ in range(2)]
    rec = pkg.Obsdep(*[p(t) for t in rec_t])
    outs = (torch.zeros(16, dtype=torch.int32, device=dev), torch.zeros(16, dtype=torch.float64, device=dev),
            torch.zeros(16, dtype=torch.float64, device=dev))

    # DESIGN.md section 13's ledger of state_to_history: every byte once
    npt, nhalo = nx * ny, ni * nj - nx * ny
    ledger = (NV3D * npt * nlev + npt + 5 * npt) * 8 + (NV3DD * npt * nk + NV2DD * npt) * 8 + 2 * nhalo * (NV3DD * nk + NV2DD) * 8
    ms_h = sorted(timed(lambda: ctx.state_to_history(hs, fl, v3, v2), args.reps))
    ms_m = sorted(timed(lambda: ctx.monit_obs(mp, prm, files, fl, set_, idx, rec, key=key, nn=nrow, outs=outs), args.reps))
    med_h, med_m = ms_h[len(ms_h) // 2], ms_m[len(ms_m) // 2]
    res = dict(workload=args.workload, nlev=nlev, nx=nx, ny=ny, rows=nrow, reps=args.reps, library=os.path.basename(pkg.LIB_PATH),
               device=torch.cuda.get_device_name(0),
               state_to_history=dict(ms=round(med_h, 3), min=round(ms_h[0], 3), max=round(ms_h[-1], 3), ledger_bytes=ledger,
                                     ledger_gb_per_s=round(ledger / (med_h * 1e-3) / 1e9, 1), finite=bool(torch.isfinite(v3).all())),
               monit_obs=dict(ms=round(med_m, 3), min=round(ms_m[0], 3), max=round(ms_m[-1], 3), rows_per_s=round(nrow / (med_m * 1e-3)),
                              good_rows=int((rec_t[2] == 0).sum()), nobs=outs[0].cpu().tolist(),
                              bias_ref=float(outs[1][8]), rmse_vr=float(outs[2][10])))
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
