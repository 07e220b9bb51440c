#!/usr/bin/env python3
"""obsmake_cal on the device (letkf_obsmake_slot_dev and letkf_obsmake_noise_dev, include/letkf_amd_obsmake.h) on C2's grid and
observation lattice (bench_workload.py: 240 x 240 x 60, lattice spacing 2900 m, every lattice point one radar row, all of
them in the slot): ms per call of one slot, then of the noise over the same rows and over --noise-rows rows (the noise alone),
the median of --reps calls after a warm-up.  For the noise the three parts are reported separately:
  host_generation_ms   letkf_rand_res53 of the same count into host memory (the SFMT recurrence, one core)
  copy_ms              the same bytes from pinned host memory to the device, alone
  copy_and_kernels_ms  the device's part: device events around a call made while the stream is still busy with a spin kernel
                       and with the staging chunk as large as the call, so that the generation is hidden and no event is
                       waited for: the copy, Box-Muller and the noise kernel back to back (the kernels alone: a kernel trace of
                       this script, profiles/obsmake_c2_kernel_stats.csv)
  call_ms              the whole call as a host sees it, with the default chunk: generation of chunk c + 1 overlaps the copy
                       and kernel of chunk c
Not the contract bench (bench.py).

  bench_obsmake.py [WORKLOAD] [--reps 5] [--noise-rows 2066700] [--out FILE]
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
import bench_obsope as bo                  # noqa: E402
import bench_workload as bw                # noqa: E402

NV3DD, NV2DD, KHALO, IHALO = bo.NV3DD, bo.NV2DD, bo.KHALO, bo.IHALO
UNDEF = -9.99e33


def med(ms):
    ms = sorted(ms)
    return dict(ms=round(ms[len(ms) // 2], 3), min=round(ms[0], 3), max=round(ms[-1], 3))


def noise_parts(pkg, ctx, dev, n, reps, seed):
    p = lambda t: C.c_void_p(t.data_ptr())
    elm = torch.where(torch.arange(n, device=dev) % 2 == 0, 4001, 4002).to(torch.int32)
    dat0 = torch.where(torch.arange(n, device=dev) % 7 == 0, UNDEF, 10.0).to(torch.float64)
    dat, err = dat0.clone(), torch.ones(n, dtype=torch.float64, device=dev)
    off = np.array([0, n], dtype=np.int64)
    files = pkg.ObsFileRows(nfile=1, off=off.ctypes.data, elm=p(elm), dat=p(dat), err=p(err))
    errs = pkg.ObsmakeErr(1.0, 1.0, 1.0, 1e-3, 0.1, 100.0, 5.0, 3.0)
    nu = 2 * ((n + 1) // 2)
    # the whole call, default chunk
    rand = pkg.Rand(seed)

    def call():
        dat.copy_(dat0)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ctx.obsmake_noise(errs, files, rand)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3
    call()
    call_ms = [call() for _ in range(reps)]
    # host generation alone
    host = np.zeros(nu)
    gen = pkg.Rand(seed)
    l = pkg.osse_lib()
    l.letkf_rand_res53(gen._r, nu, host.ctypes.data)
    gen_ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        l.letkf_rand_res53(gen._r, nu, host.ctypes.data)
        gen_ms.append((time.perf_counter() - t0) * 1e3)
    # the copy alone
    pinned, du = torch.zeros(nu, dtype=torch.float64).pin_memory(), torch.zeros(nu, dtype=torch.float64, device=dev)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    copy_ms = []
    for it in range(reps + 1):
        e0.record()
        du.copy_(pinned, non_blocking=True)
        e1.record()
        torch.cuda.synchronize()
        if it:
            copy_ms.append(e0.elapsed_time(e1))
    # copy + kernels behind a busy stream, one chunk
    one = pkg.Rand(seed)
    one.set_chunk(nu // 2)
    dev_ms = []
    for it in range(reps + 1):
        dat.copy_(dat0)
        torch.cuda._sleep(200_000_000)                               # ~0.1 s of spinning: longer than the generation
        e0.record()
        ctx.obsmake_noise(errs, files, one)
        e1.record()
        torch.cuda.synchronize()
        if it:
            dev_ms.append(e0.elapsed_time(e1))
    c, h, cp, dv = med(call_ms), med(gen_ms), med(copy_ms), med(dev_ms)
    hit = int((dat != dat0).sum())
    return dict(rows=n, call=c, host_generation=h, copy=cp, copy_and_kernels=dv,
                ns_per_uniform_host=round(h["ms"] * 1e6 / nu, 2), rows_per_s=round(n / (c["ms"] * 1e-3)), rows_perturbed=hit,
                finite=bool(torch.isfinite(dat).all()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("workload", nargs="?", default="C2")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--noise-rows", type=int, default=2066700)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    pkg = load_package()
    pkg.build()
    dev = torch.device("cuda:0")
    ctx = pkg.Context(0, torch.cuda.current_stream().cuda_stream)
    cfg = bw.CONFIGS[args.workload]
    nlev = cfg["nz"]
    v3, v2 = bo.fields(cfg, 1, dev, cfg["seed"])                     # the nature run of the slot: one state
    ox, oy, oz, _, _ = bw.lattice(cfg, dev)
    oz = oz[(oz > bw.level_heights(nlev, cfg["ztop"])[0] + 1.0) & (oz < cfg["ztop"] - 1.0)]
    zz, yy, xx = torch.meshgrid(oz, oy, ox, indexing="ij")
    xx, yy, zz = xx.reshape(-1).contiguous(), yy.reshape(-1).contiguous(), zz.reshape(-1).contiguous()
    nrow = xx.numel()
    ri, rj = IHALO + 0.5 + xx / cfg["dx"], IHALO + 0.5 + yy / cfg["dx"]
    cx, cy = 0.5 * cfg["nx"] * cfg["dx"], 0.5 * cfg["ny"] * cfg["dx"]
    lon, lat = 135.0 + (xx - cx) / 91.0e3, 35.0 + (yy - cy) / 111.0e3
    elm = torch.where(torch.arange(nrow, device=dev) % 2 == 0, 4001, 4002).to(torch.int32)
    typ = torch.full((nrow,), 22, dtype=torch.int32, device=dev)
    dat = torch.zeros(nrow, dtype=torch.float64, device=dev)
    dif = torch.zeros(nrow, dtype=torch.float64, device=dev)
    counts = torch.zeros(2, dtype=torch.int64, device=dev)
    off = np.array([0, nrow], dtype=np.int64)
    file_radar, radars = np.array([0], dtype=np.int32), np.array([[135.0, 35.0, 50.0]])
    use = np.ones(24, dtype=np.int32)
    p = lambda t: C.c_void_p(t.data_ptr())
    files = pkg.ObsFileRows(nfile=1, off=off.ctypes.data, elm=p(elm), typ=p(typ), lev=p(zz), dat=p(dat), ri=p(ri), rj=p(rj))
    prm = pkg.ObsopeParams(lon=p(lon), lat=p(lat), file_radar=file_radar.ctypes.data, radar_meta=radars.ctypes.data, rotc=None,
                           use_obs=use.ctypes.data, nobtype=24, method_ref_calc=2, use_terminal_velocity=1, stggrd=0,
                           min_radar_ref_dbz=5.0, low_ref_shift=-5.0, radar_zmax=99.0e3, ps_adjust_thres=100.0, ri_off=0.0, rj_off=0.0)
    nk, ni, nj = nlev + 2 * KHALO, cfg["nx"] + 2 * IHALO, cfg["ny"] + 2 * IHALO
    fl = pkg.ObsopeFields(nlev=nlev, nlon=cfg["nx"], nlat=cfg["ny"], khalo=KHALO, ihalo=IHALO, jhalo=IHALO, nv3dd=NV3DD, nv2dd=NV2DD,
                          nmem=1, m0=0, v3d=p(v3), s3k=1, s3i=nk, s3j=nk * ni, s3v=nk * ni * nj, s3m=nk * ni * nj * NV3DD,
                          v2d=p(v2), s2i=1, s2j=ni, s2v=ni * nj, s2m=ni * nj * NV2DD)
    slot = pkg.ObsmakeSlot(slot_lb=-300.0, slot_ub=300.0, dif=p(dif), own=None, outside_undef=1, reserved0=0)
    ms = bo.timed(lambda: ctx.obsmake_slot(slot, prm, files, fl, counts), args.reps)
    m = med(ms)
    res = dict(workload=args.workload, nlev=nlev, nx=cfg["nx"], ny=cfg["ny"], rows=nrow, reps=args.reps,
               library=os.path.basename(pkg.OSSE_LIB_PATH), device=torch.cuda.get_device_name(0),
               slot=dict(m, rows_per_s=round(nrow / (m["ms"] * 1e-3)), counts=counts.cpu().tolist(),
                         undef_rows=int((dat == UNDEF).sum()), finite=bool(torch.isfinite(dat).all())),
               noise=[noise_parts(pkg, ctx, dev, n, args.reps, 20141) for n in (nrow, args.noise_rows)])
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
