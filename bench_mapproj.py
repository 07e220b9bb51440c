#!/usr/bin/env python3
"""The map projection on the device (letkf_phys2ij_dev and letkf_mapproj_grid_dev, include/letkf_amd_mapproj.h) on the 2^24 rows
bench_superob.py makes (the same generator, the same ri / rj over C2's grid of 240 x 240 points, here with halos of 2): their lon /
lat are the statement's inverse (tests/_mapproj.py) of those ri / rj under BDA_d3_1km_9p_bf20's PARAM_MAPPROJ.  Three cases:
phys2ij with rotc, without it, and the grid loop on 240 x 240 points.  Per case: ms per call between HIP events (median of --reps
calls after two warm-up calls, with min and max), rows per second, and the ledger bytes (16 B read and 16 or 32 B written per
row; the grid loop reads nothing and writes 32 B per point) over the time, against the HBM peak.  Not the contract bench
(bench.py).

The only comparison is the wall time of the numpy statement of phys2ij on the same rows on this box's host, one thread: what a
host pays today for the same columns.  It is a record, not a pass / fail line.

  bench_mapproj.py [--rows 16777216] [--reps 7] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from __graft_entry__ import load_package  # noqa: E402
import bench_workload as bw                # noqa: E402
import _mapproj as M                       # noqa: E402

HBM_PEAK = 8.0e12          # B/s, the specification
HALO = 2
CONFIG = "BDA_d3_1km_9p_bf20"


def timed(call, reps):
    ev = []
    for rep in range(reps + 2):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        torch.cuda.synchronize()
        if rep >= 2:
            ev.append(e0.elapsed_time(e1))
    ev.sort()
    return ev


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1 << 24)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    pkg = load_package()
    pkg.build()
    dev = torch.device("cuda:0")
    ctx = pkg.Context(0, torch.cuda.current_stream().cuda_stream)
    cfg = bw.CONFIGS["C2"]
    nx, ny = cfg["nx"], cfg["ny"]
    n = args.rows
    gen = torch.Generator(device=dev)
    gen.manual_seed(cfg["seed"])
    uni = lambda lo, hi: lo + (hi - lo) * torch.rand(n, dtype=torch.float64, device=dev, generator=gen)
    ri, rj = uni(0.5, nx + 0.5) + HALO, uni(0.5, ny + 0.5) + HALO         # bench_superob.py's first two draws
    p = M.configs()[CONFIG]
    q, proj = M.setup(p), pkg.mapproj_setup(**M.setup_args(p))
    back = M.ij2phys(q, ri.cpu().numpy(), rj.cpu().numpy())               # the statement's inverse, on the host
    lon_h, lat_h = back["lon"], back["lat"]
    lon, lat = torch.from_numpy(lon_h).to(dev), torch.from_numpy(lat_h).to(dev)
    out = tuple(torch.empty(n, dtype=torch.float64, device=dev) for _ in range(2)) + (torch.empty((n, 2), dtype=torch.float64, device=dev),)
    grid = {k: torch.empty((ny, nx) + ((2,) if k == "rotc" else ()), dtype=torch.float64, device=dev) for k in ("lon", "lat", "rotc")}
    res = dict(rows=n, nx=nx, ny=ny, halo=HALO, reps=args.reps, config=CONFIG, library=os.path.basename(pkg.MAPPROJ_LIB_PATH),
               device=torch.cuda.get_device_name(0), hbm_peak_tb_s=HBM_PEAK / 1e12, cases={},
               measured="whole calls of letkf_phys2ij_dev / letkf_mapproj_grid_dev between HIP events on the context's stream",
               not_measured="letkf_ij2phys_dev, the upload of lon / lat, the host's letkf_mapproj_setup")
    cases = (("phys2ij_with_rotc", n, 16 + 32, lambda: ctx.phys2ij(proj, lon, lat, out=out)),
             ("phys2ij_without_rotc", n, 16 + 16, lambda: ctx.phys2ij(proj, lon, lat, out=(out[0], out[1], None))),
             ("grid_240x240", nx * ny, 32, lambda: ctx.mapproj_grid(proj, nx, ny, HALO, HALO, p["cxg1"], p["cyg1"], out=grid)))
    for label, rows, bytes_per_row, call in cases:
        ev = timed(call, args.reps)
        med = ev[len(ev) // 2]
        bps = rows * bytes_per_row / (med * 1e-3)
        res["cases"][label] = dict(rows=rows, ms=round(med, 4), min=round(ev[0], 4), max=round(ev[-1], 4), rows_per_s=round(rows / (med * 1e-3)),
                                   ledger_bytes=rows * bytes_per_row, ledger_gb_per_s=round(bps / 1e9, 1),
                                   pct_of_hbm_peak=round(100.0 * bps / HBM_PEAK, 2))
    # what the device made, against what it was made from
    ctx.phys2ij(proj, lon, lat, out=out)
    torch.cuda.synchronize()
    res["max_abs_ri_minus_input"] = float((out[0] - ri).abs().max())
    res["max_abs_rj_minus_input"] = float((out[1] - rj).abs().max())
    # the host: the numpy statement on the same rows, one thread
    t0 = time.perf_counter()
    st = M.phys2ij(q, lon_h, lat_h)
    st_ms = (time.perf_counter() - t0) * 1e3
    res["numpy_statement_ms"] = round(st_ms, 1)
    res["numpy_statement_ns_per_row"] = round(st_ms * 1e6 / n, 1)
    res["statement_over_device"] = round(st_ms / res["cases"]["phys2ij_with_rotc"]["ms"], 1)
    res["max_abs_ri_minus_statement"] = float(np.abs(out[0].cpu().numpy() - st["ri"]).max())
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
