#!/usr/bin/env python3
"""obssim_cal on the device (letkf_obssim_dev, include/letkf_amd_obssim.h) on C2's grid (bench_workload.py: 240 x 240 x 60), one
state: ms per call (median of --reps calls after a warm-up, with min and max) for three lists -- {REF, Vr}, {REF, Vr, U, V, T, Q}
with the GrADS records, and {T} alone -- under METHOD_REF_CALC 2 and 3 and stggrd 0 and 1, and the algorithmic bytes of
DESIGN.md section 15's ledger divided by the time, against the HBM peak.  The fields are bench_obsope.py's.  Not the contract
bench (bench.py).

The ledger, per point and state: 8 B for each field the lists need -- the radar operator reads U V W T P QR QS QG and the height,
Q adds one, {T} needs one -- plus 8 B for each staggered neighbour under stggrd = 1 (U, V and, in the radar operator, W), plus
what is written: 8 B per v3 value, 4 B per rec value.  lon / lat and the per-column azimuth and distance are 1 / nlev of that.

  bench_obssim.py [WORKLOAD] [--reps 5] [--out FILE]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
from __graft_entry__ import load_package  # noqa: E402
import bench_workload as bw                # noqa: E402
from bench_obsope import IHALO, KHALO, NV2DD, NV3DD, fields, timed  # noqa: E402

REF, VR, U, V, T, Q = 4001, 4002, 2819, 2820, 3073, 3330
HBM_PEAK, HBM_COPY = 8.0e12, 6.29e12          # B/s: the specification and the measured float4 copy
# name: (3-D list, rec asked for, fields read, of which staggered)
CASES = {
    "ref_vr": ((REF, VR), False, 9, 3),
    "six_rec": ((REF, VR, U, V, T, Q), True, 10, 3),
    "t_only": ((T,), False, 1, 0),
}


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
    nlev, nlon, nlat = cfg["nz"], cfg["nx"], cfg["ny"]
    v3, v2 = fields(cfg, 1, dev, cfg["seed"])
    x = (torch.arange(nlon, device=dev, dtype=torch.float64) + 0.5) * cfg["dx"]
    y = (torch.arange(nlat, device=dev, dtype=torch.float64) + 0.5) * cfg["dx"]
    cx, cy = 0.5 * nlon * cfg["dx"], 0.5 * nlat * cfg["dx"]
    lon = (135.0 + (x - cx) / 91.0e3)[None, :].expand(nlat, nlon).contiguous()
    lat = (35.0 + (y - cy) / 111.0e3)[:, None].expand(nlat, nlon).contiguous()
    p = lambda t: C.c_void_p(t.data_ptr())
    nk, ni, nj = nlev + 2 * KHALO, nlon + 2 * IHALO, nlat + 2 * IHALO
    fl = pkg.ObsopeFields(nlev=nlev, nlon=nlon, nlat=nlat, khalo=KHALO, ihalo=IHALO, jhalo=IHALO, nv3dd=NV3DD, nv2dd=NV2DD,
                          nmem=1, m0=0, v3d=p(v3), s3k=1, s3i=nk, s3j=nk * ni, s3v=nk * ni * nj, s3m=nk * ni * nj * NV3DD,
                          v2d=p(v2), s2i=1, s2j=ni, s2v=ni * nj, s2m=ni * nj * NV2DD)
    npts = nlev * nlon * nlat
    res = dict(workload=args.workload, nlev=nlev, nx=nlon, ny=nlat, points=npts, states=1, reps=args.reps,
               library=os.path.basename(pkg.OBSSIM_LIB_PATH), device=torch.cuda.get_device_name(0),
               hbm_peak_tb_s=HBM_PEAK / 1e12, hbm_copy_tb_s=HBM_COPY / 1e12, cases={})
    for name, (vars3, with_rec, nread, nstag) in CASES.items():
        prm = pkg.ObssimParams(nvar3=len(vars3), nvar2=0, radar_lon=135.0, radar_lat=35.0, radar_z=50.0, lon=p(lon), lat=p(lat),
                               rotc=None, method_ref_calc=2, use_terminal_velocity=1, stggrd=0, round_single=1,
                               min_radar_ref_dbz=5.0, low_ref_shift=-5.0, ps_adjust_thres=100.0)
        for n, e in enumerate(vars3):
            prm.vars3[n] = e
        o3 = torch.zeros((len(vars3), nlat, nlon, nlev), dtype=torch.float64, device=dev)
        rec = torch.zeros((len(vars3) * nlev, nlat, nlon), dtype=torch.float32, device=dev) if with_rec else None
        for method in (2, 3):
            for stg in (0, 1):
                if name == "t_only" and (method == 3 or stg == 1):
                    continue                                           # (neither switch reaches T)
                prm.method_ref_calc, prm.stggrd = method, stg
                ms = sorted(timed(lambda: ctx.obssim(prm, fl, o3, None, rec), args.reps))
                med = ms[len(ms) // 2]
                ledger = 8 * (nread + (nstag if stg else 0)) + len(vars3) * (8 + (4 if with_rec else 0))
                bps = ledger * npts / (med * 1e-3)
                res["cases"][f"{name}-m{method}-s{stg}"] = dict(
                    ms=round(med, 4), min=round(ms[0], 4), max=round(ms[-1], 4), ledger_bytes_per_point=ledger,
                    ledger_gb_per_s=round(bps / 1e9, 1), pct_of_hbm_peak=round(100.0 * bps / HBM_PEAK, 1),
                    pct_of_hbm_copy=round(100.0 * bps / HBM_COPY, 1), points_per_s=round(npts / (med * 1e-3)),
                    finite=bool(torch.isfinite(o3).all()), below_min_ref=int((o3[0] == 0.0).sum()) if vars3[0] == REF else None)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
