#!/usr/bin/env python3
"""superob on the device (letkf_superob_dev, include/letkf_amd_superob.h) on about one phased-array volume: 2^24 rows of report
type 22, REF and Vr alternating, one slot, scattered over C2's grid (bench_workload.py: 240 x 240 x 60), with the reference's
tables (method_v = method_t = 0 for that type) and method_h 3 and 2: ms per call (median of --reps calls after a warm-up, with
min and max), rows per second, and the algorithmic bytes of DESIGN.md section 16's ledger divided by the time, against the HBM
peak.  Not the contract bench (bench.py).

The ledger: 72 B read per row (elm, typ and the eight doubles), 4 B written per row (qc1) and 92 B per output row (three + three
int32 and eight doubles).  What the sort moves is not in it: it is the implementation's, not the algorithm's.

  bench_superob.py [--rows 16777216] [--reps 5] [--out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
from __graft_entry__ import load_package  # noqa: E402
import bench_workload as bw                # noqa: E402
from bench_obsope import timed             # noqa: E402

HBM_PEAK, HBM_COPY = 8.0e12, 6.29e12          # B/s: the specification and the measured float4 copy
ELEM_UID = [2819, 2820, 3073, 3074, 3330, 3331, 14593, 19999, 4001, 4004, 4002, 4003, 8800, 99991, 99992, 99993]
NOBTYPE, TYP_RADAR = 24, 22


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1 << 24)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    pkg = load_package()
    pkg.build()
    dev = torch.device("cuda:0")
    ctx = pkg.Context(0, torch.cuda.current_stream().cuda_stream)
    cfg = bw.CONFIGS["C2"]
    nlon, nlat, nlevx = cfg["nx"], cfg["ny"], cfg["nz"]
    n = args.rows
    gen = torch.Generator(device=dev)
    gen.manual_seed(cfg["seed"])
    uni = lambda lo, hi: lo + (hi - lo) * torch.rand(n, dtype=torch.float64, device=dev, generator=gen)
    rows = {"elm": torch.tensor([4001, 4002], dtype=torch.int32, device=dev).repeat(n // 2 + 1)[:n].contiguous(),
            "typ": torch.full((n,), TYP_RADAR, dtype=torch.int32, device=dev),
            "ri": uni(0.5, nlon + 0.5), "rj": uni(0.5, nlat + 0.5), "rk": uni(0.5, nlevx + 0.5),
            "dat": uni(-10.0, 60.0), "err": torch.tensor([3.0, 5.0], dtype=torch.float64, device=dev).repeat(n // 2 + 1)[:n].contiguous()}
    rows["lon"], rows["lat"], rows["lev"] = 135.0 + (rows["ri"] - 120.0) / 91.0, 35.0 + (rows["rj"] - 120.0) / 111.0, rows["rk"] * 300.0
    slot_off = np.array([0, n], dtype=np.int64)
    out = None
    res = dict(rows=n, nlon=nlon, nlat=nlat, nlevx=nlevx, nslots=1, nobtype=NOBTYPE, nid=len(ELEM_UID), reps=args.reps,
               library=os.path.basename(pkg.SUPEROB_LIB_PATH), device=torch.cuda.get_device_name(0),
               hbm_peak_tb_s=HBM_PEAK / 1e12, hbm_copy_tb_s=HBM_COPY / 1e12, cases={},
               measured="whole calls of letkf_superob_dev, host clock around a call that ends in a device synchronise",
               not_measured="stage 2 and stage 3 (method_v = method_t = 0 for type 22), several slots, cells of thousands of rows")
    for h in (3, 2):
        methods = list(pkg.superob_default_methods(NOBTYPE, len(ELEM_UID)))
        methods[3][:, TYP_RADAR - 1] = h

        def call():
            nonlocal out
            out = ctx.superob(rows, slot_off, (nlon, nlat, nlevx), 1, ELEM_UID, methods, out=out)

        ms = sorted(timed(call, args.reps))
        med = ms[len(ms) // 2]
        nout, counts = int(out["nout"][0]), [int(c) for c in out["counts"]]
        ledger = 76 * n + 92 * nout
        bps = ledger / (med * 1e-3)
        res["cases"][f"method_h{h}"] = dict(
            ms=round(med, 4), min=round(ms[0], 4), max=round(ms[-1], 4), rows_per_s=round(n / (med * 1e-3)), nout=nout, counts=counts,
            ledger_bytes=ledger, ledger_gb_per_s=round(bps / 1e9, 1), pct_of_hbm_peak=round(100.0 * bps / HBM_PEAK, 2),
            pct_of_hbm_copy=round(100.0 * bps / HBM_COPY, 2), finite=bool(torch.isfinite(out["dat"][:nout]).all()))
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
