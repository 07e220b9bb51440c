#!/usr/bin/env python3
"""obsope_cal's first scan on the device (letkf_obsscan_dev, include/letkf_amd_obsscan.h) on the 2^24 rows bench_superob.py makes
(the same generator, the same ri / rj over C2's grid of 240 x 240 points, here with halos of 2), one file, a dif per row over seven
slots and both sides of the window.  Two layouts: 1 subdomain x 1 slot, where every row of the window lands in one bucket (the
worst case for any shared counter), and 16 x 16 subdomains x 7 slots.  Per layout: ms per call between HIP events and by the host
clock (median of --reps calls after two warm-up calls, with min and max), rows per second, and the bytes of the key and fill
passes divided by the time, against the HBM peak.  Not the contract bench (bench.py).

The ledger: the key pass reads 24 B per row (ri, rj, dif) and writes 8 B (key, flat row) plus 12 B for rank, slot and own; the
fill pass reads 8 B per list row (sorted key and row) and writes 12 B (set, idx, qc).  What the sort moves is not in it: it is
the implementation's, not the algorithm's.  The only comparison is the wall time of the numpy statement (tests/_obsscan.py) on
the same rows on this box's host: what a host pays today for the same lists; with --statement-rows fewer rows it is scaled.

  bench_obsscan.py [--rows 16777216] [--reps 7] [--statement-rows N] [--out FILE]
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
from __graft_entry__ import load_package  # noqa: E402
import bench_workload as bw                # noqa: E402
import _obsscan as S                       # noqa: E402

HBM_PEAK, HBM_COPY = 8.0e12, 6.29e12          # B/s: the specification and the measured float4 copy
HALO = 2
LAYOUTS = {"1x1_subdomains_1_slot": (1, 1, (1, 1, 1, 4200.0)), "16x16_subdomains_7_slots": (16, 16, (1, 7, 4, 600.0))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1 << 24)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--statement-rows", type=int, default=None)
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
    dif = uni(-2400.0, 2400.0)                                            # the window is (-2100, 2100]
    off = np.array([0, n], dtype=np.int64)
    files = pkg.ObsFileRows()
    files.nfile, files.off = 1, off.ctypes.data_as(C.c_void_p)
    files.ri, files.rj = C.c_void_p(ri.data_ptr()), C.c_void_p(rj.data_ptr())
    res = dict(rows=n, nx=nx, ny=ny, halo=HALO, reps=args.reps, library=os.path.basename(pkg.OBSSCAN_LIB_PATH),
               device=torch.cuda.get_device_name(0), hbm_peak_tb_s=HBM_PEAK / 1e12, hbm_copy_tb_s=HBM_COPY / 1e12, cases={},
               measured="whole calls of letkf_obsscan_dev with rank, slot and own asked for: HIP events around the call and the host "
                        "clock around it (the call ends in its own synchronisation)",
               not_measured="several files, files that do not run, the operator that follows")
    host = {name: t.cpu().numpy() for name, t in (("ri", ri), ("rj", rj), ("dif", dif))}
    for label, (px, py, slots) in LAYOUTS.items():
        layout = (nx // px, ny // py, HALO, HALO, px, py)
        out = None
        ev, wall = [], []
        for rep in range(args.reps + 2):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record()
            out = ctx.obsscan(files, dif, layout, slots, myrank_d=0, out=out)
            e1.record()
            torch.cuda.synchronize()
            if rep >= 2:
                wall.append((time.perf_counter() - t0) * 1e3)
                ev.append(e0.elapsed_time(e1))
        ev.sort(), wall.sort()
        med = ev[len(ev) // 2]
        ledger = (24 + 8 + 12) * n + (8 + 12) * n
        bps = ledger / (med * 1e-3)
        ns = args.statement_rows or n
        case = dict(off=np.array([0, ns], dtype=np.int64), ri=host["ri"][:ns], rj=host["rj"][:ns], dif=host["dif"][:ns], layout=layout,
                    slots=slots, run=None)
        t0 = time.perf_counter()
        st = S.scan(case, myrank_d=0)
        st_ms = (time.perf_counter() - t0) * 1e3
        same = None
        if ns == n:
            same = all(np.array_equal(st[k], out[k] if isinstance(out[k], np.ndarray) else out[k].cpu().numpy()) for k in st)
        res["cases"][label] = dict(
            prc_num_x=px, prc_num_y=py, slots=list(slots), buckets=px * py * (slots[1] - slots[0] + 3),
            ms=round(med, 4), min=round(ev[0], 4), max=round(ev[-1], 4), host_clock_ms=round(wall[len(wall) // 2], 4),
            rows_per_s=round(n / (med * 1e-3)), ledger_bytes=ledger, ledger_gb_per_s=round(bps / 1e9, 1),
            pct_of_hbm_peak=round(100.0 * bps / HBM_PEAK, 2), pct_of_hbm_copy=round(100.0 * bps / HBM_COPY, 2),
            largest_bucket=int(out["bsn"].max()), out_of_time=int(out["bsn"][:, -2].sum()), out_of_domain=int(out["bsn"][0, -1]),
            numpy_statement_ms=round(st_ms, 1), numpy_statement_rows=ns, equals_statement=same,
            statement_over_device=round(st_ms * (n / ns) / med, 1))
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
