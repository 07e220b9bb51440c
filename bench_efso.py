#!/usr/bin/env python3
"""EFSO (das_efso, scale/letkf/letkf_tools.f90:1158-1302) on one MI355X at C2 size through the C ABI: the column search and
the EFSO passes (letkf_efso_columns_dev) for every grid point, nterm = 3, and for comparison the analysis loop
(letkf_das_columns_dev) on the same grid from the same process.  Synthetic data (bench_workload.C2); everything
device-resident.  Prints one JSON line: ms per call, pairs per second, algorithmic bytes (the ya row of every pair,
fcst / fcer of the variables in a term, the pair buffer written and read back) as GB/s and as a fraction of 8 TB/s.
Not the contract bench (bench.py)."""
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
from __graft_entry__ import load_package  # noqa: E402
import bench_workload as bw                # noqa: E402

HBM_BPS = 8.0e12
# SCALE's nv3d = 11 (U, V, W, T, P, QV, QC, QR, QI, QS, QG): das_efso's terms 1 = U/V (kinetic), 2 = T, 3 = QV
TERM_OF_VAR = [0, 0, -1, 1, -1, 2, -1, -1, -1, -1, -1]


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3


def main():
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    name = sys.argv[1] if len(sys.argv) > 1 else "C2"
    pkg = load_package()
    pkg.build()
    dev = torch.device("cuda:0")
    ctx = pkg.Context(0, torch.cuda.current_stream().cuda_stream)
    w = bw.build(name, dev, lists=False)
    cfg = w["cfg"]
    k, nv, npts, kld, nobs = w["k"], w["nv"], w["npts"], w["kld"], w["nobs"]
    nij, nlev = cfg["nx"] * cfg["ny"], cfg["nz"]
    sp, sm, sv = w["sp"], w["sm"], w["sv"]
    nterm = 3
    t_s, keep, order, pts = bw.search_tables(w, pkg, dev)
    rig, rjg = pts[0][:nij].contiguous(), pts[1][:nij].contiguous()
    ens_sorted = w["ensval"][order].contiguous()
    dep_sorted = w["dep"][order].contiguous()
    gues = w["gues"]
    ctx.to_perturbations(k, nv, npts, gues, sp, sm, sv)
    # fcst: the normed forecast perturbations (here the state's own perturbations), fcer: one value per point and variable
    g = torch.Generator(device=dev)
    g.manual_seed(5)
    fcer = torch.randn(nv * npts, dtype=torch.float64, device=dev, generator=g) * 0.05
    djdy = torch.zeros(nobs * nterm, dtype=torch.float64, device=dev)

    def efso():
        djdy.zero_()
        ctx.efso_columns(k, nv, TERM_OF_VAR, nterm, t_s, nij, nlev, rig, rjg, pts[2], pts[3], ens_sorted, kld, nobs, gues, sp,
                         sm, sv, fcer, 1, npts, djdy)
    efso_ms = timed(efso, reps)
    path = ctx.last_path()
    first = djdy.clone()
    efso()
    torch.cuda.synchronize()
    deterministic = bool(torch.equal(first.view(torch.int64), djdy.view(torch.int64)))
    obsense = torch.empty_like(djdy)
    obsense_ms = timed(lambda: ctx.efso_obsense(nterm, djdy, dep_sorted, obsense), reps)
    # pairs: the lists' length (one count pass of the column search)
    off, idx, rd, rl = ctx.obs_search_columns(t_s, nij, nlev, rig, rjg, pts[2], pts[3])
    npairs = int(off[-1])
    del off, idx, rd, rl
    torch.cuda.empty_cache()
    nvt = sum(1 for t in TERM_OF_VAR if t >= 0)
    bytes_alg = npairs * k * 8 + npts * (k + 1) * nvt * 8 + 2 * npairs * nterm * 8
    # the analysis on the same grid (das_columns; RTPS as bench.py)
    infl = torch.ones(npts * nv, dtype=torch.float64, device=dev)
    anal = torch.empty_like(gues)
    st = torch.zeros(npts, dtype=torch.int32, device=dev)
    das_ms = timed(lambda: ctx.das_columns(k, nv, t_s, nij, nlev, rig, rjg, pts[2], pts[3], ens_sorted, kld, dep_sorted, infl,
                                           gues, anal, sp, sm, sv, status=st, relax_alpha_spread=0.95), reps)
    print(json.dumps({
        "workload": f"{name}: {cfg['nx']}x{cfg['ny']}x{cfg['nz']}, k={k}, nv={nv}, {nobs} obs rows, nterm={nterm}",
        "efso_columns_ms": efso_ms, "efso_obsense_ms": obsense_ms, "pairs": npairs, "pairs_per_s": npairs / (efso_ms * 1e-3),
        "algorithmic_bytes": bytes_alg, "algorithmic_GBps": bytes_alg / (efso_ms * 1e-3) / 1e9,
        "fraction_of_8TBps": bytes_alg / (efso_ms * 1e-3) / HBM_BPS, "das_columns_ms": das_ms,
        "efso_over_das_columns": efso_ms / das_ms, "bitwise_repeatable": deterministic, "kernel": path}))


if __name__ == "__main__":
    main()
