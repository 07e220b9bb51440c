#!/usr/bin/env python3
"""EFSO (das_efso, scale/letkf/letkf_tools.f90:1158-1302) on one MI355X at C2 size through the C ABI: the column search and
the EFSO passes (letkf_efso_columns_dev) for every grid point, nterm = 3, and for comparison the analysis loop
(letkf_das_columns_dev) on the same grid from the same process.  Synthetic data (bench_workload.C2); everything
device-resident.  Prints one JSON line: ms per call, pairs per second, algorithmic bytes (the ya row of every pair,
fcst / fcer of the variables in a term, the pair buffer written and read back) as GB/s and as a fraction of 8 TB/s.
Not the contract bench (bench.py).

--locadv: EFSO with localisation advection instead (include/letkf_amd.h section 12): a fixed wind profile u = 10 + 20 lev /
(nlev - 1) m/s, v = 5 m/s at both times, eft = 1 h, locadv_rate = 0.5 (18 .. 36 cells of displacement at dx = 1 km), then
letkf_efso_locadv_dev + letkf_efso_search_dev (the point search over every point) against letkf_efso_columns_dev from the
same process.  Prints one JSON line: ms per call of each route, pairs and pairs per second of the advected route."""
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
    argv = [a for a in sys.argv[1:] if a != "--locadv"]
    if len(argv) != len(sys.argv) - 1:
        return main_locadv(argv)
    reps = int(argv[1]) if len(argv) > 1 else 3
    name = argv[0] if argv else "C2"
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


def main_locadv(argv):
    reps = int(argv[1]) if len(argv) > 1 else 3
    name = argv[0] if argv else "C2"
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
    gues = w["gues"]
    ctx.to_perturbations(k, nv, npts, gues, sp, sm, sv)
    g = torch.Generator(device=dev)
    g.manual_seed(5)
    fcer = torch.randn(nv * npts, dtype=torch.float64, device=dev, generator=g) * 0.05
    djdy = torch.zeros(nobs * nterm, dtype=torch.float64, device=dev)
    # the wind profile: not drawn from the synthetic state, the same at the initial and the evaluation time
    lev = torch.arange(nlev, dtype=torch.float64, device=dev).repeat_interleave(nij)
    u = 10.0 + 20.0 * lev / max(nlev - 1, 1)
    v = torch.full_like(u, 5.0)
    rate, eft, dx, dy = 0.5, 1.0, float(t_s.dx), float(t_s.dy)
    ri = torch.empty(npts, dtype=torch.float64, device=dev)
    rj = torch.empty_like(ri)

    def advected():
        djdy.zero_()
        ctx.efso_locadv(rig, rjg, nlev, u, v, u, v, rate, eft, dx, dy, ri, rj)
        ctx.efso_search(k, nv, TERM_OF_VAR, nterm, t_s, ri, rj, pts[2], pts[3], ens_sorted, kld, nobs, gues, sp, sm, sv, fcer, 1,
                        npts, djdy)

    def columns():
        djdy.zero_()
        ctx.efso_columns(k, nv, TERM_OF_VAR, nterm, t_s, nij, nlev, rig, rjg, pts[2], pts[3], ens_sorted, kld, nobs, gues, sp,
                         sm, sv, fcer, 1, npts, djdy)
    adv_ms = timed(advected, reps)
    path = ctx.last_path()
    first = djdy.clone()
    advected()
    torch.cuda.synchronize()
    deterministic = bool(torch.equal(first.view(torch.int64), djdy.view(torch.int64)))
    locadv_ms = timed(lambda: ctx.efso_locadv(rig, rjg, nlev, u, v, u, v, rate, eft, dx, dy, ri, rj), reps)
    col_ms = timed(columns, reps)
    disp = (rig.repeat(nlev) - ri).abs()
    # pairs of the advected route: the lists' length at the advected positions (one count pass)
    off, idx, rd, rl = ctx.obs_search(t_s, ri, rj, pts[2], pts[3])
    npairs = int(off[-1])
    del off, idx, rd, rl
    torch.cuda.empty_cache()
    print(json.dumps({
        "workload": f"{name}: {cfg['nx']}x{cfg['ny']}x{cfg['nz']}, k={k}, nv={nv}, {nobs} obs rows, nterm={nterm}, "
                    f"locadv_rate={rate}, eft={eft} h, u=10..30 m/s, v=5 m/s",
        "displacement_cells": [float(disp.min()), float(disp.max())],
        "efso_locadv_search_ms": adv_ms, "efso_locadv_only_ms": locadv_ms, "efso_columns_ms": col_ms,
        "advected_over_columns": adv_ms / col_ms, "pairs": npairs, "pairs_per_s": npairs / (adv_ms * 1e-3),
        "bitwise_repeatable": deterministic, "kernel": "efso_locadv_kernel + " + path}))


if __name__ == "__main__":
    main()
