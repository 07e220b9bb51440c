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
same process.  Prints one JSON line: ms per call of each route, pairs and pairs per second of the advected route.

--norm: EFSO's two ends (include/letkf_amd.h section 13) at the same size: letkf_efso_norm_dev on a forecast ensemble of
k members x nv variables (total fields, a pressure profile in slot 4) with the fcer assembly from three means, dp/ps from
the mean pressure (the two small passes and the one read-back included) and, separately, with dp/ps given; then
letkf_efso_summary_dev on nterm = 3 impacts of every observation row.  Each norm call gets the pressure slot back first
(outside the timed interval: the norm works in place).  Prints one JSON line: ms per call, algorithmic bytes (inputs read
once where the norm needs them, every output written once) as GB/s and as a fraction of 8 TB/s."""
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
    if "--norm" in sys.argv:
        return main_norm([a for a in sys.argv[1:] if a != "--norm"])
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


def main_norm(argv):
    reps = int(argv[1]) if len(argv) > 1 else 5
    name = argv[0] if argv else "C2"
    pkg = load_package()
    pkg.build()
    dev = torch.device("cuda:0")
    ctx = pkg.Context(0, torch.cuda.current_stream().cuda_stream)
    cfg = bw.CONFIGS[name]
    k, nv, nobs = cfg["k"], 11, 1 << 20          # (the summary: a million observation rows)
    nij, nlev = cfg["nx"] * cfg["ny"], cfg["nz"]
    npts = nij * nlev
    g = torch.Generator(device=dev)
    g.manual_seed(3)
    # the forecast ensemble, gues3d's order (p fastest): total fields, a pressure profile in slot 4 (SCALE's iv3d_p - 1)
    fcst = torch.randn(nv * k * npts, dtype=torch.float64, device=dev, generator=g).view(nv, k, npts)
    lev = torch.arange(nlev, dtype=torch.float64, device=dev).repeat_interleave(nij)
    p_prof = 1.0e5 * torch.exp(-2.5 * lev / max(nlev - 1, 1))
    fcst[4] = fcst[4] * 50.0 + p_prof
    p_slot = fcst[4].clone()
    fcer = torch.zeros(nv * npts, dtype=torch.float64, device=dev)
    xs = [torch.randn(nv * npts, dtype=torch.float64, device=dev, generator=g) for _ in range(3)]
    wlev = torch.full((npts,), 1.0 / nlev, dtype=torch.float64, device=dev)
    prm = pkg.EfsoNormParams()
    prm.k, prm.nv, prm.iv_u, prm.iv_v, prm.iv_t, prm.iv_q, prm.iv_p = k, nv, 0, 1, 3, 5, 4
    prm.tar_minlev, prm.tar_maxlev = 1, nlev
    prm.cp, prm.tref, prm.hvap, prm.wmoist = 1004.64, 280.0, 2.501e6, 1.0
    prm.tar_minlon, prm.tar_maxlon, prm.tar_minlat, prm.tar_maxlat = 0.0, 360.0, -90.0, 90.0
    flat = fcst.view(-1)

    def norm_ms(with_wlev):
        ts = []
        for _ in range(reps + 1):
            fcst[4].copy_(p_slot)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            ctx.efso_norm(prm, nij, nlev, flat, 1, npts, npts * k, fcer, 1, npts, xf=xs[0], xg=xs[1], xa=xs[2],
                          wlev=wlev if with_wlev else None)
            b.record()
            torch.cuda.synchronize()
            ts.append(a.elapsed_time(b))
        return sum(ts[1:]) / reps, ctx.last_path()
    ms_computed, path = norm_ms(False)
    ms_given, path_given = norm_ms(True)
    # algorithmic bytes (fmean not requested): the four variables with a factor read once (k members), the three fcer
    # means of those four, dp/ps; every output written once; the dp/ps passes read the pressure slot and write / read
    # the mean pressure and dp/ps
    nlive = 4
    main_bytes = 8 * npts * (nlive * k + 3 * nlive + 1 + nv * k + nv)
    pre_bytes = 8 * npts * (k + 3)
    # the summary: nterm = 3 impacts of every row
    nterm, nobtype = 3, 21
    uid = [2819, 2820, 3073, 3330, 3331, 14593, 4001, 4002]
    nrow = max(nobs, 1)
    obsense = torch.randn(nrow * nterm, dtype=torch.float64, device=dev, generator=g)
    elm = torch.tensor(uid, dtype=torch.int32, device=dev)[torch.randint(0, len(uid), (nrow,), device=dev, generator=g)]
    typ = torch.randint(1, nobtype + 2, (nrow,), device=dev, generator=g, dtype=torch.int32)
    olat = torch.rand(nrow, dtype=torch.float64, device=dev, generator=g) * 180.0 - 90.0
    outs = ctx.efso_summary(nterm, obsense, elm, typ, olat, uid, nobtype)
    sum_ms = timed(lambda: ctx.efso_summary(nterm, obsense, elm, typ, olat, uid, nobtype, outs=outs), reps)
    print(json.dumps({
        "workload": f"{name}: {cfg['nx']}x{cfg['ny']}x{cfg['nz']} = {npts} points, k={k}, nv={nv}, fcer assembled from three "
                    f"means; summary: {nrow} rows, nterm={nterm}, nobtype={nobtype}, nid={len(uid)}",
        "efso_norm_ms": ms_computed, "efso_norm_wlev_given_ms": ms_given,
        "algorithmic_bytes": main_bytes + pre_bytes, "algorithmic_GBps": (main_bytes + pre_bytes) / (ms_computed * 1e-3) / 1e9,
        "fraction_of_8TBps": (main_bytes + pre_bytes) / (ms_computed * 1e-3) / HBM_BPS,
        "wlev_given_bytes": main_bytes, "wlev_given_GBps": main_bytes / (ms_given * 1e-3) / 1e9,
        "efso_summary_ms": sum_ms, "kernel": path, "kernel_wlev_given": path_given}))


if __name__ == "__main__":
    main()
