#!/usr/bin/env python3
"""das_letkf_obs (scale/letkf/letkf_tools.f90:933-1156) on one MI355X at C2 size through the C ABI: letkf_das_obs_dev with
every row of the observation table as a target, RTPS as bench.py, and for scale the analysis loop (letkf_das_columns_dev)
on the same grid from the same process.  Synthetic data (bench_workload.C2, its ensemble size replaced by --k);
everything device-resident.  Prints one JSON line: ms per call, targets per second, local-list entries, the route
(letkf_ctx_last_path), das_columns' ms.  Not the contract bench (bench.py).

    python bench_obsanal.py [--config C2] [--k 50] [--reps 3]"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
from __graft_entry__ import load_package  # noqa: E402
import bench_workload as bw                # noqa: E402


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C2")
    ap.add_argument("--k", type=int, default=0, help="ensemble size (0: the configuration's)")
    ap.add_argument("--reps", type=int, default=3)
    o = ap.parse_args()
    name = o.config
    if o.k and o.k != bw.CONFIGS[name]["k"]:
        name = f"{o.config}-k{o.k}"
        bw.CONFIGS[name] = dict(bw.CONFIGS[o.config], k=o.k)
    pkg = load_package()
    pkg.build()
    dev = torch.device("cuda:0")
    ctx = pkg.Context(0, torch.cuda.current_stream().cuda_stream)
    w = bw.build(name, dev, lists=False)
    cfg = w["cfg"]
    k, nv, npts, kld = w["k"], w["nv"], w["npts"], w["kld"]
    nij, nlev = cfg["nx"] * cfg["ny"], cfg["nz"]
    sp, sm, sv = w["sp"], w["sm"], w["sv"]
    t_s, keep, order, pts = bw.search_tables(w, pkg, dev)
    ens_sorted = w["ensval"][order].contiguous()
    dep_sorted = w["dep"][order].contiguous()
    nobs = ens_sorted.shape[0]
    f64 = torch.float64
    ya = torch.empty(nobs * k, dtype=f64, device=dev)
    ya_mean = torch.empty(nobs, dtype=f64, device=dev)
    ya_table = torch.zeros(nobs * kld, dtype=f64, device=dev)
    dep_a = torch.empty(nobs, dtype=f64, device=dev)
    nobs_out = torch.empty(nobs, dtype=torch.int32, device=dev)
    status = torch.empty(nobs, dtype=torch.int32, device=dev)

    def obsanal():
        ctx.das_obs(k, -1, t_s, ens_sorted, kld, dep_sorted, nobs, ya, lda=k, ya_mean=ya_mean, ya_table=ya_table, dep_a=dep_a,
                    nobs_out=nobs_out, status=status, infl_mul=1.0, relax_alpha_spread=0.95)
    obs_ms = timed(obsanal, o.reps)
    path = ctx.last_path()
    first = ya.clone()
    obsanal()
    torch.cuda.synchronize()
    repeatable = bool(torch.equal(first.view(torch.int64), ya.view(torch.int64)))
    nent = int(nobs_out.to(torch.int64).sum())
    bad = int((status != 0).sum())
    rms_b = float(dep_sorted.pow(2).mean().sqrt())
    rms_a = float(dep_a.pow(2).mean().sqrt())
    # the analysis on the same grid (das_columns; RTPS as bench.py)
    gues = w["gues"]
    ctx.to_perturbations(k, nv, npts, gues, sp, sm, sv)
    infl = torch.ones(npts * nv, dtype=f64, device=dev)
    anal = torch.empty_like(gues)
    st = torch.zeros(npts, dtype=torch.int32, device=dev)
    rig, rjg = pts[0][:nij].contiguous(), pts[1][:nij].contiguous()
    das_ms = timed(lambda: ctx.das_columns(k, nv, t_s, nij, nlev, rig, rjg, pts[2], pts[3], ens_sorted, kld, dep_sorted, infl,
                                           gues, anal, sp, sm, sv, status=st, relax_alpha_spread=0.95), o.reps)
    das_path = ctx.last_path()
    print(json.dumps({
        "workload": f"{name}: {cfg['nx']}x{cfg['ny']}x{cfg['nz']}, k={k}, {nobs} obs rows, every row a target, RTPS 0.95",
        "das_obs_ms": obs_ms, "targets": nobs, "targets_per_s": nobs / (obs_ms * 1e-3), "list_entries": nent,
        "mean_local_obs": nent / max(nobs, 1), "status_nonzero": bad, "rms_o_minus_b": rms_b, "rms_o_minus_a": rms_a,
        "bitwise_repeatable": repeatable, "kernel": path, "das_columns_ms": das_ms, "das_columns_points": npts,
        "das_obs_over_das_columns": obs_ms / das_ms, "das_columns_kernel": das_path}))


if __name__ == "__main__":
    main()
