#!/usr/bin/env python3
"""A/B of weight interpolation (letkf_das_interp_dev, include/letkf_amd_interp.h) against the full analysis
(letkf_das_columns_dev) on the same inputs in one process: ms per analysis at strides 2, 3, 4 with the share of the coarse
solves, the run-to-run spread, and per variable RMS(interpolated - full) / RMS(full - first guess).  Synthetic data
(bench_workload, spatially correlated members and observation-space perturbations: interpolated weights only make sense
where neighbouring points see similar observations).  Not the contract bench (bench.py).

  bench_interp.py [WORKLOAD] [--strides 2 3 4] [--reps 3] [--out FILE]
  bench_interp.py [WORKLOAD] --full-only     the full analysis alone (with LETKF_AMD_LIB: another build of the library)

A/B against another build: LETKF_AMD_LIB=/path/to/its/libletkf_amd.so bench_interp.py ..., then the same line without it.  A
library that lacks the window entries (letkf_amd_interp_window.h; this script does not call them) is loaded without them."""
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
    """[ms] of reps runs after one warm-up, each synchronised"""
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def summary(ms):
    s = sorted(ms)
    return dict(ms=s[len(s) // 2], min=s[0], max=s[-1], spread=s[-1] - s[0], runs=[round(v, 3) for v in ms])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("workload", nargs="?", default="C2")
    ap.add_argument("--strides", type=int, nargs="+", default=[2, 3, 4])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--full-only", action="store_true")
    ap.add_argument("--ws-gb", type=float, default=0.0, help="ws_bytes of the interpolation route / list_bytes of the full one (0: 8 GiB)")
    args = ap.parse_args()
    pkg = load_package()
    if args.full_only:
        pkg.INTERP_ARGTYPES.clear()      # (another build of the library may not have the entries)
    import ctypes
    if os.path.exists(pkg.LIB_PATH) and not hasattr(ctypes.CDLL(pkg.LIB_PATH), "letkf_das_interp_window_dev"):
        pkg.INTERP_WINDOW_ARGTYPES.clear()      # (a build from before include/letkf_amd_interp_window.h: not called here)
    pkg.build()
    dev = torch.device("cuda:0")
    ctx = pkg.Context(0, torch.cuda.current_stream().cuda_stream)
    w = bw.build(args.workload, dev, ensval_kind="correlated", lists=False)
    cfg = w["cfg"]
    k, nv, npts, nens = w["k"], w["nv"], w["npts"], w["nens"]
    nx, ny, nlev = cfg["nx"], cfg["ny"], cfg["nz"]
    sp, sm, sv = w["sp"], w["sm"], w["sv"]
    ctx.ens_mean(k, nv, npts, w["gues"], sp, sm, sv)
    ctx.to_perturbations(k, nv, npts, w["gues"], sp, sm, sv)
    bw.correlate_ensval(w)
    t_s, keep, order, pts = bw.search_tables(w, pkg, dev)
    ens, dep = w["ensval"][order].contiguous(), w["dep"][order].contiguous()
    nij = nx * ny
    rig, rjg = pts[0][:nij].contiguous(), pts[1][:nij].contiguous()
    infl = torch.full((npts * nv,), 1.0, dtype=torch.float64, device=dev)
    budget = int(args.ws_gb * 2 ** 30)
    relax = dict(relax_alpha_spread=0.95)
    full = torch.zeros_like(w["gues"])
    st_full = torch.zeros(npts, dtype=torch.int32, device=dev)

    def run_full():
        ctx.das_columns(k, nv, t_s, nij, nlev, rig, rjg, pts[2], pts[3], ens, w["kld"], dep, infl, w["gues"], full, sp, sm, sv,
                        list_bytes=budget, status=st_full, **relax)
    res = dict(workload=args.workload, k=k, nv=nv, nx=nx, ny=ny, nlev=nlev, npts=npts, n_obs=int(w["nobs"]), reps=args.reps,
               library=os.path.basename(pkg.LIB_PATH), device=torch.cuda.get_device_name(0))
    res["full"] = summary(timed(run_full, args.reps))
    res["full"]["path"] = ctx.last_path()
    res["full"]["status_nonzero"] = int((st_full != 0).sum())
    if not args.full_only:
        g = w["gues"].view(nv, nens, npts)
        f = full.view(nv, nens, npts)
        rms = lambda x: float((x ** 2).mean().sqrt())
        incr = [rms(f[v, :k] - (g[v, k:k + 1] + g[v, :k])) for v in range(nv)]               # RMS(full analysis - first guess)
        anal = torch.zeros_like(w["gues"])
        status = torch.zeros(npts, dtype=torch.int32, device=dev)
        res["strides"] = {}
        for s in args.strides:
            ncoarse = len(pkg.interp_coarse_axis(nx, s)) * len(pkg.interp_coarse_axis(ny, s)) * nlev
            nobs_c = torch.zeros(ncoarse, dtype=torch.int32, device=dev)

            def run_interp():
                ctx.das_interp(k, nv, t_s, nx, ny, nlev, s, s, rig, rjg, pts[2], pts[3], ens, w["kld"], dep, infl, w["gues"], anal,
                               sp, sm, sv, ws_bytes=budget, nobs_coarse=nobs_c, status=status, **relax)
            r = summary(timed(run_interp, args.reps))
            # the coarse solves' share: HIP events around the solver launches of one more call
            ctx.timing_enable(True)
            ctx.timing_read(reset=True)
            run_interp()
            avg, n = ctx.timing_read(reset=True)
            ctx.timing_enable(False)
            r["coarse_solves_ms"] = avg * n
            r["search_gather_apply_ms"] = r["ms"] - avg * n
            r["solver_launches"] = n
            r["coarse_points"] = ncoarse
            r["coarse_nobs_mean"] = float(nobs_c.double().mean())
            r["path"] = ctx.last_path()
            r["status_nonzero"] = int((status != 0).sum())
            a = anal.view(nv, nens, npts)
            r["rms_ratio_per_variable"] = [rms(a[v, :k] - f[v, :k]) / incr[v] for v in range(nv)]
            r["speedup_vs_full"] = res["full"]["ms"] / r["ms"]
            r["pays"] = bool(res["full"]["ms"] - r["ms"] > max(res["full"]["spread"], r["spread"]))
            res["strides"][str(s)] = r
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
