#!/usr/bin/env python3
"""What NOBS_OUT costs (include/letkf_amd_nobsout.h): ms per analysis of
  (a) letkf_das_columns_dev,
  (b) letkf_das_columns_nobs_dev with both diagnostics,
  (c) today's way: (a) plus a separate letkf_obs_search_columns_dev count-and-fill with the diagnostics,
  (d) letkf_nobs_fields_dev on the grid's points, in ms and against the bytes it must move at the HBM peak,
on bench_workload's grid under --max-nobs (two limited radar types) and without a limit, with the run-to-run spread.  Synthetic
data; not the contract bench (bench.py).

  bench_nobsout.py [WORKLOAD] [--max-nobs 100] [--reps 5] [--out FILE]
  bench_nobsout.py [WORKLOAD] --only-a ...       (a) alone: with LETKF_AMD_LIB=/path/to/another/libletkf_amd.so that build's (a)
  bench_nobsout.py --merge OUT FILE [FILE ...]   one record from the runs of a session; (a) per library with the spread over the runs"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12      # bytes / s


def timed(fn, reps, torch):
    """[ms] of reps runs after two warm-ups, each synchronised"""
    for _ in range(2):
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


def one_case(pkg, torch, ctx, workload, max_nobs, reps, only_a):
    import bench_workload as bw
    dev = torch.device("cuda:0")
    w = bw.build(workload, dev, lists=False)
    cfg = w["cfg"]
    k, nv, npts, nens = w["k"], w["nv"], w["npts"], w["nens"]
    nij, nlev = cfg["nx"] * cfg["ny"], cfg["nz"]
    sp, sm, sv = w["sp"], w["sm"], w["sv"]
    ctx.ens_mean(k, nv, npts, w["gues"], sp, sm, sv)
    ctx.to_perturbations(k, nv, npts, w["gues"], sp, sm, sv)
    t_s, keep, order, pts = bw.search_tables(w, pkg, dev, max_nobs=max_nobs)
    nct = t_s.nctype
    ens, dep = w["ensval"][order].contiguous(), w["dep"][order].contiguous()
    rig, rjg = pts[0][:nij].contiguous(), pts[1][:nij].contiguous()
    infl = torch.full((npts * nv,), 1.0, dtype=torch.float64, device=dev)
    anal = torch.zeros_like(w["gues"])
    status = torch.zeros(npts, dtype=torch.int32, device=dev)
    nobs_out = torch.zeros(npts, dtype=torch.int32, device=dev)
    common = (k, nv, t_s, nij, nlev, rig, rjg, pts[2], pts[3], ens, w["kld"], dep, infl, w["gues"], anal, sp, sm, sv)
    kw = dict(status=status, nobs_out=nobs_out, relax_alpha_spread=0.95)
    res = dict(max_nobs=max_nobs, nctype=nct, k=k, nij1=nij, nlev=nlev, npts=npts)

    def run_a():
        ctx.das_columns(*common, **kw)
    res["a_das_columns"] = summary(timed(run_a, reps, torch))
    res["a_das_columns"]["path"] = ctx.last_path()
    res["local_obs_mean"] = float(nobs_out.double().mean())
    if only_a:
        return res
    anal_a, nobs_a = anal.clone(), nobs_out.clone()
    n_ct = torch.zeros(npts * nct, dtype=torch.int32, device=dev)
    c_ct = torch.zeros(npts * nct, dtype=torch.float64, device=dev)

    def run_b():
        ctx.das_columns_nobs(*common, nobs_ctype=n_ct, cutd_ctype=c_ct, **kw)
    res["b_das_columns_nobs"] = summary(timed(run_b, reps, torch))
    res["b_das_columns_nobs"]["path"] = ctx.last_path()
    res["b_same_analysis_bits"] = bool(torch.equal(anal, anal_a) and torch.equal(nobs_out, nobs_a))
    res["b_row_sums_are_nobs_out"] = bool(torch.equal(n_ct.view(npts, nct).sum(dim=1).to(torch.int32), nobs_out))
    n_b, c_b = n_ct.clone(), c_ct.clone()

    # (c) the separate search: count pass, prefix sum, fill pass with the diagnostics into lists allocated once
    counts = torch.zeros(npts, dtype=torch.int32, device=dev)
    off = torch.zeros(npts + 1, dtype=torch.int64, device=dev)
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())

    def search(fill, idx=None, rd=None, rl=None):
        rc = ctx._l.letkf_obs_search_columns_dev(ctx._c, C.byref(t_s), nij, nlev, p(rig), p(rjg), p(pts[2]), p(pts[3]), fill,
                                                 None if fill else p(counts), p(off) if fill else None, p(idx), p(rd), p(rl),
                                                 p(n_ct) if fill else None, p(c_ct) if fill else None)
        assert rc == 0, rc
    search(0)
    nnz = int(counts.long().sum())
    idx = torch.empty(max(nnz, 1), dtype=torch.int32, device=dev)
    rd, rl = (torch.empty(max(nnz, 1), dtype=torch.float64, device=dev) for _ in range(2))

    def run_search():
        search(0)
        off[1:] = torch.cumsum(counts.to(torch.int64), 0)
        search(1, idx, rd, rl)

    def run_c():
        run_a()
        run_search()
    res["c_das_columns_plus_search"] = summary(timed(run_c, reps, torch))
    res["c_search_alone"] = summary(timed(run_search, reps, torch))
    res["c_list_entries"] = nnz
    res["b_same_diagnostics_bits_as_c"] = bool(torch.equal(n_ct, n_b) and torch.equal(c_ct.view(torch.int64), c_b.view(torch.int64)))
    a, b, c = (res[n]["ms"] for n in ("a_das_columns", "b_das_columns_nobs", "c_das_columns_plus_search"))
    res["b_minus_a_ms"], res["c_minus_a_ms"] = b - a, c - a

    # (d) the fields: nobtype = 24; the ledger is what the kernel must move (all of nobs_ctype, all of cutd_ctype, both outputs)
    nobtype = 24
    elm_u, typ = ([9, 11], [22, 22]) if nct == 2 else ([9], [22])
    w3n = torch.zeros(npts * (nobtype + 6), dtype=torch.float64, device=dev)
    w3 = torch.zeros(npts * 11, dtype=torch.float64, device=dev)

    def run_d():
        ctx.nobs_fields(npts, elm_u, typ, n_ct, c_ct, work3dn=w3n, fields=w3, nobtype=nobtype)
    r = summary(timed(run_d, max(reps, 7), torch))
    r["ledger_bytes"] = npts * (12 * nct + 88 + 8 * (nobtype + 6))
    r["share_of_hbm_peak"] = r["ledger_bytes"] / HBM_PEAK / (r["ms"] * 1e-3)
    res["d_nobs_fields"] = r
    return res


def merge(out, files):
    runs = [json.load(open(f)) for f in files]
    rec = dict(runs=[dict(file=os.path.basename(f), library=r["library"], only_a=r["only_a"]) for f, r in zip(files, runs)])
    full = [r for r in runs if not r["only_a"]]
    rec["device"], rec["workload"], rec["reps"] = runs[0]["device"], runs[0]["workload"], runs[0]["reps"]
    rec["cases"] = full[0]["cases"] if full else {}
    # (a) per library over all runs of the session: the medians of each run, and their spread from run to run
    rec["a_by_library"] = {}
    for name in sorted({c for r in runs for c in r["cases"]}):
        by = {}
        for r in runs:
            if name in r["cases"]:
                by.setdefault(r["library"], []).append(r["cases"][name]["a_das_columns"]["ms"])
        rec["a_by_library"][name] = {lib: dict(medians=[round(v, 3) for v in ms], spread=max(ms) - min(ms), mean=sum(ms) / len(ms))
                                     for lib, ms in by.items()}
    with open(out, "w") as fh:
        fh.write(json.dumps(rec, indent=1) + "\n")
    print(json.dumps(rec["a_by_library"]))


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--merge":
        return merge(sys.argv[2], sys.argv[3:])
    ap = argparse.ArgumentParser()
    ap.add_argument("workload", nargs="?", default="C2")
    ap.add_argument("--max-nobs", type=int, default=100)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only-a", action="store_true")
    ap.add_argument("--library-name", default=None, help="the name this run's library goes by in the record")
    args = ap.parse_args()
    import torch
    from __graft_entry__ import load_package
    pkg = load_package()
    pkg.build()
    ctx = pkg.Context(0, torch.cuda.current_stream().cuda_stream)
    res = dict(workload=args.workload, reps=args.reps, only_a=args.only_a, device=torch.cuda.get_device_name(0),
               library=args.library_name or ("other" if os.environ.get("LETKF_AMD_LIB") else "branch"), cases={})
    res["cases"]["limited"] = one_case(pkg, torch, ctx, args.workload, args.max_nobs, args.reps, args.only_a)
    res["cases"]["unlimited"] = one_case(pkg, torch, ctx, args.workload, 0, args.reps, args.only_a)
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
