#!/usr/bin/env python3
"""What the Himawari-8 entries cost (include/letkf_amd_h08.h), on C2's grid (240 x 240 x 60, halos 2) with one profile per column
(57 600 profiles, 576 000 obsda rows) and 50 members: ms per call of
  letkf_h08_decode_dev, letkf_h08_select_dev, letkf_h08_profiles_dev (raw and rttov_units) and letkf_h08_rows_dev,
two warm-ups, then repetitions of a window of --inner calls enqueued back to back and closed by a synchronise (a window of the
large calls is a few tenths of a second): median and spread of the window's time per call.  This is CALL time on the host's clock,
not kernel time; at these sizes the difference is the floor below, about 0.02 ms.  Each against two yardsticks: the time the HBM peak of DESIGN.md
section 4 needs for the entry's algorithmic bytes (every input element it must read once, every output element once; the ledger
is computed from the shapes below), and the numpy restatement (tests/_h08.py) on this host -- timed on a sample of the profiles
and scaled, since the restatement is a per-profile loop.  `floor` is the same entry on the smallest input: what a call costs
before it does any work.  A call within twice its floor is reported as launch-bound, not as a share of the peak.  Synthetic data;
the transmittances are the stand-in's, evaluated on the device.  Not the contract bench (bench.py).  No GPU: it fails.

Counters: run it under the profiler's counter collection with --members 10 --reps 1 --inner 1 (DESIGN.md section 23 has the sets
and what they said).

  bench_h08.py [--reps 5] [--inner 50] [--members 50] [--out FILE]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HBM_PEAK = 8.0e12      # bytes / s
NLON = NLAT = 240
NLEV = 60
HALO = 2
SAMPLE = 48            # profiles the numpy restatement is timed on


INNER = 50             # calls of a timed window (--inner)


def timed(fn, reps, torch):
    """[ms per call] of reps windows of INNER calls after two warm-ups, each window closed by a synchronise"""
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        for _ in range(INNER):
            fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3 / INNER)
    return out


def summary(ms):
    s = sorted(ms)
    return dict(ms=s[len(s) // 2], min=s[0], max=s[-1], spread=s[-1] - s[0], runs=[round(v, 4) for v in ms])


def bound(r, floor_ms):
    r["floor_ms"] = floor_ms
    r["hbm_ms"] = r["ledger_bytes"] / HBM_PEAK * 1e3
    if r["ms"] < 2.0 * floor_ms:
        r["bound_by"] = "launch"
    else:
        r["share_of_hbm_peak"] = r["hbm_ms"] / r["ms"]
        r["bound_by"] = "hbm" if r["share_of_hbm_peak"] >= 0.5 else "not hbm: DESIGN.md section 23 has the counters"
    if "numpy_ms" in r:
        r["speedup_over_numpy"] = r["numpy_ms"] / r["ms"]
    return r


def main():
    global INNER
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=INNER)
    ap.add_argument("--members", type=int, default=50)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    INNER = args.inner
    import torch
    import _h08 as H
    from __graft_entry__ import load_package
    assert torch.cuda.is_available(), "bench_h08.py needs a GPU"
    pkg = load_package()
    pkg.build()
    ctx = pkg.Context(0, torch.cuda.current_stream().cuda_stream)
    dev = torch.device("cuda:0")
    nmem, nch = args.members, H.NCH
    g = H.make_grid(NLEV, khalo=HALO, nlon=NLON, nlat=NLAT, ihalo=HALO, jhalo=HALO)
    nk, ni, nj = g["nlevh"], g["nlonh"], g["nlath"]
    nprof = NLON * NLAT
    nrow = nprof * nch
    gen = torch.Generator(device=dev)
    gen.manual_seed(1)

    # ---- the fields, made on the device in the reference's layout: physically ordered columns with a little noise
    v3 = torch.zeros((nmem, H.NV3DD, nj, ni, nk), dtype=torch.float64, device=dev)
    v2 = torch.zeros((nmem, H.NV2DD, nj, ni), dtype=torch.float64, device=dev)
    z = ((torch.arange(nk, device=dev, dtype=torch.float64) - HALO + 0.5) * (15000.0 / NLEV))[None, None, :]
    for m in range(nmem):
        noise = lambda a, shape=(nj, ni, nk): 1.0 + a * (2.0 * torch.rand(shape, generator=gen, dtype=torch.float64, device=dev) - 1.0)
        topo = 300.0 * torch.rand((nj, ni), generator=gen, dtype=torch.float64, device=dev)
        zz = z + topo[:, :, None]
        v3[m, H.V_P] = 1.0e5 * torch.exp(-zz / 8000.0) * noise(1.0e-5)
        v3[m, H.V_T] = (300.0 - 6.5e-3 * zz).clamp(min=200.0) * noise(0.003)
        v3[m, H.V_Q] = 0.012 * torch.exp(-zz / 3000.0) * noise(0.05)
        for v, a in ((H.V_QC, 2.0e-5), (H.V_QI, 1.0e-5), (H.V_QS, 6.0e-6), (H.V_QG, 4.0e-6)):
            v3[m, v] = a * noise(0.9)
        v2[m, H.V2_TOPO] = topo
        v2[m, H.V2_PS] = 1.0e5 * torch.exp(-topo / 8000.0)
        v2[m, H.V2_U10], v2[m, H.V2_V10] = 5.0 * noise(0.2, (nj, ni)), -3.0 * noise(0.2, (nj, ni))
        v2[m, H.V2_Q2M], v2[m, H.V2_SKINT] = 0.01 * noise(0.1, (nj, ni)), 290.0 * noise(0.003, (nj, ni))
        v2[m, H.V2_LSMASK] = (torch.rand((nj, ni), generator=gen, dtype=torch.float64, device=dev) < 0.3).double()
    f = pkg.ObsopeFields()
    for n in ("nlev", "nlon", "nlat", "khalo", "ihalo", "jhalo"):
        setattr(f, n, g[n])
    f.nv3dd, f.nv2dd, f.nmem, f.m0 = H.NV3DD, H.NV2DD, nmem, 0
    f.v3d, f.v2d = C.c_void_p(v3.data_ptr()), C.c_void_p(v2.data_ptr())
    for n, s in H.reference_strides(g).items():
        setattr(f, n, s)

    # ---- one profile per column, off the lattice; the file's image; the obsda rows in file order
    rng = np.random.default_rng(2)
    ii, jj = np.meshgrid(np.arange(NLON), np.arange(NLAT))
    ri = (HALO + 1 + ii.reshape(-1) + rng.uniform(0.05, 0.95, nprof)).astype(np.float64)
    rj = (HALO + 1 + jj.reshape(-1) + rng.uniform(0.05, 0.95, nprof)).astype(np.float64)
    lon, lat = 120.0 + 40.0 * rng.random(nprof), -40.0 + 80.0 * rng.random(nprof)
    cols = H.file_cols(nprof, 3)
    cols["lon"], cols["lat"] = np.repeat(lon, nch), np.repeat(lat, nch)
    image = torch.from_numpy(H.encode(cols, False)).to(dev)
    obserr = np.full(nch, 3.0)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    d_ri, d_rj, d_lon, d_lat = t(ri), t(rj), t(lon), t(lat)
    set_, idx = torch.ones(nrow, dtype=torch.int32, device=dev), torch.arange(1, nrow + 1, dtype=torch.int32, device=dev)
    res = dict(grid=[NLON, NLAT, NLEV], nprof=nprof, nrow=nrow, nmem=nmem, hbm_peak=HBM_PEAK, reps=args.reps, inner=args.inner,
               timing="call time: host clock around a window of `inner` calls closed by a synchronise, per call; not kernel time")

    # ---- decode
    out_cols = ctx.h08_decode(image, obserr)
    r = summary(timed(lambda: ctx.h08_decode(image, obserr, out=out_cols), args.reps, torch))
    r["ledger_bytes"] = nprof * 64 + nrow * (2 * 4 + 6 * 8)
    t0 = time.perf_counter()
    H.decode(image.cpu().numpy(), obserr, False)
    r["numpy_ms"] = (time.perf_counter() - t0) * 1e3
    tiny = image[:64]
    floor = summary(timed(lambda: ctx.h08_decode(tiny, obserr), args.reps, torch))["ms"]
    res["decode"] = bound(r, floor)

    # ---- select
    pl, slot, nsel = ctx.h08_select(set_, idx, 1, nprof)
    assert nsel == nprof
    r = summary(timed(lambda: ctx.h08_select(set_, idx, 1, nprof, prof_list=pl, slot_of_prof=slot), args.reps, torch))
    r["ledger_bytes"] = nrow * 8 + nprof * 8
    sample_rows = SAMPLE * nch
    t0 = time.perf_counter()
    H.select(np.ones(sample_rows, dtype=np.int32), np.arange(1, sample_rows + 1, dtype=np.int32), 0, sample_rows, 1, SAMPLE)
    r["numpy_ms"] = (time.perf_counter() - t0) * 1e3 * nprof / SAMPLE
    r["numpy_scaled_from_profiles"] = SAMPLE
    floor = summary(timed(lambda: ctx.h08_select(set_[:10], idx[:10], 1, 1), args.reps, torch))["ms"]
    res["select"] = bound(r, floor)

    # ---- profiles, raw and in RTTOV's units
    in_bytes = nmem * (7 * nj * ni * NLEV + 7 * nj * ni) * 8 + nprof * (4 + 4 * 8)
    empty = pkg.h08_params(nlev=NLEV, nprof_file=nprof)
    profs = {}
    for name, units in (("profiles_raw", 0), ("profiles_rttov_units", 1)):
        p = H.params(nlev=NLEV, nprof_file=nprof, top_down=1, rttov_units=units)
        ps = pkg.h08_params(**p)
        out = ctx.h08_profiles(ps, f, nprof, pl, d_ri, d_rj, d_lon, d_lat)
        r = summary(timed(lambda: ctx.h08_profiles(ps, f, nprof, pl, d_ri, d_rj, d_lon, d_lat, out=out), args.reps, torch))
        r["ledger_bytes"] = in_bytes + nmem * nprof * (5 * NLEV + 8 + (3 * (NLEV - 1) if units else 0)) * 8 + nprof * 4
        sub = dict(g=g, v3=v3[:2].cpu().numpy(), v2=v2[:2].cpu().numpy())
        t0 = time.perf_counter()
        H.profiles(p, g, sub["v3"], sub["v2"], np.arange(SAMPLE, dtype=np.int32), ri, rj, lon, lat, None)
        r["numpy_ms"] = (time.perf_counter() - t0) * 1e3 * (nprof / SAMPLE) * (nmem / 2)
        r["numpy_scaled_from_profiles"], r["numpy_scaled_from_members"] = SAMPLE, 2
        f.nmem = 1
        floor = summary(timed(lambda: ctx.h08_profiles(ps, f, 1, pl, d_ri, d_rj, d_lon, d_lat, out=out), args.reps, torch))["ms"]
        f.nmem = nmem
        ctx.h08_profiles(ps, f, nprof, pl, d_ri, d_rj, d_lon, d_lat, out=out)          # (the floor call wrote slot 0: the whole again)
        res[name] = bound(r, floor)
        profs[units] = (p, ps, out)
    res["empty_call_ms"] = summary(timed(lambda: ctx.h08_profiles(empty, f, 0, pl, d_ri, d_rj, d_lon, d_lat, out=profs[0][2]), args.reps, torch))["ms"]

    # ---- rows, from the raw profiles (Pa, top down); the stand-in's arrays are made on the device
    p, ps, out = profs[0]
    prs = out["lev3"][:, :, 0]
    pc = (50.0e3 + 4.0e3 * torch.arange(nch, device=dev, dtype=torch.float64))[None, None, :, None]
    trans = torch.empty((nmem, nprof, nch, NLEV), dtype=torch.float64, device=dev)
    for m in range(nmem):
        trans[m] = torch.exp(-(prs[m][:, None, :] / pc[0]) ** 2)
    btclr = 230.0 + 40.0 * trans[..., -1].contiguous()
    btall = btclr - 3.0 * torch.rand(btclr.shape, generator=gen, dtype=torch.float64, device=dev)
    q = dict(p, cldsky_thrs=1.0, finish=1, member=nmem)
    qs = pkg.h08_params(**q)
    qc, ens = torch.zeros(nrow, dtype=torch.int32, device=dev), torch.zeros((nrow, nmem), dtype=torch.float64, device=dev)
    lev, val2 = torch.zeros(nrow, dtype=torch.float64, device=dev), torch.zeros(nrow, dtype=torch.float64, device=dev)
    call = lambda n=nrow: ctx.h08_rows(qs, set_, idx, 1, slot, nprof, out, btall, btclr, trans, d_ri, d_rj, qc, ens, nmem, lev, val2, nrows=n)
    r = summary(timed(call, args.reps, torch))
    r["ledger_bytes"] = (nmem * nprof * (nch * NLEV + NLEV + 2 * nch + 1) + nrow * nmem) * 8 + nrow * (8 + 4 + 16) + nprof * (4 + 4 + 16)
    host = dict(lev3=out["lev3"][:2, :SAMPLE].cpu().numpy(), sfc=out["sfc"][:2, :SAMPLE].cpu().numpy(), pflag=out["pflag"][:SAMPLE].cpu().numpy())
    rt = tuple(a[:2, :SAMPLE].cpu().numpy() for a in (btall, btclr, trans))
    t0 = time.perf_counter()
    H.rows(q, 0, sample_rows, np.ones(sample_rows, dtype=np.int32), np.arange(1, sample_rows + 1, dtype=np.int32), 1,
           np.arange(SAMPLE, dtype=np.int32), SAMPLE, 2, 0, host, *rt, ri, rj, True, np.zeros(sample_rows, dtype=np.int32),
           np.zeros((sample_rows, 2)), np.zeros(sample_rows), np.zeros(sample_rows))
    r["numpy_ms"] = (time.perf_counter() - t0) * 1e3 * (nprof / SAMPLE) * (nmem / 2)
    r["numpy_scaled_from_profiles"], r["numpy_scaled_from_members"] = SAMPLE, 2
    floor = summary(timed(lambda: call(1), args.reps, torch))["ms"]
    res["rows"] = bound(r, floor)
    # the same bits from call to call
    a = ens.clone()
    call()
    torch.cuda.synchronize()
    res["rows_repeat_bitwise"] = bool(torch.equal(a, ens))

    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
