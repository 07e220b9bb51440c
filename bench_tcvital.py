#!/usr/bin/env python3
"""What the TC vitals cost (include/letkf_amd_tcvital.h), on C2's horizontal grid (240 x 240, halos 2) with TC_SEARCH_DIS = 200 km
at dx = 2 km: ms per call of
  letkf_tcvital_search_dev at nmem = 50 and 1000,
  letkf_tcvital_fill_dev   at nproc = 1 and 16 (nmem = 1000),
  letkf_tcvital_rows_dev   at 2^24 rows,
two warm-ups, then synchronised repetitions: median and spread.  Each against two yardsticks: the time the HBM peak of DESIGN.md
section 4 needs for the bytes the entry must read (four fields over the window plus its rim for the search; 12 bytes per row for the
rows, of which the scan itself reads the 4 of elm), and the numpy restatement (tests/_tcvital.py) on this host.  `floor` is the same
entry on the smallest input (one tile outside the disc; two rows): what a call costs before it does any work.  A call within twice
its floor is reported as launch-bound, not as a share of the peak.  Synthetic data; not the contract bench (bench.py).  No GPU: it
fails.

  bench_tcvital.py [--reps 5] [--out FILE]"""
import argparse
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
HALO = 2
DX = 2000.0
DIS = 200.0e3
BASE_MEMBERS = 10      # distinct members made on the host; the device array repeats them


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
    return dict(ms=s[len(s) // 2], min=s[0], max=s[-1], spread=s[-1] - s[0], runs=[round(v, 4) for v in ms])


def bound(r, floor_ms):
    r["floor_ms"] = floor_ms
    r["hbm_ms"] = r["ledger_bytes"] / HBM_PEAK * 1e3
    if r["ms"] < 2.0 * floor_ms:
        r["bound_by"] = "launch"
    else:
        r["share_of_hbm_peak"] = r["hbm_ms"] / r["ms"]
        r["bound_by"] = "hbm" if r["share_of_hbm_peak"] >= 0.5 else "compute"
    r["speedup_over_numpy"] = r["numpy_ms"] / r["ms"]
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import ctypes as C
    import torch
    import _tcvital as T
    from __graft_entry__ import load_package
    assert torch.cuda.is_available(), "bench_tcvital.py needs a GPU"
    pkg = load_package()
    pkg.build()
    ctx = pkg.Context(0, torch.cuda.current_stream().cuda_stream)
    dev = torch.device("cuda:0")
    nlonh = nlath = NLON + 2 * HALO
    v, ci, cj = T.low_fixture(NLON, NLAT, HALO, HALO, BASE_MEMBERS, 2)
    p = T.params(dx=DX, dy=DX, cxg1=0.0, cyg1=0.0, tc_search_dis=DIS)
    ritc, rjtc = float(ci[0]), float(cj[0])
    centre = torch.tensor([ritc, rjtc], dtype=torch.float64, device=dev)
    far = torch.tensor([1.0e6, 1.0e6], dtype=torch.float64, device=dev)
    ps = pkg.TcvitalParams()
    for k, val in p.items():
        setattr(ps, k, val)

    def fields(t, nlon, nlat, nmem):
        f = pkg.ObsopeFields()
        f.nlev, f.khalo, f.nlon, f.nlat, f.ihalo, f.jhalo = 1, 0, nlon, nlat, HALO, HALO
        f.nv3dd, f.nv2dd, f.nmem, f.m0 = 13, T.NV2DD, nmem, 0
        f.v3d, f.v2d = None, C.c_void_p(t.data_ptr())
        f.s3k = f.s3i = f.s3j = f.s3v = f.s3m = 1
        f.s2i, f.s2j, f.s2v, f.s2m = 1, nlon + 2 * HALO, (nlon + 2 * HALO) * (nlat + 2 * HALO), T.NV2DD * (nlon + 2 * HALO) * (nlat + 2 * HALO)
        return f

    res = dict(device=torch.cuda.get_device_name(0), reps=args.reps, grid=[NLON, NLAT], halo=HALO, dx=DX, tc_search_dis=DIS,
               hbm_peak=HBM_PEAK, host_cpus=os.cpu_count(), cases={})
    # the window the disc cuts out of the grid, plus the stencil's rim: what the search must read of each of the four fields
    inn = T.inside(NLON, NLAT, p, ritc, rjtc)
    wi, wj = int(inn.any(axis=0).sum()) + 2 * HALO, int(inn.any(axis=1).sum()) + 2 * HALO
    res["window_cells_with_rim"] = [wi, wj]

    # ---- the floor of a search: one member, one tile, the disc elsewhere
    small = torch.from_numpy(T.low_fixture(8, 8, HALO, HALO, 1, 1)[0]).to(dev)
    cand1 = torch.empty((1, 3), dtype=torch.float64, device=dev)
    fsmall = fields(small, 8, 8, 1)
    floor_search = summary(timed(lambda: ctx.tcvital_search(ps, fsmall, far[0:1], far[1:2], cand=cand1), args.reps, torch))["ms"]

    # the restatement per member, on the members the host made
    t0 = time.perf_counter()
    want = T.search(v[:4], NLON, NLAT, HALO, HALO, p, ritc, rjtc)
    numpy_member_ms = (time.perf_counter() - t0) * 1e3 / 4
    base = torch.from_numpy(v).to(dev)
    for nmem in (50, 1000):
        t = base.repeat((nmem + BASE_MEMBERS - 1) // BASE_MEMBERS, 1, 1, 1)[:nmem].contiguous()
        cand = torch.empty((nmem, 3), dtype=torch.float64, device=dev)
        f = fields(t, NLON, NLAT, nmem)
        r = summary(timed(lambda: ctx.tcvital_search(ps, f, centre[0:1], centre[1:2], cand=cand), args.reps, torch))
        got = cand[:4].cpu().numpy()
        r["same_location_as_numpy"] = bool(np.array_equal(got[:, :2], want[:, :2]))
        r["mslp_eps_from_numpy"] = float(np.max(np.abs(got[:, 2] - want[:, 2]) / (T.EPS * want[:, 2])))
        r["ledger_bytes"] = 4 * 8 * wi * wj * nmem
        r["numpy_ms"], r["numpy_members_timed"] = numpy_member_ms * nmem, 4
        res["cases"][f"search_nmem{nmem}"] = bound(r, floor_search)

    # ---- fill at nmem = 1000
    nmem, kld = 1000, 1000
    rng = np.random.default_rng(5)
    qc = torch.full((3,), 90, dtype=torch.int32, device=dev)
    ens = torch.zeros((3, kld), dtype=torch.float64, device=dev)
    one = torch.tensor([[[1.0, 2.0, 990.0e2]]], dtype=torch.float64, device=dev)
    floor_fill = summary(timed(lambda: ctx.tcvital_fill(one, [0, 1, 2], qc, ens, kld), args.reps, torch))["ms"]
    for nproc in (1, 16):
        ca = np.full((nproc, nmem, 3), T.NONE)
        owner = rng.integers(0, nproc, nmem)
        ca[owner, np.arange(nmem)] = np.stack([rng.uniform(0, 4.8e5, nmem), rng.uniform(0, 4.8e5, nmem), rng.uniform(950e2, 1000e2, nmem)], axis=1)
        cd = torch.from_numpy(ca).to(dev)
        r = summary(timed(lambda: ctx.tcvital_fill(cd, [0, 1, 2], qc, ens, kld), args.reps, torch))
        hq, he = np.full(3, 90, dtype=np.int32), np.zeros((3, kld))
        t0 = time.perf_counter()
        T.fill(ca, [0, 1, 2], True, hq, he, 0)
        r["numpy_ms"] = (time.perf_counter() - t0) * 1e3
        r["same_bits_as_numpy"] = bool(np.array_equal(ens.cpu().numpy().view(np.int64), he.view(np.int64)) and np.array_equal(qc.cpu().numpy(), hq))
        r["ledger_bytes"] = 8 * nproc * nmem + 2 * 8 * nmem + 3 * 8 * nmem      # every mslp, the pick's x / y, the three rows written
        res["cases"][f"fill_nproc{nproc}"] = bound(r, floor_fill)

    # ---- rows at 2^24
    two = (torch.tensor([T.ID_TCX, T.ID_TCY], dtype=torch.int32, device=dev), torch.zeros(2, dtype=torch.float64, device=dev))
    floor_rows = summary(timed(lambda: ctx.tcvital_rows(two[0], two[1], -1.0, 1.0), args.reps, torch))["ms"]
    n = 1 << 24
    elm = rng.choice(np.array([2819, 2820, 3073, 3330, 14593], dtype=np.int32), n)
    dif = np.zeros(n)
    for row, e in ((n // 3, T.ID_TCX), (n // 3 + 1, T.ID_TCY), (n // 3 + 2, T.ID_TCP)):
        elm[row] = e
    elm_d, dif_d = torch.from_numpy(elm).to(dev), torch.from_numpy(dif).to(dev)
    r = summary(timed(lambda: ctx.tcvital_rows(elm_d, dif_d, -1.0, 1.0), args.reps, torch))
    t0 = time.perf_counter()
    want_rows = T.rows(elm, dif, -1.0, 1.0)
    r["numpy_ms"] = (time.perf_counter() - t0) * 1e3
    got_rows = ctx.tcvital_rows(elm_d, dif_d, -1.0, 1.0)
    r["same_as_numpy"] = bool(got_rows[0].tolist() == want_rows[0].tolist() and got_rows[1] == want_rows[1])
    r["ledger_bytes"], r["bytes_the_scan_reads"] = 12 * n, 4 * n
    res["cases"]["rows_2p24"] = bound(r, floor_rows)

    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
