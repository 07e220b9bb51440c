#!/usr/bin/env python3
"""The record codec on the device (include/letkf_amd_obsfile.h): decode and encode of 2^24 radar rows (nrec 7), assemble of 2^20
obsda rows x 50 and x 100 members (kld = members) and the encode of the same files, one letkf_obsda_encode_dev call per member.
Per case: ms per call between HIP events (median of --reps calls after two warm-up calls, with min and max), rows per second, the
ledger bytes (image + columns or table, each counted once) over the time against the HBM peak, and the ratio to the first
yardstick.  Not the contract bench (bench.py).

Two yardsticks, in the same run and on the same buffers:
  a device-to-device hipMemcpyAsync of the same number of bytes (image + table): it reads and writes each of them, so it moves
    twice the case's ledger, and `x_copy` is the case's time over the copy's -- 0.5 would be the copy engine's own rate
  the numpy statement of the assemble (frombuffer, the float32 column widened into the strided table, NINT and max for qc) on this
    box's host, one thread, at 2^20 x 50: what a host pays today.  Its table is compared with the device's, bit for bit.

  bench_obsfile.py [--rows 1048576] [--radar-rows 16777216] [--reps 7] [--out FILE]
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
from __graft_entry__ import load_package  # noqa: E402

HBM_PEAK = 8.0e12          # B/s, the specification
D2D = 3                    # hipMemcpyDeviceToDevice


def timed(call, reps):
    ev = []
    for rep in range(reps + 2):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        torch.cuda.synchronize()
        if rep >= 2:
            ev.append(e0.elapsed_time(e1))
    ev.sort()
    return ev


def bits(t):
    return t.to(torch.float32).view(torch.int32)


def radar_image(n, dev, gen):
    """head + n records of 7 floats, made on the device"""
    w = torch.empty((n, 9), dtype=torch.int32, device=dev)
    w[:, 0] = w[:, 8] = 28
    w[:, 1] = bits(torch.full((n,), 4001.0, device=dev))
    for k, (lo, hi) in enumerate(((134.0, 136.0), (34.0, 36.0), (0.0, 15000.0), (-30.0, 60.0), (1.0, 5.0)), start=2):
        w[:, k] = bits(lo + (hi - lo) * torch.rand(n, device=dev, generator=gen))
    w[:, 7] = bits(torch.full((n,), 22.0, device=dev))
    head = torch.tensor([4, 0, 4, 4, 0, 4, 4, 0, 4], dtype=torch.int32, device=dev)
    head[1::3] = bits(torch.tensor([135.523, 34.823, 120.5], device=dev))
    return torch.cat([head, w.reshape(-1)])


def obsda_image(n, set_, idx, dev, gen):
    w = torch.empty((n, 6), dtype=torch.int32, device=dev)
    w[:, 0] = w[:, 5] = 16
    w[:, 1], w[:, 2] = set_, idx
    w[:, 3] = bits(10.0 * torch.randn(n, device=dev, generator=gen))
    w[:, 4] = bits((torch.rand(n, device=dev, generator=gen) < 0.05).to(torch.float32) * 10.0)
    return w.reshape(-1)


def host_assemble(images, nobs, kld):
    """the numpy statement, vectorised: what the host loop of read_obs_da and the partial reduce come to"""
    ens = np.empty((nobs, kld))
    qc = np.zeros(nobs, dtype=np.int32)
    for m, img in enumerate(images):
        rec = np.frombuffer(img, dtype=np.float32).reshape(nobs, 6)
        if m == 0:
            x = rec[:, 1:3].astype(np.float64)
            set_, idx = (np.trunc(x[:, k] + np.copysign(0.5, x[:, k])).astype(np.int32) for k in (0, 1))
        ens[:, m] = rec[:, 3]
        q = rec[:, 4].astype(np.float64)
        np.maximum(qc, np.trunc(q + np.copysign(0.5, q)).astype(np.int32), out=qc)
    return set_, idx, qc, ens


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1 << 20)
    ap.add_argument("--radar-rows", type=int, default=1 << 24)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    pkg = load_package()
    pkg.build()
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    ctx = pkg.Context(0, stream)
    hip = C.CDLL("libamdhip64.so")                  # the process's runtime (torch loaded it)
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    gen = torch.Generator(device=dev)
    gen.manual_seed(20)
    res = dict(rows=args.rows, radar_rows=args.radar_rows, reps=args.reps, library=os.path.basename(pkg.OBSFILE_LIB_PATH),
               device=torch.cuda.get_device_name(0), hbm_peak_tb_s=HBM_PEAK / 1e12, cases={},
               measured="whole calls of the entries between HIP events on the context's stream; the assemble's upload of its image table "
                        "and its one synchronisation are inside",
               not_measured="reading or writing the files, the upload of the images, letkf_obsdep_encode_dev")

    def copy_ms(nbytes):
        src, dst = (torch.empty(nbytes, dtype=torch.uint8, device=dev) for _ in range(2))
        src.zero_()
        ev = timed(lambda: hip.hipMemcpyAsync(dst.data_ptr(), src.data_ptr(), nbytes, D2D, stream), args.reps)
        return ev[len(ev) // 2]

    def record(label, rows, ledger, ev, copy):
        med = ev[len(ev) // 2]
        bps = ledger / (med * 1e-3)
        res["cases"][label] = dict(rows=rows, ms=round(med, 4), min=round(ev[0], 4), max=round(ev[-1], 4), rows_per_s=round(rows / (med * 1e-3)),
                                   ledger_bytes=ledger, ledger_gb_per_s=round(bps / 1e9, 1), pct_of_hbm_peak=round(100.0 * bps / HBM_PEAK, 2),
                                   roof_ms=round(ledger / HBM_PEAK * 1e3, 4), copy_ms=round(copy, 4), x_copy=round(med / copy, 2))

    # ---- radar: decode and encode
    n = args.radar_rows
    img = radar_image(n, dev, gen)
    out = {k: torch.empty(n, dtype=torch.int32 if k in ("elm", "typ") else torch.float64, device=dev) for k in pkg.OBSFILE_COLUMNS}
    ledger = img.numel() * 4 + n * 56
    copy = copy_ms(ledger)
    record("decode_radar", n, ledger, timed(lambda: ctx.obs_decode(img, pkg.OBSFILE_RADAR, nrec=7, meta=False, out=out), args.reps), copy)
    back = torch.empty(img.numel() * 4, dtype=torch.uint8, device=dev)
    meta = (135.523, 34.823, 120.5)
    record("encode_radar", n, ledger, timed(lambda: ctx.obs_encode(out, pkg.OBSFILE_RADAR, nrec=7, meta=meta, out=back), args.reps), copy)
    record("encode_radar_without_undefined", n, ledger,
           timed(lambda: ctx.obs_encode(out, pkg.OBSFILE_RADAR, nrec=7, missing=False, meta=meta, out=back), args.reps), copy)
    torch.cuda.synchronize()
    res["radar_round_trip_is_the_identity"] = bool(torch.equal(back.view(torch.int32), img))
    del img, out, back

    # ---- obsda: assemble and encode
    n = args.rows
    set_ = bits(torch.randint(1, 4, (n,), device=dev, generator=gen))
    idx = bits(torch.randint(1, 1 << 20, (n,), device=dev, generator=gen))
    for nmem in (50, 100):
        images = [obsda_image(n, set_, idx, dev, gen) for _ in range(nmem)]
        o = {k: torch.zeros(n, dtype=torch.int32, device=dev) for k in ("set", "idx", "qc")}
        o["ensval"] = torch.empty((n, nmem), dtype=torch.float64, device=dev)
        ledger = nmem * n * 24 + n * nmem * 8
        copy = copy_ms(ledger)
        record(f"assemble_x{nmem}", n, ledger, timed(lambda: ctx.obsda_assemble(images, n, nmem, out=o), args.reps), copy)
        record(f"assemble_x{nmem}_with_counts", n, ledger, timed(lambda: ctx.obsda_assemble(images, n, nmem, check=True, out=o), args.reps), copy)
        outs = [torch.empty(n * 24, dtype=torch.uint8, device=dev) for _ in range(nmem)]

        def encode_all():
            for m in range(nmem):
                ctx.obsda_encode(o["set"], o["idx"], o["qc"], ensval=o["ensval"], col=m, out=outs[m])
        record(f"encode_x{nmem}", n, ledger, timed(encode_all, args.reps), copy)
        if nmem == 50:
            host = [t.cpu().numpy().tobytes() for t in images]
            t0 = time.perf_counter()
            st = host_assemble(host, n, nmem)
            st_ms = (time.perf_counter() - t0) * 1e3
            torch.cuda.synchronize()
            res["numpy_statement_ms_x50"] = round(st_ms, 1)
            res["statement_over_device_x50"] = round(st_ms / res["cases"]["assemble_x50"]["ms"], 1)
            res["table_equals_statement_x50"] = bool(np.array_equal(o["ensval"].cpu().numpy().view(np.int64), st[3].view(np.int64)) and
                                                     all(np.array_equal(o[k].cpu().numpy(), v) for k, v in zip(("set", "idx", "qc"), st[:3])))
            del host, st
        del images, outs, o
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
