"""obsope_cal's first scan (scale/obs/obsope_tools.f90:140-427) and rij_rank (scale/common/common_scale.f90:1728-1779) stated in
numpy with the reference's operation order, twice: scan() vectorised (what the GPU tests compare with, bit for bit) and
scan_literal() row by row as the Fortran loops read (what test_obsscan_statement.py holds scan() to).  Beside them the case
builder and the raw call of letkf_obsscan_dev with canary-filled outputs.

A case is a dict: off int64 [nfile + 1], ri / rj / dif float64 per file row, layout = (nlon, nlat, ihalo, jhalo, prc_num_x,
prc_num_y), slots = (slot_start, slot_end, slot_base, slot_tinterval), run = flags per file or None."""
import ctypes as C
import math

import numpy as np

IQC_TIME, IQC_OUT_H = 97, 98
CANARY = -777
LAYOUT = (3, 5, 2, 2, 3, 2)          # the main shape: nlon = 3, nlat = 5, halos 2, 3 x 2 subdomains
SLOTS = (1, 3, 2, 600.0)             # slots 1..3 with base 2


# ------------------------------------------------------------------------------------------------------ the statement
def rij_rank(ig, jg, layout):
    """common_scale.f90:1754-1762 on arrays; a NaN coordinate gives -1 (the header's NEW rule)"""
    nlon, nlat, ihalo, jhalo, px, py = layout
    ig, jg = np.asarray(ig, dtype=np.float64), np.asarray(jg, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        out = (ig < float(1 + ihalo)) | (ig > float(nlon * px + ihalo)) | (jg < float(1 + jhalo)) | (jg > float(nlat * py + jhalo))
        out |= np.isnan(ig) | np.isnan(jg)
        gi, gj = np.where(out, float(1 + ihalo), ig), np.where(out, float(1 + jhalo), jg)
        rank_i = np.ceil((gi - float(ihalo) - 0.5) / float(nlon)).astype(np.int64) - 1
        rank_j = np.ceil((gj - float(jhalo) - 0.5) / float(nlat)).astype(np.int64) - 1
    return np.where(out, -1, rank_j * px + rank_i).astype(np.int32)


def slot_of(dif, rank, slots):
    """:251-259: the slot of every row; SLOT_END + 1 outside the window (and for a non-finite dif or |dif / T - 0.5| >= 2^30, the
    header's NEW rule), SLOT_END + 2 outside the domain"""
    s0, s1, base, tint = slots
    with np.errstate(invalid="ignore", over="ignore"):
        x = np.asarray(dif, dtype=np.float64) / tint - 0.5
        ok = np.abs(x) < 2.0 ** 30                                    # (False for a NaN)
        s = np.ceil(np.where(ok, x, 0.0)).astype(np.int64) + base
    s = np.where(ok & (s >= s0) & (s <= s1), s, s1 + 1)
    return np.where(rank < 0, s1 + 2, s).astype(np.int32)


def scan(case, myrank_d=None):
    """dict: rank, slot (and own) per file row; set, idx, qc per list row; bsn (nprocs_d, nslots + 2), bsna (nprocs_d, nslots + 3)"""
    off, layout, slots = case["off"], case["layout"], case["slots"]
    nfile, n = len(off) - 1, int(off[-1])
    s0, s1 = slots[0], slots[1]
    nb, nprocs = s1 - s0 + 3, layout[4] * layout[5]
    rank = rij_rank(case["ri"], case["rj"], layout)
    slot = slot_of(case["dif"], rank, slots)
    file = np.searchsorted(off, np.arange(n), side="right") - 1      # (an empty file owns no row)
    file = np.minimum(file, nfile - 1)
    run = np.ones(nfile, dtype=bool) if case.get("run") is None else np.asarray(case["run"]).astype(bool)
    rows = np.nonzero(run[file])[0] if n else np.zeros(0, dtype=np.int64)
    key = np.maximum(rank[rows], 0).astype(np.int64) * nb + (slot[rows] - s0)
    order = np.argsort(key, kind="stable")                           # the serial scatter of :279-298 keeps file, then row order
    srt = rows[order]
    bucket = key[order] % nb
    counts = np.bincount(key, minlength=nprocs * nb)[:nprocs * nb].reshape(nprocs, nb)
    bsna = np.zeros((nprocs, nb + 1), dtype=np.int64)
    bsna[:, 1:] = np.cumsum(counts.reshape(-1)).reshape(nprocs, nb)
    bsna[1:, 0] = bsna[:-1, -1]
    out = dict(rank=rank, slot=slot, set=(file[srt] + 1).astype(np.int32), idx=(srt - off[file[srt]] + 1).astype(np.int32),
               qc=np.where(bucket < nb - 2, 0, np.where(bucket == nb - 2, IQC_TIME, IQC_OUT_H)).astype(np.int32),
               bsn=counts.astype(np.int32), bsna=bsna.astype(np.int32))
    if myrank_d is not None:
        out["own"] = np.where(rank < 0, -1, (rank == myrank_d).astype(np.int32)).astype(np.int32)
    return out


def scan_literal(case):
    """the loops of :173-298 and :413-427 as they stand, one row at a time, Python floats and math.ceil"""
    off, (nlon, nlat, ihalo, jhalo, px, py), (s0, s1, base, tint) = case["off"], case["layout"], case["slots"]
    nfile = len(off) - 1
    nprocs = px * py
    run = [True] * nfile if case.get("run") is None else [bool(v) for v in case["run"]]
    t_out, d_out = s1 + 1, s1 + 2
    rank, slot = [], []
    for r in range(int(off[-1])):
        ig, jg, dif = float(case["ri"][r]), float(case["rj"][r]), float(case["dif"][r])
        if (math.isnan(ig) or math.isnan(jg) or ig < float(1 + ihalo) or ig > float(nlon * px + ihalo)
                or jg < float(1 + jhalo) or jg > float(nlat * py + jhalo)):
            rank.append(-1)
            slot.append(d_out)
            continue
        rank_i = math.ceil((ig - float(ihalo) - 0.5) / float(nlon)) - 1
        rank_j = math.ceil((jg - float(jhalo) - 0.5) / float(nlat)) - 1
        rank.append(rank_j * px + rank_i)
        x = dif / tint - 0.5 if math.isfinite(dif) else math.nan
        if not abs(x) < 2.0 ** 30:
            slot.append(t_out)
            continue
        islot = math.ceil(x) + base
        slot.append(islot if s0 <= islot <= s1 else t_out)
    bsn = {(s, ip): 0 for ip in range(nprocs) for s in range(s0, s1 + 3)}
    bsna = {(s, ip): 0 for ip in range(nprocs) for s in range(s0 - 1, s1 + 3)}
    for iof in range(nfile):
        if run[iof]:
            for r in range(int(off[iof]), int(off[iof + 1])):
                bsn[(slot[r], max(rank[r], 0))] += 1
    bsnext = {}
    for ip in range(nprocs):
        if ip > 0:
            bsna[(s0 - 1, ip)] = bsna[(s1 + 2, ip - 1)]
        for s in range(s0, s1 + 3):
            bsna[(s, ip)] = bsna[(s - 1, ip)] + bsn[(s, ip)]
            bsnext[(s, ip)] = bsna[(s - 1, ip)]
    nall = sum(int(off[f + 1] - off[f]) for f in range(nfile) if run[f])
    set_, idx, qc = [0] * nall, [0] * nall, [0] * nall
    for iof in range(nfile):
        if run[iof]:
            for r in range(int(off[iof]), int(off[iof + 1])):
                b = (slot[r], max(rank[r], 0))
                bsnext[b] += 1
                set_[bsnext[b] - 1], idx[bsnext[b] - 1] = iof + 1, r - int(off[iof]) + 1
    for ip in range(nprocs):
        for s, flag in ((t_out, IQC_TIME), (d_out, IQC_OUT_H)):
            for nn in range(bsna[(s - 1, ip)], bsna[(s, ip)]):
                qc[nn] = flag
    i32 = lambda a: np.array(a, dtype=np.int32)
    return dict(rank=i32(rank), slot=i32(slot), set=i32(set_), idx=i32(idx), qc=i32(qc),
                bsn=i32([[bsn[(s, ip)] for s in range(s0, s1 + 3)] for ip in range(nprocs)]),
                bsna=i32([[bsna[(s, ip)] for s in range(s0 - 1, s1 + 3)] for ip in range(nprocs)]))


def rows_of(bsna, slot_start, ip, islot):
    """letkf_obsscan_rows: (first, count); islot = 0 is the whole subdomain"""
    lo = 0 if islot == 0 else islot - slot_start
    hi = bsna.shape[1] - 1 if islot == 0 else lo + 1
    return int(bsna[ip, lo]), int(bsna[ip, hi]) - int(bsna[ip, lo])


# ------------------------------------------------------------------------------------------------------ the cases
def around(v):
    v = np.float64(v)
    return [np.nextafter(v, -np.inf), v, np.nextafter(v, np.inf)]


def edge_coordinates(n, halo, prc):
    """both domain edges and every ceiling edge halo + 0.5 + m * n, each with its two neighbours, NaN and +-Inf"""
    vals = around(1 + halo) + around(n * prc + halo)
    for m in range(prc + 1):
        vals += around(halo + 0.5 + m * n)
    return np.array(vals + [np.nan, np.inf, -np.inf, 0.0])


def edge_difs(slots):
    """every (s +- 0.5) * T of the slots proper and the one on either side, with neighbours; NaN, +-Inf and 1e300"""
    s0, s1, base, tint = slots
    vals = []
    for s in range(s0 - 1, s1 + 2):
        for h in (-0.5, 0.5):
            vals += around((s - base + h) * tint)
    return np.array(vals + [np.nan, np.inf, -np.inf, 1e300, -1e300, 0.0, 2.0 ** 30 * tint, -2.0 ** 30 * tint])


def edge_case(file_rows=(0, 7, 300), run=None, layout=LAYOUT, slots=SLOTS, seed=5):
    """The main shape: every edge coordinate on either axis against an interior one on the other, every edge dif on interior
    coordinates, a few edge pairs, then seeded rows over and around the domain -- cut to the files' sizes in shuffled order."""
    nlon, nlat, ihalo, jhalo, px, py = layout
    rng = np.random.default_rng(seed)
    ei, ej, ed = edge_coordinates(nlon, ihalo, px), edge_coordinates(nlat, jhalo, py), edge_difs(slots)
    mid_i, mid_j = ihalo + 0.5 + 0.5 * nlon * px, jhalo + 0.5 + 0.5 * nlat * py
    span = (slots[1] - slots[0] + 3) * slots[3]
    rows = [(x, mid_j + 0.25, 10.0) for x in ei] + [(mid_i - 0.25, y, -10.0) for y in ej]
    rows += [(mid_i + 0.1 * q, mid_j - 0.1 * q, d) for q, d in enumerate(ed)]
    rows += [(x, y, d) for x, y, d in zip(ei, ej[::-1], ed)]
    n = sum(file_rows)
    while len(rows) < n:
        rows.append((rng.uniform(ihalo - 1.0, nlon * px + ihalo + 2.0), rng.uniform(jhalo - 1.0, nlat * py + jhalo + 2.0),
                     rng.uniform(-0.5 * span, 0.5 * span) + (slots[0] + slots[1] - 2 * slots[2]) * 0.5 * slots[3]))
    pick = rng.permutation(len(rows))[:n]
    a = np.array([rows[q] for q in pick], dtype=np.float64).reshape(n, 3)
    return dict(off=np.concatenate([[0], np.cumsum(file_rows)]).astype(np.int64), ri=a[:, 0].copy(), rj=a[:, 1].copy(),
                dif=a[:, 2].copy(), layout=layout, slots=slots, run=run)


def edge_rows_needed(layout=LAYOUT, slots=SLOTS):
    """rows edge_case lists before it starts drawing: a case with fewer rows than this leaves edges out"""
    ei, ej = edge_coordinates(layout[0], layout[2], layout[4]), edge_coordinates(layout[1], layout[3], layout[5])
    return len(ei) + len(ej) + len(edge_difs(slots)) + min(len(ei), len(ej), len(edge_difs(slots)))


def spread_case(n, layout, slots, one_bucket, seed=9, file_rows=None):
    """n seeded rows inside the domain and the window: all in one (subdomain, slot), or over every bucket (the two out ones too)"""
    nlon, nlat, ihalo, jhalo, px, py = layout
    s0, s1, base, tint = slots
    rng = np.random.default_rng(seed)
    if one_bucket:
        ri = ihalo + 1.0 + rng.uniform(0.0, 1.0, n) * min(nlon - 0.5, nlon * px - 1.0)   # the domain starts at 1 + halo
        rj = jhalo + 1.0 + rng.uniform(0.0, 1.0, n) * min(nlat - 0.5, nlat * py - 1.0)
        dif = (s0 - base + rng.uniform(-0.49, 0.49, n)) * tint
    else:
        ri = ihalo + 0.5 + rng.uniform(-0.02, 1.0, n) * nlon * px
        rj = jhalo + 0.5 + rng.uniform(0.0, 1.0, n) * nlat * py
        dif = (s0 - base - 0.5 + rng.uniform(-0.2, s1 - s0 + 1.2, n)) * tint
    off = np.array([0, n] if file_rows is None else np.concatenate([[0], np.cumsum(file_rows)]), dtype=np.int64)
    assert off[-1] == n
    return dict(off=off, ri=ri, rj=rj, dif=dif, layout=layout, slots=slots, run=None)


# ------------------------------------------------------------------------------------------------------ the device call
def list_rows(case):
    off = case["off"]
    run = case.get("run")
    return int(sum(off[f + 1] - off[f] for f in range(len(off) - 1) if run is None or run[f]))


def raw_call(pkg, case, dev, myrank_d=0, canary=CANARY):
    """(params, files, out struct, {name: canary-filled output}, keep) of one letkf_obsscan_dev call; the device outputs are
    torch tensors, bsn / bsna numpy arrays"""
    import torch
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    off = np.ascontiguousarray(case["off"], dtype=np.int64)
    n, nlist = int(off[-1]), list_rows(case)
    d = {name: t(case[name]) for name in ("ri", "rj", "dif")}
    run = None if case.get("run") is None else np.ascontiguousarray(case["run"], dtype=np.int32)
    f = pkg.ObsFileRows()
    f.nfile, f.off = len(off) - 1, off.ctypes.data_as(C.c_void_p)
    f.ri, f.rj = C.c_void_p(d["ri"].data_ptr()), C.c_void_p(d["rj"].data_ptr())
    p = pkg.ObsscanParams()
    p.dif, p.obsda_run = C.c_void_p(d["dif"].data_ptr()), None if run is None else run.ctypes.data
    p.nlon, p.nlat, p.ihalo, p.jhalo, p.prc_num_x, p.prc_num_y = case["layout"]
    p.slot_start, p.slot_end, p.slot_base, p.slot_tinterval = case["slots"]
    p.myrank_d = myrank_d
    nprocs, nb = p.prc_num_x * p.prc_num_y, p.slot_end - p.slot_start + 3
    out = {name: torch.full((max(nlist, 1),), canary, dtype=torch.int32, device=dev) for name in ("set", "idx", "qc")}
    out.update({name: torch.full((max(n, 1),), canary, dtype=torch.int32, device=dev) for name in ("rank", "slot", "own")})
    out["bsn"] = np.full((nprocs, nb), canary, dtype=np.int32)
    out["bsna"] = np.full((nprocs, nb + 1), canary, dtype=np.int32)
    o = pkg.ObsscanOut()
    for name, v in out.items():
        setattr(o, name, v.ctypes.data if isinstance(v, np.ndarray) else C.c_void_p(v.data_ptr()))
    return p, f, o, out, [off, d, run]


def host(out, case):
    """the outputs of raw_call as numpy arrays cut to their lengths"""
    n, nlist = int(case["off"][-1]), list_rows(case)
    cut = {"set": nlist, "idx": nlist, "qc": nlist, "rank": n, "slot": n, "own": n}
    return {name: (v if isinstance(v, np.ndarray) else v.cpu().numpy()[:cut[name]]) for name, v in out.items() if v is not None}


def assert_same_bits(got, want, names=None):
    for name in names or want:
        assert got[name].dtype == np.int32 and want[name].dtype == np.int32, name
        assert got[name].shape == want[name].shape, (name, got[name].shape, want[name].shape)
        bad = np.nonzero(got[name].reshape(-1) != want[name].reshape(-1))[0]
        assert bad.size == 0, (name, bad[:10].tolist(), got[name].reshape(-1)[bad[:10]].tolist(), want[name].reshape(-1)[bad[:10]].tolist())
