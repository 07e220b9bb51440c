"""The statement of superob (include/letkf_amd_superob.h): scale/obs/superob.f90 and superob_tools.f90::superob_select restated
loop by loop for SCALE's regional grid, in plain Python floats -- no np.sum, whose pairwise order is not the reference's.  There
is no compiled reference to hold the device to (superob_tools uses common_gfs, which is not in the reference's tree), so this
file is the definition; the two places where a restatement can go wrong have a deliberately different second form below
(temporal_by_class, cells_brute).  It also builds the seeded fixtures the CPU and the GPU tests share."""
import math

import numpy as np

LON, LAT, LEV, DAT, ERR, RI, RJ, RK = range(8)
FIELDS = ("lon", "lat", "lev", "dat", "err", "ri", "rj", "rk")
BIG = float(np.float32(1.e20))          # the single-precision literal 1.e20 widened (superob_tools.f90:49, :56, :69)
SURFACE_TYPES = 0x4780                  # report types 8, 9, 10, 11, 15 (superob.f90:289-291)


def slot_priority(nslots, nbslot):
    """superob.f90:164-175, 1-based slots"""
    used = [False] * (nslots + 1)
    out = []
    for _ in range(nslots):
        tdist_min, best = 99999999, None
        for s in range(1, nslots + 1):
            tdist = abs(s - nbslot)
            if not used[s] and tdist < tdist_min:
                best, tdist_min = s, tdist
        out.append(best)
        used[best] = True
    return out


def default_methods(nobtype, nid):
    """superob.f90:120-151 as (g, v, t, h), each (nid, nobtype)"""
    g, v, t, h = (np.zeros((nid, nobtype), dtype=np.int32) for _ in range(4))
    h[:] = 3
    for typ, val in ((1, 2), (5, 2), (6, 2)):
        if typ <= nobtype:
            v[:, typ - 1] = val
            h[:, typ - 1] = 0
    for typ, val in ((5, 1), (6, 1), (8, 1), (9, 2), (10, 2)):
        if typ <= nobtype:
            t[:, typ - 1] = val
    return g, v, t, h


def distance(row, i, j, k):
    dx = row[RI] - float(i)
    dy = row[RJ] - float(j)
    if k == 0:
        return math.sqrt(dx * dx + dy * dy)
    dz = row[RK] - float(k)
    return math.sqrt(dx * dx + dy * dy + dz * dz)


def superob_select(g, i, j, k, method):
    """superob_tools.f90:21-140 over the rows g (lists of the eight FIELDS); returns the rows that replace them"""
    m = len(g)
    if m <= 1:
        return g
    if method <= 0 or method >= 4:
        return g
    if method == 2:
        idx = list(range(m))
        err_min = BIG
        for n in range(m):
            if g[n][ERR] < err_min:
                err_min = g[n][ERR]
    else:
        idx = []
        err_min = BIG
        for n in range(m):
            if g[n][ERR] == err_min:
                idx.append(n)
            elif g[n][ERR] < err_min:
                idx = [n]
                err_min = g[n][ERR]
        if method == 1:
            dist_min, n_min = BIG, None
            for n in idx:
                dist = distance(g[n], i, j, k)
                if dist < dist_min:
                    n_min, dist_min = n, dist
            idx = [] if n_min is None else [n_min]      # (n_use == 0: the reference reads an unset n_min)
    out = list(g[0])
    if len(idx) > 1:
        for f in (RI, RJ, RK, LON, LAT, LEV, DAT):
            acc = 0.0
            for n in idx:
                acc = acc + g[n][f]
            out[f] = acc / float(len(idx))
        out[ERR] = err_min
    elif len(idx) == 1:
        out = list(g[idx[0]])
    return [out]


def method1_margin(g, i, j, k):
    """The smallest relative gap between the distances of two method-1 candidates of g whose coordinates are not identical
    (inf where there is none): the acceptance's one place where rounding could decide."""
    err_min = BIG
    for r in g:
        if r[ERR] < err_min:
            err_min = r[ERR]
    pts = sorted({(distance(r, i, j, k), r[RI], r[RJ], r[RK] if k else 0.0) for r in g if r[ERR] == err_min})
    gap = math.inf
    for a, b in zip(pts, pts[1:]):
        gap = min(gap, (b[0] - a[0]) / b[0] if b[0] > 0 else math.inf)
    return gap


def temporal_literal(cell_slots, prio, method, same):
    """superob.f90:650-716 for one cell: cell_slots[slot] = the cell's rows of that slot in order; returns {row: flag}"""
    flag = {}
    for is_ in range(len(prio)):
        rows = cell_slots.get(prio[is_], [])
        for m in range(len(rows)):
            n1 = rows[m]
            if method == 2 and is_ > 0:
                flag[n1] = 2
                continue
            found = False
            for is2 in range(is_ + 1):
                cand = cell_slots.get(prio[is2], [])
                mm = m if is2 == is_ else len(cand)
                for m2 in range(mm):
                    if same(n1, cand[m2]):
                        flag[n1] = 1
                        found = True
                        break
                if found:
                    break
    return flag


def temporal_by_class(cell_slots, prio, method, same):
    """The second form: a row is flagged 1 when it is not the first of its equivalence class in (priority, row) order."""
    flag = {}
    firsts = []
    for is_, slot in enumerate(prio):
        for n1 in cell_slots.get(slot, []):
            if method == 2 and is_ > 0:
                flag[n1] = 2
            elif any(same(n1, f) for f in firsts):
                flag[n1] = 1
            else:
                firsts.append(n1)
    return flag


def cells_brute(order, typ, uid, slot, ii, jj, kk, dims):
    """The second form of the cell grouping: every cell of a tiny grid visited in the reference's loop order, every row tried."""
    nobtype, nid, nslots, nlevx, nlat, nlon = dims
    out = []
    for t in range(1, nobtype + 1):
        for u in range(1, nid + 1):
            for s in range(1, nslots + 1):
                for k in range(0, nlevx + 1):
                    for j in range(1, nlat + 1):
                        for i in range(1, nlon + 1):
                            rows = [n for n in order if (typ[n], uid[n], slot[n], kk[n], jj[n], ii[n]) == (t, u, s, k, j, i)]
                            if rows:
                                out.append(((t, u, s, k, j, i), rows))
    return out


def cells_sorted(order, typ, uid, slot, ii, jj, kk):
    """`order` is in (typ, uid, slot, k, j, i, row) order: its maximal runs of one cell"""
    out = []
    for n in order:
        key = (typ[n], uid[n], slot[n], kk[n], jj[n], ii[n])
        if out and out[-1][0] == key:
            out[-1][1].append(n)
        else:
            out.append((key, [n]))
    return out


def superob(case, methods, hook=None, temporal=temporal_literal, brute=False):
    """The four stages over case (make_case's dict) with methods = (g, v, t, h), each (nid, nobtype).  hook(g, i, j, k, method)
    sees every group that goes through superob_select.  Returns a dict of numpy arrays named as letkf_superob_out's fields."""
    nlon, nlat, nlevx = case["grid"]
    mg, mv, mt, mh = ([[int(x) for x in row] for row in np.asarray(t)] for t in methods)
    nid, nobtype = len(mg), len(mg[0])
    elem_uid = [int(e) for e in case["elem_uid"]]
    slot_off = [int(s) for s in case["slot_off"]]
    nslots = len(slot_off) - 1
    prio = slot_priority(nslots, case["nbslot"])
    mask = case["surface_typ_mask"]
    elm = [int(x) for x in case["rows"]["elm"]]
    typ = [int(x) for x in case["rows"]["typ"]]
    row = [list(r) for r in zip(*[np.asarray(case["rows"][f], dtype=np.float64).tolist() for f in FIELDS])]
    n_all = len(elm)
    uid = [elem_uid.index(e) + 1 if e in elem_uid else 0 for e in elm]
    valid = [uid[n] > 0 and 1 <= typ[n] <= nobtype for n in range(n_all)]
    slot = [0] * n_all
    ii, jj, kk, qc = [0] * n_all, [0] * n_all, [0] * n_all, [0] * n_all
    counts = [0] * 7
    obsnum = np.zeros((4, nid, nobtype), dtype=np.int64)

    def meth(tab, n):
        return tab[uid[n] - 1][typ[n] - 1] if valid[n] else 0

    def select(g, i, j, k, method):
        if hook is not None and len(g) > 1 and 1 <= method <= 3:
            hook(g, i, j, k, method)
        return superob_select(g, i, j, k, method)

    def flush(recstart, recend):
        method = meth(mv, recstart)
        new = []
        for k in range(0, nlevx + 1):
            g = [row[n] for n in range(recstart, recend + 1) if kk[n] == k and qc[n] == 0]
            if len(g) > 1:
                g = select(g, ii[recstart], jj[recstart], k, method)
            new += [(list(r), k) for r in g]
        for n in range(recstart, recend + 1):
            qc[n] = 9
        for m, (r, k) in enumerate(new):
            row[recstart + m], kk[recstart + m], qc[recstart + m] = r, k, 0
            # i and j stay the position's own (:429-437).  Rows of one lon / lat have one ri / rj wherever phys2ij made them; where
            # they do not and the position lies outside the grid, the reference indexes nobsgrd out of bounds: qc 2 here
            if not (1 <= ii[recstart + m] <= nlon and 1 <= jj[recstart + m] <= nlat):
                qc[recstart + m] = 2
                counts[0] += 1
        counts[3] += recend - recstart + 1 - len(new)

    # ---- stages 1 and 2, slot by slot (:254-529)
    for islot in range(1, nslots + 1):
        lo, hi = slot_off[islot - 1], slot_off[islot]
        cont, recstart = False, lo
        for n in range(lo, hi):
            slot[n] = islot
            ri, rj, rk = row[n][RI], row[n][RJ], row[n][RK]
            if not all(math.isfinite(r) and abs(r) < 2.0 ** 30 for r in (ri, rj, rk)):
                qc[n] = 6
                counts[6] += 1
            else:
                ii[n], jj[n], kk[n] = math.floor(ri + 0.5), math.floor(rj + 0.5), math.floor(rk + 0.5)
                if (1 <= typ[n] <= 32 and (mask >> (typ[n] - 1)) & 1) or elm[n] > 9999:
                    kk[n] = 0
                else:
                    if kk[n] < 1:
                        kk[n] = 1
                    if math.ceil(rk) > nlevx:
                        qc[n] = 3
                        counts[0] += 1
                if qc[n] == 0 and (math.ceil(rj) < 2 or math.ceil(rj) > nlat):
                    qc[n] = 2
                    counts[0] += 1
                if qc[n] == 0 and (math.ceil(ri) < 2 or math.ceil(ri) > nlon):
                    qc[n] = 2
                    counts[0] += 1
                if qc[n] == 0 and valid[n] and meth(mg, n) == 1:
                    qc[n] = 4
                    counts[1] += 1
                if qc[n] == 0 and not valid[n]:
                    qc[n] = 5
                    counts[2] += 1
            if n > lo:
                if (meth(mv, n) > 0 and row[n][LON] == row[recstart][LON] and row[n][LAT] == row[recstart][LAT] and
                        uid[n] == uid[recstart] and typ[n] == typ[recstart]):
                    cont = True
                else:
                    if cont:
                        flush(recstart, n - 1)
                        cont = False
                    recstart = n
        if cont:
            flush(recstart, hi - 1)        # (repair 1: the slot's last row, not one past it)
    qc1 = list(qc)
    for n in range(n_all):
        if valid[n]:
            obsnum[0, uid[n] - 1, typ[n] - 1] += 1
            if qc[n] == 0:
                obsnum[1, uid[n] - 1, typ[n] - 1] += 1

    # ---- stage 3 (:571-761)
    order = sorted((n for n in range(n_all) if qc[n] == 0), key=lambda n: (typ[n], uid[n], slot[n], kk[n], jj[n], ii[n]))
    cells = {}
    for n in order:
        if meth(mt, n) > 0:
            cells.setdefault((typ[n], uid[n], kk[n], jj[n], ii[n]), {}).setdefault(slot[n], []).append(n)

    def same(a, b):
        return row[a][LON] == row[b][LON] and row[a][LAT] == row[b][LAT] and row[a][LEV] == row[b][LEV]

    flag = {}
    for key, cell_slots in cells.items():
        flag.update(temporal(cell_slots, prio, mt[key[1] - 1][key[0] - 1], same))
    counts[4] = len(flag)
    order = [n for n in order if n not in flag]
    for n in order:
        obsnum[2, uid[n] - 1, typ[n] - 1] += 1

    # ---- stage 4 (:770-948)
    if brute:
        groups = cells_brute(order, typ, uid, slot, ii, jj, kk, (nobtype, nid, nslots, nlevx, nlat, nlon))
    else:
        groups = cells_sorted(order, typ, uid, slot, ii, jj, kk)
    final = []                                  # (typ, uid, slot, k, j, i, row values)
    for (t, u, s, k, j, i), rows in groups:
        method = mh[u - 1][t - 1]
        g = [row[n] for n in rows]
        if method > 0:
            g = select(g, i, j, k, method)
        final += [(t, u, s, k, j, i, r) for r in g]
    counts[5] = len(order) - len(final)
    out_rows = [f for s in range(1, nslots + 1) for f in final if f[2] == s]      # the supTT.dat files one after another (:959-1001)
    res = {name: np.array([f[6][x] for f in out_rows], dtype=np.float64) for x, name in enumerate(FIELDS)}
    res["elm"] = np.array([elem_uid[f[1] - 1] for f in out_rows], dtype=np.int32)
    for name, x in (("typ", 0), ("slot", 2), ("k", 3), ("j", 4), ("i", 5)):
        res[name] = np.array([f[x] for f in out_rows], dtype=np.int32)
    for f in out_rows:
        obsnum[3, f[1] - 1, f[0] - 1] += 1
    res["nout"] = np.array([len(out_rows)], dtype=np.int64)
    res["slot_off_out"] = np.array([sum(1 for f in out_rows if f[2] <= s) for s in range(nslots + 1)], dtype=np.int64)
    res["qc1"] = np.array(qc1, dtype=np.int32)
    res["counts"] = np.array(counts, dtype=np.int64)
    res["obsnum"] = obsnum
    return res


def records(res, elem_uid_ids):
    """Per slot, the seven-value single-precision records of :992-998 with the unit conversions of :964-990 (ids: the reference's
    id_*_obs of common_obs_scale.f90:48-72) as float32 arrays (n, 7)."""
    id_u, id_v, id_t, id_tv, id_q, id_rh, id_ps, id_tcmip = elem_uid_ids
    out = []
    off = res["slot_off_out"]
    for s in range(len(off) - 1):
        recs = []
        for n in range(int(off[s]), int(off[s + 1])):
            e = int(res["elm"][n])
            lev, dat, err = float(res["lev"][n]), float(res["dat"][n]), float(res["err"][n])
            if e in (id_u, id_v, id_t, id_tv, id_q):
                lev = lev * 0.01
            elif e in (id_ps, id_tcmip):
                dat, err = dat * 0.01, err * 0.01
            elif e == id_rh:
                lev, dat, err = lev * 0.01, dat * 100.0, err * 100.0
            recs.append([float(e), float(res["lon"][n]), float(res["lat"][n]), lev, dat, err, float(res["typ"][n])])
        out.append(np.array(recs, dtype=np.float64).astype(np.float32).reshape(-1, 7))
    return out


# ---- fixtures

def _case(rows, slot_off, grid, nbslot, elem_uid, nobtype, mask):
    arr = {"elm": np.array([r[0] for r in rows], dtype=np.int32), "typ": np.array([r[1] for r in rows], dtype=np.int32)}
    for x, f in enumerate(FIELDS):
        arr[f] = np.array([r[2][x] for r in rows], dtype=np.float64)
    return {"rows": arr, "slot_off": np.array(slot_off, dtype=np.int64), "grid": grid, "nbslot": nbslot,
            "elem_uid": np.array(elem_uid, dtype=np.int32), "nobtype": nobtype, "surface_typ_mask": mask}


class Pool:
    """A small pool of points: rows that draw the same point have identical coordinates (exact ties, temporal duplicates), two
    different points are generic 2^-20 dyadics (their distances to a cell centre differ by far more than 1e-9 relative)."""

    def __init__(self, rng, grid, nh, nv, edges=True):
        nlon, nlat, nlevx = grid
        q = 2.0 ** -20
        self.h = [(1.0 + q * int(rng.integers(1, (nlon - 1) << 20)), 1.0 + q * int(rng.integers(1, (nlat - 1) << 20))) for _ in range(nh)]
        self.v = [0.5 + q * int(rng.integers(1, (nlevx << 20) - (1 << 19))) for _ in range(nv)]
        if edges:
            self.h += [(1.0, 2.25), (2.75, 1.0), (float(nlon), float(nlat)), (nlon + q, 2.0), (2.0, nlat + q), (2.5, 1.5), (1.5, 2.5),
                       (nlon + 0.75, 2.0), (0.25, 0.25)]
            self.v += [0.25, 0.5, 1.5, float(nlevx), nlevx + 0.25, nlevx + q, 1.0]
        self.errs = (0.5, 1.0, 2.0)
        self.rng = rng

    def row(self, h=None, v=None):
        rng = self.rng
        ri, rj = self.h[int(rng.integers(len(self.h)))] if h is None else h
        rk = self.v[int(rng.integers(len(self.v)))] if v is None else v
        err = self.errs[int(rng.integers(3))]
        if rng.random() < 0.02:                   # errors that superob_select never takes as a minimum
            err = (BIG, 1.0e30, math.nan)[int(rng.integers(3))]
        return [100.0 + 0.125 * ri, 20.0 + 0.0625 * rj, 100000.0 - 1000.0 * rk, float(rng.integers(-8, 9)) * 0.375, err, ri, rj, rk]


BASE_IDS = [2819, 2820, 3073, 14593]            # U, V, T and PS: the last is a surface variable (elm > 9999)
BASE_GRID = (5, 4, 3)


def base_case(seed=1, n=3000, special=True):
    """5 x 4 x 3, 3 slots, nbslot 2, 4 types (type 4 a surface type), 4 elements: singles and records from a small pool, with
    invalid rows, NaN / inf coordinates, every coordinate edge, records that end a slot and the table, one with no row at qc 0,
    one interrupted by an invalid row, an empty slot in front."""
    rng = np.random.default_rng(seed)
    pool = Pool(rng, BASE_GRID, 24, 9)
    rows = []
    slot_off = [0, 0]                            # slot 1 is empty

    def record(length, typ, elm, h=None, v=None):
        h = pool.h[int(rng.integers(len(pool.h)))] if h is None else h
        return [(elm, typ, pool.row(h, v)) for _ in range(length)]

    for part in range(2):
        while len(rows) < (part + 1) * n // 2:
            u = rng.random()
            typ, elm = int(rng.integers(1, 5)), BASE_IDS[int(rng.integers(4))]
            if u < 0.55:
                rows.append((elm, typ, pool.row()))
            elif u < 0.93:
                rows += record(int(rng.integers(2, 9)), typ, elm)
            elif u < 0.96:
                rows.append((elm if rng.random() < 0.5 else 1234, (0, 5, typ)[int(rng.integers(3))], pool.row()))
            else:
                r = pool.row()
                r[RI + int(rng.integers(3))] = (math.nan, math.inf, -math.inf, 2.0 ** 30, -3.0e9)[int(rng.integers(5))]
                rows.append((elm, typ, r))
        if special:
            h = pool.h[0]
            for length in (2, 63, 64, 65, 1001):
                rows += record(length, 1 + length % 3, BASE_IDS[length % 3])
            rows += record(5, 2, 2819, h, nlevx_above(BASE_GRID))                 # every row at qc 3: mm = 0
            rec = record(7, 1, 2820, h)                                           # interrupted by an invalid row
            rows += rec[:3] + [(1234, 1, list(rec[0][2]))] + rec[3:]
            rows += record(4, 3, 3073)                                            # ends its slot (and, the second time, the table)
        slot_off.append(len(rows))
    return _case(rows, slot_off, BASE_GRID, 2, BASE_IDS, 4, 0x8)


def nlevx_above(grid):
    return grid[2] + 0.25


def big_cell_case(m, seed=2):
    """One cell (typ 2, U, slot by row, k 2, j 2, i 3) of m rows drawn from 40 points, and a few rows elsewhere."""
    rng = np.random.default_rng(seed + m)
    pool = Pool(rng, BASE_GRID, 6, 4, edges=False)
    q = 2.0 ** -20
    pts = [(3.0 + q * int(rng.integers(-(1 << 19) + 1, 1 << 19)), 2.0 + q * int(rng.integers(-(1 << 19) + 1, 1 << 19)),
            2.0 + q * int(rng.integers(-(1 << 19) + 1, 1 << 19))) for _ in range(40)]
    rows = []
    for n in range(m):
        p = pts[int(rng.integers(40))]
        rows.append((2819, 2, pool.row((p[0], p[1]), p[2])))
        if n % 97 == 0:
            rows.append((3073, 1, pool.row()))
    cut = len(rows) // 3
    return _case(rows, [0, cut, 2 * cut, len(rows)], BASE_GRID, 2, BASE_IDS, 4, 0x8)


def wide_case(seed=3, n=2000):
    """3000 x 3000 x 100, 7 slots, 24 types, 16 elements: more than 2^32 cells; the rows sit in a few cells of every slot, type
    and element, so that the cell keys differ above bit 32."""
    rng = np.random.default_rng(seed)
    grid = (3000, 3000, 100)
    ids = [2819 + u for u in range(16)]
    pool = Pool(rng, grid, 12, 6, edges=False)
    per = n // 7
    rows = [(ids[int(rng.integers(16))], int(rng.integers(1, 25)), pool.row()) for _ in range(7 * per)]
    return _case(rows, [s * per for s in range(8)], grid, 4, ids, 24, SURFACE_TYPES)


def dense_case(seed=4, n=200000):
    """n rows on 24 x 24 x 10, 3 slots, generic coordinates from a pool of 20 000 points"""
    rng = np.random.default_rng(seed)
    grid = (24, 24, 10)
    q = 2.0 ** -20
    ri = 1.0 + q * rng.integers(1, 23 << 20, size=20000)
    rj = 1.0 + q * rng.integers(1, 23 << 20, size=20000)
    rk = 0.5 + q * rng.integers(1, (10 << 20) - (1 << 19), size=20000)
    pick = rng.integers(20000, size=n)
    arr = {"elm": np.array(BASE_IDS, dtype=np.int32)[rng.integers(4, size=n)], "typ": rng.integers(1, 5, size=n).astype(np.int32),
           "ri": ri[pick], "rj": rj[pick], "rk": rk[pick]}
    arr["lon"], arr["lat"], arr["lev"] = 100.0 + 0.125 * arr["ri"], 20.0 + 0.0625 * arr["rj"], 100000.0 - 1000.0 * arr["rk"]
    arr["dat"] = rng.integers(-8, 9, size=n) * 0.375
    arr["err"] = np.array([0.5, 1.0, 2.0])[rng.integers(3, size=n)]
    return {"rows": arr, "slot_off": np.array([0, n // 3, n // 3 * 2, n], dtype=np.int64), "grid": grid, "nbslot": 2,
            "elem_uid": np.array(BASE_IDS, dtype=np.int32), "nobtype": 4, "surface_typ_mask": 0x8}


def uniform_methods(nid, nobtype, g=0, v=0, t=0, h=0):
    return tuple(np.full((nid, nobtype), x, dtype=np.int32) for x in (g, v, t, h))


# ---- the device side of a comparison (tests marked gpu)

ROW_FIELDS = ("elm", "typ", "slot") + FIELDS + ("i", "j", "k")


def device_rows(case, dev):
    import torch
    return {name: torch.from_numpy(np.ascontiguousarray(a)).to(dev) for name, a in case["rows"].items()}


def run_device(ctx, case, methods, dev, obsnum=True, rows=None):
    """Context.superob over the case; the output rows cut at nout, everything as numpy"""
    import torch
    out = ctx.superob(device_rows(case, dev) if rows is None else rows, case["slot_off"], case["grid"], case["nbslot"],
                      case["elem_uid"], methods, surface_typ_mask=case["surface_typ_mask"], obsnum=obsnum)
    torch.cuda.synchronize()
    got = {name: t.cpu().numpy() for name, t in out.items() if t is not None}
    nout = int(got["nout"][0])
    assert 0 <= nout <= len(case["rows"]["elm"])
    for name in ROW_FIELDS:
        got[name] = got[name][:nout]
    return got


def assert_same_bits(got, want, names=None):
    """bit for bit, integers and doubles alike (a NaN err is its own bits)"""
    for name in names or want:
        x, y = np.ascontiguousarray(got[name]), np.ascontiguousarray(want[name])
        assert x.dtype == y.dtype and x.shape == y.shape, (name, x.dtype, y.dtype, x.shape, y.shape)
        if x.tobytes() != y.tobytes():
            bad = np.flatnonzero(x.reshape(-1).view(np.int64 if x.itemsize == 8 else np.int32) !=
                                 y.reshape(-1).view(np.int64 if y.itemsize == 8 else np.int32))
            raise AssertionError(f"{name}: {len(bad)} of {x.size} differ, first at {bad[0]}: {x.reshape(-1)[bad[0]]!r} != {y.reshape(-1)[bad[0]]!r}")


def raw_call(pkg, case, methods, rows, fill=-777):
    """(params, out struct, the output tensors pre-filled with `fill`, what must stay alive) for a call through ctypes"""
    import ctypes as C
    import torch
    dev = rows["elm"].device
    n = rows["elm"].numel()
    keep = [np.ascontiguousarray(case["slot_off"], dtype=np.int64), np.ascontiguousarray(case["elem_uid"], dtype=np.int32)]
    keep += [np.ascontiguousarray(t, dtype=np.int32) for t in methods]
    nid, nobtype = keep[2].shape
    p = pkg.SuperobParams()
    p.nobs = n
    for name in ("elm", "typ") + FIELDS:
        setattr(p, name, rows[name].data_ptr())
    p.slot_off = keep[0].ctypes.data
    p.nlon, p.nlat, p.nlevx = case["grid"]
    p.nslots, p.nbslot, p.nobtype, p.nid, p.surface_typ_mask = len(keep[0]) - 1, case["nbslot"], nobtype, nid, case["surface_typ_mask"]
    p.elem_uid = keep[1].ctypes.data
    p.method_g, p.method_v, p.method_t, p.method_h = (t.ctypes.data for t in keep[2:])
    out = {name: torch.full((n,), fill, dtype=torch.float64 if name in FIELDS else torch.int32, device=dev)
           for name in ROW_FIELDS + ("qc1",)}
    out["nout"] = torch.full((1,), fill, dtype=torch.int64, device=dev)
    out["slot_off_out"] = torch.full((len(keep[0]),), fill, dtype=torch.int64, device=dev)
    out["counts"] = torch.full((7,), fill, dtype=torch.int64, device=dev)
    out["obsnum"] = torch.full((4, nid, nobtype), fill, dtype=torch.int64, device=dev)
    o = pkg.SuperobOut()
    for name, _ in pkg.SuperobOut._fields_:
        setattr(o, name, out[name].data_ptr())
    return p, o, out, keep
