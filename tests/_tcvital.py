"""The TC vitals of include/letkf_amd_tcvital.h restated in numpy, and the seeded fixtures its tests share.

The restatement is the header's definition written out: prsadj cell by cell, the 3 x 3 and 5 x 5 sums accumulated term after term
in array order (row by row, the same order at every cell), the disc test rounded term by term, the winner the lowest s, then the
lowest j, then the lowest i; the pick among the ranks and the three obsda rows; the scan for the three rows of a file.  Nothing
here is taken from the library.

Fields are [nmem][NV2DD][nlath][nlonh] doubles (i fastest), interior cell (i, j), 1-based, at array element (i + ihalo, j + jhalo)
counted from 1 -- [j - 1 + jhalo][i - 1 + ihalo] here."""
import numpy as np

NONE, UNDEF, CAP, QC_BAD = 9.99e33, -9.99e33, 1100.0e2, 50
GAMMA, GG, RD = 5.0e-3, 9.81, 287.05
NV2DD, IV_TOPO, IV_PS, IV_T2M, IV_Q2M = 7, 0, 1, 5, 6
ID_TCX, ID_TCY, ID_TCP = 99991, 99992, 99993
EPS = np.finfo(np.float64).eps


def slp(v2d):
    """prsadj of every array cell of one member's fields [NV2DD][nlath][nlonh]; topo = 0 leaves ps as it is"""
    ps, dz = v2d[IV_PS], -1.0 * v2d[IV_TOPO]
    tv = v2d[IV_T2M] * (1.0 + 0.608 * v2d[IV_Q2M])
    with np.errstate(all="ignore"):
        adj = ps * np.power((-GAMMA * dz + tv) / tv, GG / (GAMMA * RD))
    return np.where(dz != 0.0, adj, ps)


def block_sum(a, nlon, nlat, ihalo, jhalo, r):
    """the sum over the (2r + 1)^2 block around every interior cell, term after term in array order"""
    acc = None
    for dj in range(-r, r + 1):
        for di in range(-r, r + 1):
            t = a[jhalo + dj:jhalo + dj + nlat, ihalo + di:ihalo + di + nlon]
            acc = t.copy() if acc is None else acc + t
    return acc


def smoothed(v2d, nlon, nlat, ihalo, jhalo):
    """s [nlat][nlon] of the interior cells"""
    a = slp(v2d)
    c = a[jhalo:jhalo + nlat, ihalo:ihalo + nlon]
    if ihalo >= 2 and jhalo >= 2:
        s3, s5 = block_sum(a, nlon, nlat, ihalo, jhalo, 1), block_sum(a, nlon, nlat, ihalo, jhalo, 2)
        with np.errstate(all="ignore"):
            return (c * 5.0 + (s3 - c) * 3.0 + (s5 - s3)) / 45.0
    return c.copy()


def inside(nlon, nlat, p, ritc, rjtc):
    """the disc test of every interior cell [nlat][nlon]"""
    ig = (np.arange(1, nlon + 1) + p["i_off"]).astype(np.float64)
    jg = (np.arange(1, nlat + 1) + p["j_off"]).astype(np.float64)
    xdis, ydis = np.abs(ig - ritc) * p["dx"], np.abs(jg - rjtc) * p["dy"]
    rdis = np.sqrt((xdis * xdis)[None, :] + (ydis * ydis)[:, None])
    return ~(rdis > p["tc_search_dis"]) & ~np.isnan(ritc) & ~np.isnan(rjtc)


def search_member(v2d, nlon, nlat, ihalo, jhalo, p, ritc, rjtc):
    """(tcx, tcy, mslp) of one member in one subdomain, and the global (ig, jg) of the winner or None"""
    s = smoothed(v2d, nlon, nlat, ihalo, jhalo)
    ok = inside(nlon, nlat, p, ritc, rjtc) & (s < NONE)
    if not ok.any():
        return (NONE, NONE, NONE), None
    low = s[ok].min()
    j, i = np.argwhere(ok & (s == low))[0]                     # row-major: the lowest j, then the lowest i
    ig, jg = int(i) + 1 + p["i_off"], int(j) + 1 + p["j_off"]
    return ((float(ig) - 1.0) * p["dx"] + p["cxg1"], (float(jg) - 1.0) * p["dy"] + p["cyg1"], float(s[j, i])), (ig, jg)


def search(v, nlon, nlat, ihalo, jhalo, p, ritc, rjtc):
    """cand [nmem][3] of the fields v [nmem][NV2DD][nlath][nlonh]"""
    return np.array([search_member(v[m], nlon, nlat, ihalo, jhalo, p, ritc, rjtc)[0] for m in range(v.shape[0])])


def gap(v2d, nlon, nlat, ihalo, jhalo, p, ritc, rjtc):
    """(second lowest s - lowest s) / lowest s among the cells inside the disc"""
    s = smoothed(v2d, nlon, nlat, ihalo, jhalo)
    inn = np.sort(s[inside(nlon, nlat, p, ritc, rjtc) & (s < NONE)])
    return (inn[1] - inn[0]) / inn[0]


def fill(cand_all, rows, qc_replace, qc, ensval, m0):
    """the pick among the ranks and the three obsda rows, in place: cand_all [nproc][nmem][3], ensval [nrow][kld]"""
    nproc, nmem = cand_all.shape[:2]
    none = False
    for m in range(nmem):
        best, pick = CAP, -1
        for n in range(nproc):
            if cand_all[n, m, 2] < best:
                best, pick = cand_all[n, m, 2], n
        none |= pick < 0
        for c in range(3):
            if rows[c] >= 0:
                ensval[rows[c], m0 + m] = cand_all[pick, m, c] if pick >= 0 else UNDEF
    t = QC_BAD if none else 0
    for c in range(3):
        if rows[c] >= 0:
            qc[rows[c]] = t if qc_replace else max(qc[rows[c]], t)


def rows(elm, dif, slot_lb, slot_ub):
    """(the last 1-based rows of TCX, TCY, TCP or 0, valid)"""
    r = [int(np.flatnonzero(elm == e)[-1]) + 1 if (elm == e).any() else 0 for e in (ID_TCX, ID_TCY, ID_TCP)]
    valid = all(r) and dif[r[0] - 1] == dif[r[1] - 1] == dif[r[2] - 1] and slot_lb < dif[r[0] - 1] <= slot_ub
    return np.array(r, dtype=np.int64), bool(valid)


# ---- fixtures
def params(dx=2000.0, dy=2000.0, cxg1=-37000.0, cyg1=-29000.0, i_off=0, j_off=0, tc_search_dis=200.0e3):
    return dict(dx=dx, dy=dy, cxg1=cxg1, cyg1=cyg1, i_off=i_off, j_off=j_off, tc_search_dis=tc_search_dis)


def centres(nlon, nlat, nmem, seed):
    """a centre per member in global grid coordinates, off the lattice, in the middle half of the grid"""
    rng = np.random.default_rng(seed + 1000)
    ci = np.floor(nlon * (0.3 + 0.4 * rng.random(nmem))) + 0.2 + 0.6 * rng.random(nmem)
    cj = np.floor(nlat * (0.3 + 0.4 * rng.random(nmem))) + 0.2 + 0.6 * rng.random(nmem)
    return ci, cj


def low_fixture(nlon, nlat, ihalo, jhalo, nmem, seed, terrain=0.7):
    """A Gaussian low per member over terrain on about `terrain` of the cells, with noise on t2m, q2m and ps:
    v [nmem][NV2DD][nlath][nlonh], and the members' centres (global grid coordinates of the whole array's interior)."""
    rng = np.random.default_rng(seed)
    nlonh, nlath = nlon + 2 * ihalo, nlat + 2 * jhalo
    ci, cj = centres(nlon, nlat, nmem, seed)
    gi = np.arange(1 - ihalo, nlon + ihalo + 1, dtype=np.float64)[None, :]
    gj = np.arange(1 - jhalo, nlat + jhalo + 1, dtype=np.float64)[:, None]
    v = np.zeros((nmem, NV2DD, nlath, nlonh))
    for m in range(nmem):
        r2 = (gi - ci[m]) ** 2 + (gj - cj[m]) ** 2
        target = 1008.0e2 - (25.0e2 + 2.0e2 * m) * np.exp(-r2 / (2.0 * 4.5 ** 2)) + 3.0 * rng.standard_normal((nlath, nlonh))
        topo = np.where(rng.random((nlath, nlonh)) < terrain, 20.0 + 600.0 * rng.random((nlath, nlonh)), 0.0)
        t2m = 295.0 + 1.5 * rng.standard_normal((nlath, nlonh))
        q2m = 0.015 + 0.002 * rng.standard_normal((nlath, nlonh))
        tv = t2m * (1.0 + 0.608 * q2m)
        ps = target / np.power((GAMMA * topo + tv) / tv, GG / (GAMMA * RD)) + 0.5 * rng.standard_normal((nlath, nlonh))
        v[m, IV_TOPO], v[m, IV_PS], v[m, IV_T2M], v[m, IV_Q2M] = topo, ps, t2m, q2m
        for other in (2, 3, 4):
            v[m, other] = rng.standard_normal((nlath, nlonh))           # (variables the search must not read)
    return v, ci, cj


def exact_fixture(nlon, nlat, ihalo, jhalo, nmem, dips, base=101000.0, depth=4500.0):
    """topo = 0 and integer-valued ps: `base` everywhere but `depth` lower at the interior cells `dips` [(i, j), ...] (1-based),
    member m another `45 m` lower there.  S3, S5 and their combinations are exact in any order, so s is correctly rounded whatever
    the order of the sums.  t2m / q2m are NaN: with topo = 0 nothing may read them into the result."""
    nlonh, nlath = nlon + 2 * ihalo, nlat + 2 * jhalo
    v = np.zeros((nmem, NV2DD, nlath, nlonh))
    v[:, IV_PS] = base
    v[:, IV_T2M] = np.nan
    v[:, IV_Q2M] = np.nan
    for m in range(nmem):
        for i, j in dips:
            v[m, IV_PS, j - 1 + jhalo, i - 1 + ihalo] = base - depth - 45.0 * m
    return v


def cut(v, ri, rj, nlon, nlat, ihalo, jhalo):
    """subdomain (ri, rj) of nlon x nlat cells, with its halo, out of the global array v [nmem][NV2DD][NLATH][NLONH]"""
    return np.ascontiguousarray(v[:, :, rj * nlat:rj * nlat + nlat + 2 * jhalo, ri * nlon:ri * nlon + nlon + 2 * ihalo])


FIXTURES = {                       # name: (nlon, nlat, ihalo, jhalo, nmem, seed)
    "main": (37, 29, 2, 2, 3, 11),
    "wide_halo": (37, 29, 3, 2, 3, 12),
    "unsmoothed": (37, 29, 1, 1, 3, 13),
    "seams": (24, 20, 2, 2, 3, 14),
    "sketch": (37, 29, 2, 2, 12, 15),
    "chain": (12, 10, 2, 2, 4, 31),            # tests/test_gpu_tcvital_chain.py; the disc covers the grid wherever the centre is
}
CUT_DISC = dict(dx=1500.0, dy=2500.0, tc_search_dis=30.0e3)
# the searches of tests/test_gpu_tcvital.py that are held to the restatement's location: (fixture, params, the member whose centre)
SEARCHES = [("main", {}, 0), ("main", {}, 1), ("main", {}, 2), ("main", CUT_DISC, 1), ("unsmoothed", CUT_DISC, 1),
            ("wide_halo", CUT_DISC, 1), ("seams", {}, 0)]


def nothing_cases():
    nlon, nlat, ih, jh, nmem, seed = FIXTURES["main"]
    v = low_fixture(nlon, nlat, ih, jh, nmem, seed)[0]
    nan_low = v.copy()
    s = smoothed(v[0], nlon, nlat, ih, jh)
    j, i = np.unravel_index(np.argmin(s), s.shape)
    nan_low[:, IV_PS, j + jh, i + ih] = np.nan                                  # the cell that would be the minimum ...
    nan_all = v.copy()
    nan_all[:, IV_PS] = np.nan
    high = exact_fixture(nlon, nlat, ih, jh, nmem, [(9, 9)], base=111000.0, depth=900.0)      # every s >= 1100 hPa
    return {
        "disc outside": (v, params(tc_search_dis=20.0e3), 80.0, 70.0),
        "dis 0 off a cell": (v, params(tc_search_dis=0.0), 20.5, 12.0),
        "nan ritc": (v, params(), np.nan, 12.0),
        "nan rjtc": (v, params(), 20.0, np.nan),
        "nan cells": (nan_all, params(), 20.0, 12.0),
        "dis 0 on a cell": (v, params(tc_search_dis=0.0), 20.0, 12.0),
        "nan minimum": (nan_low, params(), float(i + 1), float(j + 1)),
        "above the cap": (high, params(), 20.0, 12.0),
    }
