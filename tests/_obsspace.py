"""Cases for the producer of the observation table (include/letkf_amd.h sections 5 and 9) across its argument space, shared by
tests/test_gpu_obs_argspace.py (the device against the oracle) and tests/test_obsspace_helpers.py (what this file states in numpy
against the oracle, without a GPU).

The reference answer of every GPU comparison is the oracle (oracle/letkf_oracle.c through ctypes, tests/native/setobs_oracle.c for
the pre-processing and the count tables).  What this file states itself is only: which QC flag each hand-built threshold row must
get, which mesh cell each hand-built coordinate falls in, and which of the departure's three routes a kld takes."""
import ctypes as C

import numpy as np

import _oracle
from _gridspace import CANARY, ICANARY, bits, canary_buffer, same_bits  # noqa: F401  (re-exported)
from _obsprep import HaloLayout, Mesh, QcParams, fill, qc_params

UNDEF = -9.99e33
E_INVALID = -1
ID_U, ID_RAIN, ID_REF, ID_REF0, ID_VR, ID_PRH, ID_H08, ID_TCX, ID_TCY, ID_TCP = (2819, 19999, 4001, 4004, 4002, 4003, 8800,
                                                                                99991, 99992, 99993)
QC_GROSS, QC_REFMEM, QC_BAD, QC_OTYPE = 5, 12, 50, 90

# ---------------------------------------------------------------------------------------------------- the departure's routes
LDS_BYTES = 160 * 1024        # LDS of a gfx950 workgroup; the library accepts no other device


def departure_route(kld, lds=LDS_BYTES):
    """64 rows of kld | 1 doubles in LDS (the kernel every kld <= 319 has always taken), else 16 rows, else no LDS at all"""
    row = (kld | 1) * 8
    return "tile64" if 64 * row <= lds else "tile16" if 16 * row <= lds else "global"


def route_thresholds(lds=LDS_BYTES):
    """[(last kld of a route, first kld of the next)] -- (319, 320) and (1279, 1280) at 160 KiB"""
    out = []
    for rows in (64, 16):
        m = lds // (rows * 8)                          # the largest kld | 1 that fits, were it odd
        last = m if m % 2 else m - 1
        out.append((last, last + 1))
    return out


# (MEMBER, DET_RUN, kld, nobs): the ensemble sizes of BASELINE's table, a padded table on the old and on a new route, and
# either side of each threshold with 70 rows
KLD_CASES = [(319, False, 319, 130), (319, True, 320, 130), (320, False, 320, 130), (320, False, 323, 130),
             (1000, True, 1001, 130), (3, True, 7, 130)] + [(kld, False, kld, 70) for pair in route_thresholds() for kld in pair]


def kld_rows(k, kld, nobs):
    return dep_rows(1000 + kld, k, kld, nobs)


# ------------------------------------------------------------------------------------------------------------ departure rows
GROSS = dict(gross_error=5.0, gross_error_rain=4.0, gross_error_radar_ref=3.0, gross_error_radar_vr=2.5, gross_error_radar_prh=1.5,
             gross_error_tcx=6.0, gross_error_tcy=7.0, gross_error_tcp=4.5)
H08 = dict(h08_min_cld_member=2, h08_limit_lev=20000.0, gross_error_h08=3.5, h08_bt_min=180.0)


def params(cls, k, det_run, h08=0, **over):
    """letkf_qc_params with eight DIFFERENT dyadic gross-error factors, so that a row judged with the wrong one shows"""
    d = dict(GROSS, radar_ref_thres_dbz=15.0, min_radar_ref_member=3, min_radar_ref_member_obsref=2, h08=int(h08), **H08)
    d.update(over)
    return qc_params(cls, k, det_run, **d)


def dep_rows(seed, k, kld, nobs, nan_pad=True):
    """Rows of every element the departure distinguishes, every entry state of qc (0, < 0: processed; > 0: skipped), undefined
    observations, reflectivity rows where few members see rain, cloudy (negative) Himawari-8 members, gross errors; the columns
    >= k + 1 of a padded table hold canaries."""
    rng = np.random.default_rng(seed)
    elm = rng.choice(np.array([ID_U, ID_U, ID_RAIN, ID_REF, ID_REF, ID_REF0, ID_VR, ID_PRH, ID_H08, ID_H08, ID_TCX, ID_TCY, ID_TCP],
                              np.int32), nobs)
    sure = nobs >= 8                                   # rows 0, 1: a reflectivity no member sees and an undefined one, whatever the seed
    if sure:
        elm[:2] = ID_REF
    ref, h08 = np.isin(elm, (ID_REF, ID_REF0)), elm == ID_H08
    dat = np.where(ref, rng.uniform(5.0, 40.0, nobs), np.where(h08, 250.0 + 25.0 * rng.standard_normal(nobs),
                                                               rng.normal(0.0, 4.0, nobs)))
    dat[rng.random(nobs) < 0.06] = UNDEF
    dat[h08 & (rng.random(nobs) < 0.1)] = 150.0
    err = rng.choice([0.5, 1.0, 2.0], nobs)
    ens = np.where(dat[:, None] == UNDEF, 0.0, dat[:, None]) + rng.normal(0.0, 2.0, (nobs, kld))
    ens[rng.random(nobs) < 0.15] += 9.0
    low = ref & (rng.random(nobs) < 0.3)
    if sure:
        low[0], dat[0], dat[1] = True, 20.0, UNDEF
    ens[low] = rng.uniform(0.0, 14.9, (int(low.sum()), kld))
    few = ref & ~low & (rng.random(nobs) < 0.3)                      # two or three members above the threshold
    ens[few] = 10.0
    ens[few, :3] = 20.0
    ens[few & (rng.random(nobs) < 0.5), 2] = 10.0
    cloudy = h08[:, None] & (rng.random((nobs, kld)) < rng.choice([0.0, 1.5 / k, 0.4], size=(nobs, 1)))
    ens = np.where(cloudy, -np.abs(ens), ens)
    if nan_pad and kld > k + 1:
        ens[:, k + 1:] = canary_buffer(1)[0]
    qc = rng.choice(np.array([0, 0, 0, 0, 0, 0, -1, 10, 21], np.int32), nobs)
    if sure:
        qc[:2] = 0
    lev = np.where(h08, rng.choice([5000.0, 20000.0, 60000.0], nobs), 50000.0)
    val2 = np.where(h08, 255.0 + 10.0 * rng.standard_normal(nobs), rng.standard_normal(nobs))
    return dict(elm=elm, dat=dat, err=err, ens=np.ascontiguousarray(ens), qc=qc, lev=lev, val2=val2, kld=kld)


def rows_of(lst, k, kld):
    """list of dict(elm, dat, err, mem (k values or a scalar), det, qc, lev, val2, want) -> the arrays of dep_rows + `want`"""
    n = len(lst)
    ens = canary_buffer(n * kld).reshape(n, kld).copy()
    for i, r in enumerate(lst):
        ens[i, :k] = r["mem"]
        if kld > k:
            ens[i, k] = r.get("det", 0.0)
    g = lambda key, dflt, dt: np.array([r.get(key, dflt) for r in lst], dt)  # noqa: E731
    return dict(elm=g("elm", ID_U, np.int32), dat=g("dat", 0.0, np.float64), err=g("err", 2.0, np.float64), ens=ens,
                qc=g("qc", 0, np.int32), lev=g("lev", 50000.0, np.float64), val2=g("val2", 0.0, np.float64), kld=kld,
                want=g("want", 0, np.int32), name=[r["name"] for r in lst])


UP, DN = (lambda x: float(np.nextafter(x, np.inf))), (lambda x: float(np.nextafter(x, -np.inf)))
TK = 4                                             # members of the threshold rows
GE_OF = {ID_U: "gross_error", ID_RAIN: "gross_error_rain", ID_REF: "gross_error_radar_ref", ID_VR: "gross_error_radar_vr",
         ID_PRH: "gross_error_radar_prh", ID_TCX: "gross_error_tcx", ID_TCY: "gross_error_tcy", ID_TCP: "gross_error_tcp"}


def threshold_rows(h08):
    """Rows that sit exactly on a threshold of letkf_obs.f90:361-561 and one ulp either side, from dyadic values so that `exactly`
    is exact: members all 32 (mean 32 without rounding), err 2, y = 32 + GE * 2, so |y - mean| == GE * err.  `want`: the flag the
    reference's comparisons (all strict: >, <) give.  h08: the -DH08 rows as well."""
    rows = []
    add = lambda name, want, **kw: rows.append(dict(dict(mem=32.0, err=2.0), name=name, want=want, **kw))  # noqa: E731
    for elm, ge in GE_OF.items():                   # 32 > thres + 1e-6: a reflectivity row has all its members in rain
        y = 32.0 + GROSS[ge] * 2.0
        add(f"{ge} at", 0, elm=elm, dat=y)
        add(f"{ge} above", QC_GROSS, elm=elm, dat=UP(y))
        add(f"{ge} below", 0, elm=elm, dat=DN(y))
        add(f"{ge} at, below the mean", 0, elm=elm, dat=32.0 - GROSS[ge] * 2.0)
        add(f"{ge} above, below the mean", QC_GROSS, elm=elm, dat=DN(32.0 - GROSS[ge] * 2.0))
    x = 15.0 + 1.0e-6                               # RADAR_REF_THRES_DBZ + 1e-6 as the code forms it
    big = dict(err=1024.0)                          # no gross error on the member-count rows
    add("mem_ref == need", 0, elm=ID_REF, dat=8.0, mem=[32, 32, 32, 0], **big)
    add("mem_ref == need - 1", QC_REFMEM, elm=ID_REF, dat=8.0, mem=[32, 32, 0, 0], **big)
    add("mem_ref == need_obsref", 0, elm=ID_REF, dat=32.0, mem=[32, 32, 0, 0], **big)
    add("mem_ref == need_obsref - 1", QC_REFMEM, elm=ID_REF, dat=32.0, mem=[32, 0, 0, 0], **big)
    add("member at thres + 1e-6 is not in rain", QC_REFMEM, elm=ID_REF0, dat=8.0, mem=[32, 32, x, 0], **big)
    add("member above thres + 1e-6 is", 0, elm=ID_REF0, dat=8.0, mem=[32, 32, UP(x), 0], **big)
    add("dat at thres + 1e-6 needs min_radar_ref_member", QC_REFMEM, elm=ID_REF, dat=x, mem=[32, 32, 0, 0], **big)
    add("dat above thres + 1e-6 needs _obsref", 0, elm=ID_REF, dat=UP(x), mem=[32, 32, 0, 0], **big)
    add("reflectivity undef", QC_BAD, elm=ID_REF, dat=UNDEF)
    add("reflectivity one ulp off undef", QC_GROSS, elm=ID_REF, dat=UP(UNDEF))
    add("ordinary undef is an ordinary number", QC_GROSS, elm=ID_U, dat=UNDEF)
    add("qc < 0 is processed", -1, elm=ID_U, dat=33.0, qc=-1)
    add("qc < 0 is processed and flagged", QC_GROSS, elm=ID_U, dat=64.0, qc=-7)
    add("qc > 0 is skipped", 21, elm=ID_U, dat=64.0, qc=21)
    if h08:
        clear, cloudy = [32, 32, 32, -32], [32, 32, -32, -32]         # mem_cld 1 < H08_MIN_CLD_MEMBER = 2 <= mem_cld 2
        for sky, mem, ge in (("clear", clear, 1.0), ("cloudy", cloudy, H08["gross_error_h08"])):
            y = 232.0 + ge * 2.0
            m8 = [v / 32 * 232.0 for v in mem]
            add(f"h08 {sky} at", 0, elm=ID_H08, dat=y, mem=m8, val2=240.0)
            add(f"h08 {sky} above", QC_GROSS, elm=ID_H08, dat=UP(y), mem=m8, val2=240.0)
            add(f"h08 {sky} below", 0, elm=ID_H08, dat=DN(y), mem=m8, val2=240.0)
        add("mem_cld == min: cloudy bound", 0, elm=ID_H08, dat=236.0, mem=[232, 232, -232, -232])       # |dep| 4: 2 < 4 < 7
        add("mem_cld == min - 1: clear bound", QC_GROSS, elm=ID_H08, dat=236.0, mem=[232, 232, 232, -232])
        add("dat == H08_BT_MIN", 0, elm=ID_H08, dat=180.0, mem=180.0)
        add("dat below H08_BT_MIN", QC_GROSS, elm=ID_H08, dat=DN(180.0), mem=180.0)
        add("h08_lev == limit", 0, elm=ID_H08, dat=232.0, mem=232.0, lev=20000.0)
        add("h08_lev below limit", QC_BAD, elm=ID_H08, dat=232.0, mem=232.0, lev=DN(20000.0))
        add("h08 undef", QC_BAD, elm=ID_H08, dat=UNDEF, mem=232.0)
    else:
        add("8800 without h08 is an ordinary row", 0, elm=ID_H08, dat=32.0 + 5.0 * 2.0, mem=[32, 32, 32, 32], lev=0.0)
        add("8800 without h08, above", QC_GROSS, elm=ID_H08, dat=UP(42.0), mem=[32, 32, 32, 32], lev=0.0)
    return rows_of(rows, TK, TK + 1)


def oracle_departure(prm, r):
    """orc_obs_departure on copies of the rows r; val starts as canaries.  prm: a QcParams (h08_lev / h08_val2 are set here: val2
    is passed when prm.h08_val2 is not None on entry -- any non-zero value).  Returns (ens, val, qc, val2)."""
    n = len(r["qc"])
    ens, qc, v2, lev = r["ens"].copy(), r["qc"].copy(), r["val2"].copy(), r["lev"].copy()
    val = canary_buffer(max(n, 1))
    with_v2 = bool(prm.h08_val2)
    prm.h08_lev, prm.h08_val2 = lev.ctypes.data, (v2.ctypes.data if with_v2 else None)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    _oracle.oracle().orc_obs_departure(C.byref(prm), C.c_int64(n), p(r["elm"]), p(r["dat"]), p(r["err"]), p(ens),
                                       C.c_int64(r["kld"]), p(val), p(qc))
    return ens, val[:n], qc, v2


# ------------------------------------------------------------------------------------------------------------------ the mesh
NLON, NLAT, IHALO, JHALO = 8, 12, 2, 3
NGRD_PAIRS = [(4, 6), (6, 3), (1, 1), (8, 12)]


def mesh_world(ngrd, nctype, fix, rank=(0, 0)):
    """nctype combined types on the nlon x nlat = 8 x 12 subdomain of rank `rank`; type 0 has the mesh `ngrd`, the others the next
    pairs of NGRD_PAIRS"""
    at = NGRD_PAIRS.index(ngrd)
    pairs = [NGRD_PAIRS[(at + i) % len(NGRD_PAIRS)] for i in range(nctype)]
    gi, gj = (np.array([p[a] for p in pairs], np.int32) for a in (0, 1))
    return dict(nctype=nctype, nlon=NLON, nlat=NLAT, ihalo=IHALO, jhalo=JHALO, pi=rank[0], pj=rank[1], fix=int(fix), ngrd_i=gi,
                ngrd_j=gj, ncell=int((gi.astype(np.int64) * gj).sum()))


def mesh_of(cls, w):
    return fill(cls, nctype=w["nctype"], nlon=w["nlon"], nlat=w["nlat"], ihalo=w["ihalo"], jhalo=w["jhalo"], rank_i=w["pi"],
                rank_j=w["pj"], fix_ij_obsgrd=w["fix"], ngrd_i=w["ngrd_i"].ctypes.data, ngrd_j=w["ngrd_j"].ctypes.data)


def cell_np(w, ic, ri, rj):
    """ij_obsgrd with the clamps taken as doubles: 0-based (i, j) of one coordinate pair"""
    gi, gj = int(w["ngrd_i"][ic]), int(w["ngrd_j"][ic])
    with np.errstate(invalid="ignore", over="ignore"):
        ci = np.ceil((np.float64(ri) - w["pi"] * w["nlon"] - w["ihalo"] - 0.5) * gi / w["nlon"])
        cj = np.ceil((np.float64(rj) - w["pj"] * w["nlat"] - w["jhalo"] - 0.5) * (gj if w["fix"] else gi) / w["nlat"])
    i = 1 if not ci >= 1 else gi if ci > gi else int(ci)
    j = 1 if not cj >= 1 else gj if cj > gj else int(cj)
    return i - 1, j - 1


def mesh_rows(w, seed=0):
    """Rows of type 0 exactly on every cell boundary of its mesh in i and in j (the boundary belongs to the cell below it: CEILING),
    one ulp either side, on the subdomain's four edges, outside it on each side, at +-inf, NaN and +-1e300; then every type: many
    rows in one cell, rejected rows interleaved, the LAST type without an accepted row when there is more than one."""
    gi, gj = int(w["ngrd_i"][0]), int(w["ngrd_j"][0])
    i0, j0 = w["pi"] * NLON + IHALO + 0.5, w["pj"] * NLAT + JHALO + 0.5
    sj = gj if w["fix"] else gi
    xs = [i0 + b * NLON / gi for b in range(gi + 1) if (b * NLON / gi) * gi / NLON == b]
    ys = [j0 + b * NLAT / sj for b in range(sj + 1) if (b * NLAT / sj) * sj / NLAT == b]
    xs = sorted(set(xs + [UP(v) for v in xs] + [DN(v) for v in xs]))
    ys = sorted(set(ys + [UP(v) for v in ys] + [DN(v) for v in ys]))
    wild = [np.inf, -np.inf, np.nan, 1e300, -1e300, i0 - 5.0, i0 + NLON + 5.0, 3.0e9, -3.0e9]
    mid_x, mid_y = i0 + 0.3 * NLON, j0 + 0.7 * NLAT
    pts = [(x, mid_y) for x in xs + wild] + [(mid_x, y) for y in ys + wild] + [(x, y) for x in wild[:5] for y in wild[:5]]
    ri, rj = (np.array([p[a] for p in pts], np.float64) for a in (0, 1))
    ct = np.zeros(len(pts), np.int32)
    rng = np.random.default_rng(seed)
    nr = 300
    ri = np.concatenate([ri, np.full(40, mid_x), i0 + rng.uniform(0.0, NLON, nr)])
    rj = np.concatenate([rj, np.full(40, mid_y), j0 + rng.uniform(0.0, NLAT, nr)])
    live = max(w["nctype"] - 1, 1)
    ct = np.concatenate([ct, np.zeros(40, np.int32), rng.integers(0, live, nr).astype(np.int32)])
    qc = np.where(rng.random(len(ct)) < 0.25, rng.choice([5, 12, 50, -1], len(ct)), 0).astype(np.int32)
    qc[:len(pts)] = 0
    if w["nctype"] > 1:                            # rows of the empty type exist, all rejected; and a garbage ctype on a rejected row
        ct[qc != 0] = np.where(rng.random(int((qc != 0).sum())) < 0.5, w["nctype"] - 1, ct[qc != 0])
    ct[np.nonzero(qc != 0)[0][:2]] = [-5, 1 << 20]                   # never read
    return dict(ctype=ct, ri=ri, rj=rj, qc=qc, npts=len(pts))


def oracle_sort(w, r):
    """orc_obs_mesh_sort; n_cell and key start as canaries.  Returns (n_cell [ncell], key [nobs] with key[nsorted:] canaries,
    nsorted)."""
    lib = _oracle.oracle()
    lib.orc_obs_mesh_sort.restype = C.c_int64
    n = len(r["qc"])
    n_cell, key = canary_buffer(max(w["ncell"], 1), np.int32), canary_buffer(max(n, 1), np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    m = mesh_of(Mesh, w)
    ns = lib.orc_obs_mesh_sort(C.byref(m), C.c_int64(n), p(r["ctype"]), p(r["ri"]), p(r["rj"]), p(r["qc"]), p(n_cell), p(key))
    return n_cell[:w["ncell"]], key[:n], int(ns)


# ------------------------------------------------------------------------------------------------------------- the halo plan
def plan_world(px, py, fix, seed=3, empty_rank=None, nobs=900):
    """px x py ranks of the 8 x 12 subdomain, three combined types with meshes (4, 6), (6, 3), (1, 1) and search reaches
    ((1, 2), (7, 4), (1, 1)): type 1's reach of 7 cells passes the neighbour's 6 into the rank after it.  Every rank's n_cell from
    the oracle's sort of uniformly scattered rows (none on `empty_rank`)."""
    rng = np.random.default_rng(seed)
    gi, gj = np.array([4, 6, 1], np.int32), np.array([6, 3, 1], np.int32)
    si, sj = np.array([1, 7, 1], np.int32), np.array([2, 4, 1], np.int32)
    w = dict(px=px, py=py, nctype=3, nlon=NLON, nlat=NLAT, ihalo=IHALO, jhalo=JHALO, fix=int(fix), ngrd_i=gi, ngrd_j=gj,
             ngrdsch_i=si, ngrdsch_j=sj, ncell=int((gi.astype(np.int64) * gj).sum()),
             nacx=int(((gi + 2 * si + 1).astype(np.int64) * (gj + 2 * sj)).sum()))
    n_all = []
    for r in range(px * py):
        n = 0 if r == empty_rank else nobs
        wr = dict(w, pi=r % px, pj=r // px)
        rows = dict(ctype=rng.integers(0, 3, n).astype(np.int32), ri=wr["pi"] * NLON + IHALO + 0.5 + rng.uniform(0, NLON, n),
                    rj=wr["pj"] * NLAT + JHALO + 0.5 + rng.uniform(0, NLAT, n),
                    qc=np.where(rng.random(n) < 0.2, 5, 0).astype(np.int32))
        n_all.append(oracle_sort(wr, rows)[0].copy())
    w["n_all"] = np.ascontiguousarray(np.stack(n_all), np.int32)
    w["total"] = int(w["n_all"].sum())
    return w


def layout_of(cls, w, myrank):
    return fill(cls, nctype=w["nctype"], nprocs=w["px"] * w["py"], prc_num_x=w["px"], myrank=myrank,
                ngrd_i=w["ngrd_i"].ctypes.data, ngrd_j=w["ngrd_j"].ctypes.data, ngrdsch_i=w["ngrdsch_i"].ctypes.data,
                ngrdsch_j=w["ngrdsch_j"].ctypes.data)


def oracle_plan(w, myrank, cap):
    """orc_obs_halo_plan into canary buffers.  Returns (ac_ext [nacx], src_row [cap], nobstotal or -1)."""
    lib = _oracle.oracle()
    lib.orc_obs_halo_plan.restype = C.c_int64
    ac, src = canary_buffer(max(w["nacx"], 1), np.int32), canary_buffer(max(cap, 1), np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    lay = layout_of(HaloLayout, w, myrank)
    nt = lib.orc_obs_halo_plan(C.byref(lay), p(w["n_all"]), p(ac), p(src), C.c_int64(cap))
    return ac[:w["nacx"]], src[:cap], int(nt)
