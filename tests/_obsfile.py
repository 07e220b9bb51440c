"""The statement of include/letkf_amd_obsfile.h in numpy: the four record formats of the reference's files (conventional, radar,
obsda, departure) encoded and decoded row by row, in numpy.float32 arithmetic wherever the reference works on its single
precision wk, both byte orders, the TC position rows through tests/_mapproj.py's forward projection, the member loop of
letkf_obs.f90:180-237 with obs_da_value_partial_reduce_iter, and the builders of the test cases.  No GPU, no library."""
import math

import numpy as np

import _mapproj as M

F32 = np.float32
CONV, RADAR, OBSDA, DEP = 1, 2, 3, 4
ID = dict(u=2819, v=2820, t=3073, tv=3074, q=3330, rh=3331, ps=14593, tclon=99991, tclat=99992, tcmip=99993)   # common_obs_scale.f90:48-61
UNKNOWN_ID = 4001                         # (radar reflectivity: no case of the SELECT)
UNDEF = -9.99e33                          # common/common.f90:38
TINY = float(np.finfo(np.float32).tiny)   # tiny(wk(5))
OBSERR_TC = (5.0e2, 50.0e3, 50.0e3)       # OBSERR_TCP, TCX, TCY (common_nml.f90:306-308)
COLUMNS = ("elm", "typ", "lon", "lat", "lev", "dat", "err", "dif")
HEAD_WORDS = {CONV: 0, RADAR: 9, OBSDA: 0, DEP: 0}
INT_MIN, INT_MAX = -2 ** 31, 2 ** 31 - 1


def nint(x):
    """NINT of a float32, evaluated in float64: half away from zero; NaN gives 0, beyond int32 saturates (the header's NEW)"""
    x = float(F32(x))
    if x != x:
        return 0
    if math.isinf(x):
        return INT_MAX if x > 0 else INT_MIN
    return max(INT_MIN, min(INT_MAX, math.trunc(x + math.copysign(0.5, x))))


# ---- framing: marker, wk(1:nrec), marker
def frame(rec, big_endian=False, head=None):
    """the file's bytes of the float32 records rec [n, nrec]; head: the three radar values (one record of one float each)"""
    rec = np.ascontiguousarray(rec, dtype=F32)
    n, nrec = rec.shape
    words = np.empty((n, nrec + 2), dtype=np.uint32)
    words[:, 0] = words[:, -1] = 4 * nrec
    words[:, 1:-1] = rec.view(np.uint32)
    if head is not None:
        h = np.empty((3, 3), dtype=np.uint32)
        h[:, 0] = h[:, 2] = 4
        h[:, 1] = np.asarray(head, dtype=np.float64).astype(F32).view(np.uint32)
        words = np.concatenate([h.ravel(), words.ravel()])
    return words.astype(">u4" if big_endian else "<u4").tobytes()


def unframe(data, nrec, big_endian=False, head=False):
    """(rec float32 [n, nrec], markers uint32 [n, 2], head float64 [3] or None) of a file's bytes"""
    words = np.frombuffer(data, dtype=">u4" if big_endian else "<u4").astype(np.uint32)
    meta = None
    if head:
        meta = words[:9].reshape(3, 3)[:, 1].copy().view(F32).astype(np.float64)
        words = words[9:]
    assert words.size % (nrec + 2) == 0
    words = words.reshape(-1, nrec + 2)
    return np.ascontiguousarray(words[:, 1:-1]).view(F32), words[:, [0, -1]], meta


def count(fmt, nrec, nbytes):
    """get_nobs / get_nobs_radar: the rows, or None where the size is no whole number of records"""
    body = nbytes - 4 * HEAD_WORDS[fmt]
    return body // (4 * (nrec + 2)) if body >= 0 and body % (4 * (nrec + 2)) == 0 else None


# ---- read_obs / read_obs_radar
def decode_obs(rec, fmt, q=None, obserr_tc=OBSERR_TC):
    """the columns of the records rec [n, nrec]: read_obs' SELECT CASE in float32 before the widening (:2162-2198); q: the
    projection's constants (M.setup) or None, then a TC position row's dat is NaN"""
    n, nrec = rec.shape
    out = {k: np.zeros(n, dtype=np.int32 if k in ("elm", "typ") else np.float64) for k in COLUMNS}
    c100, c001 = F32(100.0), F32(0.01)
    with np.errstate(all="ignore"):
        for i in range(n):
            wk = [None] + [F32(v) for v in rec[i]] + [F32(0.0)] * (8 - nrec)
            if fmt == CONV:
                e = nint(wk[1])
                if e in (ID["u"], ID["v"], ID["t"], ID["tv"], ID["q"]):
                    wk[4] = wk[4] * c100
                elif e == ID["ps"]:
                    wk[5], wk[6] = wk[5] * c100, wk[6] * c100
                elif e == ID["rh"]:
                    wk[4], wk[5], wk[6] = wk[4] * c100, wk[5] * c001, wk[6] * c001
                elif e == ID["tcmip"]:
                    wk[4], wk[5], wk[6] = wk[4] * c100, wk[5] * c100, F32(obserr_tc[0])
                elif e in (ID["tclon"], ID["tclat"]):
                    x = y = np.nan
                    if q is not None:
                        x, y = M.forward(q, np.float64(wk[2]) * M.PI_REF / 180.0, np.float64(wk[3]) * M.PI_REF / 180.0)[:2]
                    wk[4] = wk[4] * c100
                    wk[5] = F32(x) if e == ID["tclon"] else F32(y)
                    wk[6] = F32(obserr_tc[1] if e == ID["tclon"] else obserr_tc[2])
            out["elm"][i] = nint(wk[1])
            for k, j in (("lon", 2), ("lat", 3), ("lev", 4), ("dat", 5), ("err", 6)):
                out[k][i] = np.float64(wk[j])
            out["typ"][i] = 22 if fmt == RADAR else nint(wk[7])
            out["dif"][i] = np.float64(wk[8]) if nrec == 8 else 0.0
    return out


def scale_write(wk):
    """write_obs' and write_obs_dep's SELECT CASE on the float32 list wk (1-based)"""
    c100, c001 = F32(100.0), F32(0.01)
    e = nint(wk[1])
    if e in (ID["u"], ID["v"], ID["t"], ID["tv"], ID["q"]):
        wk[4] = wk[4] * c001
    elif e in (ID["ps"], ID["tcmip"]):
        wk[5], wk[6] = wk[5] * c001, wk[6] * c001
    elif e == ID["rh"]:
        wk[4], wk[5], wk[6] = wk[4] * c001, wk[5] * c100, wk[6] * c100


def defined(dat):
    with np.errstate(all="ignore"):
        return abs(np.float64(dat) - UNDEF) > TINY


def encode_obs(cols, fmt, nrec, missing=True):
    """write_obs / write_obs_radar: the float32 records [nwritten, nrec] of the columns"""
    rows = []
    with np.errstate(all="ignore"):
        for i in range(len(cols["elm"])):
            if not (missing or defined(cols["dat"][i])):
                continue
            wk = [None] + [F32(cols[k][i]) for k in ("elm", "lon", "lat", "lev", "dat", "err", "typ")]
            wk.append(F32(cols["dif"][i]) if nrec == 8 else F32(0.0))
            if fmt == CONV:
                scale_write(wk)
            rows.append(wk[1:nrec + 1])
    return np.array(rows, dtype=F32).reshape(len(rows), nrec)


# ---- obsda
def encode_obsda(set_, idx, value, qc, lev=None, val2=None):
    """write_obs_da: float32 records [n, 4] or, with lev and val2, [n, 6]"""
    cols = [np.asarray(set_).astype(F32), np.asarray(idx).astype(F32), np.asarray(value, dtype=np.float64).astype(F32), np.asarray(qc).astype(F32)]
    if lev is not None:
        cols += [np.asarray(lev, dtype=np.float64).astype(F32), np.asarray(val2, dtype=np.float64).astype(F32)]
    return np.stack(cols, axis=1) if len(cols[0]) else np.zeros((0, len(cols)), dtype=F32)


def assemble(recs, col, ensval, qc, is_member=None, lev=None, val2=None, member=0, finish=False):
    """the member loop of letkf_obs.f90:180-237 with obs_da_value_partial_reduce_iter over the images' records recs[m] [nobs, nrec]:
    returns dict set, idx, qc, ensval, lev, val2, ninconsistent -- ensval [nobs, kld], qc, lev and val2 start from the caller's"""
    nobs, nrec = recs[0].shape
    ensval, qc = ensval.copy(), qc.copy()
    lev = None if lev is None else lev.copy()
    val2 = None if val2 is None else val2.copy()
    set_, idx, bad = np.zeros(nobs, dtype=np.int32), np.zeros(nobs, dtype=np.int32), np.zeros(nobs, dtype=bool)
    for m, rec in enumerate(recs):
        for n in range(nobs):
            s, i = nint(rec[n, 0]), nint(rec[n, 1])
            if m == 0:
                set_[n], idx[n] = s, i
            elif s != set_[n] or i != idx[n]:
                bad[n] = True
            ensval[n, col[m]] = np.float64(rec[n, 2])
            qc[n] = max(qc[n], nint(rec[n, 3]))
            if nrec == 6 and (is_member is None or is_member[m]):
                if lev is not None:
                    lev[n] = lev[n] + np.float64(rec[n, 4])
                if val2 is not None:
                    val2[n] = val2[n] + np.float64(rec[n, 5])
    if nrec == 6 and finish:
        lev = None if lev is None else lev / np.float64(member)
        val2 = None if val2 is None else val2 / np.float64(member)
    return dict(set=set_, idx=idx, qc=qc, ensval=ensval, lev=lev, val2=val2, ninconsistent=int(bad.sum()))


# ---- write_obs_dep
def encode_dep(set_, idx, qc, omb, oma, off, files):
    rows = []
    with np.errstate(all="ignore"):
        for n in range(len(set_)):
            g = off[set_[n] - 1] + idx[n] - 1
            wk = [None] + [F32(files[k][g]) for k in ("elm", "lon", "lat", "lev", "dat", "err", "typ", "dif")]
            wk += [F32(qc[n]), F32(omb[n]), F32(oma[n])]
            scale_write(wk)
            rows.append(wk[1:])
    return np.array(rows, dtype=F32).reshape(len(rows), 11)


# ---- comparisons: integers equal, floats as their bit patterns
def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    return bool(np.array_equal(a.view(np.uint8), b.view(np.uint8)))


def ulp32_apart(a, b):
    """the distance of two float64 arrays, each a widened float32, in float32 steps"""
    ia, ib = (np.asarray(v, dtype=np.float64).astype(F32).view(np.int32).astype(np.int64) for v in (a, b))
    ia, ib = (np.where(i < 0, INT_MIN - i, i) for i in (ia, ib))
    return np.abs(ia - ib)


# ---- the case builders
def conv_records(n, seed=0, tc=True):
    """n conventional records [n, 8]: every id of the SELECT CASE and an unknown one in turn, a denormal-making error, file
    values in the file's units (hPa, percent, degrees)"""
    rng = np.random.default_rng(seed)
    ids = [ID[k] for k in ("u", "v", "t", "tv", "q", "rh", "ps", "tcmip")] + ([ID["tclon"], ID["tclat"]] if tc else []) + [UNKNOWN_ID]
    rec = np.zeros((n, 8), dtype=F32)
    rec[:, 0] = [ids[i % len(ids)] for i in range(n)]
    rec[:, 1] = rng.uniform(130.0, 140.0, n)
    rec[:, 2] = rng.uniform(30.0, 40.0, n)
    rec[:, 3] = rng.uniform(100.0, 1013.25, n)
    rec[:, 4] = rng.uniform(-50.0, 1050.0, n)
    rec[:, 5] = rng.uniform(0.1, 20.0, n)
    rec[:, 6] = rng.integers(1, 24, n)
    rec[:, 7] = rng.uniform(-1800.0, 1800.0, n)
    if n > 5:
        rec[5, 5] = F32(1e-37)            # an RH row: 1e-37f * 0.01f is a denormal
    return rec


def radar_records(n, nrec, seed=0):
    rng = np.random.default_rng(seed + 100)
    rec = np.zeros((n, nrec), dtype=F32)
    rec[:, 0] = rng.choice([4001, 4002, 4004], n)
    rec[:, 1] = rng.uniform(134.0, 136.0, n)
    rec[:, 2] = rng.uniform(34.0, 36.0, n)
    rec[:, 3] = rng.uniform(0.0, 15000.0, n)
    rec[:, 4] = rng.uniform(-30.0, 60.0, n)
    rec[:, 5] = rng.uniform(1.0, 5.0, n)
    rec[:, 6] = rng.integers(1, 24, n)      # (read_obs_radar ignores it: typ = 22)
    if nrec == 8:
        rec[:, 7] = rng.uniform(-300.0, 300.0, n)
    return rec


def columns_of(n, seed=0, fmt=CONV):
    """float32-representable columns as an encoder takes them (SI units): the decode of the builders' records"""
    rec = conv_records(n, seed, tc=False) if fmt == CONV else radar_records(n, 8, seed)
    return decode_obs(rec, fmt)


def obsda_records(nobs, nmem, nrec, seed=0):
    """nmem lists of records [nobs, nrec] that agree in set / idx; qc 0 but for a sprinkle"""
    rng = np.random.default_rng(seed + 7)
    set_ = rng.integers(1, 4, nobs)
    idx = rng.integers(1, 100000, nobs)
    recs = []
    for m in range(nmem):
        rec = np.zeros((nobs, nrec), dtype=F32)
        rec[:, 0], rec[:, 1] = set_, idx
        rec[:, 2] = rng.normal(0.0, 10.0, nobs)
        rec[:, 3] = np.where(rng.random(nobs) < 0.1, rng.integers(1, 99, nobs), 0)
        if nrec == 6:
            rec[:, 4] = rng.uniform(1.0, 10.0, nobs) * 10.0 ** rng.integers(-8, 9, (nobs,))     # 17 decades: float64 sums round
            rec[:, 5] = rng.uniform(200.0, 300.0, nobs)
        recs.append(rec)
    return recs
