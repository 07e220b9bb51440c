"""obsmake_cal (scale/obs/obsope_tools.f90:767-1058) in numpy on the fixtures of tests/_obsope.py: the CPU statement that
letkf_obsmake_slot_dev and letkf_obsmake_noise_dev (include/letkf_amd_obsmake.h) are compared with, and the plumbing of a
device call.  The operator is tests/_obsope.py's, in obsmake_cal's mode: no USE_OBS test, no RADAR_ZMAX test, and qc 11 kept
(_obsope.operator folds it into 0 as obsope_tools.f90:488 does and returns only the folded qc: the few lines are restated
in operator_rows below).  Rows here are FILE rows: obsmake_cal has no obsda rows."""
import ctypes as C
import math

import numpy as np

import _obsope as O
import _sfmt as S

UNDEF = O.UNDEF
LB, UB = -300.0, 300.0                                  # the slot of the fixtures (SLOT_TINTERVAL 600 s, the base slot)
_ROWS = {}


def cfg_of(**kw):
    """The fixtures' configuration: radar_zmax far below most radar rows and report type 3 switched off -- obsmake_cal
    computes those rows all the same"""
    return O.default_cfg(radar_zmax=3000.0, **kw)


def file_row_of(case):
    """file row of every obsda row of the case"""
    return (case["off"][case["set"] - 1] + case["idx"] - 1).astype(np.int64)


def rotc_by_file_row(case):
    out = np.zeros((case["nrow"], 2))
    out[file_row_of(case)] = case["rotc"]
    return out


def operator_rows(case, cfg, m):
    """obsmake_cal's operator on every file row for member m: dict of val, qc (11 kept), tol, kind by file row.  Shared by
    the tests and left unchanged."""
    key = (id(case), cfg["method_ref_calc"], cfg["use_terminal_velocity"], cfg["stggrd"], m)
    if key not in _ROWS:
        ocfg = dict(cfg, use_obs=np.ones(O.NOBTYPE, dtype=np.int32), radar_zmax=math.inf)
        n = case["nrow"]
        out = dict(val=np.zeros(n), qc=np.zeros(n, dtype=np.int32), tol=np.zeros(n), kind=np.empty(n, dtype=object),
                   elm=np.zeros(n, dtype=np.int32), radar=np.zeros(n, dtype=bool))
        for r, fr in zip(range(n), file_row_of(case)):
            row, rc = case["rows"][r], tuple(case["rotc"][r])
            o = O.operator(ocfg, case["g"], case["v3"][m], case["v2"][m], row, rc)
            qc = o["qc"]
            if qc == 0 and row["radar"] is not None and row["elm"] in (O.ID_REF, O.ID_REF_ZERO, O.ID_VR):
                # Trans_XtoY_radar :470-487: ref < MIN_RADAR_REF gives qc 11 for reflectivity and for Doppler velocity alike
                as_ref = o if row["elm"] != O.ID_VR else O.operator(ocfg, case["g"], case["v3"][m], case["v2"][m],
                                                                    dict(row, elm=O.ID_REF), rc)
                if as_ref["kind"] == "lowref":
                    qc = O.QC_REF_LOW
            out["val"][fr], out["qc"][fr], out["tol"][fr], out["kind"][fr] = o["val"], qc, o["tol"], o["kind"]
            out["elm"][fr], out["radar"][fr] = row["elm"], row["radar"] is not None
        for a in out.values():
            a.setflags(write=False)
        _ROWS[key] = out
    return _ROWS[key]


def slot_inputs(case, seed):
    """dif and own per file row: most rows in the slot (LB, UB], some exactly on LB (out) and on UB (in), some outside; own
    of all three kinds"""
    rng = np.random.default_rng(seed)
    n = case["nrow"]
    dif = rng.uniform(LB + 1.0, UB - 1.0, size=n)
    pick = rng.permutation(n)
    dif[pick[:12]] = LB
    dif[pick[12:24]] = UB
    dif[pick[24:44]] = rng.uniform(UB + 1.0, UB + 600.0, size=20)
    dif[pick[44:54]] = rng.uniform(LB - 600.0, LB - 1.0, size=10)
    own = rng.choice(np.array([1, 1, 1, 1, 0, -1], dtype=np.int32), size=n).astype(np.int32)
    return dif, own


def slot_statement(case, cfg, m, dif, own, lb, ub, outside_undef, dat):
    """one letkf_obsmake_slot_dev call: (dat after, tol per row (0: bit for bit), counts)"""
    st = operator_rows(case, cfg, m)
    in_ = (dif > lb) & (dif <= ub)
    proc = in_ & ((own == 1) if own is not None else True)
    out, tol = dat.copy(), np.zeros(len(dat))
    out[proc] = np.where(st["qc"][proc] == 0, st["val"][proc], UNDEF)
    tol[proc] = np.where(st["qc"][proc] == 0, st["tol"][proc], 0.0)
    if own is not None and outside_undef:
        out[in_ & (own == -1)] = UNDEF
    return out, tol, np.array([in_.sum(), proc.sum()], dtype=np.int64)


ERR = dict(obserr_u=1.0, obserr_v=1.25, obserr_t=0.5, obserr_q=1e-3, obserr_rh=0.1, obserr_ps=100.0, obserr_radar_ref=5.0,
           obserr_radar_vr=3.0)
ERR_OF = {O.ID_U: "obserr_u", O.ID_V: "obserr_v", O.ID_T: "obserr_t", O.ID_TV: "obserr_t", O.ID_Q: "obserr_q", O.ID_RH: "obserr_rh",
          O.ID_PS: "obserr_ps", O.ID_REF: "obserr_radar_ref", O.ID_REF_ZERO: "obserr_radar_ref", O.ID_VR: "obserr_radar_vr"}


def noise_statement(elm, dat, err, seed, errs=ERR):
    """letkf_obsmake_noise_dev: (dat after, err after, the deviates, the rows that were perturbed)"""
    n = len(elm)
    error = S.randn(S.Sfmt(seed, 0), n)
    err = err.copy()
    for e, name in ERR_OF.items():
        err[elm == e] = errs[name]
    hit = (dat != UNDEF) & (err != UNDEF)
    out = dat.copy()
    out[hit] = dat[hit] + err[hit] * error[hit]
    return out, err, error, hit


# ------------------------------------------------------------------------------------------------------- the device calls
def device_case(pkg, case, cfg, dev, m, dat, err=None, rotc="file", **kw):
    """tests/_obsope.py's DeviceCase with member m alone, files->dat (and err), and rotc per FILE row (None: no rotation)"""
    files = dict(case["files"], dat=np.ascontiguousarray(dat, dtype=np.float64))
    if err is not None:
        files["err"] = np.ascontiguousarray(err, dtype=np.float64)
    return O.DeviceCase(pkg, dict(case, files=files), cfg, dev, members=(m, 1), rotc=rotc_by_file_row(case) if rotc == "file" else rotc, **kw)


def run_slot(pkg, ctx, dc, dif, own, lb, ub, outside_undef, want_counts=True):
    """One call on dc's files; returns (dat, counts or None) as numpy"""
    import torch
    s = pkg.ObsmakeSlot()
    ddif = torch.from_numpy(np.ascontiguousarray(dif)).to(dc.dev)
    down = None if own is None else torch.from_numpy(np.ascontiguousarray(own, dtype=np.int32)).to(dc.dev)
    s.slot_lb, s.slot_ub, s.dif, s.own = lb, ub, C.c_void_p(ddif.data_ptr()), None if down is None else C.c_void_p(down.data_ptr())
    s.outside_undef = int(outside_undef)
    counts = torch.full((2,), -7, dtype=torch.int64, device=dc.dev) if want_counts else None
    ctx.obsmake_slot(s, dc.params, dc.files, dc.fields, counts)
    torch.cuda.synchronize()
    return dc.d["dat"].cpu().numpy(), None if counts is None else counts.cpu().numpy()


def err_struct(pkg, errs=ERR):
    e = pkg.ObsmakeErr()
    for n, v in errs.items():
        setattr(e, n, v)
    return e
