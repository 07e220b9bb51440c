"""NOBS_OUT in numpy, as the reference states it (scale/letkf/letkf_tools.f90): obs_local's initial nobsl_t / cutd_t (:1380-1389),
work3dn from them (:440-447) and the eleven fields the reference writes (:768-778).  The inputs are per combined type, as
letkf_obs_search_columns_dev and letkf_das_columns_nobs_dev give them; the statement scatters them into the reference's
(nid_obs, nobtype) tables first and then reads the reference's own lines."""
import numpy as np

NID_OBS = 16
DIST_ZERO_FAC = float(np.float32(3.651483717))
UID_REF, UID_RE0, UID_VR, TYP_RADAR = 9, 10, 11, 22
PICK = (1, 3, 4, 8, 22)
NFIELDS = 11


def defaults(nctype, groups, hori_loc, criterion):
    """nobsl_t / cutd_t of one point before obs_local finds anything, per combined type (:1380-1389, :1427-1431): counts 0; under the
    distance criterion the cut-off hori_loc * dist_zero_fac on every group's master (groups: lists of 0-based ctypes, master first),
    0 on the other members and under criteria 2 / 3"""
    nobs = np.zeros(nctype, dtype=np.int32)
    cutd = np.zeros(nctype)
    if criterion == 1:
        for g in groups:
            cutd[g[0]] = hori_loc[g[0]] * DIST_ZERO_FAC
    return nobs, cutd


def tables(nobs_ctype, cutd_ctype, elm_u_ctype, typ_ctype, nobtype):
    """nobsl_t, cutd_t [npts, nid_obs, nobtype] from the per-ctype rows (1-based uid and report type): a combination no combined
    type carries keeps its zero"""
    nobs_ctype = np.asarray(nobs_ctype)
    npts, nctype = nobs_ctype.shape
    nobsl_t = np.zeros((npts, NID_OBS, nobtype), dtype=np.int64)
    cutd_t = np.zeros((npts, NID_OBS, nobtype))
    for ic in range(nctype):
        nobsl_t[:, elm_u_ctype[ic] - 1, typ_ctype[ic] - 1] = nobs_ctype[:, ic]
        if cutd_ctype is not None:
            cutd_t[:, elm_u_ctype[ic] - 1, typ_ctype[ic] - 1] = np.asarray(cutd_ctype)[:, ic]
    return nobsl_t, cutd_t


def work3dn(nobs_ctype, cutd_ctype, elm_u_ctype, typ_ctype, nobtype=24, uid=(UID_REF, UID_RE0, UID_VR), typ_radar=TYP_RADAR):
    """work3dn(:, ij, ilev, n) of every point, [npts, nobtype + 6] (:441-447)"""
    nobsl_t, cutd_t = tables(nobs_ctype, cutd_ctype, elm_u_ctype, typ_ctype, nobtype)
    w = np.zeros((nobsl_t.shape[0], nobtype + 6))
    w[:, :nobtype] = nobsl_t.sum(axis=1)                          # sum(nobsl_t, dim=1): over the variables, per report type
    for q in range(3):
        w[:, nobtype + q] = nobsl_t[:, uid[q] - 1, typ_radar - 1]
        w[:, nobtype + 3 + q] = cutd_t[:, uid[q] - 1, typ_radar - 1]
    return w


def fields(w, nobtype=24, pick=PICK):
    """work3d(:, :, 1..11) from work3dn, [npts, 11] (:768-778)"""
    rows = [p - 1 for p in pick] + [nobtype + q for q in range(6)]
    return np.ascontiguousarray(w[:, rows])
