"""Python harness binding for libletkf_amd.so (the C ABI in include/letkf_amd.h).

The product is the HIP library + the Fortran shim (scale-letkf_amd/fortran); this module is only the
ctypes plumbing that tests/, bench.py and __graft_entry__.py use to drive the C ABI with torch-owned
device memory.  It never computes anything itself and has no CPU fallback: if the library is missing
or no gfx950 device is visible, every entry raises.

Because the directory name carries a hyphen, load it with `load_package()` from __graft_entry__.py
(importlib under the module name `scale_letkf_amd`).
"""
import ctypes as C
import glob
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("LETKF_AMD_LIB") or os.path.join(HERE, "lib", "libletkf_amd.so")   # override: profiling twin (make PROF=1)
OSSE_LIB_PATH = os.path.join(HERE, "lib", "libletkf_amd_osse.so")   # the OSSE tools (include/letkf_amd_obsmake.h); links against the production library
OBSSIM_LIB_PATH = os.path.join(HERE, "lib", "libletkf_amd_obssim.so")   # the model-to-observation simulator (include/letkf_amd_obssim.h); links against the production library too
SUPEROB_LIB_PATH = os.path.join(HERE, "lib", "libletkf_amd_superob.so")   # superob (include/letkf_amd_superob.h); links against the production library too
OBSSCAN_LIB_PATH = os.path.join(HERE, "lib", "libletkf_amd_obsscan.so")   # obsope_cal's first scan (include/letkf_amd_obsscan.h); made by `make obsscan`, after the default goal
MAPPROJ_LIB_PATH = os.path.join(HERE, "lib", "libletkf_amd_mapproj.so")   # the map projection (include/letkf_amd_mapproj.h); made by `make mapproj`, in the same way
OBSFILE_LIB_PATH = os.path.join(HERE, "lib", "libletkf_amd_obsfile.so")   # the record codec of the observation files (include/letkf_amd_obsfile.h); made by `make obsfile`, in the same way
NOBSOUT_LIB_PATH = os.path.join(HERE, "lib", "libletkf_amd_nobsout.so")   # NOBS_OUT (include/letkf_amd_nobsout.h); made by `make nobsout`, in the same way
TCVITAL_LIB_PATH = os.path.join(HERE, "lib", "libletkf_amd_tcvital.so")   # the TC vitals (include/letkf_amd_tcvital.h); made by `make tcvital`, in the same way
H08_LIB_PATH = os.path.join(HERE, "lib", "libletkf_amd_h08.so")           # the Himawari-8 radiances (include/letkf_amd_h08.h); made by `make h08`, in the same way

LETKF_OK = 0
ST_OK, ST_NOT_CONVERGED, ST_NONPOSITIVE, ST_ILLCOND = 0, 1, 2, 3


class LetkfError(RuntimeError):
    pass


def build(force=False):
    """Compile the HIP sources for gfx950 (hipcc cross-compiles without a GPU)."""
    srcs = [os.path.join(HERE, "csrc", f) for f in os.listdir(os.path.join(HERE, "csrc"))]
    srcs += glob.glob(os.path.join(HERE, "csrc", "obsscan", "*")) + glob.glob(os.path.join(HERE, "csrc", "mapproj", "*"))
    srcs += glob.glob(os.path.join(HERE, "csrc", "obsfile", "*")) + glob.glob(os.path.join(HERE, "csrc", "nobsout", "*"))
    srcs += glob.glob(os.path.join(HERE, "csrc", "tcvital", "*")) + glob.glob(os.path.join(HERE, "csrc", "h08", "*"))
    srcs += glob.glob(os.path.join(HERE, "..", "include", "letkf_amd*.h"))
    srcs = [s for s in srcs if os.path.isfile(s)]      # (a directory's time is that of its last new entry, not of a source)
    if os.environ.get("LETKF_AMD_LIB") and os.path.exists(LIB_PATH) and not force:
        return LIB_PATH                      # an A/B or profiling twin: taken as it is, whatever its age
    libs = (LIB_PATH, OSSE_LIB_PATH, OBSSIM_LIB_PATH, SUPEROB_LIB_PATH, OBSSCAN_LIB_PATH, MAPPROJ_LIB_PATH, OBSFILE_LIB_PATH, NOBSOUT_LIB_PATH) + (
        TCVITAL_LIB_PATH,) + (H08_LIB_PATH,)
    stale = force or not all(os.path.exists(l) for l in libs) or any(
        os.path.getmtime(s) > min(os.path.getmtime(l) for l in libs) for s in srcs)
    if stale:                                # (make's chatter to stderr: stdout belongs to the caller's JSON line)
        subprocess.check_call(["make", "-j4", "-C", HERE] + (["-B"] if force else []), stdout=2)
        subprocess.check_call(["make", "-j4", "-C", HERE, "obsscan"], stdout=2)   # (a goal of its own, after the default one)
        subprocess.check_call(["make", "-j4", "-C", HERE, "mapproj"], stdout=2)   # (and so is this)
        subprocess.check_call(["make", "-j4", "-C", HERE, "obsfile"], stdout=2)   # (and this)
        subprocess.check_call(["make", "-j4", "-C", HERE, "nobsout"], stdout=2)   # (and this)
        subprocess.check_call(["make", "-j4", "-C", HERE, "tcvital"], stdout=2)   # (and this)
        subprocess.check_call(["make", "-j4", "-C", HERE, "h08"], stdout=2)       # (and this)
    return LIB_PATH


class CoreBatchArgs(C.Structure):
    _fields_ = [("ne", C.c_int32), ("nobs", C.c_int32), ("nbatch", C.c_int64), ("nobsl", C.c_void_p),
                ("hdxb", C.c_void_p), ("rdiag", C.c_void_p), ("rloc", C.c_void_p), ("dep", C.c_void_p),
                ("depd", C.c_void_p), ("parm_infl", C.c_void_p), ("trans", C.c_void_p), ("transm", C.c_void_p),
                ("pao", C.c_void_p), ("transmd", C.c_void_p), ("rdiag_wloc", C.c_int32),
                ("infl_update", C.c_int32), ("status", C.c_void_p), ("nsweep", C.c_void_p)]


class DasArgs(C.Structure):
    _fields_ = [("k", C.c_int32), ("nv", C.c_int32), ("det_run", C.c_int32), ("infl_adaptive", C.c_int32),
                ("relax_to_inflated_prior", C.c_int32), ("iv_p", C.c_int32), ("iv_q_first", C.c_int32),
                ("iv_q_last", C.c_int32), ("warm_stride", C.c_int32),
                ("relax_alpha", C.c_double), ("relax_alpha_spread", C.c_double), ("q_update_top", C.c_double),
                ("q_sprd_max", C.c_double), ("npts", C.c_int64), ("obs_off", C.c_void_p), ("obs_idx", C.c_void_p),
                ("rdiag_l", C.c_void_p), ("rloc_l", C.c_void_p), ("ensval", C.c_void_p), ("kld", C.c_int64),
                ("dep", C.c_void_p), ("beta", C.c_void_p), ("infl", C.c_void_p), ("gues", C.c_void_p),
                ("anal", C.c_void_p), ("sp", C.c_int64), ("sm", C.c_int64), ("sv", C.c_int64),
                ("trans_out", C.c_void_p), ("transm_out", C.c_void_p), ("pa_out", C.c_void_p),
                ("status", C.c_void_p), ("nsweep", C.c_void_p), ("rtps_infl_out", C.c_void_p),
                ("warm_run", C.c_int32), ("var_mask", C.c_uint32), ("infl_sv", C.c_int64)]


class EfsoArgs(C.Structure):
    _fields_ = [("k", C.c_int32), ("nv", C.c_int32), ("nterm", C.c_int32), ("var_mask", C.c_uint32),
                ("term_of_var", C.c_void_p), ("npts", C.c_int64), ("obs_off", C.c_void_p), ("obs_idx", C.c_void_p),
                ("rdiag_l", C.c_void_p), ("rloc_l", C.c_void_p), ("ensval", C.c_void_p), ("kld", C.c_int64),
                ("nobs", C.c_int64), ("fcst", C.c_void_p), ("sp", C.c_int64), ("sm", C.c_int64), ("sv", C.c_int64),
                ("fcer", C.c_void_p), ("fsp", C.c_int64), ("fsv", C.c_int64), ("djdy", C.c_void_p),
                ("pair_bytes", C.c_int64)]


class EfsoNormParams(C.Structure):
    """letkf_efso_norm_params (include/letkf_amd.h section 13)"""
    _fields_ = [("k", C.c_int32), ("nv", C.c_int32), ("iv_u", C.c_int32), ("iv_v", C.c_int32), ("iv_t", C.c_int32),
                ("iv_q", C.c_int32), ("iv_p", C.c_int32), ("tar_minlev", C.c_int32), ("tar_maxlev", C.c_int32),
                ("cp", C.c_double), ("tref", C.c_double), ("hvap", C.c_double), ("wmoist", C.c_double),
                ("tar_minlon", C.c_double), ("tar_maxlon", C.c_double), ("tar_minlat", C.c_double),
                ("tar_maxlat", C.c_double)]


class DasObsArgs(C.Structure):
    """letkf_das_obs_args (include/letkf_amd.h section 11)"""
    _fields_ = [("k", C.c_int32), ("det_run", C.c_int32), ("tvar", C.c_int32), ("relax_to_inflated_prior", C.c_int32),
                ("iv_q_first", C.c_int32), ("iv_q_last", C.c_int32), ("relax_alpha", C.c_double),
                ("relax_alpha_spread", C.c_double), ("q_update_top", C.c_double), ("q_sprd_max", C.c_double),
                ("ntgt", C.c_int64), ("tgt_row", C.c_void_p), ("ensval", C.c_void_p), ("kld", C.c_int64),
                ("dep", C.c_void_p), ("nobs", C.c_int64), ("rlev_tgt", C.c_void_p), ("rz_tgt", C.c_void_p),
                ("beta", C.c_void_p), ("infl", C.c_void_p), ("infl_mul", C.c_double), ("ya", C.c_void_p),
                ("lda", C.c_int64), ("ya_mean", C.c_void_p), ("ya_table", C.c_void_p), ("dep_a", C.c_void_p),
                ("nobs_out", C.c_void_p), ("status", C.c_void_p), ("list_bytes", C.c_int64)]


class SearchTables(C.Structure):
    """letkf_search_tables (include/letkf_amd.h section 3)"""
    _fields_ = [("nctype", C.c_int32), ("ngroup", C.c_int32), ("criterion", C.c_int32), ("nlon", C.c_int32),
                ("nlat", C.c_int32), ("limit_hint", C.c_int32), ("dx", C.c_double), ("dy", C.c_double),
                ("i_org", C.c_double), ("j_org", C.c_double), ("rain_base", C.c_double),
                ("group_start", C.c_void_p), ("group_member", C.c_void_p), ("vmode", C.c_void_p),
                ("hori_loc", C.c_void_p), ("vert_loc", C.c_void_p), ("varloc", C.c_void_p), ("max_nobs", C.c_void_p),
                ("ngrd_i", C.c_void_p), ("ngrd_j", C.c_void_p), ("ngrdsch_i", C.c_void_p), ("ngrdsch_j", C.c_void_p),
                ("ngrdext_i", C.c_void_p), ("ngrdext_j", C.c_void_p), ("ac_off", C.c_void_p), ("ac_ext", C.c_void_p),
                ("ob_ri", C.c_void_p), ("ob_rj", C.c_void_p), ("ob_lev", C.c_void_p), ("ob_dat", C.c_void_p),
                ("ob_err", C.c_void_p)]


class QcParams(C.Structure):
    """letkf_qc_params (include/letkf_amd.h section 5); defaults = the reference namelist defaults
    (scale/common/common_nml.f90)"""
    _fields_ = [("member", C.c_int32), ("det_run", C.c_int32), ("use_radar_ref", C.c_int32),
                ("use_radar_vr", C.c_int32), ("min_radar_ref_member", C.c_int32),
                ("min_radar_ref_member_obsref", C.c_int32), ("radar_ref_thres_dbz", C.c_double),
                ("gross_error", C.c_double), ("gross_error_rain", C.c_double), ("gross_error_radar_ref", C.c_double),
                ("gross_error_radar_vr", C.c_double), ("gross_error_radar_prh", C.c_double),
                ("gross_error_tcx", C.c_double), ("gross_error_tcy", C.c_double), ("gross_error_tcp", C.c_double),
                ("h08", C.c_int32), ("h08_min_cld_member", C.c_int32), ("h08_limit_lev", C.c_double),
                ("gross_error_h08", C.c_double), ("h08_bt_min", C.c_double), ("h08_lev", C.c_void_p),
                ("h08_val2", C.c_void_p)]


class Mesh(C.Structure):
    """letkf_mesh (section 5); ngrd_i / ngrd_j are HOST int32 arrays"""
    _fields_ = [("nctype", C.c_int32), ("nlon", C.c_int32), ("nlat", C.c_int32), ("ihalo", C.c_int32),
                ("jhalo", C.c_int32), ("rank_i", C.c_int32), ("rank_j", C.c_int32), ("fix_ij_obsgrd", C.c_int32),
                ("ngrd_i", C.c_void_p), ("ngrd_j", C.c_void_p)]


class HaloLayout(C.Structure):
    """letkf_halo_layout (section 5); the four arrays are HOST int32 arrays"""
    _fields_ = [("nctype", C.c_int32), ("nprocs", C.c_int32), ("prc_num_x", C.c_int32), ("myrank", C.c_int32),
                ("ngrd_i", C.c_void_p), ("ngrd_j", C.c_void_p), ("ngrdsch_i", C.c_void_p), ("ngrdsch_j", C.c_void_p)]


class SetObsParams(C.Structure):
    """letkf_setobs_params (include/letkf_amd.h section 9); the per-report-type arrays are HOST arrays"""
    _fields_ = [("nobtype", C.c_int32), ("use_obserr_radar_ref", C.c_int32), ("use_obserr_radar_vr", C.c_int32),
                ("nlon", C.c_int32), ("nlat", C.c_int32), ("ihalo", C.c_int32), ("jhalo", C.c_int32),
                ("nprocs", C.c_int32), ("prc_num_x", C.c_int32), ("myrank", C.c_int32), ("fix_ij_obsgrd", C.c_int32),
                ("criterion", C.c_int32), ("min_radar_ref_dbz", C.c_double), ("low_ref_shift", C.c_double),
                ("obserr_radar_ref", C.c_double), ("obserr_radar_vr", C.c_double),
                ("hori_local_radar_obsnoref", C.c_double), ("hori_local_radar_vr", C.c_double),
                ("vert_local_radar_vr", C.c_double), ("dx", C.c_double), ("dy", C.c_double), ("rain_base", C.c_double),
                ("hori_local", C.c_void_p), ("vert_local", C.c_void_p), ("obs_sort_grid_spacing", C.c_void_p),
                ("obs_min_spacing", C.c_void_p), ("max_nobs_per_grid", C.c_void_p), ("ctype_merge", C.c_void_p)]


class ObsFileRows(C.Structure):
    """letkf_obs_file_rows (section 9): off is a HOST int64 array, the rest device pointers"""
    _fields_ = [("nfile", C.c_int32), ("reserved0", C.c_int32), ("off", C.c_void_p), ("elm", C.c_void_p),
                ("typ", C.c_void_p), ("lev", C.c_void_p), ("dat", C.c_void_p), ("err", C.c_void_p), ("ri", C.c_void_p),
                ("rj", C.c_void_p)]


class ObsTableInfo(C.Structure):
    """letkf_obs_table_info (section 9)"""
    _fields_ = ([("nctype", C.c_int32), ("kld", C.c_int32), ("finished", C.c_int32), ("nobtype", C.c_int32)] +
                [(n, C.c_int64) for n in ("nobs", "nsorted", "ncell", "nacx", "nobstotal", "ld_send")] +
                [(n, C.c_void_p) for n in ("elm_ctype", "elm_u_ctype", "typ_ctype", "hori_loc_ctype", "vert_loc_ctype",
                                           "ctype_elmtyp", "ngrd_i", "ngrd_j", "ngrdsch_i", "ngrdsch_j", "ngrdext_i",
                                           "ngrdext_j", "grdspc_i", "grdspc_j", "ac_off", "tot_sub", "tot_g", "n_cell",
                                           "key", "sendbuf", "row_elm", "row_ctype", "row_dat", "row_err", "row_ri",
                                           "row_rj", "row_lev", "val", "ensval", "val_sort", "qc_sort")])


def obs_mesh_dims(typ_ctype, hori_loc_ctype, obs_sort_grid_spacing, max_nobs_per_grid, obs_min_spacing, dx, dy, nlon, nlat):
    """letkf_obs_mesh_dims (host only).  Returns dict of numpy arrays ngrd_i .. ngrdext_j, grdspc_i / grdspc_j."""
    import numpy as np
    ty = np.ascontiguousarray(typ_ctype, dtype=np.int32)
    hl = np.ascontiguousarray(hori_loc_ctype, dtype=np.float64)
    sp = np.ascontiguousarray(obs_sort_grid_spacing, dtype=np.float64)
    mx = np.ascontiguousarray(max_nobs_per_grid, dtype=np.int32)
    ms = np.ascontiguousarray(obs_min_spacing, dtype=np.float64)
    nc = len(ty)
    outs = ("ngrd_i", "ngrd_j", "grdspc_i", "grdspc_j", "ngrdsch_i", "ngrdsch_j", "ngrdext_i", "ngrdext_j")   # the entry's order
    o = {n: np.zeros(max(nc, 1), dtype=np.float64 if n.startswith("grdspc") else np.int32) for n in outs}
    p = _hptr
    rc = lib().letkf_obs_mesh_dims(nc, p(ty), p(hl), len(sp), p(sp), p(mx), p(ms), dx, dy, nlon, nlat, *[p(v) for v in o.values()])
    if rc != LETKF_OK:
        raise LetkfError(f"letkf_obs_mesh_dims: {rc}: {lib().letkf_amd_last_error().decode()}")
    return {k: v[:nc].copy() for k, v in o.items()}


class ObsTable:
    """A library-owned set_letkf_obs table (letkf_obs_table); released by close() / garbage collection."""

    def __init__(self, ctx, handle, keep):
        self._ctx, self._h, self._keep = ctx, handle, keep

    def close(self):
        if self._h:
            self._ctx._l.letkf_obs_table_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def info(self):
        i = ObsTableInfo()
        self._ctx._check(self._ctx._l.letkf_obs_table_info_get(self._h, C.byref(i)))
        return i

    def host(self):
        """The small host tables and counts as numpy arrays."""
        import numpy as np
        i = self.info()
        nc = i.nctype

        def arr(ptr, ctype, n):
            if n == 0 or not ptr:
                return np.zeros(0, dtype=ctype)
            return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(np.ctypeslib.as_ctypes_type(ctype))), (n,)).copy()
        out = dict(nctype=nc, nobs=i.nobs, nsorted=i.nsorted, ncell=i.ncell, nacx=i.nacx, nobstotal=i.nobstotal,
                   kld=i.kld, ld_send=i.ld_send)
        for n in ("elm_ctype", "elm_u_ctype", "typ_ctype", "ngrd_i", "ngrd_j", "ngrdsch_i", "ngrdsch_j", "ngrdext_i",
                  "ngrdext_j"):
            out[n] = arr(getattr(i, n), np.int32, nc)
        for n in ("hori_loc_ctype", "vert_loc_ctype", "grdspc_i", "grdspc_j"):
            out[n] = arr(getattr(i, n), np.float64, nc)
        out["ac_off"] = arr(i.ac_off, np.int64, nc)
        out["ctype_elmtyp"] = arr(i.ctype_elmtyp, np.int32, 16 * i.nobtype).reshape(i.nobtype, 16)
        out["tot_sub"] = arr(i.tot_sub, np.int32, 2 * nc).reshape(nc, 2)
        out["tot_g"] = arr(i.tot_g, np.int32, 2 * nc).reshape(nc, 2) if i.tot_g else None
        return out

    def target_groups(self):
        """das_letkf_obs's targets of this rank: {tvar: rows} (int32 numpy, ascending) of the rows that lie in the INTERIOR
        cells of each ctype's sorting mesh (not the ngrdsch halo), grouped by letkf_obs_target_var(elm of the ctype) -- so
        that a sum over the ranks covers every observation once."""
        import numpy as np
        h = self.host()
        ac = self.download()["ac_ext"].astype(np.int64)
        groups = {}
        for c in range(h["nctype"]):
            ni, nsi, nxi = int(h["ngrd_i"][c]), int(h["ngrdsch_i"][c]), int(h["ngrdext_i"][c])
            nj, nsj = int(h["ngrd_j"][c]), int(h["ngrdsch_j"][c])
            base = int(h["ac_off"][c])
            tv = obs_target_var(int(h["elm_ctype"][c]))
            for j in range(nsj + 1, nsj + nj + 1):        # entry (i, j) at ac_off + i + (ngrdext_i + 1) * (j - 1)
                r0 = ac[base + nsi + (nxi + 1) * (j - 1)]
                r1 = ac[base + nsi + ni + (nxi + 1) * (j - 1)]
                if r1 > r0:
                    groups.setdefault(tv, []).append(np.arange(r0, r1, dtype=np.int32))
        return {tv: np.sort(np.concatenate(r)).astype(np.int32) for tv, r in sorted(groups.items())}

    def search_tables(self):
        t = SearchTables()
        self._ctx._check(self._ctx._l.letkf_obs_table_search(self._h, C.byref(t)))
        return t

    def set_varloc(self, varloc):
        import numpy as np
        v = np.ascontiguousarray(varloc, dtype=np.float64)
        self._ctx._check(self._ctx._l.letkf_obs_table_set_varloc(self._ctx._c, self._h, _hptr(v)))

    def download(self):
        """obsda_sort and the metadata as numpy arrays (letkf_obs_table_download)."""
        import numpy as np
        i = self.info()
        nt, n1 = i.nobstotal, max(i.nobstotal, 1)
        o = dict(ensval=np.zeros((n1, i.kld)), val=np.zeros(n1), qc=np.zeros(n1, np.int32), ob_ri=np.zeros(n1), ob_rj=np.zeros(n1),
                 ob_lev=np.zeros(n1), ob_dat=np.zeros(n1), ob_err=np.zeros(n1), ac_ext=np.zeros(max(i.nacx, 1), np.int32))
        ptrs = [_hptr(v) for v in o.values()]      # (o is in the entry's argument order)
        self._ctx._check(self._ctx._l.letkf_obs_table_download(self._ctx._c, self._h, *ptrs))
        return {k: (v[:i.nacx] if k == "ac_ext" else v[:nt]) for k, v in o.items()}


class StateConsts(C.Structure):
    """letkf_state_consts (include/letkf_amd.h section 4)"""
    _fields_ = [("rdry", C.c_double), ("rvap", C.c_double), ("cvdry", C.c_double), ("pre00", C.c_double),
                ("tracer_cv", C.c_double * 8), ("iv_rho", C.c_int32), ("iv_rhou", C.c_int32), ("iv_rhov", C.c_int32),
                ("iv_rhow", C.c_int32), ("iv_rhot", C.c_int32), ("iv_u", C.c_int32), ("iv_v", C.c_int32),
                ("iv_w", C.c_int32), ("iv_t", C.c_int32), ("iv_p", C.c_int32), ("iv_q", C.c_int32),
                ("positive_definite_q", C.c_int32), ("positive_definite_qhyd", C.c_int32), ("reserved0", C.c_int32)]


def scale_rm_consts(clamp=True):
    """SCALE-RM's constants (scale_const / scale_tracer; NOT in the reference tree, values of SCALE-RM 5.x) with the
    variable slots of scale/common/common_scale.f90:36-51 (rho/u, rhou/v? no: u=1 v=2 w=3 t=4 p=5 q=6..11, 0-based
    0..10; prognostic twins share the slots: rho<->... see below)."""
    c = StateConsts()
    c.rdry, c.rvap, c.pre00 = 287.04, 461.46, 1.0e5
    c.cvdry = 1004.64 - 287.04
    for i, v in enumerate([1407.0, 4218.0, 4218.0, 2006.0, 2006.0, 2006.0]):   # QV, QC, QR, QI, QS, QG
        c.tracer_cv[i] = v
    # common_scale.f90:36-51: iv3d_rho=1 iv3d_rhou=2 iv3d_rhov=3 iv3d_rhow=4 iv3d_rhot=5 share the slots of
    # iv3d_u=1 iv3d_v=2 iv3d_w=3 iv3d_t=4 iv3d_p=5 (the transform overwrites in place)
    c.iv_rho, c.iv_rhou, c.iv_rhov, c.iv_rhow, c.iv_rhot = 0, 1, 2, 3, 4
    c.iv_u, c.iv_v, c.iv_w, c.iv_t, c.iv_p, c.iv_q = 0, 1, 2, 3, 4, 5
    c.positive_definite_q = c.positive_definite_qhyd = int(clamp)
    return c


class BetaParams(C.Structure):
    """letkf_beta_params (include/letkf_amd.h section 7)"""
    _fields_ = [("radar_only", C.c_int32), ("ihalo", C.c_int32), ("jhalo", C.c_int32), ("nlong", C.c_int32),
                ("nlatg", C.c_int32), ("reserved0", C.c_int32), ("radar_zmax", C.c_double),
                ("vert_local_radar", C.c_double), ("boundary_buffer_width", C.c_double), ("dx", C.c_double),
                ("dy", C.c_double)]


# ctypes signature of every entry include/letkf_amd.h declares, in its order (pointers of any kind as void *): ctypes converts or
# refuses a bare Python number at the call.  Written out by hand, the header is not read here; tests/test_abi.py keeps them in step.
_VP, _I32, _I64, _F64, _INT = C.c_void_p, C.c_int32, C.c_int64, C.c_double, C.c_int
ARGTYPES = {
    "letkf_amd_abi_version": [],
    "letkf_amd_last_error": [],
    "letkf_ctx_create": [_INT, _VP],
    "letkf_ctx_destroy": [_VP],
    "letkf_ctx_set_stream": [_VP, _VP],
    "letkf_ctx_synchronize": [_VP],
    "letkf_ctx_set_option": [_VP, _INT, _INT],
    "letkf_core_c": [_INT, _INT, _INT, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP],
    "letkf_core_batch_dev": [_VP, _VP],
    "letkf_das_points_dev": [_VP, _VP],
    "letkf_ens_to_perturbations_dev": [_VP, _I32, _I32, _I64, _VP, _I64, _I64, _I64],
    "letkf_ens_mean_dev": [_VP, _I32, _I32, _I64, _VP, _I64, _I64, _I64],
    "letkf_obs_search_dev": [_VP, _VP, _I64, _VP, _VP, _VP, _VP, _I32, _VP, _VP, _VP, _VP, _VP],
    "letkf_obs_search_columns_dev": [_VP, _VP, _I64, _I32, _VP, _VP, _VP, _VP, _I32, _VP, _VP, _VP, _VP, _VP, _VP, _VP],
    "letkf_das_points_fused_dev": [_VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP],
    "letkf_das_columns_dev": [_VP, _VP, _VP, _I64, _I32, _VP, _VP, _VP, _VP, _I64, _VP],
    "letkf_state_trans_dev": [_VP, _VP, _I32, _I32, _I32, _I32, _VP, _I32],
    "letkf_member_points_dev": [_VP, _I32, _I32, _I32, _I32, _I32, _I32, _I32, _I32, _VP, _VP, _I64, _I64, _I64, _I64],
    "letkf_ens_spread_dev": [_VP, _I32, _I32, _I64, _VP, _I64, _I64, _I64, _VP],
    "letkf_obs_departure_dev": [_VP, _VP, _I64, _VP, _VP, _VP, _VP, _I64, _VP, _VP],
    "letkf_obs_mesh_sort_dev": [_VP, _VP, _I64, _VP, _VP, _VP, _VP, _VP, _VP, _VP],
    "letkf_obs_halo_plan_dev": [_VP, _VP, _VP, _VP, _VP, _I64, _VP],
    "letkf_obs_gather_rows_dev": [_VP, _I64, _VP, _I32, _VP, _I64, _VP, _I64],
    "letkf_obs_gather_i32_dev": [_VP, _I64, _VP, _VP, _VP],
    "letkf_monit_dep_dev": [_VP, _I32, _VP, _I64, _VP, _VP, _VP, _VP, _VP, _VP],
    "letkf_additive_inflation_dev": [_VP, _I32, _I32, _I64, _I64, _VP, _VP, _I64, _I64, _I64, _F64, _VP, _VP, _I64, _I64, _I32,
                                     _I32, _VP],
    "letkf_addinfl_weight_dev": [_VP, _I64, _VP, _VP, _I64, _VP, _VP, _F64, _F64, _F64, _VP],
    "letkf_var_local_classes": [_I32, _I32, _VP, _VP, _VP, _VP],
    "letkf_ctype_merge_groups": [_I32, _VP, _VP, _I32, _I32, _VP, _VP, _VP, _VP],
    "letkf_radar_only": [_I32, _VP, _I32],
    "letkf_relax_beta_dev": [_VP, _VP, _I64, _I32, _VP, _VP, _VP, _VP],
    "letkf_infl_init_dev": [_VP, _I64, _VP, _F64, _F64],
    "letkf_obs_allgatherv_dev": [_VP, _VP, _I32, _I32, _VP, _I64, _VP, _VP],
    "letkf_alltoallv_dev": [_VP, _VP, _I32, _I32, _VP, _VP, _VP, _VP, _I64, _VP, _VP],
    "letkf_allreduce_sum_i32_dev": [_VP, _VP, _I32, _I64, _VP],
    "letkf_members_alltoall_dev": [_VP, _VP, _I32, _I32, _I32, _I32, _I32, _I32, _I32, _I32, _I32, _VP, _VP, _I64, _I64, _I64],
    "letkf_obs_mesh_dims": [_I32, _VP, _VP, _I32, _VP, _VP, _VP, _F64, _F64, _I32, _I32, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP],
    "letkf_set_obs_local_dev": [_VP, _VP, _VP, _VP, _I64, _VP, _VP, _VP, _VP, _I64, _VP],
    "letkf_set_obs_finish_dev": [_VP, _VP, _VP, _VP, _I64, _VP],
    "letkf_set_obs_dev": [_VP, _VP, _VP, _VP, _I64, _VP, _VP, _VP, _VP, _I64, _VP],
    "letkf_obs_table_info_get": [_VP, _VP],
    "letkf_obs_table_search": [_VP, _VP],
    "letkf_obs_table_set_varloc": [_VP, _VP, _VP],
    "letkf_obs_table_download": [_VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP],
    "letkf_obs_table_destroy": [_VP],
    "letkf_efso_points_dev": [_VP, _VP],
    "letkf_efso_columns_dev": [_VP, _VP, _VP, _I64, _I32, _VP, _VP, _VP, _VP, _I64],
    "letkf_efso_obsense_dev": [_VP, _I32, _I64, _VP, _VP, _VP],
    "letkf_das_obs_dev": [_VP, _VP, _VP],
    "letkf_obs_target_var": [_I32],
    "letkf_efso_locadv_dev": [_VP, _I64, _I32, _VP, _VP, _VP, _VP, _VP, _VP, _F64, _F64, _F64, _F64, _VP, _VP],
    "letkf_efso_search_dev": [_VP, _VP, _VP, _I64, _VP, _VP, _VP, _VP, _I64],
    "letkf_efso_norm_dev": [_VP, _VP, _I64, _I32, _VP, _I64, _I64, _I64, _VP, _VP, _I64, _I64, _VP, _VP, _VP, _VP, _VP, _VP,
                            _VP],
    "letkf_efso_summary_dev": [_VP, _I32, _I64, _VP, _VP, _VP, _VP, _VP, _I32, _VP, _I32, _F64, _VP, _VP, _VP],
    "letkf_ctx_last_path": [_VP, _VP, _I32],
    "letkf_ctx_timing_enable": [_VP, _INT],
    "letkf_ctx_timing_read": [_VP, _VP, _VP, _INT],
    "letkf_sched_plan_check": [_I64, _I64, _I32, _I32, _I32, _I32],
    "letkf_sched_plan_check_units": [_I64, _I64, _I32, _I32, _I32, _I32, _I32],
}
RESTYPES = {"letkf_amd_last_error": C.c_char_p, "letkf_core_c": None}     # every other entry returns int
EXPORTS = list(ARGTYPES)


class InterpArgs(C.Structure):
    """letkf_interp_args (include/letkf_amd_interp.h)"""
    _fields_ = [("nx", C.c_int32), ("ny", C.c_int32), ("nlev", C.c_int32), ("stride_x", C.c_int32),
                ("stride_y", C.c_int32), ("reserved0", C.c_int32), ("ws_bytes", C.c_int64), ("rig", C.c_void_p),
                ("rjg", C.c_void_p), ("rlev", C.c_void_p), ("rz", C.c_void_p), ("nobs_coarse", C.c_void_p)]


# ... and of the entries of the companion header include/letkf_amd_interp.h, a table of their own, as for every companion
# header below (DESIGN.md section 17 lists what a new one touches)
INTERP_VERSION = 1
INTERP_ARGTYPES = {
    "letkf_interp_coarse_axis": [_I32, _I32, _VP, _VP],
    "letkf_das_interp_dev": [_VP, _VP, _VP, _VP],
}


class InterpWindow(C.Structure):
    """letkf_interp_window (include/letkf_amd_interp_window.h)"""
    _fields_ = [("gnx", C.c_int32), ("gny", C.c_int32), ("gi0", C.c_int32), ("gj0", C.c_int32), ("oi0", C.c_int32),
                ("oj0", C.c_int32), ("onx", C.c_int32), ("ony", C.c_int32)]


# ... and of the second companion header include/letkf_amd_interp_window.h, a table of its own
INTERP_WINDOW_VERSION = 1
INTERP_WINDOW_ARGTYPES = {
    "letkf_interp_window_axis": [_I32, _I32, _I32, _I32, _I32, _I32, _VP, _VP],
    "letkf_das_interp_window_dev": [_VP, _VP, _VP, _VP, _VP],
}



class ObsopeFields(C.Structure):
    """letkf_obsope_fields (include/letkf_amd_obsope.h)"""
    _fields_ = ([(n, C.c_int32) for n in ("nlev", "nlon", "nlat", "khalo", "ihalo", "jhalo", "nv3dd", "nv2dd", "nmem", "m0")] +
                [("v3d", C.c_void_p)] + [(n, C.c_int64) for n in ("s3k", "s3i", "s3j", "s3v", "s3m")] +
                [("v2d", C.c_void_p)] + [(n, C.c_int64) for n in ("s2i", "s2j", "s2v", "s2m")])


class ObsopeParams(C.Structure):
    """letkf_obsope_params (include/letkf_amd_obsope.h): file_radar, radar_meta and use_obs are HOST arrays"""
    _fields_ = ([(n, C.c_void_p) for n in ("lon", "lat", "file_radar", "radar_meta", "rotc", "use_obs")] +
                [(n, C.c_int32) for n in ("nobtype", "method_ref_calc", "use_terminal_velocity", "stggrd")] +
                [(n, C.c_double) for n in ("min_radar_ref_dbz", "low_ref_shift", "radar_zmax", "ps_adjust_thres", "ri_off",
                                           "rj_off")])


# ... and of the third companion header include/letkf_amd_obsope.h, a table of its own
OBSOPE_VERSION = 1
OBSOPE_ARGTYPES = {
    "letkf_obsope_dev": [_VP, _VP, _VP, _VP, _I64, _I64, _VP, _VP, _VP, _VP, _I64],
}



class HistState(C.Structure):
    """letkf_hist_state (include/letkf_amd_monit.h): cz is a HOST array"""
    _fields_ = ([("nv3d", C.c_int32), ("edge_fill", C.c_int32), ("x", C.c_void_p)] +
                [(n, C.c_int64) for n in ("si", "sj", "sl", "sv")] + [("topo", C.c_void_p), ("cz", C.c_void_p), ("ztop", C.c_double)])


class MonitParams(C.Structure):
    """letkf_monit_params (include/letkf_amd_monit.h): elem_uid is a HOST array"""
    _fields_ = ([(n, C.c_int32) for n in ("step", "departure_stat_radar", "nid", "reserved0")] +
                [("elem_uid", C.c_void_p), ("t_range", C.c_double), ("dif", C.c_void_p)])


class Obsdep(C.Structure):
    """letkf_obsdep (include/letkf_amd_monit.h): the obsdep records, device arrays [nn]"""
    _fields_ = [(n, C.c_void_p) for n in ("set", "idx", "qc", "omb", "oma")]


# ... and of the fourth companion header include/letkf_amd_monit.h, a table of its own
MONIT_VERSION = 1
MONIT_ARGTYPES = {
    "letkf_state_to_history_dev": [_VP, _VP, _VP, _VP, _VP],
    "letkf_monit_obs_dev": [_VP, _VP, _VP, _VP, _VP, _I64, _VP, _VP, _VP, _VP, _VP, _VP, _VP],
    "letkf_monit_type": [_I32, _VP, _I32, _I32, _VP],
}



class ObsmakeSlot(C.Structure):
    """letkf_obsmake_slot (include/letkf_amd_obsmake.h): dif and own are device arrays per file row"""
    _fields_ = [("slot_lb", C.c_double), ("slot_ub", C.c_double), ("dif", C.c_void_p), ("own", C.c_void_p),
                ("outside_undef", C.c_int32), ("reserved0", C.c_int32)]


class ObsmakeErr(C.Structure):
    """letkf_obsmake_err (include/letkf_amd_obsmake.h): the OBSERR_* of the namelist"""
    _fields_ = [(n, C.c_double) for n in ("obserr_u", "obserr_v", "obserr_t", "obserr_q", "obserr_rh", "obserr_ps",
                                          "obserr_radar_ref", "obserr_radar_vr")]


# ... and of the fifth companion header include/letkf_amd_obsmake.h, a table of its own: these entries are exported by the library
# of the OSSE tools (OSSE_LIB_PATH, osse_lib()), not by the main one
OBSMAKE_VERSION = 1
OBSMAKE_ARGTYPES = {
    "letkf_rand_create": [_I32, _VP],
    "letkf_rand_destroy": [_VP],
    "letkf_rand_set_chunk": [_VP, _I64],
    "letkf_rand_res53": [_VP, _I64, _VP],
    "letkf_randn_dev": [_VP, _VP, _I64, _VP],
    "letkf_obsmake_slot_dev": [_VP, _VP, _VP, _VP, _VP, _VP],
    "letkf_obsmake_noise_dev": [_VP, _VP, _VP, _VP],
}



class ObssimParams(C.Structure):
    """letkf_obssim_params (include/letkf_amd_obssim.h): the lists and the radar are values, lon / lat / rotc device arrays"""
    _fields_ = ([("nvar3", C.c_int32), ("vars3", C.c_int32 * 16), ("nvar2", C.c_int32), ("vars2", C.c_int32 * 16)] +
                [(n, C.c_double) for n in ("radar_lon", "radar_lat", "radar_z")] +
                [(n, C.c_void_p) for n in ("lon", "lat", "rotc")] +
                [(n, C.c_int32) for n in ("method_ref_calc", "use_terminal_velocity", "stggrd", "round_single")] +
                [(n, C.c_double) for n in ("min_radar_ref_dbz", "low_ref_shift", "ps_adjust_thres")])


class ObssimOut(C.Structure):
    """letkf_obssim_out (include/letkf_amd_obssim.h): v3 / v2 double, rec float device arrays (any may be NULL, not all)"""
    _fields_ = [("v3", C.c_void_p), ("v2", C.c_void_p), ("rec", C.c_void_p), ("sm3", C.c_int64), ("sm2", C.c_int64)]


# ... and of the sixth companion header include/letkf_amd_obssim.h, a table of its own: the entry is exported by the library of the
# simulator (OBSSIM_LIB_PATH, obssim_lib()), not by the other two
OBSSIM_VERSION = 1
OBSSIM_ARGTYPES = {
    "letkf_obssim_dev": [_VP, _VP, _VP, _VP],
}



class SuperobParams(C.Structure):
    """letkf_superob_params (include/letkf_amd_superob.h): slot_off, elem_uid and the method tables are HOST arrays, the rows
    device arrays"""
    _fields_ = ([("nobs", C.c_int64)] +
                [(n, C.c_void_p) for n in ("elm", "typ", "lon", "lat", "lev", "dat", "err", "ri", "rj", "rk", "slot_off")] +
                [(n, C.c_int32) for n in ("nlon", "nlat", "nlevx", "nslots", "nbslot", "nobtype", "nid", "surface_typ_mask")] +
                [(n, C.c_void_p) for n in ("elem_uid", "method_g", "method_v", "method_t", "method_h")])


class SuperobOut(C.Structure):
    """letkf_superob_out (include/letkf_amd_superob.h): device arrays; slot_off_out, qc1, counts and obsnum may be NULL"""
    _fields_ = [(n, C.c_void_p) for n in ("elm", "typ", "slot", "lon", "lat", "lev", "dat", "err", "ri", "rj", "rk", "i", "j", "k",
                                          "nout", "slot_off_out", "qc1", "counts", "obsnum")]


# ... and of the seventh companion header include/letkf_amd_superob.h, a table of its own: the entries are exported by the library
# of superob (SUPEROB_LIB_PATH, superob_lib()), not by the other three
SUPEROB_VERSION = 1
SUPEROB_ARGTYPES = {
    "letkf_superob_dev": [_VP, _VP, _VP],
    "letkf_superob_default_methods": [_I32, _I32, _VP, _VP, _VP, _VP],
    "letkf_superob_slot_priority": [_I32, _I32, _VP],
}
SUPEROB_SURFACE_TYPES = 0x4780   # report types 8, 9, 10, 11, 15 (scale/obs/superob.f90:289-291)



class ObsscanParams(C.Structure):
    """letkf_obsscan_params (include/letkf_amd_obsscan.h): dif is a device array per file row, obsda_run a HOST array or NULL"""
    _fields_ = ([("dif", C.c_void_p), ("obsda_run", C.c_void_p)] +
                [(n, C.c_int32) for n in ("nlon", "nlat", "ihalo", "jhalo", "prc_num_x", "prc_num_y", "slot_start", "slot_end",
                                          "slot_base", "myrank_d")] + [("slot_tinterval", C.c_double)])


class ObsscanOut(C.Structure):
    """letkf_obsscan_out (include/letkf_amd_obsscan.h): bsn / bsna are HOST arrays, the rest device arrays; rank, slot and own
    may be NULL"""
    _fields_ = [(n, C.c_void_p) for n in ("set", "idx", "qc", "bsn", "bsna", "rank", "slot", "own")]


class ObsscanLists(C.Structure):
    """letkf_obsscan_lists (include/letkf_amd_obsscan.h): a scan's lists as letkf_obsope_slot_dev takes them; bsna is a HOST array"""
    _fields_ = ([(n, C.c_int32) for n in ("nprocs_d", "slot_start", "slot_end", "reserved0")] +
                [(n, C.c_void_p) for n in ("bsna", "set", "idx", "qc")])


# ... and of the eighth companion header include/letkf_amd_obsscan.h, a table of its own: the entries are exported by the library
# of the scan (OBSSCAN_LIB_PATH, obsscan_lib()), not by the other four
OBSSCAN_VERSION = 1
OBSSCAN_ARGTYPES = {
    "letkf_obsscan_dev": [_VP, _VP, _VP, _VP],
    "letkf_obsscan_rows": [_VP, _I32, _I32, _I32, _I32, _I32, _VP, _VP],
    "letkf_obsscan_slot_bounds": [_I32, _I32, _I32, _F64, _VP, _VP],
    "letkf_obsope_slot_dev": [_VP, _VP, _I32, _I32, _VP, _VP, _VP, _VP, _I64],
}
OBSSCAN_MAX_BUCKETS = 1 << 22
IQC_TIME, IQC_OUT_H = 97, 98


class MapprojParams(C.Structure):
    """letkf_mapproj_params (include/letkf_amd_mapproj.h): PARAM_MAPPROJ and what phys2ij reads of the grid; degrees and metres"""
    _fields_ = ([("type", C.c_int32), ("reserved0", C.c_int32)] +
                [(n, C.c_double) for n in ("basepoint_lon", "basepoint_lat", "basepoint_x", "basepoint_y", "lc_lat1", "lc_lat2",
                                           "radius", "cxg1", "cyg1", "dx", "dy")])


class Mapproj(C.Structure):
    """letkf_mapproj (include/letkf_amd_mapproj.h): what letkf_mapproj_setup derives; plain data"""
    _fields_ = ([("type", C.c_int32), ("reserved0", C.c_int32)] +
                [(n, C.c_double) for n in ("hemisphere", "lon0", "c", "fact", "radius", "pole_x", "pole_y", "cxg1", "cyg1", "dx",
                                           "dy")])


# ... and of the ninth companion header include/letkf_amd_mapproj.h: the entries are exported by the library of the projection
# (MAPPROJ_LIB_PATH, mapproj_lib()).  (The table's name does not end in ARGTYPES: tests/test_obsscan_binding.py counts the names
# that do, and stays as it is.)
MAPPROJ_VERSION = 1
MAPPROJ_SIGNATURES = {
    "letkf_mapproj_setup": [_VP, _VP],
    "letkf_phys2ij_dev": [_VP, _VP, _I64, _VP, _VP, _VP, _VP, _VP],
    "letkf_ij2phys_dev": [_VP, _VP, _I64, _VP, _VP, _VP, _VP, _VP],
    "letkf_mapproj_grid_dev": [_VP, _VP, _I32, _I32, _I32, _I32, _F64, _F64, _VP, _VP, _VP],
    "letkf_phys2ij_host": [_VP, _F64, _F64, _VP, _VP, _VP],
    "letkf_ij2phys_host": [_VP, _F64, _F64, _VP, _VP, _VP],
}
MAPPROJ_LC = 1
MAPPROJ_RADIUS_SCALE = 6.37122e6
MAPPROJ_PI_REF = 3.1415926535

class ObsfileCols(C.Structure):
    """letkf_obsfile_cols (include/letkf_amd_obsfile.h): the decoded columns of a conventional or radar file, device arrays"""
    _fields_ = [(n, C.c_void_p) for n in ("elm", "typ", "lon", "lat", "lev", "dat", "err", "dif")]


class ObsfileParams(C.Structure):
    """letkf_obsfile_params (include/letkf_amd_obsfile.h): format 1 conventional, 2 radar"""
    _fields_ = ([(n, C.c_int32) for n in ("format", "nrec", "big_endian", "missing", "proj_given", "reserved0")] +
                [(n, C.c_double) for n in ("obserr_tcp", "obserr_tcx", "obserr_tcy")])


class ObsdaParams(C.Structure):
    """letkf_obsda_params (include/letkf_amd_obsfile.h)"""
    _fields_ = ([(n, C.c_int32) for n in ("nrec", "big_endian", "nmem", "finish", "member", "reserved0")] +
                [(n, C.c_int64) for n in ("nobs", "kld")])


class ObsdaCols(C.Structure):
    """letkf_obsda_cols (include/letkf_amd_obsfile.h): the obsda arrays, device arrays"""
    _fields_ = [(n, C.c_void_p) for n in ("set", "idx", "qc", "ensval", "lev", "val2")]


class ObsfileRows(C.Structure):
    """letkf_obsfile_rows (include/letkf_amd_obsfile.h): off is a HOST int64 array, the columns device arrays"""
    _fields_ = ([("nfile", C.c_int32), ("reserved0", C.c_int32)] +
                [(n, C.c_void_p) for n in ("off", "elm", "typ", "lon", "lat", "lev", "dat", "err", "dif")])


# ... and of the tenth companion header include/letkf_amd_obsfile.h: the entries are exported by the library of the record codec
# (OBSFILE_LIB_PATH, obsfile_lib()).  (SIGNATURES, as the projection's table: the frozen binding tests count the names that end in
# ARGTYPES.)
OBSFILE_VERSION = 1
OBSFILE_SIGNATURES = {
    "letkf_obsfile_count": [_I32, _I32, _I64, _VP],
    "letkf_obsfile_bytes": [_I32, _I32, _I64, _VP],
    "letkf_obs_decode_dev": [_VP, _VP, _VP, _VP, _I64, _VP, _VP, _VP],
    "letkf_obs_encode_dev": [_VP, _VP, _I64, _VP, _VP, _VP, _VP],
    "letkf_obsda_assemble_dev": [_VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP],
    "letkf_obsda_encode_dev": [_VP, _I32, _I32, _I64, _VP, _VP, _VP, _VP, _I64, _I32, _VP, _VP, _VP, _VP],
    "letkf_obsdep_encode_dev": [_VP, _I32, _I64, _VP, _VP, _VP, _VP, _VP, _VP, _VP],
}
OBSFILE_CONV, OBSFILE_RADAR, OBSFILE_OBSDA, OBSFILE_DEP = 1, 2, 3, 4
OBSFILE_TILE_ROWS, OBSFILE_TILE_MEMBERS, OBSFILE_MAX_MEMBERS, OBSFILE_TYP_RADAR = 64, 16, 65536, 22
OBSFILE_COLUMNS = ("elm", "typ", "lon", "lat", "lev", "dat", "err", "dif")



class NobsoutParams(C.Structure):
    """letkf_nobsout_params (include/letkf_amd_nobsout.h): elm_u_ctype / typ_ctype are HOST int32 arrays"""
    _fields_ = ([(n, C.c_int32) for n in ("nctype", "nobtype", "uid_ref", "uid_re0", "uid_vr", "typ_radar")] +
                [("pick", C.c_int32 * 5), ("reserved0", C.c_int32), ("elm_u_ctype", C.c_void_p), ("typ_ctype", C.c_void_p)])


# ... and of the eleventh companion header include/letkf_amd_nobsout.h: the entries are exported by the library of NOBS_OUT
# (NOBSOUT_LIB_PATH, nobsout_lib()).  (SIGNATURES, as the two tables before it.)
NOBSOUT_VERSION = 1
NOBSOUT_SIGNATURES = {
    "letkf_das_columns_nobs_dev": [_VP, _VP, _VP, _I64, _I32, _VP, _VP, _VP, _VP, _I64, _VP, _VP, _VP],
    "letkf_nobs_fields_dev": [_VP, _VP, _I64, _VP, _VP, _VP, _VP, _I64, _I64],
}
NOBSOUT_MAX_CTYPE, NOBSOUT_MAX_OBTYPE, NOBSOUT_NFIELDS = 64, 32, 11


class TcvitalParams(C.Structure):
    """letkf_tcvital_params (include/letkf_amd_tcvital.h): the grid as the projection has it, this rank's offsets, TC_SEARCH_DIS"""
    _fields_ = ([(n, C.c_double) for n in ("dx", "dy", "cxg1", "cyg1")] + [("i_off", C.c_int32), ("j_off", C.c_int32)] +
                [("tc_search_dis", C.c_double)])


# ... and of the twelfth companion header include/letkf_amd_tcvital.h: the entries are exported by the library of the TC vitals
# (TCVITAL_LIB_PATH, tcvital_lib()).  (SIGNATURES, as the three tables before it.)
TCVITAL_VERSION = 1
TCVITAL_SIGNATURES = {
    "letkf_tcvital_rows_dev": [_VP, _I64, _VP, _VP, _F64, _F64, _VP, _VP],
    "letkf_tcvital_search_dev": [_VP, _VP, _VP, _VP, _VP, _VP],
    "letkf_tcvital_fill_dev": [_VP, _I32, _I32, _I32, _VP, _VP, _I32, _VP, _VP, _I64],
}
TCVITAL_ID_TCX, TCVITAL_ID_TCY, TCVITAL_ID_TCP, TCVITAL_QC_BAD = 99991, 99992, 99993, 50
TCVITAL_NONE = 9.99e33


class H08Params(C.Structure):
    """letkf_h08_params (include/letkf_amd_h08.h): sizes and switches, H08_CH_USE, this rank's offsets, the constants of the
    profile conversion and of the zenith angle, H08_CLDSKY_THRS and the buffer box"""
    _fields_ = ([(n, C.c_int32) for n in ("nlev", "nprof_file", "top_down", "stggrd", "rttov_units", "reject_land", "use_obs23",
                                          "finish", "member", "reserved0")] + [("ch_use", C.c_int32 * 10)] +
                [(n, C.c_double) for n in ("ri_off", "rj_off", "rd", "rv", "q_ppmv", "qmin", "minq", "cfrac_cnst", "sub_lon", "r_pol",
                                           "r_sat", "ell_tan", "ell_ecc", "cldsky_thrs", "bris", "brie", "brjs", "brje")])


class H08Profiles(C.Structure):
    """letkf_h08_profiles (include/letkf_amd_h08.h): the outputs of letkf_h08_profiles_dev, device arrays"""
    _fields_ = [(n, C.c_void_p) for n in ("lev3", "sfc", "cloud", "pflag")]


# ... and of the thirteenth companion header include/letkf_amd_h08.h: the entries are exported by the library of the Himawari-8
# radiances (H08_LIB_PATH, h08_lib()).  (SIGNATURES, as the four tables before it.)
H08_VERSION = 1
H08_SIGNATURES = {
    "letkf_h08_count": [_I64, _VP],
    "letkf_h08_bytes": [_I64, _VP],
    "letkf_h08_decode_dev": [_VP, _I32, _VP, _I64, _VP, _VP, _VP],
    "letkf_h08_encode_dev": [_VP, _I32, _I64, _VP, _VP],
    "letkf_h08_select_dev": [_VP, _VP, _VP, _I64, _I64, _I32, _I64, _VP, _VP, _VP],
    "letkf_h08_profiles_dev": [_VP, _VP, _VP, _I64, _VP, _VP, _VP, _VP, _VP, _VP, _VP],
    "letkf_h08_rows_dev": [_VP, _VP, _I64, _I64, _VP, _VP, _I32, _VP, _I64, _I32, _I32, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _I32,
                           _VP, _VP, _I64, _VP, _VP],
}
H08_NCH, H08_ID, H08_QC_BAD = 10, 8800, 50


def h08_params(**kw):
    """H08Params with the reference's constants (scale_H08_fwd.F90:137-139, :553-555; scale_const's Rdry / Rvap; RTTOV's
    q_mixratio_to_ppmv and qmin; H08_CLDSKY_THRS = -5, H08_RTTOV_MINQ = 0.1, H08_RTTOV_CFRAC_CNST = 0.1, every channel used, no
    buffer), overridden by the keywords; ch_use takes a sequence of ten"""
    d = dict(use_obs23=1, member=1, rd=287.04, rv=461.46, q_ppmv=1.60771704e6, qmin=0.1e-10, minq=0.1, cfrac_cnst=0.1, sub_lon=140.7,
             r_pol=6356.7523e3, r_sat=42164.0e3, ell_tan=0.993305616, ell_ecc=0.00669438444, cldsky_thrs=-5.0, bris=-1.0e300,
             brie=1.0e300, brjs=-1.0e300, brje=1.0e300, ch_use=(1,) * 10)
    d.update(kw)
    p = H08Params()
    for k, v in d.items():
        if k == "ch_use":
            p.ch_use[:] = [int(x) for x in v]
        else:
            setattr(p, k, v)
    return p


_libs = {}


def _load(path, tables, restypes={}):
    """dlopen the library at path, once, and type every entry of the tables: a declared symbol that is missing raises
    AttributeError, and every entry returns int but those restypes names."""
    if path not in _libs:
        if not os.path.exists(path):
            raise LetkfError(f"{path} not built: run `make -C scale-letkf_amd` (no CPU fallback exists)")
        loaded = C.CDLL(path)
        for table in tables:
            for name, at in table.items():
                f = getattr(loaded, name)
                f.argtypes, f.restype = at, restypes.get(name, _INT)
        _libs[path] = loaded
    return _libs[path]


def lib():
    """dlopen the library.  `import torch` first when torch is in the process so both share one HIP runtime
    (torch's libamdhip64.so and /opt/rocm's carry the same SONAME; the first one loaded wins)."""
    if LIB_PATH not in _libs:
        try:            # make torch's HIP runtime the process's one BEFORE ours binds /opt/rocm's copy: loaded the other
            import torch  # noqa: F401  way round, the two runtimes coexist and ours sees no device
        except ImportError:
            pass
    return _load(LIB_PATH, (ARGTYPES, INTERP_ARGTYPES, INTERP_WINDOW_ARGTYPES, OBSOPE_ARGTYPES, MONIT_ARGTYPES), RESTYPES)


def osse_lib():
    """dlopen the library of the OSSE tools, after the main one whose context and operator it uses."""
    lib()
    return _load(OSSE_LIB_PATH, (OBSMAKE_ARGTYPES,))


def obssim_lib():
    """dlopen the library of the simulator, after the main one whose context it uses."""
    lib()
    return _load(OBSSIM_LIB_PATH, (OBSSIM_ARGTYPES,))


def superob_lib():
    """dlopen the library of superob, after the main one whose context it uses."""
    lib()
    return _load(SUPEROB_LIB_PATH, (SUPEROB_ARGTYPES,))


def obsscan_lib():
    """dlopen the library of the first scan, after the main one whose context and operator it uses."""
    lib()
    return _load(OBSSCAN_LIB_PATH, (OBSSCAN_ARGTYPES,))


def mapproj_lib():
    """dlopen the library of the map projection, after the main one whose context it uses."""
    lib()
    return _load(MAPPROJ_LIB_PATH, (MAPPROJ_SIGNATURES,))


def obsfile_lib():
    """dlopen the library of the record codec, after the main one whose context and scan it uses."""
    lib()
    return _load(OBSFILE_LIB_PATH, (OBSFILE_SIGNATURES,))


def nobsout_lib():
    """dlopen the library of NOBS_OUT, after the main one whose context and main loop it uses."""
    lib()
    return _load(NOBSOUT_LIB_PATH, (NOBSOUT_SIGNATURES,))


def tcvital_lib():
    """dlopen the library of the TC vitals, after the main one whose context and scratch buffer it uses."""
    lib()
    return _load(TCVITAL_LIB_PATH, (TCVITAL_SIGNATURES,))


def h08_lib():
    """dlopen the library of the Himawari-8 radiances, after the main one whose context, scratch buffer and scan it uses."""
    lib()
    return _load(H08_LIB_PATH, (H08_SIGNATURES,))


def h08_count(nbytes):
    """letkf_h08_count: the profiles of a Himawari-8 file of nbytes (ten rows each); LetkfError unless a whole number of records"""
    out = C.c_int64()
    rc = h08_lib().letkf_h08_count(nbytes, C.addressof(out))
    if rc != LETKF_OK:
        raise LetkfError(rc, lib().letkf_amd_last_error().decode())
    return out.value


def h08_bytes(nprof):
    """letkf_h08_bytes: the bytes of a Himawari-8 file of nprof profiles"""
    out = C.c_int64()
    rc = h08_lib().letkf_h08_bytes(nprof, C.addressof(out))
    if rc != LETKF_OK:
        raise LetkfError(rc, lib().letkf_amd_last_error().decode())
    return out.value


def _obsfile_size(entry, fmt, nrec, n):
    out = C.c_int64()
    rc = getattr(obsfile_lib(), entry)(fmt, nrec, n, C.addressof(out))
    if rc != LETKF_OK:
        raise LetkfError(f"{entry}: {lib().letkf_amd_last_error().decode()}")
    return out.value


def obsfile_count(fmt, nrec, nbytes):
    """letkf_obsfile_count: the rows of a file of nbytes (get_nobs / get_nobs_radar); raises where it is no whole number"""
    return _obsfile_size("letkf_obsfile_count", fmt, nrec, nbytes)


def obsfile_bytes(fmt, nrec, nrows):
    """letkf_obsfile_bytes: the bytes of a file image of nrows rows"""
    return _obsfile_size("letkf_obsfile_bytes", fmt, nrec, nrows)


def obsfile_rows(off, cols):
    """an ObsfileRows over the device columns of `cols` (a dict with OBSFILE_COLUMNS) and the HOST offsets off [nfile + 1]; the
    struct keeps both alive"""
    import numpy as np
    f = ObsfileRows()
    f._keep = (np.ascontiguousarray(off, dtype=np.int64), dict(cols))
    f.nfile, f.off = len(f._keep[0]) - 1, f._keep[0].ctypes.data
    for n in OBSFILE_COLUMNS:
        setattr(f, n, cols[n].data_ptr())
    return f


def mapproj_setup(basepoint_lon, basepoint_lat, basepoint_x, basepoint_y, lc_lat1, lc_lat2, cxg1, cyg1, dx, dy,
                  radius=MAPPROJ_RADIUS_SCALE, type=MAPPROJ_LC):
    """letkf_mapproj_setup: the derived constants (a Mapproj) of a Lambert conformal conic projection; degrees and metres"""
    p, proj = MapprojParams(), Mapproj()
    p.type = type
    (p.basepoint_lon, p.basepoint_lat, p.basepoint_x, p.basepoint_y, p.lc_lat1, p.lc_lat2, p.radius, p.cxg1, p.cyg1, p.dx,
     p.dy) = basepoint_lon, basepoint_lat, basepoint_x, basepoint_y, lc_lat1, lc_lat2, radius, cxg1, cyg1, dx, dy
    rc = mapproj_lib().letkf_mapproj_setup(C.addressof(p), C.addressof(proj))
    if rc != LETKF_OK:
        raise LetkfError(f"letkf_mapproj_setup: {lib().letkf_amd_last_error().decode()}")
    return proj


def _mapproj_host(entry, proj, a, b, rotc):
    u, v, r = C.c_double(), C.c_double(), (C.c_double * 2)()
    rc = getattr(mapproj_lib(), entry)(C.addressof(proj), a, b, C.addressof(u), C.addressof(v), C.addressof(r) if rotc else None)
    if rc != LETKF_OK:
        raise LetkfError(f"{entry}: {lib().letkf_amd_last_error().decode()}")
    return (u.value, v.value, (r[0], r[1])) if rotc else (u.value, v.value)


def phys2ij_host(proj, lon, lat, rotc=False):
    """letkf_phys2ij_host: (ri, rj) of one point in degrees, with rotc (ri, rj, (rotc0, rotc1))"""
    return _mapproj_host("letkf_phys2ij_host", proj, lon, lat, rotc)


def ij2phys_host(proj, ri, rj, rotc=False):
    """letkf_ij2phys_host: (lon, lat) in degrees of one point, with rotc (lon, lat, (rotc0, rotc1))"""
    return _mapproj_host("letkf_ij2phys_host", proj, ri, rj, rotc)


def obsscan_rows(bsna, slot_start, ip, islot=0):
    """letkf_obsscan_rows: (first, count) of the list rows of subdomain ip in slot islot (0: the whole subdomain); bsna is the
    int32 table (nprocs_d, nslots + 3) a scan returned"""
    import numpy as np
    t = np.ascontiguousarray(bsna, dtype=np.int32)
    first, count = C.c_int64(), C.c_int64()
    rc = obsscan_lib().letkf_obsscan_rows(t.ctypes.data, t.shape[0], slot_start, slot_start + t.shape[1] - 4, ip, islot,
                                          C.addressof(first), C.addressof(count))
    if rc != LETKF_OK:
        raise LetkfError(f"letkf_obsscan_rows: {lib().letkf_amd_last_error().decode()}")
    return first.value, count.value


def obsscan_slot_bounds(slot_start, slot_end, slot_base, slot_tinterval):
    """letkf_obsscan_slot_bounds: (slot_lb, slot_ub), float64 [nslots]"""
    import numpy as np
    lb, ub = (np.zeros(max(slot_end - slot_start + 1, 0)) for _ in range(2))
    rc = obsscan_lib().letkf_obsscan_slot_bounds(slot_start, slot_end, slot_base, slot_tinterval, lb.ctypes.data, ub.ctypes.data)
    if rc != LETKF_OK:
        raise LetkfError(f"letkf_obsscan_slot_bounds: {lib().letkf_amd_last_error().decode()}")
    return lb, ub


def superob_default_methods(nobtype, nid):
    """letkf_superob_default_methods: the reference's hard-coded tables as four int32 arrays (nid, nobtype): g, v, t, h"""
    import numpy as np
    tabs = [np.zeros((nid, nobtype), dtype=np.int32) for _ in range(4)]
    rc = superob_lib().letkf_superob_default_methods(nobtype, nid, *[t.ctypes.data for t in tabs])
    if rc != LETKF_OK:
        raise LetkfError(f"letkf_superob_default_methods: {lib().letkf_amd_last_error().decode()}")
    return tabs


def superob_slot_priority(nslots, nbslot):
    """letkf_superob_slot_priority: the 1-based slots, the nearest to nbslot first, the lower on ties"""
    import numpy as np
    out = np.zeros(max(nslots, 0), dtype=np.int32)
    rc = superob_lib().letkf_superob_slot_priority(nslots, nbslot, out.ctypes.data)
    if rc != LETKF_OK:
        raise LetkfError(f"letkf_superob_slot_priority: {lib().letkf_amd_last_error().decode()}")
    return out


class Rand:
    """letkf_rand (include/letkf_amd_obsmake.h): the SFMT19937 stream of a process's first init_gen_rand(seed), host state."""

    def __init__(self, seed):
        self._l = osse_lib()
        self._r = C.c_void_p()
        self._check(self._l.letkf_rand_create(int(seed), C.byref(self._r)))

    def _check(self, rc):
        if rc != LETKF_OK:
            raise LetkfError(f"letkf_amd error {rc}: {lib().letkf_amd_last_error().decode()}")

    def close(self):
        if self._r:
            self._l.letkf_rand_destroy(self._r)
            self._r = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_chunk(self, pairs):
        """pairs of uniforms per staging buffer of randn (the results do not depend on it)"""
        self._check(self._l.letkf_rand_set_chunk(self._r, pairs))

    def res53(self, n):
        """the next n values of genrand_res53 as a float64 numpy array (com_rand without its clock seeding)"""
        import numpy as np
        out = np.zeros(max(int(n), 0), dtype=np.float64)
        self._check(self._l.letkf_rand_res53(self._r, n, out.ctypes.data_as(C.c_void_p)))
        return out


def interp_coarse_axis(n, stride):
    """letkf_interp_coarse_axis (host only): the coarse indices of an axis of n points, as an int32 numpy array."""
    import numpy as np
    idx = np.zeros(max(int(n), 1), dtype=np.int32)
    cnt = C.c_int32(0)
    rc = lib().letkf_interp_coarse_axis(n, stride, idx.ctypes.data_as(C.c_void_p), C.byref(cnt))
    if rc != LETKF_OK:
        raise LetkfError(f"letkf_interp_coarse_axis: {rc}")
    return idx[:cnt.value].copy()


def interp_window_axis(gn, stride, g0, n, o0, on):
    """letkf_interp_window_axis (host only): the coarse lines of one axis that the owned range [o0, o0 + on) of arrays of n
    points at global index g0 needs, of a domain of gn points -- ascending array indices as an int32 numpy array.  Raises
    LetkfError where the entry refuses (a needed line outside the arrays among the reasons)."""
    import numpy as np
    idx = np.zeros(max(int(on), 0) + 2, dtype=np.int32)
    cnt = C.c_int32(0)
    rc = lib().letkf_interp_window_axis(gn, stride, g0, n, o0, on, idx.ctypes.data_as(C.c_void_p), C.byref(cnt))
    if rc != LETKF_OK:
        raise LetkfError(f"letkf_interp_window_axis: {rc}")
    return idx[:cnt.value].copy()


def monit_type(elem_uid, departure_stat_radar=False, departure_stat_h08=False):
    """letkf_monit_type (host only): which elements of elem_uid monit_obs reports, as an int32 numpy array of 0 / 1."""
    import numpy as np
    ids = np.ascontiguousarray(elem_uid, dtype=np.int32)
    out = np.zeros(len(ids), dtype=np.int32)
    rc = lib().letkf_monit_type(len(ids), ids.ctypes.data_as(C.c_void_p), int(bool(departure_stat_radar)),
                                int(bool(departure_stat_h08)), out.ctypes.data_as(C.c_void_p))
    if rc != LETKF_OK:
        raise LetkfError(f"letkf_monit_type: {rc}: {lib().letkf_amd_last_error().decode()}")
    return out


def _ptr(t):
    """device tensor -> void * (None: NULL)"""
    return None if t is None else C.c_void_p(t.data_ptr())


def _hptr(a):
    """host numpy array -> void * (None: NULL)"""
    return None if a is None else a.ctypes.data_as(C.c_void_p)


class Context:
    """One device + stream + workspace (letkf_ctx)."""

    def __init__(self, device=-1, stream=None):
        self._l = lib()
        self._c = C.c_void_p()
        self._check(self._l.letkf_ctx_create(device, C.byref(self._c)))
        if stream is not None:
            self.set_stream(stream)

    def _check(self, rc):
        if rc != LETKF_OK:
            raise LetkfError(f"letkf_amd error {rc}: {self._l.letkf_amd_last_error().decode()}")

    def close(self):
        if self._c:
            self._l.letkf_ctx_destroy(self._c)
            self._c = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_stream(self, stream_handle):
        self._check(self._l.letkf_ctx_set_stream(self._c, C.c_void_p(stream_handle)))

    OPT_STAGED_POLY = 1     # include/letkf_amd.h LETKF_OPT_STAGED_POLY
    OPT_COLUMN_SURVIVORS = 2   # LETKF_OPT_COLUMN_SURVIVORS
    OPT_LIMITED_RINGS = 3      # LETKF_OPT_LIMITED_RINGS
    OPT_RING_BATCH_MB = 4      # LETKF_OPT_RING_BATCH_MB
    OPT_RING_RELEASE = 5       # LETKF_OPT_RING_RELEASE
    OPT_SMALL_K_TRIO = 6       # LETKF_OPT_SMALL_K_TRIO

    def set_option(self, option, value):
        self._check(self._l.letkf_ctx_set_option(self._c, option, value))

    def synchronize(self):
        self._check(self._l.letkf_ctx_synchronize(self._c))

    def timing_enable(self, on=True):
        self._check(self._l.letkf_ctx_timing_enable(self._c, 1 if on else 0))

    def last_path(self):
        buf = C.create_string_buffer(256)
        self._check(self._l.letkf_ctx_last_path(self._c, buf, 256))
        return buf.value.decode()

    def timing_read(self, reset=True):
        avg = C.c_double(0.0)
        n = C.c_int64(0)
        self._check(self._l.letkf_ctx_timing_read(self._c, C.byref(avg), C.byref(n), 1 if reset else 0))
        return avg.value, n.value

    # ---- (1b) batched letkf_core on device tensors
    def core_batch(self, ne, nobs, nobsl, hdxb, rdiag, rloc, dep, parm_infl, trans, transm=None, pao=None,
                   depd=None, transmd=None, rdiag_wloc=False, infl_update=False, status=None, nsweep=None):
        a = CoreBatchArgs()
        a.ne, a.nobs, a.nbatch = ne, nobs, nobsl.numel()
        a.nobsl, a.hdxb, a.rdiag, a.rloc, a.dep = _ptr(nobsl), _ptr(hdxb), _ptr(rdiag), _ptr(rloc), _ptr(dep)
        a.depd, a.parm_infl, a.trans, a.transm = _ptr(depd), _ptr(parm_infl), _ptr(trans), _ptr(transm)
        a.pao, a.transmd = _ptr(pao), _ptr(transmd)
        a.rdiag_wloc, a.infl_update = int(bool(rdiag_wloc)), int(bool(infl_update))
        a.status, a.nsweep = _ptr(status), _ptr(nsweep)
        self._check(self._l.letkf_core_batch_dev(self._c, C.byref(a)))

    # ---- (2) das_letkf point update on device tensors
    def _das_args(self, k, nv, npts, ensval, kld, dep, infl, gues, anal, sp, sm, sv, beta, det_run, infl_adaptive,
                  relax_to_inflated_prior, relax_alpha, relax_alpha_spread, q_update_top, q_sprd_max, iv_p, iv_q_first,
                  iv_q_last, status, nsweep, rtps_infl_out, warm_run, var_mask, infl_sv):
        """the letkf_das_args both loop-body entries share; the lists, the k x k outputs and warm_stride stay NULL / 0"""
        a = DasArgs()
        a.k, a.nv, a.det_run, a.infl_adaptive = k, nv, int(bool(det_run)), int(bool(infl_adaptive))
        a.relax_to_inflated_prior = int(bool(relax_to_inflated_prior))
        a.iv_p, a.iv_q_first, a.iv_q_last = iv_p, iv_q_first, iv_q_last
        a.relax_alpha, a.relax_alpha_spread = relax_alpha, relax_alpha_spread
        a.q_update_top, a.q_sprd_max, a.npts = q_update_top, q_sprd_max, npts
        a.ensval, a.kld, a.dep, a.beta, a.infl = _ptr(ensval), kld, _ptr(dep), _ptr(beta), _ptr(infl)
        a.gues, a.anal, a.sp, a.sm, a.sv = _ptr(gues), _ptr(anal), sp, sm, sv
        a.status, a.nsweep, a.rtps_infl_out = _ptr(status), _ptr(nsweep), _ptr(rtps_infl_out)
        a.warm_run, a.var_mask, a.infl_sv = int(warm_run), int(var_mask), int(infl_sv)
        return a

    def das_points(self, k, nv, obs_off, obs_idx, rdiag_l, rloc_l, ensval, kld, dep, infl, gues, anal, sp, sm, sv,
                   beta=None, det_run=False, infl_adaptive=False, relax_to_inflated_prior=False, relax_alpha=0.0,
                   relax_alpha_spread=0.0, q_update_top=0.0, q_sprd_max=0.0, iv_p=4, iv_q_first=5, iv_q_last=10,
                   trans_out=None, transm_out=None, pa_out=None, status=None, nsweep=None, rtps_infl_out=None,
                   warm_run=0, var_mask=0, fused=None, nobs_out=None, warm_stride=0, infl_sv=0):
        """fused = (tables, ri, rj, rlev, rz): obs_local fused into the kernel (obs_off .. rloc_l may be None)"""
        a = self._das_args(k, nv, (obs_off.numel() - 1) if fused is None else fused[1].numel(), ensval, kld, dep, infl, gues,
                           anal, sp, sm, sv, beta, det_run, infl_adaptive, relax_to_inflated_prior, relax_alpha,
                           relax_alpha_spread, q_update_top, q_sprd_max, iv_p, iv_q_first, iv_q_last, status, nsweep,
                           rtps_infl_out, warm_run, var_mask, infl_sv)
        a.obs_off, a.obs_idx, a.rdiag_l, a.rloc_l = _ptr(obs_off), _ptr(obs_idx), _ptr(rdiag_l), _ptr(rloc_l)
        a.trans_out, a.transm_out, a.pa_out, a.warm_stride = _ptr(trans_out), _ptr(transm_out), _ptr(pa_out), int(warm_stride)
        if fused is None:
            self._check(self._l.letkf_das_points_dev(self._c, C.byref(a)))
        else:
            t, ri, rj, rlev, rz = fused
            self._check(self._l.letkf_das_points_fused_dev(self._c, C.byref(a), C.byref(t), _ptr(ri), _ptr(rj),
                                                           _ptr(rlev), _ptr(rz), _ptr(nobs_out)))

    def das_columns(self, k, nv, tables, nij1, nlev, rig, rjg, rlev, rz, ensval, kld, dep, infl, gues, anal, sp, sm, sv,
                    list_bytes=0, nobs_out=None, beta=None, det_run=False, infl_adaptive=False, relax_to_inflated_prior=False,
                    relax_alpha=0.0, relax_alpha_spread=0.0, q_update_top=0.0, q_sprd_max=0.0, iv_p=4, iv_q_first=5,
                    iv_q_last=10, status=None, nsweep=None, rtps_infl_out=None, warm_run=0, var_mask=0, infl_sv=0):
        """letkf_das_columns_dev: obs_local + loop body for the points p = ij + nij1*lev -- list-free where the one-wave kernel
        serves the call (horizontal survivors per column, batches of columns that fit list_bytes), else by slabs of levels whose
        lists fit list_bytes of library workspace."""
        a = self._das_args(k, nv, nij1 * nlev, ensval, kld, dep, infl, gues, anal, sp, sm, sv, beta, det_run, infl_adaptive,
                           relax_to_inflated_prior, relax_alpha, relax_alpha_spread, q_update_top, q_sprd_max, iv_p, iv_q_first,
                           iv_q_last, status, nsweep, rtps_infl_out, warm_run, var_mask, infl_sv)
        self._check(self._l.letkf_das_columns_dev(self._c, C.byref(a), C.byref(tables), nij1, nlev, _ptr(rig), _ptr(rjg),
                                                  _ptr(rlev), _ptr(rz), list_bytes, _ptr(nobs_out)))

    def das_columns_nobs(self, k, nv, tables, nij1, nlev, rig, rjg, rlev, rz, ensval, kld, dep, infl, gues, anal, sp, sm, sv,
                         list_bytes=0, nobs_out=None, beta=None, det_run=False, infl_adaptive=False, relax_to_inflated_prior=False,
                         relax_alpha=0.0, relax_alpha_spread=0.0, q_update_top=0.0, q_sprd_max=0.0, iv_p=4, iv_q_first=5,
                         iv_q_last=10, status=None, nsweep=None, rtps_infl_out=None, warm_run=0, var_mask=0, infl_sv=0,
                         nobs_ctype=None, cutd_ctype=None):
        """letkf_das_columns_nobs_dev (include/letkf_amd_nobsout.h): das_columns with the NOBS_OUT diagnostics of its points,
        nobs_ctype int32 / cutd_ctype float64 [nij1*nlev][nctype] (either may be None), out of the search passes the call runs
        anyway; zeros where beta = 0."""
        a = self._das_args(k, nv, nij1 * nlev, ensval, kld, dep, infl, gues, anal, sp, sm, sv, beta, det_run, infl_adaptive,
                           relax_to_inflated_prior, relax_alpha, relax_alpha_spread, q_update_top, q_sprd_max, iv_p, iv_q_first,
                           iv_q_last, status, nsweep, rtps_infl_out, warm_run, var_mask, infl_sv)
        self._check(nobsout_lib().letkf_das_columns_nobs_dev(self._c, C.addressof(a), C.addressof(tables), nij1, nlev, _ptr(rig),
                                                             _ptr(rjg), _ptr(rlev), _ptr(rz), list_bytes, _ptr(nobs_out),
                                                             _ptr(nobs_ctype), _ptr(cutd_ctype)))

    def nobs_fields(self, npts, elm_u_ctype, typ_ctype, nobs_ctype, cutd_ctype=None, work3dn=None, fields=None, sp=1, sv=None,
                    nobtype=24, uid_ref=9, uid_re0=10, uid_vr=11, typ_radar=22, pick=(1, 3, 4, 8, 22)):
        """letkf_nobs_fields_dev (include/letkf_amd_nobsout.h): work3dn [npts][nobtype + 6] and / or the eleven fields, element
        (p, f) at p*sp + f*sv (sv = None: npts, the (nij1, nlev, 11) array), from the diagnostics of das_columns_nobs;
        elm_u_ctype / typ_ctype are host sequences (1-based, as obs_table_info gives them)."""
        import numpy as np
        eu = np.ascontiguousarray(elm_u_ctype, dtype=np.int32)
        ty = np.ascontiguousarray(typ_ctype, dtype=np.int32)
        p = NobsoutParams()
        p.nctype, p.nobtype = len(eu), nobtype
        p.uid_ref, p.uid_re0, p.uid_vr, p.typ_radar = uid_ref, uid_re0, uid_vr, typ_radar
        p.pick = (C.c_int32 * 5)(*[int(v) for v in pick])
        p.elm_u_ctype, p.typ_ctype = eu.ctypes.data, ty.ctypes.data
        self._check(nobsout_lib().letkf_nobs_fields_dev(self._c, C.addressof(p), npts, _ptr(nobs_ctype), _ptr(cutd_ctype), _ptr(work3dn),
                                                        _ptr(fields), sp, npts if sv is None else sv))

    def tcvital_rows(self, elm, dif, slot_lb, slot_ub, n=None):
        """letkf_tcvital_rows_dev (include/letkf_amd_tcvital.h): the last 1-based rows of the TCX / TCY / TCP elements among the
        decoded columns elm (int32) and dif (float64) of one file, 0 where there is none, and whether they are one report of the
        slot (slot_lb, slot_ub].  Returns (rows int64 [3], valid)."""
        import numpy as np
        rows, valid = np.full(3, -1, dtype=np.int64), C.c_int32(-1)
        self._check(tcvital_lib().letkf_tcvital_rows_dev(self._c, elm.numel() if n is None else n, _ptr(elm), _ptr(dif), slot_lb,
                                                         slot_ub, _hptr(rows), C.addressof(valid)))
        return rows, bool(valid.value)

    def tcvital_search(self, params, fields, ritc, rjtc, cand=None):
        """letkf_tcvital_search_dev: (tcx, tcy, mslp) of the lowest smoothed sea-level pressure within params.tc_search_dis of the
        grid coordinates ritc / rjtc (device tensors of one float64 each) for the fields.nmem members of one subdomain, 9.99e33
        thrice where there is none.  params: TcvitalParams; fields: ObsopeFields (v2d, its strides, sizes and halos are read).
        Returns cand float64 [nmem, 3] (or writes into the one given)."""
        import torch
        if cand is None:
            cand = torch.empty((fields.nmem, 3), dtype=torch.float64, device=ritc.device)
        self._check(tcvital_lib().letkf_tcvital_search_dev(self._c, C.addressof(params), C.addressof(fields), _ptr(ritc), _ptr(rjtc),
                                                           _ptr(cand)))
        return cand

    def tcvital_fill(self, cand_all, rows, qc, ensval, kld, m0=0, qc_replace=True, nproc=None, nmem=None):
        """letkf_tcvital_fill_dev: cand_all float64 [nproc, nmem, 3] (every rank's candidates) to the obsda rows `rows` (0-based
        TCX, TCY, TCP; negative: not on this rank): per member the lowest rank among those with the lowest mslp below 1100 hPa
        into ensval[row, m0 + m], undef without one; qc 50 on the rows if any member has none, else 0 (qc_replace) or merged by
        maximum."""
        import numpy as np
        r = np.ascontiguousarray(rows, dtype=np.int64)
        nproc = cand_all.shape[0] if nproc is None else nproc
        nmem = cand_all.shape[1] if nmem is None else nmem
        self._check(tcvital_lib().letkf_tcvital_fill_dev(self._c, nproc, nmem, m0, _ptr(cand_all), _hptr(r), int(qc_replace), _ptr(qc),
                                                         _ptr(ensval), kld))

    # ---- the Himawari-8 radiances (include/letkf_amd_h08.h)
    def h08_decode(self, image, obserr, big_endian=False, want=OBSFILE_COLUMNS, check=False, out=None, nprof=None):
        """letkf_h08_decode_dev: a Himawari-8 file image to a dict of the columns of `want`, ten rows per profile (lev = 7 .. 16,
        err = obserr[channel], dif = 0), with "nbad" (check=True).  `out`: a dict of tensors to write into."""
        import numpy as np
        import torch
        n = h08_count(self._image_bytes(image)) if nprof is None else nprof
        if out is None:
            out = {k: torch.empty(n * H08_NCH, dtype=torch.int32 if k in ("elm", "typ") else torch.float64, device=image.device)
                   if k in want else None for k in OBSFILE_COLUMNS}
        o = ObsfileCols()
        for k in OBSFILE_COLUMNS:
            setattr(o, k, _ptr(out.get(k)))
        e = np.ascontiguousarray(obserr, dtype=np.float64)
        assert e.size == H08_NCH
        nbad = C.c_int64(-1)
        self._check(h08_lib().letkf_h08_decode_dev(self._c, int(big_endian), _ptr(image), n, _hptr(e), C.addressof(o),
                                                   C.addressof(nbad) if check else None))
        res = dict(out)
        res["nbad"] = nbad.value if check else None
        return res

    def h08_encode(self, cols, big_endian=False, out=None, nprof=None):
        """letkf_h08_encode_dev: the columns (a dict of device tensors, ten rows per profile) to the file image, a uint8 device
        tensor: per profile elm, typ, lon, lat of its first row and the dat of its ten rows."""
        import torch
        n = cols["dat"].numel() // H08_NCH if nprof is None else nprof
        c = ObsfileCols()
        for k in OBSFILE_COLUMNS:
            setattr(c, k, _ptr(cols.get(k)))
        if out is None:
            out = torch.empty(h08_bytes(n), dtype=torch.uint8, device=cols["dat"].device)
        self._check(h08_lib().letkf_h08_encode_dev(self._c, int(big_endian), n, C.addressof(c), _ptr(out)))
        return out

    def h08_select(self, set_, idx, h08_set, nprof_file, row0=0, nrows=None, prof_list=None, slot_of_prof=None):
        """letkf_h08_select_dev: the profiles of file h08_set (1-based) that the obsda rows [row0, row0 + nrows) name.  Returns
        (prof_list int32 [nprof_file] of which the first nsel are written, ascending; slot_of_prof int32 [nprof_file], -1 where
        not selected; nsel)."""
        import torch
        nrows = set_.numel() - row0 if nrows is None else nrows
        if prof_list is None:
            prof_list = torch.full((nprof_file,), -1, dtype=torch.int32, device=set_.device)
        if slot_of_prof is None:
            slot_of_prof = torch.empty(nprof_file, dtype=torch.int32, device=set_.device)
        nsel = C.c_int64(-1)
        self._check(h08_lib().letkf_h08_select_dev(self._c, _ptr(set_), _ptr(idx), row0, nrows, h08_set, nprof_file, _ptr(prof_list),
                                                   _ptr(slot_of_prof), C.addressof(nsel)))
        return prof_list, slot_of_prof, nsel.value

    def h08_profiles(self, params, fields, nsel, prof_list, ri, rj, lon, lat, rotc=None, out=None):
        """letkf_h08_profiles_dev: the profile arrays of the fields.nmem members at the nsel profiles of prof_list; ri, rj, lon,
        lat (and rotc [., 2]) are per FILE profile.  params: H08Params; fields: ObsopeFields.  Returns a dict lev3 [nmem, nsel, 5,
        nlev], sfc [nmem, nsel, 8], pflag int32 [nsel] and, under params.rttov_units, cloud [nmem, nsel, 3, nlev - 1] (else None);
        or writes into the dict given."""
        import torch
        nmem, nlev, dev = fields.nmem, fields.nlev, prof_list.device
        if out is None:
            out = dict(lev3=torch.empty((nmem, nsel, 5, nlev), dtype=torch.float64, device=dev),
                       sfc=torch.empty((nmem, nsel, 8), dtype=torch.float64, device=dev),
                       cloud=torch.empty((nmem, nsel, 3, nlev - 1), dtype=torch.float64, device=dev) if params.rttov_units else None,
                       pflag=torch.empty(nsel, dtype=torch.int32, device=dev))
        o = H08Profiles()
        for k, _ in H08Profiles._fields_:
            setattr(o, k, _ptr(out.get(k)))
        self._check(h08_lib().letkf_h08_profiles_dev(self._c, C.addressof(params), C.addressof(fields), nsel, _ptr(prof_list), _ptr(ri),
                                                     _ptr(rj), _ptr(lon), _ptr(lat), _ptr(rotc), C.addressof(o)))
        return out

    def h08_rows(self, params, set_, idx, h08_set, slot_of_prof, nsel, prof, btall, btclr, trans, rig, rjg, qc, ensval, kld, lev, val2,
                 nmem=None, m0=0, qc_replace=True, row0=0, nrows=None):
        """letkf_h08_rows_dev: the obsda rows [row0, row0 + nrows) of file h08_set whose profile is selected, from the radiative
        transfer's btall, btclr [nmem, nsel, 10] and trans [nmem, nsel, 10, nlev] and the dict `prof` of h08_profiles: ensval[row,
        m0 + m], qc (replaced or merged by maximum), lev += the weighting function's peak, val2 += btclr, member after member,
        divided by params.member where params.finish."""
        nrows = set_.numel() - row0 if nrows is None else nrows
        nmem = btall.shape[0] if nmem is None else nmem
        self._check(h08_lib().letkf_h08_rows_dev(self._c, C.addressof(params), row0, nrows, _ptr(set_), _ptr(idx), h08_set,
                                                 _ptr(slot_of_prof), nsel, nmem, m0, _ptr(prof["lev3"]), _ptr(prof["sfc"]),
                                                 _ptr(prof["pflag"]), _ptr(btall), _ptr(btclr), _ptr(trans), _ptr(rig), _ptr(rjg),
                                                 int(qc_replace), _ptr(qc), _ptr(ensval), kld, _ptr(lev), _ptr(val2)))

    def das_interp(self, k, nv, tables, nx, ny, nlev, stride_x, stride_y, rig, rjg, rlev, rz, ensval, kld, dep, infl, gues,
                   anal, sp, sm, sv, ws_bytes=0, nobs_coarse=None, npts=None, beta=None, det_run=False, infl_adaptive=False,
                   relax_to_inflated_prior=False, relax_alpha=0.0, relax_alpha_spread=0.0, q_update_top=0.0, q_sprd_max=0.0,
                   iv_p=4, iv_q_first=5, iv_q_last=10, status=None, nsweep=None, rtps_infl_out=None, var_mask=0, infl_sv=0,
                   trans_out=None, transm_out=None, pa_out=None):
        """letkf_das_interp_dev (include/letkf_amd_interp.h): letkf_core on every stride-th column of the nx x ny x nlev tile
        (point p = i + nx*j + nx*ny*lev), T and w-bar interpolated bilinearly, the loop body's rules at every point.  npts,
        infl_adaptive, nsweep and the k x k outputs only reach the entry's argument checks, which refuse them."""
        a = self._das_args(k, nv, nx * ny * nlev if npts is None else npts, ensval, kld, dep, infl, gues, anal, sp, sm, sv,
                           beta, det_run, infl_adaptive, relax_to_inflated_prior, relax_alpha, relax_alpha_spread, q_update_top,
                           q_sprd_max, iv_p, iv_q_first, iv_q_last, status, nsweep, rtps_infl_out, 0, var_mask, infl_sv)
        a.trans_out, a.transm_out, a.pa_out = _ptr(trans_out), _ptr(transm_out), _ptr(pa_out)
        i = InterpArgs()
        i.nx, i.ny, i.nlev, i.stride_x, i.stride_y, i.ws_bytes = nx, ny, nlev, stride_x, stride_y, int(ws_bytes)
        i.rig, i.rjg, i.rlev, i.rz, i.nobs_coarse = _ptr(rig), _ptr(rjg), _ptr(rlev), _ptr(rz), _ptr(nobs_coarse)
        self._check(self._l.letkf_das_interp_dev(self._c, C.byref(a), C.byref(tables), C.byref(i)))

    def das_interp_window(self, k, nv, tables, nx, ny, nlev, stride_x, stride_y, rig, rjg, rlev, rz, ensval, kld, dep,
                          infl, gues, anal, sp, sm, sv, window=None, ws_bytes=0, nobs_coarse=None, npts=None, beta=None, det_run=False,
                          infl_adaptive=False, relax_to_inflated_prior=False, relax_alpha=0.0, relax_alpha_spread=0.0,
                          q_update_top=0.0, q_sprd_max=0.0, iv_p=4, iv_q_first=5, iv_q_last=10, status=None, nsweep=None,
                          rtps_infl_out=None, var_mask=0, infl_sv=0, trans_out=None, transm_out=None, pa_out=None):
        """letkf_das_interp_window_dev (include/letkf_amd_interp_window.h): das_interp's arguments, with nx, ny, nlev the
        extents of the arrays handed in, and the window (an InterpWindow, a tuple (gnx, gny, gi0, gj0, oi0, oj0, onx, ony), or
        None for the whole arrays as the whole domain): the coarse lattice is the domain's, the owned rectangle is analysed,
        and of the halo only the coarse columns interp_window_axis names are read."""
        a = self._das_args(k, nv, nx * ny * nlev if npts is None else npts, ensval, kld, dep, infl, gues, anal, sp, sm, sv,
                           beta, det_run, infl_adaptive, relax_to_inflated_prior, relax_alpha, relax_alpha_spread, q_update_top,
                           q_sprd_max, iv_p, iv_q_first, iv_q_last, status, nsweep, rtps_infl_out, 0, var_mask, infl_sv)
        a.trans_out, a.transm_out, a.pa_out = _ptr(trans_out), _ptr(transm_out), _ptr(pa_out)
        i = InterpArgs()
        i.nx, i.ny, i.nlev, i.stride_x, i.stride_y, i.ws_bytes = nx, ny, nlev, stride_x, stride_y, int(ws_bytes)
        i.rig, i.rjg, i.rlev, i.rz, i.nobs_coarse = _ptr(rig), _ptr(rjg), _ptr(rlev), _ptr(rz), _ptr(nobs_coarse)
        if window is not None and not isinstance(window, InterpWindow):
            window = InterpWindow(*[int(v) for v in window])
        self._check(self._l.letkf_das_interp_window_dev(self._c, C.byref(a), C.byref(tables), C.byref(i),
                                                        None if window is None else C.byref(window)))

    # ---- (3) obs_local on the device: two-phase CSR build (count, scan, fill)
    def _csr_lists(self, npts, device, search):
        """Count pass, counts -> offsets, the three list tensors, fill pass.  search(fill, counts, obs_off, obs_idx, rdiag_l,
        rloc_l) makes one call of a search entry; returns (obs_off, obs_idx, rdiag_l, rloc_l)."""
        import torch
        counts = torch.zeros(npts, dtype=torch.int32, device=device)
        search(0, counts, None, None, None, None)
        obs_off = torch.zeros(npts + 1, dtype=torch.int64, device=device)
        obs_off[1:] = torch.cumsum(counts.to(torch.int64), 0)
        nnz = int(obs_off[-1].item())
        obs_idx, rdiag, rloc = (torch.empty(max(nnz, 1), dtype=t, device=device)
                                for t in (torch.int32, torch.float64, torch.float64))
        search(1, None, obs_off, obs_idx, rdiag, rloc)
        return obs_off, obs_idx[:nnz], rdiag[:nnz], rloc[:nnz]

    def obs_search(self, tables, ri, rj, rlev, rz):
        """Returns (obs_off, obs_idx, rdiag_l, rloc_l) device tensors for the points (ri, rj, rlev, rz)."""
        def search(fill, counts, obs_off, obs_idx, rdiag, rloc):
            self._check(self._l.letkf_obs_search_dev(self._c, C.byref(tables), ri.numel(), _ptr(ri), _ptr(rj), _ptr(rlev),
                                                     _ptr(rz), fill, _ptr(counts), _ptr(obs_off), _ptr(obs_idx), _ptr(rdiag),
                                                     _ptr(rloc)))
        return self._csr_lists(ri.numel(), ri.device, search)

    def obs_search_columns(self, tables, nij1, nlev, rig, rjg, rlev, rz, nobs_ctype=None, cutd_ctype=None):
        """Column-cooperative obs_local for points p = ij + nij1*lev; same return as obs_search."""
        def search(fill, counts, obs_off, obs_idx, rdiag, rloc):
            nobs_c, cutd_c = (nobs_ctype, cutd_ctype) if fill else (None, None)   # (diagnostics with the fill pass: the count
            self._check(self._l.letkf_obs_search_columns_dev(                       # pass then needs no selection)
                self._c, C.byref(tables), nij1, nlev, _ptr(rig), _ptr(rjg), _ptr(rlev), _ptr(rz), fill, _ptr(counts),
                _ptr(obs_off), _ptr(obs_idx), _ptr(rdiag), _ptr(rloc), _ptr(nobs_c), _ptr(cutd_c)))
        return self._csr_lists(nij1 * nlev, rig.device, search)

    # ---- (10) EFSO: das_efso's loop on device tensors
    def _efso_args(self, k, nv, term_of_var, nterm, npts, ensval, kld, nobs, fcst, sp, sm, sv, fcer, fsp, fsv, djdy,
                   var_mask, obs_off=None, obs_idx=None, rdiag_l=None, rloc_l=None, pair_bytes=0):
        import numpy as np
        tv = np.ascontiguousarray(np.asarray(term_of_var, dtype=np.int32))
        a = EfsoArgs()
        a.k, a.nv, a.nterm, a.var_mask = k, nv, nterm, int(var_mask)
        a.term_of_var = tv.ctypes.data if tv.size else None
        a.npts = npts
        a.obs_off, a.obs_idx, a.rdiag_l, a.rloc_l = _ptr(obs_off), _ptr(obs_idx), _ptr(rdiag_l), _ptr(rloc_l)
        a.ensval, a.kld, a.nobs = _ptr(ensval), kld, nobs
        a.fcst, a.sp, a.sm, a.sv = _ptr(fcst), sp, sm, sv
        a.fcer, a.fsp, a.fsv = _ptr(fcer), fsp, fsv
        a.djdy, a.pair_bytes = _ptr(djdy), int(pair_bytes)
        return a, tv

    def efso_points(self, k, nv, term_of_var, nterm, obs_off, obs_idx, rdiag_l, rloc_l, ensval, kld, nobs, fcst, sp, sm, sv,
                    fcer, fsp, fsv, djdy, var_mask=0, pair_bytes=0):
        """letkf_efso_points_dev: djdy[j*nterm + t] += das_efso's contributions of the points of the CSR lists (INOUT)."""
        a, keep = self._efso_args(k, nv, term_of_var, nterm, obs_off.numel() - 1, ensval, kld, nobs, fcst, sp, sm, sv, fcer,
                                  fsp, fsv, djdy, var_mask, obs_off, obs_idx, rdiag_l, rloc_l, pair_bytes)
        self._check(self._l.letkf_efso_points_dev(self._c, C.byref(a)))

    def efso_columns(self, k, nv, term_of_var, nterm, tables, nij1, nlev, rig, rjg, rlev, rz, ensval, kld, nobs, fcst, sp, sm,
                     sv, fcer, fsp, fsv, djdy, var_mask=0, list_bytes=0):
        """letkf_efso_columns_dev: the column search and EFSO for the points p = ij + nij1*lev, by slabs of levels."""
        a, keep = self._efso_args(k, nv, term_of_var, nterm, nij1 * nlev, ensval, kld, nobs, fcst, sp, sm, sv, fcer, fsp, fsv,
                                  djdy, var_mask)
        self._check(self._l.letkf_efso_columns_dev(self._c, C.byref(a), C.byref(tables), nij1, nlev, _ptr(rig), _ptr(rjg),
                                                   _ptr(rlev), _ptr(rz), list_bytes))

    def efso_obsense(self, nterm, djdy, dep, obsense):
        """letkf_efso_obsense_dev: obsense[j*nterm + t] = djdy[j*nterm + t] * dep[j]."""
        self._check(self._l.letkf_efso_obsense_dev(self._c, nterm, dep.numel(), _ptr(djdy), _ptr(dep), _ptr(obsense)))

    # ---- (12) EFSO with localisation advection
    def efso_locadv(self, rig, rjg, nlev, u0, v0, u1, v1, locadv_rate, eft, dx, dy, ri=None, rj=None):
        """letkf_efso_locadv_dev: the advected search positions (ri, rj) [nij1*nlev] of the points p = ij + nij1*lev,
        ri = rig[ij] - (0.5 (u0 + u1)) * locadv_rate*eft*3600/dx (rj likewise with v, dy); allocated when not given."""
        import torch
        nij1 = rig.numel()
        if ri is None:
            ri = torch.empty(nij1 * nlev, dtype=torch.float64, device=rig.device)
        if rj is None:
            rj = torch.empty(nij1 * nlev, dtype=torch.float64, device=rig.device)
        self._check(self._l.letkf_efso_locadv_dev(self._c, nij1, nlev, _ptr(rig), _ptr(rjg), _ptr(u0), _ptr(v0), _ptr(u1),
                                                  _ptr(v1), locadv_rate, eft, dx, dy, _ptr(ri), _ptr(rj)))
        return ri, rj

    def efso_search(self, k, nv, term_of_var, nterm, tables, ri, rj, rlev, rz, ensval, kld, nobs, fcst, sp, sm, sv, fcer, fsp,
                    fsv, djdy, var_mask=0, list_bytes=0, npts=None):
        """letkf_efso_search_dev: the point search and EFSO at per-point positions, in runs of points that fit list_bytes
        (npts: the count passed beside args->npts = ri.numel(), for argument checks)."""
        n = ri.numel() if ri is not None else int(npts)
        a, keep = self._efso_args(k, nv, term_of_var, nterm, n, ensval, kld, nobs, fcst, sp, sm, sv, fcer, fsp, fsv, djdy,
                                  var_mask)
        self._check(self._l.letkf_efso_search_dev(self._c, C.byref(a), C.byref(tables), n if npts is None else npts, _ptr(ri),
                                                  _ptr(rj), _ptr(rlev), _ptr(rz), int(list_bytes)))

    # ---- (13) EFSO's forecast-error norm and impact summary
    def efso_norm(self, prm, nij1, nlev, fcst, sp, sm, sv, fcer, fsp, fsv, fmean=None, xf=None, xg=None, xa=None, wlev=None,
                  wg1=None, lon=None, lat=None):
        """letkf_efso_norm_dev: fcst (total fields in, C^1/2 X^f out) and fcer (C^1/2 times the error, assembled from xf, xg,
        xa when given) in place; prm an EfsoNormParams; fmean [npts*nv] written when given."""
        self._check(self._l.letkf_efso_norm_dev(self._c, C.byref(prm), nij1, nlev, _ptr(fcst), sp, sm, sv, _ptr(fmean),
                                                _ptr(fcer), fsp, fsv, _ptr(xf), _ptr(xg), _ptr(xa), _ptr(wlev), _ptr(wg1),
                                                _ptr(lon), _ptr(lat)))

    def efso_summary(self, nterm, obsense, elm, typ, lat, elem_uid, nobtype, latbound=20.0, qc=None, nobs=None, outs=None):
        """letkf_efso_summary_dev: print_obsense's table; returns (count int32 [3][nobtype+1][nid], sum [nterm][3][nobtype+1][nid],
        nneg int32, same shape) device tensors (outs: the three to write instead)."""
        import numpy as np
        import torch
        ids = np.ascontiguousarray(elem_uid, dtype=np.int32)
        nid = len(ids)
        n = (obsense.numel() // nterm if obsense is not None else 0) if nobs is None else nobs
        if outs is None:
            d = obsense.device if obsense is not None else torch.device("cuda")
            shape = (3, nobtype + 1, max(nid, 1))
            outs = (torch.empty(shape, dtype=torch.int32, device=d), torch.empty((nterm,) + shape, dtype=torch.float64, device=d),
                    torch.empty((nterm,) + shape, dtype=torch.int32, device=d))
        count, ssum, nneg = outs
        self._check(self._l.letkf_efso_summary_dev(self._c, nterm, n, _ptr(obsense), _ptr(elm), _ptr(typ), _ptr(lat), _ptr(qc),
                                                   nid, _hptr(ids) if nid else None, nobtype, latbound, _ptr(count), _ptr(ssum),
                                                   _ptr(nneg)))
        return count, ssum, nneg

    # ---- (11) das_letkf_obs: the analysis ensemble in observation space
    def das_obs(self, k, tvar, tables, ensval, kld, dep, nobs, ya, lda=None, tgt_row=None, ntgt=None, ya_mean=None,
                ya_table=None, dep_a=None, nobs_out=None, status=None, rlev_tgt=None, rz_tgt=None, beta=None, infl=None,
                infl_mul=1.0, det_run=False, relax_to_inflated_prior=False, relax_alpha=0.0, relax_alpha_spread=0.0,
                q_update_top=0.0, q_sprd_max=0.0, iv_q_first=5, iv_q_last=10, list_bytes=0):
        """letkf_das_obs_dev: the LETKF at every target row's own location (tgt_row None: rows 0..ntgt-1, ntgt = nobs by
        default); ya [ntgt][lda] the analysis members, the other outputs optional."""
        a = DasObsArgs()
        a.k, a.det_run, a.tvar = k, int(bool(det_run)), int(tvar)
        a.relax_to_inflated_prior = int(bool(relax_to_inflated_prior))
        a.iv_q_first, a.iv_q_last = iv_q_first, iv_q_last
        a.relax_alpha, a.relax_alpha_spread, a.q_update_top, a.q_sprd_max = relax_alpha, relax_alpha_spread, q_update_top, q_sprd_max
        a.ntgt = tgt_row.numel() if tgt_row is not None else (nobs if ntgt is None else ntgt)
        a.tgt_row, a.ensval, a.kld, a.dep, a.nobs = _ptr(tgt_row), _ptr(ensval), kld, _ptr(dep), nobs
        a.rlev_tgt, a.rz_tgt, a.beta, a.infl, a.infl_mul = _ptr(rlev_tgt), _ptr(rz_tgt), _ptr(beta), _ptr(infl), infl_mul
        a.ya, a.lda = _ptr(ya), (k + (1 if det_run else 0)) if lda is None else lda
        a.ya_mean, a.ya_table, a.dep_a = _ptr(ya_mean), _ptr(ya_table), _ptr(dep_a)
        a.nobs_out, a.status, a.list_bytes = _ptr(nobs_out), _ptr(status), int(list_bytes)
        self._check(self._l.letkf_das_obs_dev(self._c, C.byref(a), C.byref(tables)))

    # ---- (5) set_letkf_obs on the device
    def obs_departure(self, params, elm, dat, err, ensval, kld, val, qc):
        self._check(self._l.letkf_obs_departure_dev(self._c, C.byref(params), elm.numel(), _ptr(elm), _ptr(dat), _ptr(err),
                                                    _ptr(ensval), kld, _ptr(val), _ptr(qc)))

    def obs_mesh_sort(self, mesh, ncell, ctype, ri, rj, qc):
        """Returns (n_cell [ncell] int32, key [nsorted] int32) device tensors."""
        import torch
        nobs = ctype.numel()
        n_cell = torch.zeros(max(ncell, 1), dtype=torch.int32, device=ctype.device)
        key = torch.empty(max(nobs, 1), dtype=torch.int32, device=ctype.device)
        ns = C.c_int64(0)
        self._check(self._l.letkf_obs_mesh_sort_dev(self._c, C.byref(mesh), nobs, _ptr(ctype), _ptr(ri), _ptr(rj), _ptr(qc),
                                                    _ptr(n_cell), _ptr(key), C.byref(ns)))
        return n_cell[:ncell], key[:ns.value]

    def obs_halo_plan(self, layout, n_all, nacx, cap):
        """Returns (ac_ext [nacx] int32, src_row [nobstotal] int32) device tensors."""
        import torch
        ac_ext = torch.zeros(max(nacx, 1), dtype=torch.int32, device=n_all.device)
        src_row = torch.empty(max(cap, 1), dtype=torch.int32, device=n_all.device)
        nt = C.c_int64(0)
        self._check(self._l.letkf_obs_halo_plan_dev(self._c, C.byref(layout), _ptr(n_all), _ptr(ac_ext), _ptr(src_row), cap,
                                                    C.byref(nt)))
        return ac_ext[:nacx], src_row[:nt.value]

    def obs_gather_rows(self, src_row, ncols, src, ld_src, dst, ld_dst):
        self._check(self._l.letkf_obs_gather_rows_dev(self._c, src_row.numel(), _ptr(src_row), ncols, _ptr(src), ld_src,
                                                      _ptr(dst), ld_dst))

    def obs_gather_i32(self, src_row, src, dst):
        self._check(self._l.letkf_obs_gather_i32_dev(self._c, src_row.numel(), _ptr(src_row), _ptr(src), _ptr(dst)))

    # ---- (9) set_letkf_obs behind one call
    def _set_obs(self, entry, params, qcp, files, set_, idx, qc, ensval, kld, keep):
        h = C.c_void_p()
        self._check(entry(self._c, C.byref(params), C.byref(qcp), C.byref(files), set_.numel(), _ptr(set_), _ptr(idx), _ptr(qc),
                          _ptr(ensval), kld, C.byref(h)))
        return ObsTable(self, h, keep)

    def set_obs(self, params, qcp, files, set_, idx, qc, ensval, kld, keep=()):
        """letkf_set_obs_dev (one rank).  `keep`: objects the table's file rows / params depend on."""
        return self._set_obs(self._l.letkf_set_obs_dev, params, qcp, files, set_, idx, qc, ensval, kld, keep)

    def set_obs_local(self, params, qcp, files, set_, idx, qc, ensval, kld, keep=()):
        return self._set_obs(self._l.letkf_set_obs_local_dev, params, qcp, files, set_, idx, qc, ensval, kld, keep)

    def obsope(self, params, files, fields, set_, idx, qc, ensval, kld, row0=0, nrows=None):
        """letkf_obsope_dev (include/letkf_amd_obsope.h): H(x) of fields.nmem members for the obsda rows row0 .. row0 + nrows - 1
        (default: all of set_) into ensval[row, m0 .. m0 + nmem - 1], qc merged by maximum.  Call it before set_obs, which
        pre-processes `files` in place."""
        n = set_.numel() - row0 if nrows is None else nrows
        self._check(self._l.letkf_obsope_dev(self._c, C.byref(params), C.byref(files), C.byref(fields), row0, n, _ptr(set_),
                                             _ptr(idx), _ptr(qc), _ptr(ensval), kld))

    def state_to_history(self, state, layout, v3d, v2d):
        """letkf_state_to_history_dev (include/letkf_amd_monit.h): the state `state` (HistState) into member slot 0 of the
        history fields v3d / v2d laid out as `layout` (ObsopeFields) says."""
        self._check(self._l.letkf_state_to_history_dev(self._c, C.byref(state), C.byref(layout), _ptr(v3d), _ptr(v2d)))

    def monit_obs(self, mparams, params, files, fields, set_, idx, rec, key=None, nn=None, outs=None):
        """letkf_monit_obs_dev (include/letkf_amd_monit.h): monit_obs of step mparams.step over the rows key[0 .. nn - 1] of
        set_ / idx (key None: the first nn, default all; a device int32 tensor, or a raw device address such as
        ObsTableInfo.key together with nn); `rec` (Obsdep) is updated in place.  Returns (nobs int32 [nid], bias, rmse) device
        tensors (`outs`: the three to write into)."""
        import torch
        raw = isinstance(key, int)
        n = (key.numel() if key is not None else set_.numel()) if nn is None else nn
        if outs is None:
            outs = (torch.zeros(mparams.nid, dtype=torch.int32, device=set_.device),
                    torch.zeros(mparams.nid, dtype=torch.float64, device=set_.device),
                    torch.zeros(mparams.nid, dtype=torch.float64, device=set_.device))
        self._check(self._l.letkf_monit_obs_dev(self._c, C.byref(mparams), C.byref(params), C.byref(files), C.byref(fields), n,
                                                C.c_void_p(key) if raw else _ptr(key), _ptr(set_), _ptr(idx), C.byref(rec),
                                                _ptr(outs[0]), _ptr(outs[1]),
                                                _ptr(outs[2])))
        return outs

    def randn(self, rand, n, out):
        """letkf_randn_dev (include/letkf_amd_obsmake.h): com_randn(n) from the stream `rand` (Rand) into the device tensor out."""
        self._check(osse_lib().letkf_randn_dev(self._c, rand._r, n, _ptr(out)))

    def obsmake_slot(self, slot, params, files, fields, counts=None):
        """letkf_obsmake_slot_dev: one time slot of obsmake_cal -- files.dat of the slot's rows becomes H(x) of the one state in
        `fields`, or undef; counts (device int64 [2], or None) = rows in the slot, rows processed."""
        self._check(osse_lib().letkf_obsmake_slot_dev(self._c, C.byref(slot), C.byref(params), C.byref(files), C.byref(fields),
                                                      _ptr(counts)))

    def obsmake_noise(self, err, files, rand):
        """letkf_obsmake_noise_dev: files.err by element, files.dat += err * com_randn over all rows in file order."""
        self._check(osse_lib().letkf_obsmake_noise_dev(self._c, C.byref(err), C.byref(files), rand._r))

    def obssim(self, params, fields, v3=None, v2=None, rec=None, sm3=None, sm2=None):
        """letkf_obssim_dev (include/letkf_amd_obssim.h): obssim_cal for the fields.nmem states of `fields` (ObsopeFields) with the
        lists and the radar of `params` (ObssimParams) into the device tensors v3 (float64, per state (nvar3, nlat, nlon, nlev)),
        v2 (float64, (nvar2, nlat, nlon)) and rec (float32, (nrec, nlat, nlon)); any may be None, not all.  sm3 / sm2: elements
        between two states (default: dense)."""
        out = ObssimOut()
        out.v3, out.v2, out.rec = _ptr(v3), _ptr(v2), _ptr(rec)
        npl = fields.nlon * fields.nlat
        out.sm3 = params.nvar3 * fields.nlev * npl if sm3 is None else sm3
        out.sm2 = params.nvar2 * npl if sm2 is None else sm2
        self._check(obssim_lib().letkf_obssim_dev(self._c, C.byref(params), C.byref(fields), C.byref(out)))

    def superob(self, rows, slot_off, grid, nbslot, elem_uid, methods, surface_typ_mask=SUPEROB_SURFACE_TYPES, obsnum=True,
                out=None):
        """letkf_superob_dev (include/letkf_amd_superob.h): superob's four stages over `rows`, a dict of device tensors elm, typ
        (int32) and lon, lat, lev, dat, err, ri, rj, rk (float64).  slot_off: host int64 [nslots + 1]; grid = (nlon, nlat, nlevx);
        elem_uid: host int32 [nid]; methods = (g, v, t, h), host int32 arrays (nid, nobtype).  Returns a dict of device tensors:
        the output rows at capacity nobs, nout [1], slot_off_out, qc1, counts [7] and obsnum (4, nid, nobtype) (None with
        obsnum=False).  Nothing is read back: slice by nout after a synchronisation of your own.  `out`: the dict to write into
        (an entry that is None stays NULL where the header allows it)."""
        import numpy as np
        import torch
        so = np.ascontiguousarray(slot_off, dtype=np.int64)
        ids = np.ascontiguousarray(elem_uid, dtype=np.int32)
        m = [np.ascontiguousarray(t, dtype=np.int32) for t in methods]
        nid, nobtype = m[0].shape
        n = rows["elm"].numel()
        dev = rows["elm"].device
        p = SuperobParams()
        p.nobs = n
        for name in ("elm", "typ", "lon", "lat", "lev", "dat", "err", "ri", "rj", "rk"):
            setattr(p, name, _ptr(rows[name]))
        p.slot_off = so.ctypes.data
        p.nlon, p.nlat, p.nlevx = grid
        p.nslots, p.nbslot, p.nobtype, p.nid = len(so) - 1, nbslot, nobtype, nid
        p.surface_typ_mask = surface_typ_mask - (1 << 32) if surface_typ_mask >= 1 << 31 else surface_typ_mask
        p.elem_uid = ids.ctypes.data
        p.method_g, p.method_v, p.method_t, p.method_h = (t.ctypes.data for t in m)
        if out is None:
            out = {name: torch.zeros(n, dtype=torch.int32, device=dev) for name in ("elm", "typ", "slot", "i", "j", "k", "qc1")}
            out.update({name: torch.zeros(n, dtype=torch.float64, device=dev)
                        for name in ("lon", "lat", "lev", "dat", "err", "ri", "rj", "rk")})
            out["nout"] = torch.zeros(1, dtype=torch.int64, device=dev)
            out["slot_off_out"] = torch.zeros(len(so), dtype=torch.int64, device=dev)
            out["counts"] = torch.zeros(7, dtype=torch.int64, device=dev)
            out["obsnum"] = torch.zeros((4, nid, nobtype), dtype=torch.int64, device=dev) if obsnum else None
        o = SuperobOut()
        for name, _ in SuperobOut._fields_:
            setattr(o, name, _ptr(out.get(name)))
        self._check(superob_lib().letkf_superob_dev(self._c, C.byref(p), C.byref(o)))
        return out

    def obsscan(self, files, dif, layout, slots, obsda_run=None, myrank_d=None, extras=True, out=None):
        """letkf_obsscan_dev (include/letkf_amd_obsscan.h): obsope_cal's first scan over all rows of `files` (ObsFileRows; off, ri
        and rj are read) and the device tensor dif.  layout = (nlon, nlat, ihalo, jhalo, prc_num_x, prc_num_y); slots =
        (slot_start, slot_end, slot_base, slot_tinterval); obsda_run: host flags per file (None: all run).  Returns a dict: the
        device tensors set, idx, qc (one per row of the files that run), the host int32 arrays bsn (nprocs_d, nslots + 2) and bsna
        (nprocs_d, nslots + 3), and with extras the device tensors rank and slot per file row and, given myrank_d, own.  `out`:
        the dict to write into (a device entry that is None stays NULL)."""
        import numpy as np
        import torch
        nfile = files.nfile
        off = np.ctypeslib.as_array(C.cast(files.off, C.POINTER(C.c_int64)), shape=(nfile + 1,))
        run = None if obsda_run is None else np.ascontiguousarray(obsda_run, dtype=np.int32)
        n = int(off[-1])
        nlist = int(sum(off[f + 1] - off[f] for f in range(nfile) if run is None or run[f]))
        p = ObsscanParams()
        p.dif, p.obsda_run = _ptr(dif), None if run is None else run.ctypes.data
        p.nlon, p.nlat, p.ihalo, p.jhalo, p.prc_num_x, p.prc_num_y = layout
        p.slot_start, p.slot_end, p.slot_base, p.slot_tinterval = slots
        p.myrank_d = 0 if myrank_d is None else myrank_d
        nprocs, nb = p.prc_num_x * p.prc_num_y, p.slot_end - p.slot_start + 3
        if out is None:
            dev = dif.device
            out = {name: torch.zeros(nlist, dtype=torch.int32, device=dev) for name in ("set", "idx", "qc")}
            for name in ("rank", "slot", "own"):
                want = extras and (name != "own" or myrank_d is not None)
                out[name] = torch.zeros(n, dtype=torch.int32, device=dev) if want else None
            out["bsn"] = np.zeros((nprocs, nb), dtype=np.int32)
            out["bsna"] = np.zeros((nprocs, nb + 1), dtype=np.int32)
        o = ObsscanOut()
        for name, _ in ObsscanOut._fields_:
            v = out.get(name)
            setattr(o, name, v.ctypes.data if isinstance(v, np.ndarray) else _ptr(v))
        self._check(obsscan_lib().letkf_obsscan_dev(self._c, C.byref(p), C.byref(files), C.byref(o)))
        return out

    def obsope_slot(self, scan, slot_start, ip, islot, params, files, fields, ensval, kld):
        """letkf_obsope_slot_dev (include/letkf_amd_obsscan.h): the operator on the list rows of subdomain ip in slot islot of
        `scan`, the dict Context.obsscan returned; ensval is indexed by the global list row."""
        bsna = scan["bsna"]
        l = ObsscanLists()
        l.nprocs_d, l.slot_start, l.slot_end = bsna.shape[0], slot_start, slot_start + bsna.shape[1] - 4
        l.bsna, l.set, l.idx, l.qc = bsna.ctypes.data, _ptr(scan["set"]), _ptr(scan["idx"]), _ptr(scan["qc"])
        self._check(obsscan_lib().letkf_obsope_slot_dev(self._c, C.byref(l), ip, islot, C.byref(params), C.byref(files),
                                                        C.byref(fields), _ptr(ensval), kld))

    def _mapproj_rows(self, entry, proj, a, b, rotc, out):
        import torch
        n = a.numel()
        if out is None:
            out = tuple(torch.empty(n, dtype=torch.float64, device=a.device) for _ in range(2))
            out += (torch.empty((n, 2), dtype=torch.float64, device=a.device) if rotc else None,)
        self._check(getattr(mapproj_lib(), entry)(self._c, C.addressof(proj), n, _ptr(a), _ptr(b), *(_ptr(t) for t in out)))
        return out

    def phys2ij(self, proj, lon, lat, rotc=True, out=None):
        """letkf_phys2ij_dev (include/letkf_amd_mapproj.h): the device tensors lon, lat (float64, degrees) to (ri, rj, rotc): ri,
        rj [n] and rotc [n, 2], or None without it.  `out`: the three tensors to write into (rotc may be None)."""
        return self._mapproj_rows("letkf_phys2ij_dev", proj, lon, lat, rotc, out)

    def ij2phys(self, proj, ri, rj, rotc=True, out=None):
        """letkf_ij2phys_dev: the device tensors ri, rj to (lon, lat, rotc) in degrees, as phys2ij the other way"""
        return self._mapproj_rows("letkf_ij2phys_dev", proj, ri, rj, rotc, out)

    def mapproj_grid(self, proj, nlon, nlat, ihalo, jhalo, cx1, cy1, want=("lon", "lat", "rotc"), device=None, out=None):
        """letkf_mapproj_grid_dev: lon2d, lat2d [nlat, nlon] in degrees and rotc2d [nlat, nlon, 2] of a subdomain whose GRID_CX(1)
        / GRID_CY(1) are cx1 / cy1, as a dict with the keys of `want` (the others None); the layouts Context.obssim takes.
        `out`: the dict to write into."""
        import torch
        if out is None:
            dev = device if device is not None else torch.device("cuda", torch.cuda.current_device())
            out = {k: torch.empty((nlat, nlon) + ((2,) if k == "rotc" else ()), dtype=torch.float64, device=dev) if k in want else None
                   for k in ("lon", "lat", "rotc")}
        self._check(mapproj_lib().letkf_mapproj_grid_dev(self._c, C.addressof(proj), nlon, nlat, ihalo, jhalo, cx1, cy1,
                                                         _ptr(out.get("lon")), _ptr(out.get("lat")), _ptr(out.get("rotc"))))
        return out

    # ---- the record codec (include/letkf_amd_obsfile.h); an image is a device tensor of the file's bytes, of any dtype
    @staticmethod
    def _image_bytes(image):
        return image.numel() * image.element_size()

    def obs_decode(self, image, fmt, nrec=None, big_endian=False, proj=None, obserr_tc=(5.0e2, 50.0e3, 50.0e3), want=OBSFILE_COLUMNS,
                   meta=True, check=False, out=None):
        """letkf_obs_decode_dev: a conventional (fmt 1) or radar (fmt 2) file image to a dict of the columns of `want` (int32 elm,
        typ; float64 the rest; the others None), with "meta" (float64 [3], radar with meta=True) and "nbad" (check=True).  `out`: a
        dict of tensors to write into."""
        import numpy as np
        import torch
        nrec = nrec if nrec is not None else 8
        n = obsfile_count(fmt, nrec, self._image_bytes(image))
        p = ObsfileParams()
        p.format, p.nrec, p.big_endian, p.proj_given = fmt, nrec, int(big_endian), int(proj is not None)
        p.obserr_tcp, p.obserr_tcx, p.obserr_tcy = obserr_tc
        if out is None:
            out = {k: torch.empty(n, dtype=torch.int32 if k in ("elm", "typ") else torch.float64, device=image.device) if k in want else None
                   for k in OBSFILE_COLUMNS}
        o = ObsfileCols()
        for k in OBSFILE_COLUMNS:
            setattr(o, k, _ptr(out.get(k)))
        head = np.zeros(3) if (meta and fmt == OBSFILE_RADAR) else None
        nbad = C.c_int64(-1)
        self._check(obsfile_lib().letkf_obs_decode_dev(self._c, C.addressof(p), C.addressof(proj) if proj is not None else None, _ptr(image),
                                                       n, C.addressof(o), _hptr(head), C.addressof(nbad) if check else None))
        res = dict(out)
        res["meta"], res["nbad"] = head, nbad.value if check else None
        return res

    def obs_encode(self, cols, fmt, nrec=None, big_endian=False, missing=True, meta=None, out=None):
        """letkf_obs_encode_dev: the columns (a dict of device tensors) to (image, nwritten): image a uint8 device tensor sized for
        every row, of which the first obsfile_bytes(fmt, nrec, nwritten) are the file.  missing=False leaves the undefined rows
        out (one read-back)."""
        import numpy as np
        import torch
        nrec = nrec if nrec is not None else 8
        n = cols["elm"].numel()
        p = ObsfileParams()
        p.format, p.nrec, p.big_endian, p.missing = fmt, nrec, int(big_endian), int(missing)
        c = ObsfileCols()
        for k in OBSFILE_COLUMNS:
            setattr(c, k, _ptr(cols.get(k)))
        if out is None:
            out = torch.empty(obsfile_bytes(fmt, nrec, n), dtype=torch.uint8, device=cols["elm"].device)
        head = None if meta is None else np.ascontiguousarray(meta, dtype=np.float64)
        nw = C.c_int64(-1)
        self._check(obsfile_lib().letkf_obs_encode_dev(self._c, C.addressof(p), n, C.addressof(c), _hptr(head), _ptr(out), C.addressof(nw)))
        return out, nw.value

    def obsda_assemble(self, images, nobs, kld, col=None, nrec=4, big_endian=False, is_member=None, member=0, finish=False, check=False,
                       out=None):
        """letkf_obsda_assemble_dev: the obsda file images (device tensors of nobs records each) into a dict set, idx, qc (int32
        [nobs]), ensval (float64 [nobs, kld]) and, under nrec 6, lev, val2; image m goes to column col[m] (default m).  `out`: the
        dict to write into (qc, lev and val2 are INOUT; a fresh qc starts at 0, as obs_da_value_allocate leaves it).  check=True
        adds "ninconsistent" and "nbad"."""
        import numpy as np
        import torch
        nmem = len(images)
        p = ObsdaParams()
        p.nrec, p.big_endian, p.nmem, p.finish, p.member, p.nobs, p.kld = nrec, int(big_endian), nmem, int(finish), member, nobs, kld
        if out is None:
            dev = images[0].device
            out = {k: torch.zeros(nobs, dtype=torch.int32, device=dev) for k in ("set", "idx", "qc")}
            out["ensval"] = torch.zeros((nobs, kld), dtype=torch.float64, device=dev)
            for k in ("lev", "val2"):
                out[k] = torch.zeros(nobs, dtype=torch.float64, device=dev) if nrec == 6 else None
        o = ObsdaCols()
        for k, _ in ObsdaCols._fields_:
            setattr(o, k, _ptr(out.get(k)))
        ptrs = (C.c_void_p * max(nmem, 1))(*[t.data_ptr() for t in images])
        cols = np.ascontiguousarray(np.arange(nmem) if col is None else col, dtype=np.int32)
        flags = None if is_member is None else np.ascontiguousarray(is_member, dtype=np.int32)
        ninc, nbad = C.c_int64(-1), C.c_int64(-1)
        self._check(obsfile_lib().letkf_obsda_assemble_dev(self._c, C.addressof(p), C.addressof(ptrs), _hptr(cols), _hptr(flags),
                                                           C.addressof(o), C.addressof(ninc) if check else None,
                                                           C.addressof(nbad) if check else None))
        res = dict(out)
        res["ninconsistent"], res["nbad"] = (ninc.value, nbad.value) if check else (None, None)
        return res

    def obsda_encode(self, set, idx, qc, ensval=None, col=-1, val=None, lev=None, val2=None, nrec=4, big_endian=False, out=None):
        """letkf_obsda_encode_dev: write_obs_da's file image (a uint8 device tensor) for column col of ensval [nobs, kld], or for
        val when col < 0"""
        import torch
        n = set.numel()
        if out is None:
            out = torch.empty(obsfile_bytes(OBSFILE_OBSDA, nrec, n), dtype=torch.uint8, device=set.device)
        kld = ensval.shape[1] if ensval is not None and ensval.dim() == 2 else 0
        self._check(obsfile_lib().letkf_obsda_encode_dev(self._c, nrec, int(big_endian), n, _ptr(set), _ptr(idx), _ptr(qc), _ptr(ensval), kld,
                                                         col, _ptr(val), _ptr(lev), _ptr(val2), _ptr(out)))
        return out

    def obsdep_encode(self, set, idx, qc, omb, oma, files, big_endian=False, out=None):
        """letkf_obsdep_encode_dev: write_obs_dep's file image (a uint8 device tensor); files: an ObsfileRows (obsfile_rows())"""
        import torch
        n = set.numel()
        if out is None:
            out = torch.empty(obsfile_bytes(OBSFILE_DEP, 11, n), dtype=torch.uint8, device=set.device)
        self._check(obsfile_lib().letkf_obsdep_encode_dev(self._c, int(big_endian), n, _ptr(set), _ptr(idx), _ptr(qc), _ptr(omb), _ptr(oma),
                                                          C.addressof(files), _ptr(out)))
        return out

    def read_obs_file(self, path, fmt, device=None, **kw):
        """numpy.fromfile -> device -> obs_decode: one call per observation file; kw as obs_decode's"""
        import numpy as np
        import torch
        dev = device if device is not None else torch.device("cuda", torch.cuda.current_device())
        return self.obs_decode(torch.from_numpy(np.fromfile(path, dtype=np.uint8)).to(dev), fmt, **kw)

    def read_obsda_files(self, paths, kld=None, nrec=4, device=None, **kw):
        """numpy.fromfile -> device -> obsda_assemble: one call per set of obsda files (one per member, the mean's where col says);
        kw as obsda_assemble's"""
        import numpy as np
        import torch
        dev = device if device is not None else torch.device("cuda", torch.cuda.current_device())
        images = [torch.from_numpy(np.fromfile(f, dtype=np.uint8)).to(dev) for f in paths]
        nobs = obsfile_count(OBSFILE_OBSDA, nrec, self._image_bytes(images[0]))
        for f, t in zip(paths, images):
            if self._image_bytes(t) != self._image_bytes(images[0]):
                raise LetkfError(f"{f}: {self._image_bytes(t)} bytes, {paths[0]} has {self._image_bytes(images[0])}")
        return self.obsda_assemble(images, nobs, kld if kld is not None else len(images), nrec=nrec, **kw)

    def set_obs_finish(self, table, n_all, recv, tot_g=None):
        self._check(self._l.letkf_set_obs_finish_dev(self._c, table._h, _ptr(n_all), _ptr(tot_g),
                                                     recv.shape[0] if recv is not None else 0, _ptr(recv)))

    # ---- (6) after the loop
    def monit_dep(self, elem_uid, elm, dep, qc):
        """Returns (nobs int32 [nid], bias, rmse) device tensors."""
        import numpy as np
        import torch
        ids = np.ascontiguousarray(elem_uid, dtype=np.int32)
        nid = len(ids)
        nobs = torch.zeros(nid, dtype=torch.int32, device=dep.device)
        bias = torch.zeros(nid, dtype=torch.float64, device=dep.device)
        rmse = torch.zeros(nid, dtype=torch.float64, device=dep.device)
        self._check(self._l.letkf_monit_dep_dev(self._c, nid, _hptr(ids), dep.numel(), _ptr(elm), _ptr(dep), _ptr(qc),
                                                _ptr(nobs), _ptr(bias), _ptr(rmse)))
        return nobs, bias, rmse

    def additive_inflation(self, k, nv, npts, nij1, anal, add, sp, sm, sv, infl_add, weight=None, qmean=None, q_sp=0,
                           q_sv=0, iv_q_first=5, iv_q_last=10, ishuf=None):
        self._check(self._l.letkf_additive_inflation_dev(self._c, k, nv, npts, nij1, _ptr(anal), _ptr(add), sp, sm, sv, infl_add,
                                                         _ptr(weight), _ptr(qmean), q_sp, q_sv, iv_q_first, iv_q_last,
                                                         _ptr(ishuf)))

    def addinfl_weight(self, rig, rjg, ob_ri, ob_rj, dx, dy, hori_loc):
        import torch
        w = torch.zeros(rig.numel(), dtype=torch.float64, device=rig.device)
        self._check(self._l.letkf_addinfl_weight_dev(self._c, rig.numel(), _ptr(rig), _ptr(rjg), ob_ri.numel(), _ptr(ob_ri),
                                                     _ptr(ob_rj), dx, dy, hori_loc, _ptr(w)))
        return w

    # ---- (8) the exchange, on an RCCL communicator the caller owns (an integer / c_void_p ncclComm_t)
    def obs_allgatherv(self, nccl_comm, myrank, counts, send, recv):
        """counts: python ints per rank (rows); send / recv: device tensors whose rows are contiguous."""
        import numpy as np
        cnt = np.array([int(x) for x in counts], dtype=np.int64)
        row_bytes = send.element_size() * (send[0].numel() if send.dim() > 1 and send.shape[0] > 0 else
                                           (recv[0].numel() if recv.dim() > 1 else 1))
        self._check(self._l.letkf_obs_allgatherv_dev(self._c, C.c_void_p(nccl_comm), len(cnt), myrank, _hptr(cnt), row_bytes,
                                                     _ptr(send), _ptr(recv)))

    # ---- (7) das_letkf set-up
    def alltoallv(self, nccl_comm, myrank, send_counts, send_offs, recv_counts, recv_offs, row_bytes, send, recv):
        """letkf_alltoallv_dev: counts / offsets are host lists in rows of row_bytes bytes"""
        import numpy as np
        arr = lambda v: _hptr(np.array([int(a) for a in v], dtype=np.int64))
        self._check(self._l.letkf_alltoallv_dev(self._c, C.c_void_p(nccl_comm), len(send_counts), myrank, arr(send_counts),
                                                arr(send_offs), arr(recv_counts), arr(recv_offs), row_bytes, _ptr(send), _ptr(recv)))

    def allreduce_sum_i32(self, nccl_comm, nranks, buf):
        self._check(self._l.letkf_allreduce_sum_i32_dev(self._c, C.c_void_p(nccl_comm), nranks, buf.numel(), _ptr(buf)))

    def members_alltoall(self, nccl_comm, nranks, myrank, direction, nlev, nlon, nlat, nv3d, mstart, mcount, v3dg, x, sp, sm, sv):
        self._check(self._l.letkf_members_alltoall_dev(self._c, C.c_void_p(nccl_comm), nranks, myrank, direction, nlev, nlon,
                                                       nlat, nv3d, mstart, mcount, _ptr(v3dg), _ptr(x), sp, sm, sv))

    def relax_beta(self, params, nij1, nlev, rig, rjg, hgt, beta):
        self._check(self._l.letkf_relax_beta_dev(self._c, C.byref(params), nij1, nlev, _ptr(rig), _ptr(rjg), _ptr(hgt),
                                                 _ptr(beta)))

    def infl_init(self, work3d, infl_mul, infl_mul_min):
        self._check(self._l.letkf_infl_init_dev(self._c, work3d.numel(), _ptr(work3d), infl_mul, infl_mul_min))

    # ---- (4) the steps either side of the loop
    def state_trans(self, consts, nlev, nlon, nlat, nv3d, v3dg, inverse=False):
        self._check(self._l.letkf_state_trans_dev(self._c, C.byref(consts), nlev, nlon, nlat, nv3d, _ptr(v3dg),
                                                  1 if inverse else 0))

    def member_points(self, direction, nlev, nlon, nlat, nv3d, np_, rank, m, v3dg, x, nij1, sp, sm, sv):
        self._check(self._l.letkf_member_points_dev(self._c, direction, nlev, nlon, nlat, nv3d, np_, rank, m, _ptr(v3dg),
                                                    _ptr(x), nij1, sp, sm, sv))

    def ens_spread(self, k, nv, npts, x, sp, sm, sv, sprd):
        self._check(self._l.letkf_ens_spread_dev(self._c, k, nv, npts, _ptr(x), sp, sm, sv, _ptr(sprd)))

    def to_perturbations(self, k, nv, npts, x, sp, sm, sv):
        self._check(self._l.letkf_ens_to_perturbations_dev(self._c, k, nv, npts, _ptr(x), sp, sm, sv))

    def ens_mean(self, k, nv, npts, x, sp, sm, sv):
        self._check(self._l.letkf_ens_mean_dev(self._c, k, nv, npts, _ptr(x), sp, sm, sv))


def letkf_core_host(ne, nobs, nobsl, hdxb, rdiag, rloc, dep, parm_infl, want_transm=True, want_pao=True,
                    rdiag_wloc=None, infl_update=None, depd=None, want_transmd=False, fill=0.0,
                    transmd_without_depd=False):
    """The host-pointer drop-in letkf_core_c (what the Fortran shim calls), on numpy arrays.  The outputs start as
    `fill`; transmd is returned only with depd unless transmd_without_depd."""
    import numpy as np
    f = _hptr
    hdxb = np.asfortranarray(hdxb, dtype=np.float64)
    trans = np.full((ne, ne), fill, order="F")
    transm = np.full(ne, fill) if want_transm else None
    pao = np.full((ne, ne), fill, order="F") if want_pao else None
    transmd = np.full(ne, fill) if want_transmd else None
    infl = C.c_double(parm_infl)
    wl = C.c_int(1 if rdiag_wloc else 0)
    iu = C.c_int(1 if infl_update else 0)
    st = C.c_int(-99)
    lib().letkf_core_c(ne, nobs, nobsl, f(hdxb), f(rdiag), f(rloc), f(dep), C.byref(infl), f(trans), f(transm), f(pao),
                       C.byref(wl) if rdiag_wloc is not None else None, C.byref(iu) if infl_update is not None else None,
                       f(depd), f(transmd), C.byref(st))
    return dict(trans=trans, transm=transm, pao=pao,
                transmd=transmd if (depd is not None or transmd_without_depd) else None,
                parm_infl=infl.value, status=st.value)


# ---- (7) host-side table derivations of das_letkf's set-up (no device needed)
def var_local_classes(var_local):
    """var_local: numpy (nvar, nlt).  Returns (n2nc, n2n, nclass), 0-based (letkf_tools.f90:130-157)."""
    import numpy as np
    v = np.asfortranarray(var_local, dtype=np.float64)
    nvar, nlt = v.shape
    n2nc = np.zeros(nvar, dtype=np.int32)
    n2n = np.zeros(nvar, dtype=np.int32)
    nc = C.c_int32(0)
    rc = lib().letkf_var_local_classes(nvar, nlt, _hptr(v), _hptr(n2nc), _hptr(n2n), C.byref(nc))
    if rc != LETKF_OK:
        raise LetkfError(f"letkf_var_local_classes: {rc}")
    return n2nc, n2n, nc.value


def ctype_merge_groups(elm_u_ctype, typ_ctype, ctype_merge):
    """ctype_merge: numpy (nid_obs, nobtype) int32.  Returns (group_start [ngroup+1], group_member [nctype])."""
    import numpy as np
    eu = np.ascontiguousarray(elm_u_ctype, dtype=np.int32)
    ty = np.ascontiguousarray(typ_ctype, dtype=np.int32)
    cm = np.asfortranarray(ctype_merge, dtype=np.int32)
    nct = len(eu)
    gs = np.zeros(nct + 1, dtype=np.int32)
    gm = np.zeros(max(nct, 1), dtype=np.int32)
    ng = C.c_int32(0)
    p = _hptr
    rc = lib().letkf_ctype_merge_groups(nct, p(eu), p(ty), cm.shape[0], cm.shape[1], p(cm), p(gs), p(gm), C.byref(ng))
    if rc != LETKF_OK:
        raise LetkfError(f"letkf_ctype_merge_groups: {rc}")
    return gs[:ng.value + 1].copy(), gm[:nct].copy()


def obs_target_var(elm):
    """letkf_obs_target_var (host only): the 0-based grid variable das_letkf_obs regards an observation element as, -1 none."""
    return int(lib().letkf_obs_target_var(int(elm)))


def radar_only(typ_ctype, typ_radar=22):
    import numpy as np
    ty = np.ascontiguousarray(typ_ctype, dtype=np.int32)
    return int(lib().letkf_radar_only(len(ty), _hptr(ty), typ_radar))
