"""The argument space of letkf_das_points_dev (include/letkf_amd.h, letkf_das_args): the solver routes and how to reach
them, and das_case's inputs re-laid out -- other state strides, slab views, other observation-table leading dimensions --
inside buffers whose every element the call must not write holds a fixed canary bit pattern.  The oracle always gets
das_case's own arrays, so its answer is the one already trusted; only the library sees the re-laid-out copies."""
import numpy as np

from _cases import das_case

# a signalling-NaN bit pattern: an element that still holds it was not written, and any arithmetic use of it is a NaN
CANARY = 0x7FF4DEADBEEF0001
TAIL = 64                                   # NaN doubles behind the observation table (over-reads land there)

# route name -> (k, nv, k x k outputs requested, substrings ctx().last_path() must contain, ... it must not contain).
# Where each route is decided: letkf_api.hip pick_route.
ROUTES = {
    "trio16": (9, 11, None, ["letkf_trio_kernel<KR=16"], []),
    "trio16_k16": (16, 11, None, ["letkf_trio_kernel<KR=16"], []),
    "trio20_k17": (17, 11, None, ["letkf_trio_kernel<KR=20"], []),
    "trio20": (20, 11, None, ["letkf_trio_kernel<KR=20"], []),
    "wave1_k21": (21, 11, None, ["letkf_wave_kernel<", "NW=1"], []),
    "wave1_k33": (33, 11, None, ["letkf_wave_kernel<", "NW=1"], []),
    "wave1": (50, 11, None, ["letkf_wave_kernel<", "NW=1"], []),
    "wave1_k62": (62, 11, None, ["letkf_wave_kernel<", "NW=1"], []),
    "wave1_trans_k20": (20, 11, "trans", ["letkf_wave_kernel<", "NW=1"], []),
    "wave1_pa_k9": (9, 11, "pa", ["letkf_wave_kernel<", "NW=1"], []),
    "wave2_trans_k63": (63, 11, "trans", ["letkf_wave_kernel<", "NW=2"], []),
    "wave2_pa_k64": (64, 11, "pa", ["letkf_wave_kernel<", "NW=2"], []),
    "wave2_pa": (100, 11, "pa", ["letkf_wave_kernel<", "NW=2"], []),
    "wave2_nopoly": (100, 11, "nopoly", ["letkf_wave_kernel<", "NW=2"], []),
    "staged_poly_k63": (63, 11, None, ["staged:", "letkf_stage_krylov_kernel"], []),
    "staged_poly": (100, 11, None, ["staged:", "letkf_stage_krylov_kernel"], []),
    "staged_poly_k144": (144, 11, None, ["staged:", "letkf_stage_krylov_kernel"], []),
    "staged_poly_nv7": (20, 7, None, ["staged:", "letkf_stage_krylov_kernel"], []),
    "staged_wg": (144, 11, "trans", ["staged:", "letkf_eig_wg_kernel"], ["letkf_eig_block_kernel", "krylov"]),
    "staged_block": (250, 11, None, ["staged:", "letkf_eig_block_kernel"], []),
    "staged_block_nopoly": (250, 11, "nopoly", ["staged:", "/ letkf_eig_block_kernel"], ["krylov"]),
    "point": (20, 15, None, ["letkf_point_kernel"], []),
    "point_big": (144, 15, None, ["letkf_point_kernel<BIG>"], []),
}
# one representative of every route for the per-axis tests (each axis reaches every route at least once)
AXIS_ROUTES = ["trio16", "trio20", "wave1", "wave1_trans_k20", "wave2_pa", "staged_poly", "staged_poly_nv7", "staged_wg",
               "staged_block", "point"]

# RTPS + adaptive inflation + DET_RUN (+ Q_UPDATE_TOP where asked): every switch that writes something of its own
CFG = dict(relax_alpha_spread=0.9, infl_adaptive=1, relax_to_inflated_prior=1)


def route_case(name, seed, det, npts=None, n_mean=None, vary_n=True):
    k, nv = ROUTES[name][:2]
    npts = npts or (8 if k >= 144 else 24)
    n_mean = n_mean or (40 if k <= 20 else k)
    c = das_case(k=k, nv=nv, npts=npts, nobs_tot=max(300, 2 * k + 40), n_mean=n_mean, seed=seed, det_run=det,
                 vary_n=vary_n, infl0=1.07)
    c["infl"] = c["infl"] * (1.0 + 0.02 * np.arange(c["infl"].size) / c["infl"].size)   # distinct slots
    return c


def state_layout(c, layout):
    """(sp, sm, sv, offset, size) of the state arrays in one of the layouts the header allows."""
    npts, nens, nv = c["npts"], c["nens"], c["nv"]
    if layout == "ref":                      # gues3d(nij1*nlev, nens, nv3d)
        return 1, npts, npts * nens, 0, npts * nens * nv
    if layout == "member":                   # member-fastest
        return nens, 1, npts * nens, 0, npts * nens * nv
    if layout == "var":                      # variable-fastest
        return nv * nens, nv, 1, 0, npts * nens * nv
    if layout == "padded":                   # every stride larger than dense, and a lead-in
        sp = 2
        sm = sp * npts + 3
        sv = sm * (nens + 1) + 5
        off = 7
        return sp, sm, sv, off, off + sv * nv + 11
    raise ValueError(layout)


def state_index(c, sp, sm, sv, off):
    """flat index of element (v, m, p) -- shaped like das_case's dense state (nv, nens, npts)"""
    v = np.arange(c["nv"])[:, None, None]
    m = np.arange(c["nens"])[None, :, None]
    p = np.arange(c["npts"])[None, None, :]
    return off + p * sp + m * sm + v * sv


def canary_buffer(size):
    return np.full(size, CANARY, dtype=np.int64).view(np.float64)


def place_state(c, sp, sm, sv, off, size, base=None):
    """das_case's gues in the given layout inside a canary buffer (or inside `base`)"""
    buf = canary_buffer(size) if base is None else base.copy()
    buf[state_index(c, sp, sm, sv, off)] = c["gues"].reshape(c["nv"], c["nens"], c["npts"])
    return buf


def obs_table(c, kld, det):
    """das_case's observation table with leading dimension kld >= k (+1 with det); every column the call must not read
    (column k without det, any padding) is NaN, and so is a tail behind the last row."""
    k, ens = c["k"], c["ensval"].reshape(-1, c["kld"])
    nobs = ens.shape[0]
    tab = np.full(nobs * kld + TAIL, np.nan)
    t = tab[:nobs * kld].reshape(nobs, kld)
    t[:, :k] = ens[:, :k]
    if det:
        t[:, k] = ens[:, k]
    return tab


def members(k, det):
    return list(range(k)) + ([k + 1] if det else [])


def mask_vars(nv, mask):
    return [v for v in range(nv) if mask == 0 or (mask >> v) & 1]
