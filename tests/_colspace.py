"""The argument space of letkf_das_columns_dev (include/letkf_amd.h (3c)): the routes of the entry and how to reach them, a
grid of columns with search tables (tests/_search.py build_case) and an ensemble on it, and the oracle's answer for it --
obs_local (oracle_csr) for the points p = ij + nij1*lev, then the loop body (orc_das_letkf_points) -- per variable-localisation
class.  The state layouts, the canary and the observation table come from tests/_argspace.py; a slab of levels of a larger field
is laid out here (field_view).  Pure numpy and the oracle: the CPU checks in tests/test_colspace_helpers.py import it."""
import numpy as np

import _oracle
from _argspace import CFG, canary_buffer, mask_vars, state_index, state_layout
from _search import build_case, host_struct, oracle_csr

FREE = "FUSED: column survivors"        # ctx().last_path() of the list-free route (letkf_api.hip route_path, mode 3)
# context options by short name (Context.OPT_*) and the library's defaults, restored after every call
OPTIONS = {"surv": "OPT_COLUMN_SURVIVORS", "poly": "OPT_STAGED_POLY", "rings": "OPT_LIMITED_RINGS", "release": "OPT_RING_RELEASE"}
DEFAULTS = {"surv": 2, "poly": 1, "rings": 2, "release": 0}
WG_MAX_ORDER = 208                       # the workgroup Jacobi's largest order (header, LETKF_OPT_STAGED_POLY); block Jacobi beyond
BIG = 1 << 30
# classes' var_local factors per combined type (radar, radar zero, upper-air T, surface pressure); "gen": two factors in the
# merged radar group 0 + 1 (criterion 2's general ring key)
VARLOC = {"free": (1.0, 1.0, 0.8, 1.0), "c1": (1.0, 1.0, 0.8, 1.0), "c2gen": (1.0, 0.6, 0.8, 1.0)}
VARLOC_B = {"free": (1.0, 1.0, 0.4, 1.0), "c1": (1.0, 1.0, 0.4, 1.0), "c2gen": (0.7, 1.0, 0.4, 1.0)}
LIMITS = (12, 12, 0, 3)

# route name -> (k, nv, tables, options, list_bytes, substrings ctx().last_path() must contain, ... must not contain).
# tables: "free" no MAX_NOBS_PER_GRID, "c1" limits under the distance criterion, "c2gen" the weight criterion with two factors
# in the merged group.  list_bytes: "all" one batch / slab, "columns" below one column's survivors x 32 B (batches of about one
# column), "level" below one level's lists x 20 B (one level per slab), "slabs" about 1.5 levels' lists (several slabs).
COL_ROUTES = {
    "free_k9": (9, 11, "free", {"surv": 1}, "all", [FREE, "NW=1"], []),
    "free_k20": (20, 11, "free", {"surv": 1}, "all", [FREE, "NW=1"], []),
    "free_k33": (33, 11, "free", {"surv": 1}, "all", [FREE, "NW=1"], []),
    "free_k50": (50, 11, "free", {"surv": 1}, "all", [FREE, "NW=1"], []),
    "free_k62": (62, 11, "free", {"surv": 1}, "all", [FREE, "NW=1"], []),
    "free_batches": (33, 11, "free", {"surv": 1}, "columns", [FREE, "NW=1"], []),
    "list_trio16": (9, 11, "free", {"surv": 0}, "all", ["letkf_trio_kernel<KR=16"], ["FUSED"]),
    "list_trio20": (20, 11, "free", {"surv": 0}, "all", ["letkf_trio_kernel<KR=20"], ["FUSED"]),
    "list_wave1": (50, 11, "free", {"surv": 0}, "all", ["letkf_wave_kernel<", "NW=1"], ["FUSED"]),
    "list_wave2_k63": (63, 11, "free", {"surv": 0, "poly": 0}, "all", ["letkf_wave_kernel<", "NW=2"], ["FUSED"]),
    "list_wave2": (100, 11, "free", {"surv": 0, "poly": 0}, "all", ["letkf_wave_kernel<", "NW=2"], ["FUSED"]),
    "list_staged_poly": (100, 11, "free", {"surv": 0}, "all", ["staged:", "letkf_stage_krylov_kernel"], []),
    "list_staged_poly_k144": (144, 11, "free", {"surv": 0}, "all", ["staged:", "letkf_stage_krylov_kernel"], []),
    "list_staged_poly_nv7": (20, 7, "free", {"surv": 0}, "all", ["staged:", "letkf_stage_krylov_kernel"], []),
    "list_staged_wg": (144, 11, "free", {"surv": 0, "poly": 0}, "all", ["staged:", "letkf_eig_wg_kernel"],
                       ["letkf_eig_block_kernel", "krylov"]),
    "list_staged_block": (250, 11, "free", {"surv": 0, "poly": 0}, "all", ["staged:", "letkf_eig_block_kernel"], ["krylov"]),
    "list_point": (20, 15, "free", {"surv": 0}, "all", ["letkf_point_kernel"], []),
    "list_levels": (50, 11, "free", {"surv": 0}, "level", ["letkf_wave_kernel<", "NW=1"], ["FUSED"]),
    "lim_lds": (20, 11, "c1", {"rings": 0}, "all", ["letkf_trio_kernel<KR=20"], ["FUSED"]),
    "lim_rings": (50, 11, "c1", {"rings": 1}, "slabs", ["letkf_wave_kernel<", "NW=1"], ["FUSED"]),
    "lim_rings_gen": (33, 11, "c2gen", {"rings": 1}, "slabs", ["letkf_wave_kernel<", "NW=1"], ["FUSED"]),
    "lim_rings_release": (9, 11, "c1", {"rings": 1, "release": 1}, "slabs", ["letkf_trio_kernel<KR=16"], ["FUSED"]),
}
# one row of every route family for the per-axis tests (each axis reaches every family)
AXIS_ROUTES = ["free_k20", "free_batches", "list_trio16", "list_trio20", "list_wave1", "list_wave2", "list_staged_poly",
               "list_staged_poly_nv7", "list_staged_wg", "list_staged_block", "list_point", "list_levels", "lim_lds",
               "lim_rings"]


def route_family(name):
    """the route the ABI's rules give a row (include/letkf_amd.h (3c), letkf_api.hip pick_route), from its inputs alone"""
    k, nv, tables, opt, lb = COL_ROUTES[name][:5]
    o = dict(DEFAULTS, **opt)
    if tables == "free" and o["surv"] == 1 and nv == 11 and k <= 62:
        return "free_batches" if lb == "columns" else "free"
    if tables != "free":
        return "lim_lds" if o["rings"] == 0 else "lim_rings_gen" if tables == "c2gen" else \
            "lim_rings_release" if o["release"] else "lim_rings"
    if lb == "level":
        return "list_levels"
    if nv + 2 > 16:
        return "point"
    if nv == 11 and k <= 20:
        return "trio16" if k <= 16 else "trio20"
    if nv == 11 and k <= 62:
        return "wave1"
    if nv == 11 and k <= 100 and not o["poly"]:
        return "wave2"
    if o["poly"]:
        return "staged_poly_nv7" if nv != 11 else "staged_poly"
    return "staged_wg" if k <= WG_MAX_ORDER else "staged_block"


def krylov(name):
    """points of this row are solved without an eigen-decomposition where the CG converges (nsweep < 0)"""
    k, nv, tables, opt = COL_ROUTES[name][:4]
    o = dict(DEFAULTS, **opt)
    fam = route_family(name)
    return o["poly"] == 1 and fam not in ("free", "free_batches", "point") and (nv != 11 or k >= 63)


def col_case(name, seed, det=True, nij1=None, nlev=None, west_empty=False, no_obs=False, infl_flat=False):
    """nij1 columns (random positions) of nlev levels on a 32 x 12 domain of 2 km, observations of the four combined types of
    build_case (limits where the row has them), heights rising with the level and the pressure of a point = the mean of
    iv_p (das_letkf_amd passes that slot of gues as rlev).  west_empty: a quarter of the columns lie west of every
    horizontal cut-off (no survivors) beside columns among the observations; no_obs: all of them lie there."""
    k, nv, tables = COL_ROUTES[name][:3]
    nij1 = nij1 or (6 if k >= 144 else 40)
    nlev = nlev or (3 if k >= 144 else 4)
    rng = np.random.default_rng(seed)
    dens = max(1.0, k / 60.0)
    nobs_c = tuple(int(round(n * dens)) for n in (240, 160, 160, 80))
    tc = build_case(seed, nlon=32, nlat=12, dx=2000.0, nobs_per_ctype=nobs_c,
                    max_nobs=LIMITS if tables != "free" else (0, 0, 0, 0), criterion=2 if tables == "c2gen" else 1,
                    npts=nij1, obs_east_of=18.0 if (west_empty or no_obs) else None)
    tc["arr"]["varloc"] = np.array(VARLOC[tables])
    i_org = tc["scal"]["i_org"]
    rig, rjg = tc["pts"]["ri"].copy(), tc["pts"]["rj"].copy()
    nw = nij1 if no_obs else (max(1, nij1 // 4) if west_empty else 0)
    rig[:nw] = i_org + rng.uniform(0.5, 2.5, nw)          # > 15.5 grid lengths from every observation: cut-off 14.6 at most
    if west_empty:
        rig[nw:] = i_org + rng.uniform(16.0, 31.5, nij1 - nw)   # ... beside columns among the observations
    npts = nij1 * nlev
    zlev = np.linspace(300.0, 9000.0, nlev)
    rz = (zlev[:, None] + rng.uniform(-100.0, 100.0, (nlev, nij1))).ravel()
    rlev = 1.0e5 * np.exp(-rz / 7500.0)
    nobs = tc["nobs"]
    kld = k + 1
    ens = rng.standard_normal((nobs, kld))
    ens[:, :k] -= ens[:, :k].mean(axis=1, keepdims=True)
    dep = rng.standard_normal(nobs) * 1.5
    nens = k + 1 + int(det)
    x = rng.standard_normal((nv, nens, npts))
    x[:, :k] *= np.array([2.0, 2.0, 2.0, 1.0, 50.0] + [1e-3] * max(nv - 5, 0))[:nv, None, None]
    x[:, :k] -= x[:, :k].mean(axis=1, keepdims=True)
    mean = rng.standard_normal((nv, npts)) * 5.0 + 50.0
    if nv > 5:
        mean[5:] = np.abs(mean[5:]) * 1e-3 + 1e-3
    mean[4] = rlev
    x[:, k] = mean
    if det:
        x[:, k + 1] = mean + rng.standard_normal((nv, npts)) * np.abs(x[:, 0]).max(axis=1, keepdims=True)
    beta = np.ones(npts)
    beta[rng.integers(0, npts, size=max(1, npts // 10))] = 0.0
    beta[rng.integers(0, npts, size=max(1, npts // 10))] = 0.37
    if infl_flat:
        infl = np.tile(1.07 + 0.02 * rng.uniform(size=npts), nv)
    else:
        infl = 1.07 * (1.0 + 0.02 * np.arange(npts * nv) / (npts * nv))
    return dict(name=name, k=k, nv=nv, tables=tables, nij1=nij1, nlev=nlev, npts=npts, nens=nens, kld=kld, det=det, tc=tc,
                rig=rig, rjg=rjg, rlev=rlev, rz=rz, ensval=np.ascontiguousarray(ens), dep=dep,
                gues=np.ascontiguousarray(x).reshape(-1), beta=beta, infl=infl, sp=1, sm=npts, sv=npts * nens)


def oracle_lists(c, varloc=None):
    """obs_local of the oracle for every point p = ij + nij1*lev of c, with the class's var_local factors:
    (off, idx, rdiag, rloc, tied)"""
    tc = c["tc"]
    arr = dict(tc["arr"])
    arr["varloc"] = np.array(VARLOC[c["tables"]] if varloc is None else varloc, dtype=np.float64)
    h, keep = host_struct(dict(tc, arr=arr))
    nlev = c["nlev"]
    off, idx, rd, rl, tied = oracle_csr(h, np.tile(c["rig"], nlev), np.tile(c["rjg"], nlev), c["rlev"], c["rz"])
    return off, idx, rd, rl, tied.astype(bool)


def list_bytes(c, spec, off=None):
    if spec == "all":
        return BIG
    if spec == "columns":
        return 4096            # two chunks of 64 survivors: a column of two or more combined types fills a batch alone
    if spec == "level":
        return 1
    assert spec == "slabs"
    return max(1, int(20 * 1.5 * int(off[-1]) / c["nlev"]))


def oracle_class(c, cfg, mask, lists, beta, infl, want_rtps=True):
    k, nv, npts, nens = c["k"], c["nv"], c["npts"], c["nens"]
    off, idx, rd, rl = lists[:4]
    prm = _oracle.DasParams(k=k, nv=nv, det_run=int(c["det"]), infl_adaptive=cfg.get("infl_adaptive", 0),
                            relax_to_inflated_prior=cfg.get("relax_to_inflated_prior", 0),
                            relax_alpha=cfg.get("relax_alpha", 0.0), relax_alpha_spread=cfg.get("relax_alpha_spread", 0.0),
                            q_update_top=cfg.get("q_update_top", 0.0), q_sprd_max=cfg.get("q_sprd_max", 0.0), iv_p=4,
                            iv_q_first=5, iv_q_last=min(10, nv - 1), nthreads=8, var_mask=mask)
    r = _oracle.das_points(prm, off, idx, rd, rl, c["ensval"], c["dep"], beta, infl, c["gues"], 1, npts, npts * nens,
                           want_rtps=want_rtps)
    assert r["rc"] == 0
    return r


def oracle(c, classes, cfg=CFG, beta="case"):
    """das_letkf's loop for c, one oracle run per variable-localisation class [(mask, varloc)], each class keeping its own
    variables (as test_fortran_das.py composes it): anal (nv, nens, npts; NaN outside the classes), infl, rtps (npts*nv),
    counts of the first class's lists, tied points of any class"""
    k, nv, npts, nens = c["k"], c["nv"], c["npts"], c["nens"]
    b = c["beta"] if isinstance(beta, str) else beta
    anal = np.full((nv, nens, npts), np.nan)
    infl = c["infl"].copy()
    rtps = np.full(npts * nv, np.nan)
    tied = np.zeros(npts, bool)
    counts = None
    for mask, varloc in classes:
        lists = oracle_lists(c, varloc)
        tied |= lists[4]
        if counts is None:
            counts = np.diff(lists[0])
        r = oracle_class(c, cfg, mask, lists, b, c["infl"])
        ra = r["anal"].reshape(nv, nens, npts)
        for v in mask_vars(nv, mask):
            anal[v] = ra[v]
            infl[v * npts:(v + 1) * npts] = r["infl"][v * npts:(v + 1) * npts]
            rtps[v * npts:(v + 1) * npts] = r["rtps"][v * npts:(v + 1) * npts]
    return dict(anal=anal, infl=infl, rtps=rtps, counts=counts, tied=tied)


def field_view(c, layout, nlev_total=None, l0=0):
    """c's levels as levels l0 .. l0 + nlev - 1 of a field of nlev_total levels in one of the layouts of state_layout:
    (sp, sm, sv, off, size, p0, idx) with the FIELD's strides, p0 = l0 * nij1 the slab's first point, and idx the flat
    index of every element (v, m, p) of c's state, shaped (nv, nens, npts)"""
    nlev_total = nlev_total or c["nlev"]
    f = dict(c, npts=c["nij1"] * nlev_total)
    sp, sm, sv, off, size = state_layout(f, layout)
    p0 = l0 * c["nij1"]
    idx = state_index(f, sp, sm, sv, off)[:, :, p0:p0 + c["npts"]]
    return sp, sm, sv, off, size, p0, idx


def place_field(c, idx, size):
    buf = canary_buffer(size)
    buf[idx] = c["gues"].reshape(c["nv"], c["nens"], c["npts"])
    return buf
