"""letkf_das_columns_dev across the argument space include/letkf_amd.h (3c) allows, on every route of the entry, against the oracle
(tests/_colspace.py: obs_local by oracle_csr, the loop body by orc_das_letkf_points, one run per variable-localisation class).
The axes: the route table itself (list-free route in one and in many batches of columns, list route in one slab and one level per
slab with every solver family behind it, limited tables on the LDS column search and on the ring route), state layouts and a slab
of levels of a larger field, the observation table's leading dimension, the optional outputs and beta, var_mask and the two-class
pattern of das_letkf_amd, gues == anal, edge grids and argument errors.  Every element the call must not write starts as a
canary (anal: a signalling-NaN bit pattern; infl: the field's own values; rtps_infl_out: NaN; status / nsweep / nobs_out:
NOT_WRITTEN) and is compared bit for bit afterwards.  Tolerances as tests/test_gpu_das_argspace.py: 1e-10 per variable on the
analysis, 1e-12 on the inflation, 1e-11 relative on the RTPS factor.  Points where a limited group's selection fell between equal
keys (oracle_csr's `tied`) are left out of the value checks; they must stay a small share."""
import ctypes as C

import numpy as np
import pytest
import torch

from _argspace import CANARY, CFG, canary_buffer, mask_vars, members, obs_table
from _colspace import (AXIS_ROUTES, COL_ROUTES, DEFAULTS, OPTIONS, VARLOC, VARLOC_B, col_case, field_view, krylov,
                       list_bytes, oracle, place_field)

pytestmark = pytest.mark.gpu

NAN = float("nan")
NOT_WRITTEN = -(1 << 30)
OUTS = ("status", "nsweep", "rtps", "nobs")
E_INVALID = -1


class Run:
    """the device buffers of one call: the state of a field of nlev_total levels in a layout, c's levels at l0 .. (a slab view
    when nlev_total > nlev), the per-point / per-(point, variable) fields of the same field, prefilled"""

    def __init__(self, c, layout="ref", slab=None, outs=OUTS, alias=False, kld=None, table=None, beta="case"):
        from _gpu import dev
        from _search import device_struct
        nv, npts, nij1 = c["nv"], c["npts"], c["nij1"]
        nlev_total, l0 = slab or (c["nlev"], 0)
        self.c, self.nf = c, nij1 * nlev_total
        self.sp, self.sm, self.sv, self.off, size, self.p0, self.idx = field_view(c, layout, nlev_total, l0)
        g_host = place_field(c, self.idx, size)
        self.gues = dev(g_host)
        self.anal = self.gues if alias else dev(canary_buffer(size))
        self.anal_before = g_host if alias else canary_buffer(size)
        nf, p0 = self.nf, self.p0
        infl = 1.0 + 0.001 * np.arange(nf * nv)
        infl.reshape(nv, nf)[:, p0:p0 + npts] = c["infl"].reshape(nv, npts)
        self.infl_before = infl
        self.infl = dev(infl)
        b = c["beta"] if isinstance(beta, str) else beta
        self.beta_host = None if b is None else b
        if b is not None:
            bf = np.full(nf, NAN)
            bf[p0:p0 + npts] = b
            self.beta = dev(bf)
        else:
            self.beta = None
        i32 = lambda: torch.full((nf,), NOT_WRITTEN, dtype=torch.int32, device="cuda")
        self.outs = {"status": i32, "nsweep": i32, "nobs": i32,
                     "rtps": lambda: torch.full((nf * nv,), NAN, dtype=torch.float64, device="cuda")}
        self.outs = {o: self.outs[o]() for o in outs}
        self.kld = kld or c["k"] + 1
        self.table = dev(obs_table(c, self.kld, c["det"]) if table is None else table)
        self.dep = dev(c["dep"])
        self.rig, self.rjg, self.rlev, self.rz = dev(c["rig"]), dev(c["rjg"]), dev(c["rlev"]), dev(c["rz"])
        if alias and layout == "ref" and slab is None:
            # das_letkf_amd's call: rlev is the mean slot of iv_p inside gues itself (letkf_tools_amd.f90:322-323)
            o = self.off + c["k"] * self.sm + 4 * self.sv
            self.rlev = self.gues[o:o + npts]
            assert np.array_equal(self.rlev.cpu().numpy(), c["rlev"])
        self.t, self.keep = device_struct(c["tc"], "cuda")

    def view(self, t, scale=1):
        return None if t is None else t[self.p0 * scale:]

    def set_varloc(self, varloc):
        """the class's factors into the SAME table buffers (das_letkf_amd uploads them per class)"""
        from _search import ARRAY_FIELDS
        self.keep[ARRAY_FIELDS.index("varloc")].copy_(torch.tensor(varloc, dtype=torch.float64))


def ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def call(r, name, cfg=CFG, mask=0, lb=None, warm_run=0, npts=None, options=None, **raw):
    """letkf_das_columns_dev through the C ABI on the buffers of r (pointers at the slab's first point, infl_sv of the field);
    raw: DasArgs fields / coordinate pointers to override.  Returns (rc, last error)."""
    from _gpu import ctx, pkg
    c = r.c
    k, nv = c["k"], c["nv"]
    cx = ctx()
    a = pkg.DasArgs()
    a.k, a.nv, a.det_run = k, nv, int(c["det"])
    a.infl_adaptive = int(cfg.get("infl_adaptive", 0))
    a.relax_to_inflated_prior = int(cfg.get("relax_to_inflated_prior", 0))
    a.iv_p, a.iv_q_first, a.iv_q_last = 4, 5, min(10, nv - 1)
    a.relax_alpha, a.relax_alpha_spread = cfg.get("relax_alpha", 0.0), cfg.get("relax_alpha_spread", 0.0)
    a.q_update_top, a.q_sprd_max = cfg.get("q_update_top", 0.0), cfg.get("q_sprd_max", 0.0)
    a.npts = c["npts"] if npts is None else npts
    a.ensval, a.kld, a.dep = ptr(r.table), r.kld, ptr(r.dep)
    a.beta, a.infl = ptr(r.view(r.beta)), ptr(r.view(r.infl))
    o = r.off + r.p0 * r.sp
    a.gues, a.anal, a.sp, a.sm, a.sv = ptr(r.gues[o:]), ptr(r.anal[o:]), r.sp, r.sm, r.sv
    a.status, a.nsweep = ptr(r.view(r.outs.get("status"))), ptr(r.view(r.outs.get("nsweep")))
    a.rtps_infl_out = ptr(r.view(r.outs.get("rtps")))
    a.warm_run, a.var_mask, a.infl_sv = warm_run, mask, r.nf
    coords = dict(rig=r.rig, rjg=r.rjg, rlev=r.rlev, rz=r.rz)
    for f, v in raw.items():
        if f in coords:
            coords[f] = v
        else:
            setattr(a, f, v)
    nobs = r.view(r.outs.get("nobs"))
    opts = dict(DEFAULTS, **COL_ROUTES[name][3], **(options or {}))
    if lb is None:
        spec = COL_ROUTES[name][4]
        lb = list_bytes(c, spec, r.lists_off if spec == "slabs" else None)
    try:
        for o_, v in opts.items():
            cx.set_option(getattr(cx, OPTIONS[o_]), v)
        rc = cx._l.letkf_das_columns_dev(cx._c, C.byref(a), C.byref(r.t), C.c_int64(c["nij1"]), C.c_int32(c["nlev"]),
                                         ptr(coords["rig"]), ptr(coords["rjg"]), ptr(coords["rlev"]), ptr(coords["rz"]),
                                         C.c_int64(lb), ptr(nobs))
        torch.cuda.synchronize()
    finally:
        for o_, v in DEFAULTS.items():
            cx.set_option(getattr(cx, OPTIONS[o_]), v)
    return rc, cx._l.letkf_amd_last_error().decode()


def check_route(name):
    from _gpu import ctx
    path = ctx().last_path()
    for s in COL_ROUTES[name][5]:
        assert s in path, (name, path)
    for s in COL_ROUTES[name][6]:
        assert s not in path, (name, path)


def classes_of(c, mask=0, varloc=None):
    return [(mask, VARLOC[c["tables"]] if varloc is None else varloc)]


def check(r, ref, name, mask=0):
    """the class's variables of the slab against the oracle, every other element of every buffer bit for bit its prefill"""
    c = r.c
    k, nv, npts, nens, nf, p0 = c["k"], c["nv"], c["npts"], c["nens"], r.nf, r.p0
    ok = ~ref["tied"]
    assert ok.mean() >= 0.9, ("too many tied points", (~ok).sum())
    vs = mask_vars(nv, mask)
    # analysis
    got = r.anal.cpu().numpy()
    x = c["gues"].reshape(nv, nens, npts)
    mem = members(k, c["det"])
    written = np.zeros(got.size, bool)
    for v in vs:
        scale = max(np.abs(x[v, k]).max(), np.abs(x[v, :k]).max())
        sel = r.idx[v][mem]
        g = got[sel]
        assert np.isfinite(g).all(), v
        err = np.abs(g - ref["anal"][v][mem])[:, ok].max()
        assert err <= 1e-10 * scale, (v, err, scale)
        written[sel.ravel()] = True
    bad = np.flatnonzero((got.view(np.int64) != r.anal_before.view(np.int64)) & ~written)
    assert bad.size == 0, ("anal elements the call must not write were written", bad[:8], bad.size)
    # inflation: the class's slots of the slab are the oracle's, every other slot of the field unchanged
    gi = r.infl.cpu().numpy().reshape(nv, nf)
    wi = r.infl_before.reshape(nv, nf)
    inside = np.zeros((nv, nf), bool)
    inside[vs, p0:p0 + npts] = True
    assert np.array_equal(gi[~inside], wi[~inside])
    ri = ref["infl"].reshape(nv, npts)
    assert np.abs(gi[vs, p0:p0 + npts][:, ok] - ri[vs][:, ok]).max() <= 1e-12
    # RTPS factor
    if "rtps" in r.outs:
        g = r.outs["rtps"].cpu().numpy().reshape(nv, nf)
        assert np.isnan(g[~inside]).all()
        e = ref["rtps"].reshape(nv, npts)[vs]
        gs = g[vs, p0:p0 + npts]
        assert np.isfinite(gs).all()
        assert np.abs(gs[:, ok] - e[:, ok]).max() <= 1e-11 * np.abs(e).max()
    pts = np.zeros(nf, bool)
    pts[p0:p0 + npts] = True
    beta = r.beta_host if r.beta_host is not None else np.ones(npts)
    live = beta != 0.0
    if "status" in r.outs:
        st = r.outs["status"].cpu().numpy()
        assert (st[~pts] == NOT_WRITTEN).all() and (st[pts] == 0).all(), st[pts]
    if "nobs" in r.outs:
        nb = r.outs["nobs"].cpu().numpy()
        assert (nb[~pts] == NOT_WRITTEN).all()
        assert np.array_equal(nb[pts], np.where(live, ref["counts"], 0)), (nb[pts], ref["counts"])
    if "nsweep" in r.outs:
        ns = r.outs["nsweep"].cpu().numpy()
        assert (ns[~pts] == NOT_WRITTEN).all()
        ns = ns[pts]
        solve = live & (ref["counts"] > 0)
        assert (ns[~solve] == 0).all(), ns
        if krylov(name):
            assert (ns[solve] != 0).all() and (not solve.any() or (ns[solve] < 0).any()), ns
        else:
            assert (ns[solve] > 0).all(), ns


def run(c, name, layout="ref", slab=None, outs=OUTS, mask=0, varloc=None, cfg=CFG, beta="case", route=True, **kw):
    """one call of the route's row on c, checked against the oracle; returns the Run"""
    ref = oracle(c, classes_of(c, mask, varloc), cfg=cfg, beta=beta)
    r = Run(c, layout=layout, slab=slab, outs=outs, beta=beta, **{k_: kw.pop(k_) for k_ in ("alias", "kld", "table") if k_ in kw})
    r.lists_off = np.concatenate([[0], np.cumsum(ref["counts"])])
    if varloc is not None:
        r.set_varloc(varloc)
    rc, err = call(r, name, cfg=cfg, mask=mask, **kw)
    assert rc == 0, err
    if route:
        check_route(name)
    check(r, ref, name, mask)
    return r


# ---------------------------------------------------------------------------------------------------------------------
# 1. the route table
@pytest.mark.parametrize("name", list(COL_ROUTES))
def test_route_table(name):
    """every row lands on its route (ctx().last_path() of the last loop-body launch) with every optional output, and every
    buffer is the oracle's answer or untouched"""
    c = col_case(name, seed=11 + COL_ROUTES[name][0])
    run(c, name)


# ---------------------------------------------------------------------------------------------------------------------
# 2a. state layouts, and a slab of levels of a larger field in each of them
@pytest.mark.parametrize("layout,slab", [("member", None), ("var", None), ("padded", None), ("ref", (3, 2)),
                                         ("member", (0, 3)), ("var", (4, 0)), ("padded", (2, 3))],
                         ids=["member", "var", "padded", "ref-slab", "member-slab", "var-slab", "padded-slab"])
@pytest.mark.parametrize("name", AXIS_ROUTES)
def test_layouts_and_slab_views(name, layout, slab):
    """the state in another layout, or levels l0 .. l1 of an nlev_total field: gues, anal, beta, infl, rtps, status, nsweep and
    nobs_out at the slab's first point with the FIELD's strides and infl_sv, rlev / rz of the slab only; everything outside the
    slab stays canary (anal) or its prefill"""
    c = col_case(name, seed=21 + COL_ROUTES[name][0], det=layout != "member")
    if slab:                                     # (levels below the slab, levels above it) -> (nlev_total, l0)
        slab = (slab[0] + c["nlev"] + slab[1], slab[0])
    run(c, name, layout=layout, slab=slab)


# 2b. the observation table's leading dimension
@pytest.mark.parametrize("dk,det", [(0, False), (1, False), (1, True), (2, True), (7, False), (7, True)],
                         ids=["kld_eq_k", "kld_k_plus_1", "kld_k_plus_1_det", "kld_k_plus_2_det", "kld_k_plus_7",
                              "kld_k_plus_7_det"])
@pytest.mark.parametrize("name", AXIS_ROUTES)
def test_obs_table_leading_dimension(name, dk, det):
    """kld = k .. k + 7, every column the call must not read (column k without DET_RUN, the padding) NaN and a NaN tail: the
    oracle's answer, and the dense table's answer bit for bit with the same stage per point (nsweep's sign)"""
    c = col_case(name, seed=41 + COL_ROUTES[name][0], det=det)
    k = c["k"]
    r = run(c, name, kld=k + dk)
    dense = run(c, name, kld=k + 1, table=np.concatenate([c["ensval"].ravel(), np.full(64, NAN)]))
    assert np.array_equal(r.anal.cpu().numpy().view(np.int64), dense.anal.cpu().numpy().view(np.int64))
    assert np.array_equal(np.sign(r.outs["nsweep"].cpu().numpy()), np.sign(dense.outs["nsweep"].cpu().numpy()))


# 2c. the optional outputs and beta
@pytest.mark.parametrize("which", ["none", "status", "nsweep", "rtps", "nobs", "all"])
@pytest.mark.parametrize("name", AXIS_ROUTES)
def test_optional_outputs(name, which):
    """each output alone, all, none: each is the oracle's where the call writes it; the analysis does not depend on them"""
    c = col_case(name, seed=51 + COL_ROUTES[name][0])
    outs = () if which == "none" else OUTS if which == "all" else (which,)
    plain = run(c, name, outs=())
    r = run(c, name, outs=outs)
    assert np.array_equal(r.anal.cpu().numpy().view(np.int64), plain.anal.cpu().numpy().view(np.int64))


@pytest.mark.parametrize("kind", ["null", "columns_and_levels", "fractions"])
@pytest.mark.parametrize("name", AXIS_ROUTES)
def test_beta(name, kind):
    """beta NULL (1 everywhere), beta = 0 on whole columns and on every other level of others, beta in (0, 1) beside them"""
    c = col_case(name, seed=61 + COL_ROUTES[name][0])
    nij1, nlev = c["nij1"], c["nlev"]
    if kind == "null":
        beta = None
    else:
        beta = np.ones((nlev, nij1))
        if kind == "columns_and_levels":
            beta[:, : nij1 // 4] = 0.0
            beta[0::2, nij1 // 4: nij1 // 2] = 0.0
        else:
            beta[:, ::3] = 0.25
            beta[1::2, 1::3] = 0.0
        beta = beta.ravel()
    run(c, name, beta=beta)


# 2d. variable-localisation classes
MASKS = {"wind": 0b111, "moisture": None}


@pytest.mark.parametrize("mask_name", list(MASKS))
@pytest.mark.parametrize("name", AXIS_ROUTES)
def test_var_mask(name, mask_name):
    """one class of a few variables (3-D wind; the moisture species under Q_UPDATE_TOP, which moves the inflation slot that
    drives the solve where a point's pressure is below it): variables, infl and RTPS entries outside the class untouched"""
    c = col_case(name, seed=71 + COL_ROUTES[name][0])
    nv = c["nv"]
    mask = MASKS[mask_name] or sum(1 << v for v in range(5, nv))
    cfg = dict(CFG, q_update_top=6.0e4) if mask_name == "moisture" else CFG
    run(c, name, mask=mask, cfg=cfg)


@pytest.mark.parametrize("name", ["free_k33", "free_batches", "list_trio20", "list_wave1", "list_staged_poly", "list_levels",
                                  "lim_lds", "lim_rings", "lim_rings_gen"])
def test_two_classes_like_das_letkf_amd(name):
    """das_letkf_amd's pattern: one call per class on the SAME anal / infl / table buffers, complementary masks, the class's
    var_local factors uploaded into the table's varloc between the calls.  On the ring route the second call must not reuse
    the survivors the first one kept (RingKeep)."""
    c = col_case(name, seed=81 + COL_ROUTES[name][0])
    nv, tables = c["nv"], c["tables"]
    ma, mb = 0b11111, sum(1 << v for v in range(5, nv))
    cls = [(ma, VARLOC[tables]), (mb, VARLOC_B[tables])]
    ref = oracle(c, cls)
    r = Run(c)
    r.lists_off = np.concatenate([[0], np.cumsum(ref["counts"])])
    for mask, vl in cls:
        r.set_varloc(vl)
        rc, err = call(r, name, mask=mask)
        assert rc == 0, err
        check_route(name)
    check(r, ref, name)


# 2e. gues == anal
@pytest.mark.parametrize("name", AXIS_ROUTES)
def test_in_place(name):
    """anal is gues, in the reference layout with rlev inside the same buffer (the mean slot of iv_p, das_letkf_amd's call): the
    mean slot comes back unchanged; on the list-free route the answer is the out-of-place one bit for bit (the same kernel), on
    the list route within 1e-11 (at k <= 20 the call leaves the three-points-per-wave kernel)"""
    c = col_case(name, seed=91 + COL_ROUTES[name][0])
    out = run(c, name)
    inp = run(c, name, alias=True, route=not name.startswith("list_trio") and name != "lim_lds")
    a, b = inp.anal.cpu().numpy(), out.anal.cpu().numpy()
    k, nv, nens, npts = c["k"], c["nv"], c["nens"], c["npts"]
    x = c["gues"].reshape(nv, nens, npts)
    mem = members(k, c["det"])
    for v in range(nv):
        sel = out.idx[v][mem]
        if COL_ROUTES[name][5][0].startswith("FUSED"):
            assert np.array_equal(a[sel].view(np.int64), b[sel].view(np.int64)), v
        else:
            scale = max(np.abs(x[v, k]).max(), np.abs(x[v, :k]).max())
            assert np.abs(a[sel] - b[sel]).max() <= 1e-11 * scale, v
        assert np.array_equal(a[out.idx[v][k]], x[v, k])


# 2f. edges
EDGES = ["one_column", "one_level", "no_observations", "all_beta_zero", "empty_columns", "warm_run_1", "warm_run_3"]


@pytest.mark.parametrize("edge", EDGES)
@pytest.mark.parametrize("name", AXIS_ROUTES)
def test_edges(name, edge):
    k = COL_ROUTES[name][0]
    seed = 101 + k
    kw = {}
    if edge == "one_column":
        c = col_case(name, seed, nij1=1, nlev=5)
    elif edge == "one_level":
        c = col_case(name, seed, nlev=1)
    elif edge == "no_observations":
        c = col_case(name, seed, no_obs=True)
    elif edge == "empty_columns":
        c = col_case(name, seed, west_empty=True)
    else:
        c = col_case(name, seed)
    if edge == "all_beta_zero":
        c["beta"][:] = 0.0
    if edge.startswith("warm_run"):
        kw["warm_run"] = int(edge[-1])
    ref_counts = oracle(c, classes_of(c))["counts"]
    if edge == "no_observations":
        assert (ref_counts == 0).all()
    if edge == "empty_columns":
        cnt = ref_counts.reshape(c["nlev"], c["nij1"])
        assert (cnt[:, : c["nij1"] // 4] == 0).all() and (cnt[:, c["nij1"] // 4:] > 0).mean() > 0.75
    # (no point to solve: the last launch may be the streaming pre-pass alone)
    trivial = edge in ("no_observations", "all_beta_zero")
    run(c, name, route=not trivial, **kw)


# 2g. argument errors
@pytest.mark.parametrize("error", ["npts", "trans_out", "transm_out", "pa_out", "kld", "kld_det", "rig", "rjg", "rlev", "rz"])
@pytest.mark.parametrize("name", ["free_k20", "list_wave1", "lim_rings"])
def test_argument_errors_write_nothing(name, error):
    """LETKF_E_INVALID, and every output buffer (anal, infl, rtps, status, nsweep, nobs_out) still holds its prefill"""
    det = error != "kld"
    c = col_case(name, seed=5, det=det)
    r = Run(c, kld=c["k"] + 1 if det else c["k"])
    r.lists_off = np.concatenate([[0], np.cumsum(np.full(c["npts"], 50))])
    raw = {}
    if error == "npts":
        raw["npts"] = c["npts"] - 1
    elif error in ("trans_out", "transm_out", "pa_out"):
        n = c["npts"] * (c["k"] if error == "transm_out" else c["k"] ** 2)
        bad = torch.full((n,), NAN, dtype=torch.float64, device="cuda")
        raw[error] = ptr(bad)
    elif error.startswith("kld"):
        r.kld = c["k"] - 1 + int(det)           # one column short
    else:
        raw[error] = None
    rc, err = call(r, name, **raw)
    assert rc == E_INVALID, (rc, err)
    assert (r.anal.cpu().numpy().view(np.int64) == CANARY).all()
    assert np.array_equal(r.infl.cpu().numpy(), r.infl_before)
    assert np.isnan(r.outs["rtps"].cpu().numpy()).all()
    for o in ("status", "nsweep", "nobs"):
        assert (r.outs[o].cpu().numpy() == NOT_WRITTEN).all(), o
    if error in ("trans_out", "transm_out", "pa_out"):
        assert torch.isnan(bad).all()
