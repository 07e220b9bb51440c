"""letkf_das_points_dev across the argument space include/letkf_amd.h allows, on every solver route, against the oracle.
The axes: the route table itself (which inputs land where, tests/_argspace.py ROUTES), state layouts and slab views, the
observation table's leading dimension, the optional outputs, var_mask, edge batches and gues == anal.  Every element the
call must not write starts as a canary bit pattern and is compared bit for bit afterwards; every column of the observation
table the call must not read is NaN.  Tolerances as tests/test_gpu_das.py: 1e-10 per variable on the analysis, 1e-12 on the
inflation, 1e-11 relative on T, w-bar and Pa."""
import numpy as np
import pytest
import torch

import _oracle
from _argspace import (AXIS_ROUTES, CANARY, CFG, ROUTES, canary_buffer, mask_vars, members, obs_table, place_state,
                       route_case, state_index, state_layout)
from _cases import das_case

pytestmark = pytest.mark.gpu

NAN = float("nan")
NOT_WRITTEN = -(1 << 30)   # integer outputs' prefill (nsweep = -7 is a point the Krylov stage solved in 7 iterations)


def oracle(c, cfg, det, mask=0, want_trans=False, want_pa=False, want_rtps=False):
    k, nv = c["k"], c["nv"]
    prm = _oracle.DasParams(k=k, nv=nv, det_run=int(det), infl_adaptive=cfg.get("infl_adaptive", 0),
                            relax_to_inflated_prior=cfg.get("relax_to_inflated_prior", 0),
                            relax_alpha=cfg.get("relax_alpha", 0.0), relax_alpha_spread=cfg.get("relax_alpha_spread", 0.0),
                            q_update_top=cfg.get("q_update_top", 0.0), q_sprd_max=cfg.get("q_sprd_max", 0.0), iv_p=4,
                            iv_q_first=5, iv_q_last=min(10, nv - 1), nthreads=4, var_mask=mask)
    r = _oracle.das_points(prm, c["obs_off"], c["obs_idx"], c["rdiag"], c["rloc"], c["ensval"], c["dep"], c["beta"],
                           c["infl"], c["gues"], c["sp"], c["sm"], c["sv"], want_trans=want_trans, want_pa=want_pa,
                           want_rtps=want_rtps)
    assert r["rc"] == 0
    return r


def call(c, cfg, det, gues, anal, infl, sp, sm, sv, kld=None, table=None, infl_sv=0, mask=0, **outs):
    """letkf_das_points_dev on device buffers (gues / anal / infl may be views); returns the library's return code"""
    from _gpu import ctx, dev
    k, nv = c["k"], c["nv"]
    kld = kld or k + 1
    table = obs_table(c, kld, det) if table is None else table
    try:
        ctx().das_points(k, nv, dev(c["obs_off"]), dev(c["obs_idx"]), dev(c["rdiag"]), dev(c["rloc"]), dev(table), kld,
                         dev(c["dep"]), infl, gues, anal, sp, sm, sv, beta=dev(c["beta"]), det_run=det,
                         infl_adaptive=cfg.get("infl_adaptive", 0),
                         relax_to_inflated_prior=cfg.get("relax_to_inflated_prior", 0),
                         relax_alpha=cfg.get("relax_alpha", 0.0), relax_alpha_spread=cfg.get("relax_alpha_spread", 0.0),
                         q_update_top=cfg.get("q_update_top", 0.0), q_sprd_max=cfg.get("q_sprd_max", 0.0), iv_p=4,
                         iv_q_first=5, iv_q_last=min(10, nv - 1), var_mask=mask, infl_sv=infl_sv, **outs)
    except RuntimeError as e:                                      # (LetkfError)
        torch.cuda.synchronize()
        return str(e)
    torch.cuda.synchronize()
    return 0


def route_options(name=None):
    """the context options a route needs (None: the library's defaults)"""
    from _gpu import ctx
    ctx().set_option(ctx().OPT_STAGED_POLY, 0 if name and ROUTES[name][2] == "nopoly" else 1)


def kk_outputs(name, c):
    """the k x k outputs that select the route (ROUTES[name][2])"""
    k, npts = c["k"], c["npts"]
    kind = ROUTES[name][2]
    if kind == "trans":
        return dict(trans_out=torch.full((npts, k * k), NAN, dtype=torch.float64, device="cuda"))
    if kind == "pa":
        return dict(pa_out=torch.full((npts, k * k), NAN, dtype=torch.float64, device="cuda"))
    return {}


def check_route(name):
    from _gpu import ctx
    path = ctx().last_path()
    for s in ROUTES[name][3]:
        assert s in path, (name, path)
    for s in ROUTES[name][4]:
        assert s not in path, (name, path)


def check_state(c, ref, got, before, idx, det, mask=0):
    """the analysis of the members of the class's variables against the oracle (1e-10 per variable, as compare_anal);
    every other element of the buffer bit for bit what it held before the call"""
    k, nv = c["k"], c["nv"]
    x = c["gues"].reshape(nv, c["nens"], c["npts"])
    e = ref["anal"].reshape(nv, c["nens"], c["npts"])
    mem = members(k, det)
    written = np.zeros(got.size, bool)
    for v in mask_vars(nv, mask):
        scale = max(np.abs(x[v, k]).max(), np.abs(x[v, :k]).max())
        g = got[idx[v][mem]]
        assert np.isfinite(g).all(), v
        err = np.abs(g - e[v, mem]).max()
        assert err <= 1e-10 * scale, (v, err, scale)
        written[idx[v][mem].ravel()] = True
    b, a = before.view(np.int64), got.view(np.int64)
    bad = np.flatnonzero((a != b) & ~written)
    assert bad.size == 0, ("elements the call must not write were written", bad[:8], bad.size)


def check_infl(c, ref, infl):
    assert np.abs(infl - ref["infl"]).max() <= 1e-12


def state_run(name, c, layout, det, cfg=CFG, mask=0, kld=None, table=None, alias=False, outs=None, route=True):
    """das_case c in the given layout; the analysis, the inflation and every untouched element checked against the oracle.
    Returns (oracle answer, host copy of anal's buffer, index of the state elements, outputs, inflation)."""
    from _gpu import dev
    sp, sm, sv, off, size = state_layout(c, layout)
    g_host = place_state(c, sp, sm, sv, off, size)
    gues = dev(g_host)
    anal = gues if alias else dev(canary_buffer(size))
    before = g_host if alias else canary_buffer(size)
    infl = dev(c["infl"])
    outs = dict(kk_outputs(name, c) if outs is None else outs)
    route_options(name)
    try:
        rc = call(c, cfg, det, gues[off:], anal[off:], infl, sp, sm, sv, kld=kld, table=table, mask=mask, **outs)
        assert rc == 0, rc
        if route and outs.keys() == kk_outputs(name, c).keys():
            check_route(name)
    finally:
        route_options()
    ref = oracle(c, cfg, det, mask=mask)
    idx = state_index(c, sp, sm, sv, off)
    got = anal.cpu().numpy()
    check_state(c, ref, got, before, idx, det, mask)
    got_infl = infl.cpu().numpy()
    check_infl(c, ref, got_infl)
    return ref, got, idx, outs, got_infl


# ---------------------------------------------------------------------------------------------------------------------
# A. the route table
@pytest.mark.parametrize("name", [n for n in ROUTES if n])
def test_route_table(name):
    """every row of ROUTES lands on its route (ctx().last_path()) and gives the oracle's analysis there"""
    c = route_case(name, seed=11 + ROUTES[name][0], det=True)
    state_run(name, c, "ref", det=True)


def test_trivial_points_only():
    """every point without observations or with beta = 0: no solve, the analysis is still the reference's (:333-359)"""
    for name in ("trio20", "wave1", "staged_poly", "point"):
        c = route_case(name, seed=5, det=True)
        n = np.diff(c["obs_off"])
        assert (n == 0).any() and (n > 0).any()
        c["beta"][n > 0] = 0.0
        state_run(name, c, "ref", det=True, route=False)


# ---------------------------------------------------------------------------------------------------------------------
# B1. state layouts
@pytest.mark.parametrize("layout,det", [("ref", True), ("member", False), ("var", False), ("padded", True),
                                        ("padded", False)])
@pytest.mark.parametrize("name", AXIS_ROUTES)
def test_state_layouts(name, layout, det):
    c = route_case(name, seed=21 + ROUTES[name][0], det=det)
    state_run(name, c, layout, det)


# B2. a slab of levels of a larger field
@pytest.mark.parametrize("name", AXIS_ROUTES)
def test_slab_view(name):
    """gues + p0, anal + p0, infl + p0 and rtps_infl_out + p0 with the FIELD's strides and infl_sv (das_letkf_amd's call
    for a slab of levels): the slab is the oracle's answer, every other level of the field bit for bit untouched"""
    from _gpu import dev
    det = True
    c = route_case(name, seed=31 + ROUTES[name][0], det=det)
    k, nv, npts, nens = c["k"], c["nv"], c["npts"], c["nens"]
    nf, p0 = 3 * npts + 5, npts + 2                      # field points; the slab's first point
    f = das_case(k=k, nv=nv, npts=nf, nobs_tot=50, n_mean=5, seed=99, det_run=det)   # the other levels' contents
    fg = f["gues"].reshape(nv, nens, nf)
    fg[:, :, p0:p0 + npts] = c["gues"].reshape(nv, nens, npts)
    sp, sm, sv = 1, nf, nf * nens
    gues = dev(fg.reshape(-1))
    anal_host = canary_buffer(fg.size)
    anal = dev(anal_host)
    infl_f = 1.0 + 0.001 * np.arange(nf * nv)
    infl_f.reshape(nv, nf)[:, p0:p0 + npts] = c["infl"].reshape(nv, npts)
    infl = dev(infl_f)
    rtps = torch.full((nf * nv,), NAN, dtype=torch.float64, device="cuda")
    route_options(name)
    try:
        outs = kk_outputs(name, c)
        rc = call(c, CFG, det, gues[p0:], anal[p0:], infl[p0:], sp, sm, sv, infl_sv=nf, rtps_infl_out=rtps[p0:], **outs)
        assert rc == 0, rc
        check_route(name)
    finally:
        route_options()
    ref = oracle(c, CFG, det, want_rtps=True)
    idx = state_index(c, sp, sm, sv, p0)
    check_state(c, ref, anal.cpu().numpy(), anal_host, idx, det)
    got_infl = infl.cpu().numpy().reshape(nv, nf)
    want_infl = infl_f.reshape(nv, nf).copy()
    want_infl[:, p0:p0 + npts] = ref["infl"].reshape(nv, npts)   # scattered back: the oracle's infl is dense (pt + npts*v)
    outside = np.ones(nf, bool)
    outside[p0:p0 + npts] = False
    assert np.array_equal(got_infl[:, outside], want_infl[:, outside])
    assert np.abs(got_infl - want_infl).max() <= 1e-12
    r = rtps.cpu().numpy().reshape(nv, nf)
    assert np.isnan(r[:, outside]).all()
    assert np.abs(r[:, p0:p0 + npts] - ref["rtps"].reshape(nv, npts)).max() <= 1e-11 * np.abs(ref["rtps"]).max()


# ---------------------------------------------------------------------------------------------------------------------
# B3. the observation table's leading dimension
@pytest.mark.parametrize("dk,det", [(0, False), (1, False), (2, True), (7, False)],
                         ids=["kld_eq_k", "kld_k_plus_1", "kld_k_plus_2_det", "kld_k_plus_7"])
@pytest.mark.parametrize("name", AXIS_ROUTES)
def test_obs_table_leading_dimension(name, dk, det):
    """kld = k (the reference's own shape without DET_RUN: obsda_sort%ensval(MEMBER, nobs)), k + 1, k + 2, k + 7; every
    column the call must not read is NaN, the table sits at the start of an allocation with a NaN tail.  Beside the analysis:
    the same points as with the dense table are solved by the same stage (nsweep > 0 Jacobi, < 0 Krylov) -- a NaN met by
    the eigen-free stage sends its point to the eigen stage instead of into the analysis."""
    c = route_case(name, seed=41 + ROUTES[name][0], det=det)
    k = c["k"]
    ns = []
    for kld, table in ((k + dk, None), (k + 1, np.concatenate([c["ensval"].ravel(), np.full(64, np.nan)]))):
        nsweep = torch.full((c["npts"],), NOT_WRITTEN, dtype=torch.int32, device="cuda")
        outs = dict(kk_outputs(name, c), nsweep=nsweep)
        state_run(name, c, "ref", det, kld=kld, table=table, outs=outs)
        ns.append(nsweep.cpu().numpy())
    assert np.array_equal(np.sign(ns[0]), np.sign(ns[1])), (ns[0], ns[1])


@pytest.mark.parametrize("det", [False, True])
def test_kld_too_small_is_refused(det):
    from _gpu import dev
    c = route_case("wave1", seed=3, det=det)
    k = c["k"]
    kld = k - 1 + (1 if det else 0)
    sp, sm, sv, off, size = state_layout(c, "ref")
    anal = dev(canary_buffer(size))
    infl = dev(c["infl"])
    status = torch.full((c["npts"],), NOT_WRITTEN, dtype=torch.int32, device="cuda")
    rc = call(c, CFG, det, dev(place_state(c, sp, sm, sv, off, size)), anal, infl, sp, sm, sv, kld=kld,
              table=np.full(c["ensval"].size, np.nan), status=status)
    assert rc != 0 and "kld" in rc, rc
    assert (anal.cpu().numpy().view(np.int64) == CANARY).all()
    assert np.array_equal(infl.cpu().numpy(), c["infl"])
    assert (status.cpu().numpy() == NOT_WRITTEN).all()


# ---------------------------------------------------------------------------------------------------------------------
# B4. the optional outputs
OUTPUTS = ["trans_out", "transm_out", "pa_out", "rtps_infl_out", "status", "nsweep"]


@pytest.mark.parametrize("which", OUTPUTS + ["all"])
@pytest.mark.parametrize("name", AXIS_ROUTES)
def test_optional_outputs(name, which):
    """each output alone and all together, every buffer prefilled (NaN, NOT_WRITTEN): T, w-bar and Pa are the oracle's at every
    point it writes them (n = 0 points: sqrt(rho) I, rho / (k - 1) I, common_letkf.f90:89-107) and untouched at beta = 0
    points, where the oracle skips letkf_core (letkf_tools.f90:333-359); status and the RTPS factor are written at every
    point; the analysis with outputs is the one without them (they change the route at 63 <= k <= 100)"""
    det = True
    c = route_case(name, seed=51 + ROUTES[name][0], det=det)
    k, nv, npts = c["k"], c["nv"], c["npts"]
    f = lambda *shape: torch.full(shape, NAN, dtype=torch.float64, device="cuda")
    i = lambda: torch.full((npts,), NOT_WRITTEN, dtype=torch.int32, device="cuda")
    make = dict(trans_out=lambda: f(npts, k * k), transm_out=lambda: f(npts, k), pa_out=lambda: f(npts, k * k),
                rtps_infl_out=lambda: f(npts * nv), status=i, nsweep=i)
    outs = {w: make[w]() for w in (OUTPUTS if which == "all" else [which])}
    _, anal_plain, idx, _, _ = state_run(name, c, "ref", det, outs=kk_outputs(name, c))
    _, anal_out, _, outs, _ = state_run(name, c, "ref", det, outs=outs)
    x = c["gues"].reshape(nv, c["nens"], npts)
    for v in range(nv):
        scale = max(np.abs(x[v, k]).max(), np.abs(x[v, :k]).max())
        a, b = anal_out[idx[v][members(k, det)]], anal_plain[idx[v][members(k, det)]]
        assert np.abs(a - b).max() <= 1e-11 * scale, v
    ref = oracle(c, CFG, det, want_trans=True, want_pa=True, want_rtps=True)
    live = c["beta"] != 0.0
    for key, rkey in (("trans_out", "trans"), ("transm_out", "transm"), ("pa_out", "pa")):
        if key not in outs:
            continue
        g = outs[key].cpu().numpy()
        assert np.isnan(g[~live]).all(), key                        # beta = 0: not written (include/letkf_amd.h)
        for p in np.flatnonzero(live):
            e = ref[rkey][p]
            assert np.abs(g[p] - e).max() <= 1e-11 * max(np.abs(e).max(), 1.0 if rkey == "transm" else 0.0), (key, p)
    if "rtps_infl_out" in outs:
        g = outs["rtps_infl_out"].cpu().numpy()
        assert np.isfinite(g).all()
        assert np.abs(g - ref["rtps"]).max() <= 1e-11 * np.abs(ref["rtps"]).max()
        assert (g[np.repeat(~live[None, :], nv, 0).ravel()] == 1.0).all()
    if "status" in outs:
        st = outs["status"].cpu().numpy()
        assert np.isin(st, (0, 3)).all(), st
        assert (st[~live] == 0).all()
    if "nsweep" in outs:
        ns = outs["nsweep"].cpu().numpy()
        assert (ns != NOT_WRITTEN).all(), ns
        assert (ns[(np.diff(c["obs_off"]) == 0) | ~live] == 0).all(), ns


# ---------------------------------------------------------------------------------------------------------------------
# B5. var_mask
MASKS = {"scattered": 0b10100110101, "single": 1 << 3, "no_iv_p": 0b11111101111, "q_first": 0b11111100000}


@pytest.mark.parametrize("mask_name", list(MASKS))
@pytest.mark.parametrize("name", AXIS_ROUTES)
def test_var_mask(name, mask_name):
    """non-contiguous, single-variable, without iv_p while Q_UPDATE_TOP is on, and starting in the q range (the inflation
    slot that drives the solve moves, letkf_wave.hip v0): the class's variables are the oracle's, every other variable,
    its infl and its RTPS factor untouched"""
    det = True
    c = route_case(name, seed=61 + ROUTES[name][0], det=det)
    nv, npts = c["nv"], c["npts"]
    mask = MASKS[mask_name] & ((1 << nv) - 1)
    assert mask
    cfg = dict(CFG, q_update_top=49.0)
    rtps = torch.full((npts * nv,), NAN, dtype=torch.float64, device="cuda")
    _, _, _, _, infl = state_run(name, c, "padded", det, cfg=cfg, mask=mask,
                                 outs=dict(kk_outputs(name, c), rtps_infl_out=rtps))
    ref = oracle(c, cfg, det, mask=mask, want_rtps=True)
    g = rtps.cpu().numpy().reshape(nv, npts)
    e = ref["rtps"].reshape(nv, npts)
    for v in range(nv):
        if (mask >> v) & 1:
            assert np.abs(g[v] - e[v]).max() <= 1e-11 * np.abs(e).max(), v
        else:
            assert np.isnan(g[v]).all(), v
    outside = [v for v in range(nv) if not (mask >> v) & 1]
    assert np.array_equal(infl.reshape(nv, npts)[outside], c["infl"].reshape(nv, npts)[outside])


# ---------------------------------------------------------------------------------------------------------------------
# B6. edge batches
@pytest.mark.parametrize("name", AXIS_ROUTES)
def test_edge_batches(name):
    """npts = 0 (nothing written), npts = 1, a batch without any local observation, and points with n = 1, k - 1, k, k + 1
    local observations (the staged path turns from observation space to ensemble space at n < k)"""
    from _gpu import dev
    det = True
    k = ROUTES[name][0]
    # npts = 0: OK, nothing written
    c = route_case(name, seed=71, det=det, npts=1)
    sp, sm, sv, off, size = state_layout(c, "ref")
    anal = dev(canary_buffer(size))
    from _gpu import ctx
    ctx().das_points(k, c["nv"], dev(np.zeros(1, np.int64)), dev(np.zeros(0, np.int32)), dev(np.zeros(0)), dev(np.zeros(0)),
                     dev(obs_table(c, k + 1, det)), k + 1, dev(c["dep"]), dev(c["infl"]), dev(c["gues"]), anal, sp, sm, sv,
                     det_run=det)
    torch.cuda.synchronize()
    assert (anal.cpu().numpy().view(np.int64) == CANARY).all()
    # npts = 1
    c = route_case(name, seed=72, det=det, npts=1, n_mean=k // 2 + 1, vary_n=False)
    c["beta"][:] = 1.0
    state_run(name, c, "padded", det)
    # no local observation anywhere
    c = route_case(name, seed=73, det=det)
    c["obs_off"][:] = 0
    c["obs_idx"], c["rdiag"], c["rloc"] = c["obs_idx"][:0], c["rdiag"][:0], c["rloc"][:0]
    state_run(name, c, "ref", det, route=False)
    # n = 1, k - 1, k, k + 1 at every point, beta = 1
    c = route_case(name, seed=74, det=det, npts=8)
    rng = np.random.default_rng(74)
    counts = np.array([1, k - 1, k, k + 1] * 2, dtype=np.int64)
    nobs_tot = c["ensval"].size // c["kld"]
    off = np.zeros(9, dtype=np.int64)
    np.cumsum(counts, out=off[1:])
    c["obs_off"] = off
    c["obs_idx"] = np.concatenate([rng.choice(nobs_tot, size=n, replace=False) for n in counts]).astype(np.int32)
    c["rloc"] = np.exp(-0.5 * rng.uniform(0.0, 13.0, size=int(off[-1])))
    c["rdiag"] = rng.choice([1.0, 9.0, 25.0], size=int(off[-1])) / c["rloc"]
    c["beta"][:] = 1.0
    state_run(name, c, "ref", det)


# ---------------------------------------------------------------------------------------------------------------------
# B7. gues == anal
@pytest.mark.parametrize("name", AXIS_ROUTES)
def test_in_place(name):
    """anal aliasing gues exactly: the out-of-place answer within 1e-11, and the elements the call must not write (the mean
    slot among them) keep what gues held there (include/letkf_amd.h).  At k <= 20 the three-points-per-wave kernel needs the
    streaming pass, which is off in place: such calls take the one-wave kernel (letkf_trivial.hip trivial_pass_supports)."""
    det = True
    c = route_case(name, seed=81 + ROUTES[name][0], det=det)
    _, out_of_place, idx, _, infl_a = state_run(name, c, "padded", det)
    _, in_place, _, _, infl_b = state_run(name, c, "padded", det, alias=True, route=not name.startswith("trio"))
    k, nv = c["k"], c["nv"]
    x = c["gues"].reshape(nv, c["nens"], c["npts"])
    for v in range(nv):
        scale = max(np.abs(x[v, k]).max(), np.abs(x[v, :k]).max())
        sel = idx[v][members(k, det)]
        assert np.abs(in_place[sel] - out_of_place[sel]).max() <= 1e-11 * scale, v
    assert np.abs(infl_a - infl_b).max() <= 1e-12
