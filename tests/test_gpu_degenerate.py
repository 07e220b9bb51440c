"""Every solver route on the degenerate inputs radar data produces (tests/_degenerate.py): observation rows that are exactly zero,
copies or multiples of one another, exactly low rank or floored, and state variables without spread.
  a. the fine boundary (letkf_core_batch_dev, letkf_core_c) against a 50-digit solution of the equations
     (tests/golden/degenerate_truth.npz) at the README's parity claim 1e-11, unscaled by cond(A); the adaptive inflation NaN
     exactly where the reference's own letkf_core gives NaN (tests/golden/degenerate_reference.npz);
  b. the loop body (letkf_das_points_dev) on every route of _argspace.AXIS_ROUTES against the oracle, the classes mixed from point
     to point so that every class meets every position of a three-point wave and of a warm-start run, with the exact statements
     the reference implies for variables without spread;
  c. the column entry (letkf_das_columns_dev) with such rows in the search table;
  d. metamorphic relations that need no oracle.
tests/test_degenerate_cpu.py holds the oracle to the same truth, ten times closer.  No case is left out of any check."""
import os

import numpy as np
import pytest
import torch

import _oracle
from _argspace import AXIS_ROUTES, CFG, ROUTES, members
from _cases import expected_status, relerr
from _degenerate import (META_CFG, OBS_CLASSES, TRUTH_K, core_errors, das_degenerate, inputs_sha, load_store, meta_error,
                         meta_pairs, truth_n, truth_name, truth_problem, twin_error, twin_state, vec_error, y_is_zero)

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NAN = float("nan")
NOT_WRITTEN = -(1 << 30)
TOL = 1e-11                       # README: parity with the reference at 1e-11 (the norm of tests/test_gpu_core_batch.py)
KRYLOV_MAX_ITER = 128             # the eigen-free stage's iteration limit (letkf_krylov.hip)
CORE_K = TRUTH_K + [17, 62, 63]   # + the KR instantiation bounds and the NW = 2 twin's first size: compared with the oracle
CORE_C_K = [20, 50, 64, 144]      # letkf_core_c: three-points-per-wave sizes, one wave, two waves, workgroup Jacobi
# the loop body's routes: one of each (AXIS_ROUTES), and -- the eigen-free stage serves AXIS_ROUTES' k = 250 row, so that its
# points never see the block Jacobi behind it -- the same order with the stage switched off: every point through
# letkf_eig_block_kernel
LOOP_ROUTES = AXIS_ROUTES + ["staged_block_nopoly"]


@pytest.fixture(scope="module")
def truth():
    return load_store(np.load(os.path.join(GOLDEN, "degenerate_truth.npz")))


@pytest.fixture(scope="module")
def reference():
    return load_store(np.load(os.path.join(GOLDEN, "degenerate_reference.npz")))


def core_cases(k):
    ns = truth_n(k) if k in TRUTH_K else [k // 2, 3 * k]
    return [(cls, n, truth_problem(cls, k, n)) for cls in OBS_CLASSES for n in ns]


def oracle_core(c):
    r = _oracle.letkf_core("oracle", c["k"], c["nobs"], c["n"], c["hdxb"], c["rdiag"], c["rloc"], c["dep"], c["infl"],
                           rdiag_wloc=True, infl_update=True, depd=c["depd"], want_transmd=True)
    assert r["rc"] == 0
    return r


def check_core(k, cls, n, c, r, truth, reference):
    """one problem's answer r (trans, pao, transm, transmd, parm_infl) against the truth where it is stored, else the oracle"""
    nm = truth_name(cls, k, n)
    assert expected_status(c, c) == 0              # (cond(A) of a few hundred: far from LETKF_ST 3's threshold)
    o = oracle_core(c)
    if nm + "/transm" in truth:
        assert np.array_equal(inputs_sha(c), truth[nm + "/sha"].astype(np.uint8)), "input generator drifted from the fixture"
        errs = core_errors(r, truth, nm)
        want_nan = bool(np.isnan(reference["ref/" + nm + "/parm_infl"][0]))
        against = "truth"
    else:
        errs = (relerr(r["trans"], o["trans"]), relerr(r["pao"], o["pao"]), vec_error(r["transm"], o["transm"]),
                vec_error(r["transmd"], o["transmd"]))
        want_nan = bool(np.isnan(o["parm_infl"]))
        against = "oracle"
    print(f"gpu vs {against} {nm}: T {errs[0]:.2e} Pa {errs[1]:.2e} w {errs[2]:.2e} wd {errs[3]:.2e}")
    assert max(errs) <= TOL, (nm, errs)
    assert want_nan == (not c["hdxb"][:n].any()), nm
    if want_nan:
        assert np.isnan(r["parm_infl"]), (nm, r["parm_infl"])
    else:
        assert abs(r["parm_infl"] - o["parm_infl"]) <= 1e-12, (nm, r["parm_infl"], o["parm_infl"])


# ---------------------------------------------------------------------------------------------------------------------
# a. the fine boundary
@pytest.mark.parametrize("k", CORE_K)
def test_core_batch(truth, reference, k):
    """every class and the control, n < k and n > k, in ONE batch: T, Pa, w-bar, w-bar_det with rdiag_wloc and infl_update"""
    from _gpu import ctx, dev
    cases = core_cases(k)
    nb = len(cases)
    nobs = max(c["n"] for _, _, c in cases) + 3
    H = np.full((nb, k, nobs), 1.0e30)
    rd, rl, dp, dd = (np.full((nb, nobs), 1.0e30) for _ in range(4))
    for b, (_, n, c) in enumerate(cases):
        H[b, :, :n] = c["hdxb"][:n].T
        rd[b, :n], rl[b, :n], dp[b, :n], dd[b, :n] = c["rdiag"][:n], c["rloc"][:n], c["dep"][:n], c["depd"][:n]
    infl = dev(np.array([c["infl"] for _, _, c in cases]))
    trans = torch.full((nb, k * k), NAN, dtype=torch.float64, device="cuda")
    pao = torch.full_like(trans, NAN)
    transm = torch.full((nb, k), NAN, dtype=torch.float64, device="cuda")
    transmd = torch.full_like(transm, NAN)
    status = torch.full((nb,), NOT_WRITTEN, dtype=torch.int32, device="cuda")
    nsweep = torch.full((nb,), NOT_WRITTEN, dtype=torch.int32, device="cuda")
    ctx().core_batch(k, nobs, dev(np.array([n for _, n, _ in cases], dtype=np.int32)), dev(H), dev(rd), dev(rl), dev(dp), infl,
                     trans, transm=transm, pao=pao, depd=dev(dd), transmd=transmd, rdiag_wloc=True, infl_update=True,
                     status=status, nsweep=nsweep)
    torch.cuda.synchronize()
    assert status.cpu().numpy().tolist() == [0] * nb
    ns = nsweep.cpu().numpy()
    assert (ns != NOT_WRITTEN).all() and ns.max() < 30, ns
    T, P, W, WD, I = (t.cpu().numpy() for t in (trans, pao, transm, transmd, infl))
    for b, (cls, n, c) in enumerate(cases):
        r = dict(trans=T[b].reshape(k, k).T, pao=P[b].reshape(k, k).T, transm=W[b], transmd=WD[b], parm_infl=I[b])
        for key in ("trans", "pao", "transm", "transmd"):
            assert np.isfinite(r[key]).all(), (cls, n, key)
        check_core(k, cls, n, c, r, truth, reference)


@pytest.mark.parametrize("k", CORE_C_K)
def test_core_c(truth, reference, k):
    """the host-pointer drop-in the Fortran shim calls, one ensemble size per kernel family"""
    from _gpu import ctx, pkg
    ctx()
    for cls, n, c in core_cases(k):
        r = pkg.letkf_core_host(k, c["nobs"], n, c["hdxb"], c["rdiag"], c["rloc"], c["dep"], c["infl"], rdiag_wloc=True,
                                infl_update=True, depd=c["depd"], want_transmd=True, fill=NAN)
        assert r["status"] == 0, (cls, n, r["status"])
        check_core(k, cls, n, c, r, truth, reference)


# ---------------------------------------------------------------------------------------------------------------------
# b. the loop body
CFGS = {"rtps": dict(CFG, q_sprd_max=0.5),
        "rtpp": dict(relax_alpha=0.7, infl_adaptive=1, relax_to_inflated_prior=1),
        "none": dict(infl_adaptive=1)}


def oracle_das(c, cfg, det):
    prm = _oracle.DasParams(k=c["k"], nv=c["nv"], det_run=int(det), infl_adaptive=cfg.get("infl_adaptive", 0),
                            relax_to_inflated_prior=cfg.get("relax_to_inflated_prior", 0),
                            relax_alpha=cfg.get("relax_alpha", 0.0), relax_alpha_spread=cfg.get("relax_alpha_spread", 0.0),
                            q_update_top=cfg.get("q_update_top", 0.0), q_sprd_max=cfg.get("q_sprd_max", 0.0), iv_p=4,
                            iv_q_first=5, iv_q_last=min(10, c["nv"] - 1), nthreads=8, var_mask=0)
    r = _oracle.das_points(prm, c["obs_off"], c["obs_idx"], c["rdiag"], c["rloc"], c["ensval"], c["dep"], c["beta"],
                           c["infl"], c["gues"], c["sp"], c["sm"], c["sv"], want_rtps=True)
    assert r["rc"] == 0
    return r


def library_das(name, c, cfg, det, alias=False):
    """letkf_das_points_dev on the route's row, the case's warm_run / warm_stride; every output prefilled.  alias: anal is gues
    itself.  Returns host copies: anal (NaN where not written; in place: gues there), infl, rtps, status, nsweep."""
    import test_gpu_das_argspace as da
    from _gpu import ctx, dev
    npts, nv = c["npts"], c["nv"]
    gues = dev(c["gues"])
    anal = gues if alias else torch.full((c["gues"].size,), NAN, dtype=torch.float64, device="cuda")
    infl = dev(c["infl"])
    outs = dict(da.kk_outputs(name, c),
                status=torch.full((npts,), NOT_WRITTEN, dtype=torch.int32, device="cuda"),
                nsweep=torch.full((npts,), NOT_WRITTEN, dtype=torch.int32, device="cuda"),
                rtps_infl_out=torch.full((npts * nv,), NAN, dtype=torch.float64, device="cuda"))
    da.route_options(name)
    try:
        rc = da.call(c, cfg, det, gues, anal, infl, c["sp"], c["sm"], c["sv"], warm_run=c["warm_run"],
                     warm_stride=c["warm_stride"], **outs)
        assert rc == 0, rc
        if alias and is_trio(name):                     # in place the pre-pass is off (trivial_pass_supports), and with it the
            path = ctx().last_path()                    # three-points-per-wave kernel: the one-wave kernel serves these rows
            assert "letkf_wave_kernel<" in path and "NW=1" in path, (name, path)
        else:
            da.check_route(name)
    finally:
        da.route_options()
    return dict(anal=anal.cpu().numpy(), infl=infl.cpu().numpy(), rtps=outs["rtps_infl_out"].cpu().numpy(),
                status=outs["status"].cpu().numpy(), nsweep=outs["nsweep"].cpu().numpy())


def check_das(name, c, cfg, det, got, ref):
    k, nv, npts, nens = c["k"], c["nv"], c["npts"], c["nens"]
    x = c["gues"].reshape(nv, nens, npts)
    a, e = got["anal"].reshape(nv, nens, npts), ref["anal"].reshape(nv, nens, npts)
    mem = members(k, det)
    n = np.diff(c["obs_off"])
    solved = (n > 0) & (c["beta"] != 0.0)
    # the analysis: the loop body's bar, 1e-10 max(|mean|, |perturbation|) per variable; finite everywhere
    assert np.isfinite(e[:, mem]).all()
    for v in range(nv):
        scale = max(np.abs(x[v, k]).max(), np.abs(x[v, :k]).max())
        assert np.isfinite(a[v, mem]).all(), (v, np.argwhere(~np.isfinite(a[v, mem]))[:4])
        err = np.abs(a[v, mem] - e[v, mem]).max()
        assert err <= 1e-10 * scale, (v, err, scale)
    # the inflation: NaN where the oracle has NaN -- the adaptive estimate of a point whose rows are all zero -- and only there
    gi, ei = got["infl"].reshape(nv, npts), ref["infl"].reshape(nv, npts)
    want_nan = np.tile(solved & y_is_zero(c), (nv, 1)) if cfg.get("infl_adaptive") else np.zeros((nv, npts), bool)
    assert np.array_equal(np.isnan(ei), want_nan)
    assert np.array_equal(np.isnan(gi), want_nan), np.argwhere(np.isnan(gi) != want_nan)[:6]
    assert np.isfinite(gi[~want_nan]).all()
    assert np.abs(gi[~want_nan] - ei[~want_nan]).max() <= 1e-12
    # what the reference implies exactly for variables without spread
    sc = c["state_cls"]
    gr, er = got["rtps"].reshape(nv, npts), ref["rtps"].reshape(nv, npts)
    for v in range(nv):
        zv, zs = sc["zero_var"][v], sc["zero_spread"][v] & ~sc["zero_var"][v]
        assert (a[v][mem][:, zv] == 0.0).all(), ("zero_var", v)
        assert (a[v, :k][:, zs] == x[v, k][zs]).all(), ("zero_spread", v)
        assert (gr[v][zv | zs] == 1.0).all(), ("rtps factor of a variable without spread", v)
    assert np.isfinite(gr).all()
    if cfg.get("relax_alpha_spread"):
        assert np.abs(gr - er).max() <= 1e-11 * np.abs(er).max()
    else:
        assert (gr == 1.0).all()
    # status and the solver's own count
    assert (got["status"] == 0).all(), got["status"]
    ns = got["nsweep"]
    assert (ns[~solved] == 0).all(), ns
    if ROUTES[name][2] is None and "staged:" in ROUTES[name][3]:       # staged path, stage on, no k x k output: the eigen-free stage
        # (staged_block too: its row names the block Jacobi only as what stands behind the stage)
        # the eigen-free stage serves every point: a degenerate spectrum (an exact Lanczos breakdown after rank(Y) steps, a zero
        # right-hand side) must not send a point to the eigensolver behind it
        bad = np.flatnonzero(solved & ~((ns < 0) & (ns >= -KRYLOV_MAX_ITER)))
        assert bad.size == 0, ("points that left the eigen-free stage", bad[:8], ns[bad[:8]],
                               [OBS_CLASSES[i] for i in c["cls_of_point"][bad[:8]]])
    else:                                          # a Jacobi solved every point (staged_block_nopoly: the block Jacobi)
        assert (ns[solved] > 0).all() and ns.max() < 30, ns


_case_cache = {}


def is_trio(name):
    return "letkf_trio_kernel" in ROUTES[name][3][0]


def das_case_for(name, det, arr, seed=13):
    k, nv = ROUTES[name][:2]
    key = (k, nv, det, arr, seed, is_trio(name))
    if key not in _case_cache:
        _case_cache.clear()
        _case_cache[key] = das_degenerate(k, nv, seed=seed + k, det=det, arr=arr, trio=is_trio(name))
    return _case_cache[key]


@pytest.mark.parametrize("det", [True, False], ids=["det", "nodet"])
@pytest.mark.parametrize("name", LOOP_ROUTES)
def test_loop_body(name, det):
    """every route, RTPS + adaptive inflation + the Q_SPRD_MAX clamp, then RTPP, then no relaxation, with and without DET_RUN:
    the classes mixed over the points in runs of four, the state classes applied"""
    c = das_case_for(name, det, "run4")
    for cfg_name, cfg in CFGS.items():
        got = library_das(name, c, cfg, det)
        check_das(name, c, cfg, det, got, oracle_das(c, cfg, det))


@pytest.mark.parametrize("name", LOOP_ROUTES)
def test_loop_body_in_place(name):
    """anal aliasing gues: the streaming pass that serves the points without observations and with beta = 0 out of place is off,
    so those points -- zero-spread variables among them -- go through the solver kernels' own branch for them (the RTPS guard of
    letkf_wave_dev.h's unsolved points is reached by nothing else)"""
    c = das_case_for(name, True, "run4")
    n = np.diff(c["obs_off"])
    sc = c["state_cls"]
    assert ((n == 0)[None, :] & (sc["zero_spread"] | sc["zero_var"])).any()
    cfg = CFGS["rtps"]
    check_das(name, c, cfg, True, library_das(name, c, cfg, True, alias=True), oracle_das(c, cfg, True))


@pytest.mark.parametrize("arr", ["run16", "off", "stride"])
@pytest.mark.parametrize("name", LOOP_ROUTES)
def test_loop_body_arrangements(name, arr):
    """warm-start runs of 16 (the cap of the library's default, warm_run = 0, which itself gives shorter runs -- one point -- on
    a batch of this size: the length is asked for by its number), warm_run = 1, and runs of four up the columns
    (warm_stride = nij1).  The three-points-per-wave kernel shortens runs to four points on such a batch, so its rows are
    arranged for runs of four under warm_run = 16.  Every class sits at every position of the run the kernel really makes and,
    there, in every slot of a three-point wave; bit-identical consecutive points; degenerate points between benign ones."""
    c = das_case_for(name, True, arr)
    cfg = CFGS["rtps"]
    check_das(name, c, cfg, True, library_das(name, c, cfg, True), oracle_das(c, cfg, True))


# ---------------------------------------------------------------------------------------------------------------------
# c. the column entry
@pytest.mark.parametrize("name", ["free_k20", "free_k33"])
def test_columns(name):
    """all_zero, one_rainy and rank1 rows in the search table's ensval, by longitude band (the westernmost columns see nothing
    but clear air: Y = 0 at every one of their levels); letkf_das_columns_dev on the list-free route, _colspace's oracle and bar,
    the inflation NaN where the oracle's is and nowhere else"""
    import test_gpu_columns_argspace as ca
    from _colspace import col_case, oracle
    from _degenerate import obs_rows
    c = col_case(name, seed=17)
    k, nv, npts = c["k"], c["nv"], c["npts"]
    rng = np.random.default_rng(171)
    x = c["tc"]["arr"]["ob_ri"] - c["tc"]["scal"]["i_org"]
    band = np.digitize(x, [16.0, 22.0, 27.0])
    for b, cls in enumerate(["all_zero", "one_rainy", "rank1"]):
        rows = np.flatnonzero(band == b)
        assert rows.size > 20, cls
        c["ensval"][rows, :k] = obs_rows(cls, rows.size, k, rng) * 0.2
    c["rig"][:4] = c["tc"]["scal"]["i_org"] + rng.uniform(0.2, 1.2, 4)
    ref = oracle(c, ca.classes_of(c))
    r = ca.Run(c)
    rc, err = ca.call(r, name)
    assert rc == 0, err
    ca.check_route(name)
    counts = ref["counts"]
    live = c["beta"] != 0.0
    assert (counts[live] > 0).any()
    assert np.array_equal(r.outs["nobs"].cpu().numpy(), np.where(live, counts, 0))
    got = r.anal.cpu().numpy()
    xg = c["gues"].reshape(nv, c["nens"], npts)
    mem = members(k, c["det"])
    ok = ~ref["tied"]
    assert ok.all()
    for v in range(nv):
        scale = max(np.abs(xg[v, k]).max(), np.abs(xg[v, :k]).max())
        g = got[r.idx[v][mem]]
        assert np.isfinite(g).all(), v
        assert np.abs(g - ref["anal"][v][mem]).max() <= 1e-10 * scale, v
    gi, ei = r.infl.cpu().numpy().reshape(nv, npts), ref["infl"].reshape(nv, npts)
    nan = np.isnan(ei)
    assert nan[:, :4].any() and not nan.all()
    assert np.array_equal(np.isnan(gi), nan)
    assert np.abs(gi[~nan] - ei[~nan]).max() <= 1e-12
    gr, er = r.outs["rtps"].cpu().numpy(), ref["rtps"]
    assert np.isfinite(gr).all() and np.abs(gr - er).max() <= 1e-11 * np.abs(er).max()
    assert (r.outs["status"].cpu().numpy() == 0).all()


# ---------------------------------------------------------------------------------------------------------------------
# d. metamorphic relations
@pytest.mark.parametrize("name", ["trio20", "wave1", "staged_poly", "staged_wg"])
def test_metamorphic(name):
    """independent of the oracle: deleting the exact-zero rows of a list, m copies of a row at rdiag for one at rdiag / m,
    permuting a list, permuting the members, twin members.  Bar: twice the loop body's (each side is within one bar of the exact
    answer).  tests/test_degenerate_cpu.py shows the same relations on the oracle."""
    det = True
    k, nv = ROUTES[name][:2]
    c = das_degenerate(k, nv, seed=7, det=det, arr="run4")
    base = library_das(name, c, META_CFG, det)["anal"]
    for rel, _, cb, perm in meta_pairs(c):
        other = library_das(name, cb, META_CFG, det)["anal"]
        err = meta_error(c, base, other, perm, det)
        print(f"gpu metamorphic {name} {rel}: {err:.2e}")
        assert err <= 2e-10, (name, rel, err)
    t = das_degenerate(k, nv, seed=7, det=det, arr="run4")
    pair = twin_state(t)
    err = twin_error(t, library_das(name, t, META_CFG, det)["anal"], pair)
    print(f"gpu metamorphic {name} twins: {err:.2e}")
    assert err <= 2e-10, (name, "twins", err)
