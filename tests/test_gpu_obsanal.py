"""das_letkf_obs on the device (letkf_das_obs_dev, scale/letkf/letkf_tools.f90:933-1156) against the oracle's loop body on
the pseudo-state (tests/_obsanal.py composed(), itself checked against the reference's formula on CPU): ya, ya_mean, dep_a
and the ya_table rows within 1e-10 relative (max-norm) for every k the staged family serves, the relaxations, det_run, the q
rules, beta, per-target inflation, a limited search, mixed vertical coordinates, subsets and duplicates; bit-identical
results across list_bytes and repeated calls; the EFSO chain and O - A statistics on the outputs."""
import numpy as np
import pytest
import torch

import _efso
import _obsanal
from _search import build_case, device_struct, oracle_csr, host_struct

pytestmark = pytest.mark.gpu

TOL = 1e-10


def _ctx():
    from _gpu import ctx
    return ctx()


def _d(a, dt=None):
    from _gpu import dev
    return dev(a, dt)


_CASE = {}


def the_case(seed=71, max_nobs=(0, 0, 0, 0)):
    """tables with radar (z), T (ln p) and ps (obs pressure) ctypes; T rows hold temperature-sized values"""
    key = (seed, max_nobs)
    if key not in _CASE:
        case = _obsanal.temperatures(build_case(seed, nobs_per_ctype=(260, 70, 360, 110), max_nobs=max_nobs, npts=40), seed)
        _CASE[key] = (case, device_struct(case, "cuda"))
    return _CASE[key]


def other_coords(case, rows, seed=5):
    rng = np.random.default_rng(seed)
    return rng.uniform(3.0e4, 1.0e5, len(rows)), rng.uniform(0.0, 12000.0, len(rows))


def run(case, tabs, rows, ev, dep, p, infl=None, infl_mul=1.0, beta=None, rlev_tgt=None, rz_tgt=None, list_bytes=0,
        table0=None, lda=None, tgt_none=False):
    k, det = p["k"], bool(p.get("det_run", False))
    n = len(rows)
    lda = lda or k + int(det)
    nan = float("nan")
    ya = torch.full((n, lda), nan, dtype=torch.float64, device="cuda")
    ym = torch.full((n,), nan, dtype=torch.float64, device="cuda")
    da = torch.full((n,), nan, dtype=torch.float64, device="cuda")
    no = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    st = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    tab0 = table0 if table0 is not None else np.full(ev.shape, 7.0)
    yt = _d(tab0)
    q = {key: p[key] for key in ("relax_alpha", "relax_alpha_spread", "q_update_top", "q_sprd_max", "iv_q_first", "iv_q_last",
                                 "relax_to_inflated_prior") if key in p}
    _ctx().das_obs(k, p["tvar"], tabs[0], _d(ev), ev.shape[1], _d(dep), case["nobs"], ya, lda=lda,
                   tgt_row=None if tgt_none else _d(np.asarray(rows, dtype=np.int32)), ntgt=n, ya_mean=ym, ya_table=yt,
                   dep_a=da, nobs_out=no, status=st, rlev_tgt=None if rlev_tgt is None else _d(rlev_tgt),
                   rz_tgt=None if rz_tgt is None else _d(rz_tgt), beta=None if beta is None else _d(beta),
                   infl=None if infl is None else _d(infl), infl_mul=infl_mul, det_run=det, list_bytes=list_bytes, **q)
    torch.cuda.synchronize()
    return dict(ya=ya.cpu().numpy(), mean=ym.cpu().numpy(), dep_a=da.cpu().numpy(), table=yt.cpu().numpy(),
                nobs=no.cpu().numpy(), status=st.cpu().numpy())


def expect(case, rows, ev, dep, p, infl, beta=None, rlev_tgt=None, rz_tgt=None):
    lst = _obsanal.lists(case, rows, rlev_tgt, rz_tgt)
    return _obsanal.composed(case, rows, ev, dep, p, infl, beta, lst)


def check(got, exp, rows, k, det, tab0=None):
    kk = k + int(det)
    assert _obsanal.relerr(got["ya"][:, :kk], exp["ya"]) < TOL
    assert _obsanal.relerr(got["mean"], exp["mean"]) < TOL
    assert _obsanal.relerr(got["dep_a"], exp["dep_a"]) < TOL
    assert _obsanal.relerr(got["table"][rows, :kk], exp["table"]) < TOL
    assert (got["status"] == 0).all()
    if tab0 is not None:   # rows that are no target: untouched, bit for bit
        other = np.setdiff1d(np.arange(tab0.shape[0]), rows)
        assert len(other) > 0
        assert np.array_equal(got["table"][other].view(np.int64), tab0[other].view(np.int64))


def t_rows(case, m=None):
    rows = _obsanal.interior_rows(case, (2,))
    return rows if m is None else rows[:m]


@pytest.mark.parametrize("k", [3, 10, 20, 50, 64, 100, 320])
def test_every_k_against_oracle(k):
    case, tabs = the_case()
    rows = t_rows(case, 60 if k >= 100 else None)
    _, rz = other_coords(case, rows)
    ev, dep = _obsanal.table(case, k, k + 2, seed=k)
    infl = np.random.default_rng(k).uniform(1.0, 1.5, len(rows))
    p = dict(k=k, tvar=3)
    tab0 = np.random.default_rng(1).standard_normal(ev.shape)
    got = run(case, tabs, rows, ev, dep, p, infl=infl, rz_tgt=rz, table0=tab0)
    exp = expect(case, rows, ev, dep, p, infl, rz_tgt=rz)
    check(got, exp, rows, k, False, tab0)
    assert np.array_equal(got["nobs"], exp["nobs"])
    path = _ctx().last_path()
    assert path.startswith("obs_search + staged") and "obsanal_finish_kernel" in path


@pytest.mark.parametrize("opts", [dict(relax_alpha=0.5), dict(relax_alpha_spread=0.8),
                                  dict(relax_alpha_spread=0.8, relax_to_inflated_prior=True),
                                  dict(relax_alpha=0.4, relax_to_inflated_prior=True, det_run=True)])
def test_relaxation_and_det(opts):
    case, tabs = the_case()
    rows = t_rows(case)
    _, rz = other_coords(case, rows)
    k = 20
    ev, dep = _obsanal.table(case, k, k + 3, seed=4)
    infl = np.random.default_rng(4).uniform(1.0, 1.8, len(rows))
    p = dict(k=k, tvar=0, **opts)
    got = run(case, tabs, rows, ev, dep, p, infl=infl, rz_tgt=rz)
    exp = expect(case, rows, ev, dep, p, infl, rz_tgt=rz)
    check(got, exp, rows, k, p.get("det_run", False))


@pytest.mark.parametrize("tvar", [5, 6])
def test_q_rules(tvar):
    """QV (tvar = iv_q_first): Q_UPDATE_TOP and Q_SPRD_MAX; QC: Q_UPDATE_TOP only"""
    case, tabs = the_case()
    rows = t_rows(case)
    _, rz = other_coords(case, rows)
    k = 16
    ev, dep = _obsanal.table(case, k, k + 1, seed=9, spread=20.0)
    lev = case["arr"]["ob_lev"][rows]
    top = float(np.quantile(lev, 0.3))
    p = dict(k=k, tvar=tvar, q_update_top=top, q_sprd_max=0.005, det_run=True)
    got = run(case, tabs, rows, ev, dep, p, infl_mul=1.2, rz_tgt=rz)
    exp = expect(case, rows, ev, dep, p, np.full(len(rows), 1.2), rz_tgt=rz)
    check(got, exp, rows, k, True)
    above = lev < top   # kept their background
    bg = case["arr"]["ob_dat"][rows] - dep[rows]
    assert above.sum() > 5
    assert np.allclose(got["ya"][above, :k], bg[above, None] + ev[rows[above], :k], rtol=0, atol=1e-12)
    if tvar == 5:   # the clamp acted somewhere
        sprd = got["ya"][~above, :k].std(axis=1, ddof=1) / got["mean"][~above]
        assert np.isclose(sprd.max(), 0.005, rtol=1e-9) and (sprd < 0.005 * (1 - 1e-6)).any()


def test_beta_zeros_and_per_target_rho_against_scalar():
    case, tabs = the_case()
    rows = t_rows(case)
    _, rz = other_coords(case, rows)
    k = 12
    ev, dep = _obsanal.table(case, k, k, seed=12)
    rng = np.random.default_rng(12)
    beta = np.where(rng.uniform(size=len(rows)) < 0.25, 0.0, rng.uniform(0.2, 1.0, len(rows)))
    p = dict(k=k, tvar=3, relax_alpha_spread=0.6)
    infl = rng.uniform(1.0, 1.7, len(rows))
    got = run(case, tabs, rows, ev, dep, p, infl=infl, beta=beta, rz_tgt=rz)
    check(got, expect(case, rows, ev, dep, p, infl, beta, rz_tgt=rz), rows, k, False)
    z = beta == 0.0
    assert z.sum() > 3 and (got["nobs"][z] == 0).all() and (got["nobs"][~z] > 0).all()
    bg = case["arr"]["ob_dat"][rows] - dep[rows]
    assert np.array_equal(got["ya"][z], bg[z, None] + ev[rows[z], :k])
    # one rho per target, all equal, gives the bits of the scalar
    a = run(case, tabs, rows, ev, dep, p, infl=np.full(len(rows), 1.35), beta=beta, rz_tgt=rz)
    b = run(case, tabs, rows, ev, dep, p, infl_mul=1.35, beta=beta, rz_tgt=rz)
    for key in ("ya", "mean", "dep_a", "table"):
        assert np.array_equal(a[key].view(np.int64), b[key].view(np.int64)), key
    check(b, expect(case, rows, ev, dep, p, np.full(len(rows), 1.35), beta, rz_tgt=rz), rows, k, False)


def test_limited_search():
    case, tabs = the_case(seed=72, max_nobs=(0, 0, 12, 5))
    rows = t_rows(case)
    _, rz = other_coords(case, rows)
    k = 10
    ev, dep = _obsanal.table(case, k, k, seed=2)
    p = dict(k=k, tvar=1)
    got = run(case, tabs, rows, ev, dep, p, infl_mul=1.1, rz_tgt=rz)
    exp = expect(case, rows, ev, dep, p, np.full(len(rows), 1.1), rz_tgt=rz)
    assert got["nobs"].max() <= 12 + 5 + 70 + 260
    check(got, exp, rows, k, False)


def test_mixed_coordinates():
    """T, ps and radar targets in tables holding pressure and radar ctypes: with the other coordinate they pass; without
    it the call fails; radar targets alone need rlev only"""
    case, tabs = the_case()
    rows = np.sort(np.concatenate([_obsanal.interior_rows(case, (2,))[:40], _obsanal.interior_rows(case, (3,))[:30],
                                   _obsanal.interior_rows(case, (0, 1))[:40]]))
    rlev, rz = other_coords(case, rows, seed=8)
    k = 20
    ev, dep = _obsanal.table(case, k, k, seed=20)
    p = dict(k=k, tvar=-1)
    got = run(case, tabs, rows, ev, dep, p, infl_mul=1.05, rlev_tgt=rlev, rz_tgt=rz)
    check(got, expect(case, rows, ev, dep, p, np.full(len(rows), 1.05), rlev_tgt=rlev, rz_tgt=rz), rows, k, False)
    from _gpu import pkg
    with pytest.raises(pkg.LetkfError):
        run(case, tabs, rows, ev, dep, p, rlev_tgt=rlev)
    with pytest.raises(pkg.LetkfError):
        run(case, tabs, rows, ev, dep, p, rz_tgt=rz)
    radar = _obsanal.interior_rows(case, (0, 1))[:50]
    rl2, _ = other_coords(case, radar, seed=9)
    got = run(case, tabs, radar, ev, dep, p, rlev_tgt=rl2)
    check(got, expect(case, radar, ev, dep, p, np.ones(len(radar)), rlev_tgt=rl2), radar, k, False)


def test_subsets_duplicates_chunks_and_repeats_are_bitwise():
    case, tabs = the_case()
    base = t_rows(case)
    rows = np.concatenate([base[::3], base[5:9], base[::3][:6]])   # a subset, then duplicates
    rz = np.random.default_rng(3).uniform(0.0, 12000.0, case["nobs"])[rows]   # (a duplicate is the same target)
    k = 50
    ev, dep = _obsanal.table(case, k, k + 1, seed=50)
    p = dict(k=k, tvar=3, relax_alpha_spread=0.5, det_run=True)
    infl = np.full(len(rows), 1.2)
    tab0 = np.random.default_rng(2).standard_normal(ev.shape)
    ref = run(case, tabs, rows, ev, dep, p, infl=infl, rz_tgt=rz, table0=tab0)
    check(ref, expect(case, rows, ev, dep, p, infl, rz_tgt=rz), rows, k, True, tab0)
    assert np.array_equal(ref["ya"][-6:].view(np.int64), ref["ya"][:6].view(np.int64))
    nent = int(ref["nobs"].sum())
    for lb in (0, nent * 20 // 5, 20):   # one chunk, five chunks, one target per chunk
        for _ in range(2):
            got = run(case, tabs, rows, ev, dep, p, infl=infl, rz_tgt=rz, table0=tab0, list_bytes=lb)
            for key in ("ya", "mean", "dep_a", "table", "nobs"):
                assert np.array_equal(got[key].view(np.int64) if got[key].dtype == np.float64 else got[key],
                                      ref[key].view(np.int64) if ref[key].dtype == np.float64 else ref[key]), (lb, key)


def test_bad_arguments():
    case, tabs = the_case()
    rows = t_rows(case, 10)
    _, rz = other_coords(case, rows)
    ev, dep = _obsanal.table(case, 5, 5, seed=1)
    from _gpu import pkg
    p = dict(k=5, tvar=3)
    for kw in (dict(lda=4), dict(rz_tgt=None)):
        with pytest.raises(pkg.LetkfError):
            run(case, tabs, rows, ev, dep, p, **{**dict(rz_tgt=rz), **kw})
    with pytest.raises(pkg.LetkfError):   # kld = k with det_run
        run(case, tabs, rows, ev, dep, dict(p, det_run=True), rz_tgt=rz, lda=6)
    with pytest.raises(pkg.LetkfError):   # a row outside the table
        run(case, tabs, np.array([0, case["nobs"]]), ev, dep, p, rz_tgt=np.zeros(2))
    with pytest.raises(pkg.LetkfError):   # k < 2
        run(case, tabs, rows, ev, dep, dict(p, k=1), rz_tgt=rz)


def test_efso_chain_and_o_minus_a():
    """das_obs's ya_table is the Y^a of letkf_efso_columns_dev: the djdy of _efso.efso_loop on the restated Y^a; and dep_a
    through letkf_monit_dep_dev gives O - A's count, bias and rmse"""
    case, tabs = the_case()
    rows = t_rows(case)
    _, rz = other_coords(case, rows)
    k = 20
    ev, dep = _obsanal.table(case, k, k, seed=33)
    p = dict(k=k, tvar=3)
    infl = np.full(len(rows), 1.1)
    tab0 = np.ascontiguousarray(ev[:, :k])   # rows that are no target keep the background's perturbations
    got = run(case, tabs, rows, ev, dep, p, infl=infl, rz_tgt=rz, table0=tab0)
    exp = expect(case, rows, ev, dep, p, infl, rz_tgt=rz)
    ya_exp = tab0.copy()
    ya_exp[rows] = exp["table"]
    pts = case["pts"]
    npts = len(pts["ri"])
    h, keep = host_struct(case)
    off, idx, rd, rl, _ = oracle_csr(h, pts["ri"], pts["rj"], pts["rlev"], pts["rz"])
    nterm, term = 3, [0, 0, 1, 2, -1, 1]
    fcst, fcer, _, _ = _efso.inputs(np.random.default_rng(5), npts, k, len(term), case["nobs"])
    want, scale = _efso.efso_loop(off, idx, rd, rl, ya_exp, fcst, fcer, term, nterm)
    f, fs, e, es = _efso.ref_layout(fcst, fcer)
    dj = torch.zeros(case["nobs"] * nterm, dtype=torch.float64, device="cuda")
    c = _ctx()
    c.efso_columns(k, len(term), term, nterm, tabs[0], npts, 1, _d(pts["ri"]), _d(pts["rj"]), _d(pts["rlev"]), _d(pts["rz"]),
                   _d(got["table"]), k, case["nobs"], _d(f), *fs, _d(e), *es, dj)
    torch.cuda.synchronize()
    assert _efso.within(dj.cpu().numpy().reshape(-1, nterm), want, scale) < TOL
    # O - A: one element id for the targets (3073 = T), all QC-passed
    elm = _d(np.full(len(rows), 3073, dtype=np.int32))
    qc = _d(np.zeros(len(rows), dtype=np.int32))
    n, bias, rmse = c.monit_dep([2819, 3073], elm, _d(got["dep_a"]), qc)
    torch.cuda.synchronize()
    assert n.cpu().tolist() == [0, len(rows)]
    assert bias.cpu().numpy()[1] == pytest.approx(exp["dep_a"].mean(), rel=1e-10)
    assert rmse.cpu().numpy()[1] == pytest.approx(np.sqrt((exp["dep_a"] ** 2).mean()), rel=1e-10)
    # the analysis fits the observations better than the background
    assert rmse.cpu().numpy()[1] < np.sqrt((dep[rows] ** 2).mean())


def test_target_groups_of_a_set_obs_table():
    """ObsTable.target_groups() of a table that set_letkf_obs built on the device: disjoint sorted rows of the interior cells,
    grouped by letkf_obs_target_var of the row's element; one das_obs call per group with that group's varloc runs clean and
    fits the observations better than the background"""
    from _gpu import pkg
    from _setobs import make_world, namelist, oracle_local
    from test_gpu_setobs import run_local
    nml = namelist()
    w = make_world(31, k=10, det_run=True, nfile_rows=(4000, 2000))
    g = run_local(w, w["ranks"][0], nml, both=True)
    tab = g["tab"]
    h, dl = tab.host(), tab.download()
    groups = tab.target_groups()
    rows = np.concatenate(list(groups.values()))
    assert len(rows) > 100 and len(np.unique(rows)) == len(rows)
    assert all(np.all(np.diff(r) > 0) for r in groups.values())
    # interior rows: inside the subdomain's interior by their own location
    ri, rj = dl["ob_ri"], dl["ob_rj"]
    i0 = w["ihalo"] + 0.5
    inside = (ri - i0 > 0) & (ri - i0 <= w["nlon"]) & (rj - i0 > 0) & (rj - i0 <= w["nlat"])
    assert np.array_equal(np.sort(rows), np.nonzero(inside)[0])
    # each row's group is the target variable of its ctype's element
    ac = dl["ac_ext"].astype(np.int64)
    for c in range(h["nctype"]):
        ext = (int(h["ngrdext_i"][c]) + 1) * int(h["ngrdext_j"][c])
        lo, hi = ac[h["ac_off"][c]], ac[h["ac_off"][c] + ext - 1]
        tv = pkg.obs_target_var(int(h["elm_ctype"][c]))
        mine = rows[(rows >= lo) & (rows < hi)]
        assert np.isin(mine, groups.get(tv, np.zeros(0, np.int32))).all()
    k, kld, nobs = w["k"], h["kld"], h["nobstotal"]
    ens, dep = _d(dl["ensval"]), _d(dl["val"])
    c = _ctx()
    var_local = np.full((11, 9), 0.7)
    fits = []
    for tv, r in groups.items():
        vl = np.array([var_local[tv, 0] if tv >= 0 else 1.0] * h["nctype"])
        tab.set_varloc(vl)
        t = tab.search_tables()
        n = len(r)
        ya = torch.empty(n * (k + 1), dtype=torch.float64, device="cuda")
        da = torch.empty(n, dtype=torch.float64, device="cuda")
        st = torch.full((n,), -1, dtype=torch.int32, device="cuda")
        c.das_obs(k, tv, t, ens, kld, dep, nobs, ya, tgt_row=_d(r), dep_a=da, status=st, det_run=True, infl_mul=1.1,
                  rlev_tgt=_d(np.full(n, 5.0e4)), rz_tgt=_d(np.full(n, 3000.0)), relax_alpha_spread=0.9)
        torch.cuda.synchronize()
        assert (st.cpu().numpy() == 0).all() and torch.isfinite(da).all()
        fits.append(((da.cpu().numpy() ** 2).sum(), (dl["val"][r] ** 2).sum()))
    tab.set_varloc(np.ones(h["nctype"]))
    assert sum(f[0] for f in fits) < sum(f[1] for f in fits)


def test_tgt_row_null_is_rows_in_order():
    """tgt_row = NULL: target t is row t.  The same bits as tgt_row = 0..ntgt-1, the interior ones against the oracle; ntgt
    beyond nobs is an error"""
    case, tabs = the_case()
    n = int(case["ctype_rows"][2])                       # the radar rows (vmode 1): the tables also need their pressure
    rows = np.arange(n)
    rlev, _ = other_coords(case, rows, seed=11)
    k = 10
    ev, dep = _obsanal.table(case, k, k, seed=13)
    p = dict(k=k, tvar=-1)
    tab0 = np.random.default_rng(4).standard_normal(ev.shape)
    a = run(case, tabs, rows, ev, dep, p, infl_mul=1.15, rlev_tgt=rlev, table0=tab0, tgt_none=True)
    b = run(case, tabs, rows, ev, dep, p, infl_mul=1.15, rlev_tgt=rlev, table0=tab0)
    for key in ("ya", "mean", "dep_a", "table", "nobs"):
        assert np.array_equal(a[key].view(np.int64) if a[key].dtype == np.float64 else a[key],
                              b[key].view(np.int64) if b[key].dtype == np.float64 else b[key]), key
    inner = np.nonzero(np.isin(rows, _obsanal.interior_rows(case, (0, 1))))[0]
    assert len(inner) > 20
    exp = expect(case, rows[inner], ev, dep, p, np.full(len(inner), 1.15), rlev_tgt=rlev[inner])
    sub = {key: a[key][inner] for key in ("ya", "mean", "dep_a", "status")}
    sub["table"] = a["table"]
    check(sub, exp, rows[inner], k, False)
    from _gpu import pkg
    with pytest.raises(pkg.LetkfError):   # rows ntgt - 1 >= nobs
        run(case, tabs, np.arange(case["nobs"] + 1), ev, dep, p, rlev_tgt=np.full(case["nobs"] + 1, 5.0e4),
            rz_tgt=np.zeros(case["nobs"] + 1), tgt_none=True)
