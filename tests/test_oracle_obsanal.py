"""CPU checks of das_letkf_obs's two restatements (tests/_obsanal.py): the reference's formula on letkf_core equals the oracle's
loop body on the pseudo-state; a lone observation gives the scalar Kalman filter; letkf_obs_target_var restates the
reference's SELECT CASE; the ctypes mirror of letkf_das_obs_args has the header's size."""
import ctypes as C

import numpy as np
import pytest

import _header
import _obsanal
from _search import build_case
from __graft_entry__ import load_package


@pytest.fixture(scope="module")
def pkg():
    p = load_package()
    p.build()
    return p


_CASES = {}


def case_and_lists(seed=61):
    if seed not in _CASES:
        case = _obsanal.temperatures(build_case(seed, nobs_per_ctype=(200, 60, 240, 80), npts=1))
        rows = _obsanal.interior_rows(case, (2,))   # T rows (the tables also hold radar ctypes, which need rz)
        rz = np.random.default_rng(seed).uniform(0.0, 12000.0, len(rows))      # (the tables also hold radar ctypes)
        _CASES[seed] = (case, rows, rz, _obsanal.lists(case, rows, rz_tgt=rz))
    return _CASES[seed]


@pytest.mark.parametrize("k,opts", [
    (5, dict(tvar=3)),
    (12, dict(tvar=3, relax_alpha_spread=0.9)),
    (8, dict(tvar=0, relax_alpha=0.6, relax_to_inflated_prior=True, det_run=True)),
    (10, dict(tvar=5, q_update_top=4.0e4, q_sprd_max=0.05, relax_alpha_spread=0.7, relax_to_inflated_prior=True)),
    (6, dict(tvar=-1, det_run=True, beta=True)),
])
def test_formula_equals_loop_body_on_pseudo_state(k, opts):
    case, rows, rz, lst = case_and_lists()
    opts = dict(opts)
    use_beta = opts.pop("beta", False)
    p = dict(k=k, **opts)
    det = p.get("det_run", False)
    ev, dep = _obsanal.table(case, k, k + 3, seed=k)
    rng = np.random.default_rng(100 + k)
    infl = rng.uniform(1.0, 1.6, len(rows))
    beta = np.where(rng.uniform(size=len(rows)) < 0.2, 0.0, rng.uniform(0.3, 1.0, len(rows))) if use_beta else None
    a = _obsanal.formula(case, rows, ev, dep, p, infl, beta, lst)
    b = _obsanal.composed(case, rows, ev, dep, p, infl, beta, lst)
    assert np.diff(lst[0]).min() >= 0 and lst[0][-1] > 10 * len(rows)
    dat = case["arr"]["ob_dat"][rows]
    assert _obsanal.relerr(a["ya"], b["ya"]) < 1e-12
    assert _obsanal.relerr(a["mean"], b["mean"]) < 1e-12
    assert _obsanal.relerr(a["table"], b["table"]) < 1e-12
    assert _obsanal.relerr(a["dep_a"], b["dep_a"]) < 1e-12
    # the analysis moved the targets: smaller departures on average than the background's
    assert np.abs(a["dep_a"]).mean() < np.abs(dep[rows]).mean()
    if det:
        assert np.abs(a["ya"][:, k] - (dat - ev[rows, k])).max() > 0


@pytest.mark.parametrize("rho", [1.0, 1.3])
def test_lone_observation_is_the_scalar_kalman_filter(rho):
    seed = next(s for s in range(62, 200) if len(_obsanal.interior_rows(build_case(s, nobs_per_ctype=(0, 0, 1, 0), npts=1), (2,))))
    case = _obsanal.temperatures(build_case(seed, nobs_per_ctype=(0, 0, 1, 0), npts=1))   # one T row, inside the subdomain
    rows = np.array([0])
    k = 7
    ev, dep = _obsanal.table(case, k, k, seed=3)
    lst = _obsanal.lists(case, rows)
    off, idx, rd, rl, _ = lst
    assert off[-1] == 1 and idx[0] == 0
    rho_loc = rl[0]
    assert rho_loc == pytest.approx(case["arr"]["varloc"][2])
    err = case["arr"]["ob_err"][0]
    p = dict(k=k, tvar=3)
    for res in (_obsanal.formula(case, rows, ev, dep, p, np.array([rho]), lst=lst),
                _obsanal.composed(case, rows, ev, dep, p, np.array([rho]), lst=lst)):
        x = ev[0, :k]
        sb2 = x @ x / (k - 1)
        r = err ** 2 / (rho_loc * rho)
        d = dep[0]
        yb = case["arr"]["ob_dat"][0] - d
        assert res["mean"][0] - yb == pytest.approx(sb2 / (sb2 + r) * d, rel=1e-12)
        ya = res["ya"][0, :k]
        sa2 = ((ya - ya.mean()) ** 2).sum() / (k - 1)
        assert sa2 == pytest.approx(rho * sb2 * r / (sb2 + r), rel=1e-12)   # (inflated prior: rho sb2 in the spread)


# common_obs_scale.f90:48-68 -> common_scale.f90:41-51, 0-based
TARGET_VAR = {2819: 0, 2820: 1, 3073: 3, 3074: 3, 3330: 5, 3331: 5, 14593: -1, 19999: -1, 99991: -1, 99992: -1, 99993: -1,
              4001: -1, 4004: -1, 4002: -1, 4003: -1, 8800: -1}


def test_obs_target_var_over_every_id(pkg):
    for elm, tv in TARGET_VAR.items():
        assert pkg.obs_target_var(elm) == tv, elm
    assert pkg.obs_target_var(0) == -1


def test_das_obs_args_layout_matches_header(pkg):
    assert _header.sizeof("letkf_das_obs_args") == C.sizeof(pkg.DasObsArgs)
    assert _header.offsetof("letkf_das_obs_args", "ntgt") == pkg.DasObsArgs.ntgt.offset
    assert _header.offsetof("letkf_das_obs_args", "list_bytes") == pkg.DasObsArgs.list_bytes.offset
