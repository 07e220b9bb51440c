"""The checkers on the degenerate inputs of tests/_degenerate.py, CPU only.  The oracle (oracle/letkf_oracle.c) is what every GPU
route is compared with, and it had only seen generic spectra: here it is held against a 50-digit solution of letkf_core's
equations (tests/golden/degenerate_truth.npz) and against the reference's own answers (tests/golden/degenerate_reference.npz) on
exactly-zero, duplicated, low-rank and floored observation rows, and the metamorphic relations tests/test_gpu_degenerate.py
applies to the library are first shown to hold for the oracle."""
import os

import numpy as np
import pytest

import _oracle
from _argspace import CFG
from _degenerate import (ARRANGEMENTS, META_CFG, OBS_CLASSES, TRIO_RUN_CAP, core_errors, das_degenerate, inputs_sha, kk_error,
                         load_store, meta_error, meta_pairs, run_positions, truth_cases, truth_name, truth_problem, twin_error,
                         twin_state, vec_error, y_is_zero)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = truth_cases()
IDS = [truth_name(*c) for c in CASES]
ORACLE_BAR = 1e-12        # ten times inside the bar the library is held to against the same truth
REF_BAR = 1e-13           # tests/test_oracle_vs_ref.py


@pytest.fixture(scope="module")
def truth():
    return load_store(np.load(os.path.join(GOLDEN, "degenerate_truth.npz")))


@pytest.fixture(scope="module")
def reference():
    return load_store(np.load(os.path.join(GOLDEN, "degenerate_reference.npz")))


def run_oracle(c):
    r = _oracle.letkf_core("oracle", c["k"], c["nobs"], c["n"], c["hdxb"], c["rdiag"], c["rloc"], c["dep"], c["infl"],
                           rdiag_wloc=True, infl_update=True, depd=c["depd"], want_transmd=True)
    assert r["rc"] == 0
    return r


def test_stored_cases_are_the_generators(truth, reference):
    names = set(IDS)
    assert {n.rsplit("/", 1)[0] for n in truth} == names
    assert {n[4:].rsplit("/", 1)[0] for n in reference} == names
    for cls in OBS_CLASSES:
        assert sum(c[0] == cls for c in CASES) >= 12, cls


@pytest.mark.parametrize("cls,k,n", CASES, ids=IDS)
def test_oracle_against_truth(truth, cls, k, n):
    """the condition on the inputs: the oracle alone is within 1e-12 of the 50-digit solution on every stored case (T, Pa
    max-norm relative, w-bar relative to max(1, |w|)); cond(A) stays within a few hundred"""
    c = truth_problem(cls, k, n)
    nm = truth_name(cls, k, n)
    assert np.array_equal(inputs_sha(c), truth[nm + "/sha"].astype(np.uint8)), "input generator drifted from the fixture"
    assert truth[nm + "/cond"][0] < 500.0
    errs = core_errors(run_oracle(c), truth, nm)
    print(f"oracle vs truth {nm}: T {errs[0]:.2e} Pa {errs[1]:.2e} w {errs[2]:.2e} wd {errs[3]:.2e}")
    assert max(errs) <= ORACLE_BAR, errs


@pytest.mark.parametrize("cls,k,n", CASES, ids=IDS)
def test_oracle_against_stored_reference(reference, cls, k, n):
    """the reference's own letkf_core on the same inputs, parm_infl with infl_update included: NaN where Y = 0 (the adaptive
    inflation divides by parm(2) = 0, common/common_letkf.f90:230-257) and nowhere else, and the oracle says the same"""
    c = truth_problem(cls, k, n)
    nm = "ref/" + truth_name(cls, k, n)
    assert np.array_equal(inputs_sha(c), reference[nm + "/sha"].astype(np.uint8)), "input generator drifted from the fixture"
    r = run_oracle(c)
    assert max(core_errors(r, reference, nm)) <= REF_BAR
    want = float(reference[nm + "/parm_infl"][0])
    assert np.isnan(want) == (not c["hdxb"][:n].any()), (cls, want)         # Y = 0: all_zero, and zero_rows' single row
    assert cls != "all_zero" or np.isnan(want)
    if np.isnan(want):
        assert np.isnan(r["parm_infl"])
    else:
        assert abs(r["parm_infl"] - want) <= 1e-14
    for key in ("trans", "pao", "transm", "transmd"):
        assert np.isfinite(r[key]).all(), key


@pytest.mark.parametrize("cls,k,n", [c for c in CASES if c[1] <= 20], ids=[i for i, c in zip(IDS, CASES) if c[1] <= 20])
def test_truth_regenerates(truth, cls, k, n):
    """where mpmath imports: the stored truth of the small cases is what the generator computes today"""
    pytest.importorskip("mpmath")
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_degenerate_truth", os.path.join(GOLDEN, "make_degenerate_truth.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    nm = truth_name(cls, k, n)
    T, Pa, w, wd, cond = gen.truth(truth_problem(cls, k, n))
    assert kk_error(T, truth, nm, "trans") <= 1e-15 and kk_error(Pa, truth, nm, "pao") <= 1e-15
    assert vec_error(w, truth[nm + "/transm"]) <= 1e-15 and vec_error(wd, truth[nm + "/transmd"]) <= 1e-15
    assert abs(cond - truth[nm + "/cond"][0]) <= 1e-12 * cond


# ---------------------------------------------------------------------------------------------------------------------
def oracle_das(c, cfg, det, **want):
    prm = _oracle.DasParams(k=c["k"], nv=c["nv"], det_run=int(det), infl_adaptive=cfg.get("infl_adaptive", 0),
                            relax_to_inflated_prior=cfg.get("relax_to_inflated_prior", 0),
                            relax_alpha=cfg.get("relax_alpha", 0.0), relax_alpha_spread=cfg.get("relax_alpha_spread", 0.0),
                            q_update_top=cfg.get("q_update_top", 0.0), q_sprd_max=cfg.get("q_sprd_max", 0.0), iv_p=4,
                            iv_q_first=5, iv_q_last=min(10, c["nv"] - 1), nthreads=4, var_mask=0)
    r = _oracle.das_points(prm, c["obs_off"], c["obs_idx"], c["rdiag"], c["rloc"], c["ensval"], c["dep"], c["beta"],
                           c["infl"], c["gues"], c["sp"], c["sm"], c["sv"], **want)
    assert r["rc"] == 0
    return r


def test_run_positions():
    """the slot in a three-point wave is the run's number modulo 3 (letkf_trio.hip gives a wave three consecutive runs and walks
    them in step), the position in a run the point's index inside it; strided runs go up a column"""
    slot, pos = run_positions(24, 4, 0)
    assert pos.tolist() == [0, 1, 2, 3] * 6
    assert slot.tolist() == [0] * 4 + [1] * 4 + [2] * 4 + [0] * 4 + [1] * 4 + [2] * 4
    slot, pos = run_positions(6, 1, 0)
    assert pos.tolist() == [0] * 6 and slot.tolist() == [0, 1, 2, 0, 1, 2]
    slot, pos = run_positions(16, 2, 4)                   # columns of four levels, runs of two levels
    assert pos.tolist() == [0] * 4 + [1] * 4 + [0] * 4 + [1] * 4
    assert slot.tolist() == [0, 1, 2, 0] * 2 + [1, 2, 0, 1] * 2          # runs 0..3 in the lower half, 4..7 above


@pytest.mark.parametrize("trio", [False, True], ids=["wave", "trio"])
@pytest.mark.parametrize("arr", list(ARRANGEMENTS))
@pytest.mark.parametrize("k,nv", [(9, 11), (20, 11), (50, 11), (20, 15)])
def test_loop_body_generator(k, nv, arr, trio):
    """the arrangements hold what they promise, and the oracle's loop body answers them as the reference's equations imply:
    finite everywhere but the inflation of the Y = 0 points, an all-zero variable exactly 0, a zero-spread variable exactly its
    mean with RTPS factor 1, and an analysis mean of the clamped variable that is not rounding noise where its prior mean is 0"""
    det = True
    c = das_degenerate(k, nv, seed=3, det=det, arr=arr, trio=trio)
    npts, nens = c["npts"], c["nens"]
    assert c["warm_run"] == ARRANGEMENTS[arr][0] and c["run_len"] == (min(ARRANGEMENTS[arr][1], TRIO_RUN_CAP) if trio else ARRANGEMENTS[arr][1])
    n = np.diff(c["obs_off"])
    assert (n == 0).any() and (c["beta"] == 0.0).any()
    solved = (n > 0) & (c["beta"] != 0.0)
    for ci in range(len(OBS_CLASSES)):
        here = solved & (c["cls_of_point"] == ci)
        assert (n[here] < k).any() and (n[here] > k).any(), OBS_CLASSES[ci]
    if not c["warm_stride"]:
        off, tail = c["obs_off"], range(npts - 4, npts)
        assert all(np.array_equal(c["obs_idx"][off[p]:off[p + 1]], c["obs_idx"][off[npts - 4]:off[npts - 3]]) for p in tail)
    cfg = dict(CFG, q_sprd_max=0.5)
    r = oracle_das(c, cfg, det, want_rtps=True)
    a = r["anal"].reshape(nv, nens, npts)
    x = c["gues"].reshape(nv, nens, npts)
    mem = list(range(k)) + [k + 1]
    assert np.isfinite(a[:, mem]).all()
    y0 = solved & y_is_zero(c)
    assert y0[c["cls_of_point"] == OBS_CLASSES.index("all_zero")].any()
    assert np.array_equal(np.isnan(r["infl"].reshape(nv, npts)), np.tile(y0, (nv, 1)))
    sc = c["state_cls"]
    for v in range(nv):
        zv, zs = sc["zero_var"][v], sc["zero_spread"][v] & ~sc["zero_var"][v]
        assert (a[v][mem][:, zv] == 0.0).all(), v
        assert (a[v, :k][:, zs] == x[v, k][zs]).all(), v
        assert (r["rtps"].reshape(nv, npts)[v][zs | zv] == 1.0).all(), v
    qz = sc["q_mean_zero"][5]
    assert qz.sum() >= 3
    am = a[5, :k].mean(axis=0)
    sp = x[5, :k].std(axis=0)
    assert (np.abs(am[qz]) > 1e-6 * sp[qz]).all(), "the clamp's divisor is rounding noise at a q_mean_zero point"


@pytest.mark.parametrize("k", [20, 50])
def test_metamorphic_relations_hold_for_the_oracle(k):
    """the relations of tests/test_gpu_degenerate.py section d, on the oracle: they are properties of the equations, so the
    checker itself must satisfy them at the bar the library is given (twice the loop body's 1e-10)"""
    det = True
    c = das_degenerate(k, 11, seed=7, det=det, arr="run4")
    base = oracle_das(c, META_CFG, det)["anal"]
    for name, ca, cb, perm in meta_pairs(c):
        other = oracle_das(cb, META_CFG, det)["anal"]
        err = meta_error(c, base, other, perm, det)
        print(f"oracle metamorphic k={k} {name}: {err:.2e}")
        assert err <= 2e-10, name
    t = das_degenerate(k, 11, seed=7, det=det, arr="run4")
    pair = twin_state(t)
    err = twin_error(t, oracle_das(t, META_CFG, det)["anal"], pair)
    print(f"oracle metamorphic k={k} twins: {err:.2e}")
    assert err <= 2e-10
