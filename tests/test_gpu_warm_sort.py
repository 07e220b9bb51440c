"""Hand-over order of the warm start (csrc/letkf_wave_dev.h warm_rank, LETKF_WARM_SORT): a one-wave point leaves its eigenvectors
in the workspace sorted by eigenvalue instead of in the lane order its rotate-and-swap iteration stopped in.  The next point's
solve starts from a column-permuted Q -- the same eigenvectors, so the analysis must stay what the cold start gives
(1e-10 * max(|x-bar|, |x'|) per variable, SURVEY.md section 8(c), and the oracle at the same bar), results must stay reproducible
call to call, and the order must pay: fewer Jacobi sweeps on warm-started points than the lane order, in one build."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _oracle
from _cases import das_case

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NIJ1, NLEV = 3, 16
NPTS = NIJ1 * NLEV
EMPTY = (7, 22)        # points without observations ...
BAD = (13, 37)         # ... and points whose solve ends with status != 0, inside the runs (consecutive runs and runs up a column)


def make_case(k):
    """das_case with list lengths 0 .. 2k (n < k: the eigenvalue (k-1)/rho with multiplicity k - n; n > k), two points without
    observations and two ill-conditioned ones (5 observations with an error variance of 1e-12: lambda_max / lambda_min > 1e12,
    status 3) placed inside the runs."""
    c = das_case(k=k, nv=11, npts=NPTS, nobs_tot=700, n_mean=k, seed=6000 + k, det_run=True, infl0=1.07)
    off, idx, rdiag, rloc = c["obs_off"], c["obs_idx"], c["rdiag"], c["rloc"]
    cnt = np.diff(off)
    new_idx, new_rd, new_rl, new_cnt = [], [], [], []
    rng = np.random.default_rng(k)
    for p in range(NPTS):
        if p in EMPTY:
            new_cnt.append(0)
            continue
        if p in BAD:
            rows = rng.choice(700, size=5, replace=False).astype(np.int32)
            new_idx.append(rows)
            new_rd.append(np.full(5, 1e-12))
            new_rl.append(np.full(5, 1.0))
            new_cnt.append(5)
            continue
        s = slice(off[p], off[p + 1])
        new_idx.append(idx[s])
        new_rd.append(rdiag[s])
        new_rl.append(rloc[s])
        new_cnt.append(int(cnt[p]))
    c["obs_off"] = np.concatenate([[0], np.cumsum(new_cnt)]).astype(np.int64)
    c["obs_idx"] = np.concatenate(new_idx).astype(np.int32)
    c["rdiag"] = np.concatenate(new_rd)
    c["rloc"] = np.concatenate(new_rl)
    c["beta"][list(EMPTY + BAD)] = 1.0
    n = np.diff(c["obs_off"])
    assert (n == 0).any() and ((n > 0) & (n < k)).any() and (n > k).any()
    return c


_cases, _refs = {}, {}


def case_and_ref(k):
    if k not in _cases:
        c = make_case(k)
        prm = _oracle.DasParams(k=k, nv=11, det_run=1, infl_adaptive=1, relax_to_inflated_prior=1, relax_alpha=0.0,
                                relax_alpha_spread=0.8, q_update_top=0.0, q_sprd_max=0.0, iv_p=4, iv_q_first=5, iv_q_last=10,
                                nthreads=4)
        ref = _oracle.das_points(prm, c["obs_off"], c["obs_idx"], c["rdiag"], c["rloc"], c["ensval"], c["dep"], c["beta"],
                                 c["infl"], c["gues"], c["sp"], c["sm"], c["sv"])
        assert ref["rc"] == 0
        _cases[k], _refs[k] = c, ref
    return _cases[k], _refs[k]


def run_gpu(c, k, warm_run, warm_stride):
    """through letkf_das_points_dev on the one-wave register kernel (k <= 20: the three-points-per-wave kernel switched off)"""
    from _gpu import ctx, dev
    anal = torch.full((c["gues"].size,), float("nan"), dtype=torch.float64, device="cuda")
    infl = dev(c["infl"])
    status = torch.full((NPTS,), -1, dtype=torch.int32, device="cuda")
    nsweep = torch.full((NPTS,), -1, dtype=torch.int32, device="cuda")
    ctx().set_option(ctx().OPT_SMALL_K_TRIO, 0)
    try:
        ctx().das_points(k, 11, dev(c["obs_off"]), dev(c["obs_idx"]), dev(c["rdiag"]), dev(c["rloc"]), dev(c["ensval"]), c["kld"],
                         dev(c["dep"]), infl, dev(c["gues"]), anal, c["sp"], c["sm"], c["sv"], beta=dev(c["beta"]), det_run=True,
                         infl_adaptive=1, relax_to_inflated_prior=1, relax_alpha_spread=0.8, iv_p=4, iv_q_first=5, iv_q_last=10,
                         status=status, nsweep=nsweep, warm_run=warm_run, warm_stride=warm_stride)
        torch.cuda.synchronize()
        assert ctx().last_path().startswith("letkf_wave_kernel") and "NW=1" in ctx().last_path(), ctx().last_path()
    finally:
        ctx().set_option(ctx().OPT_SMALL_K_TRIO, 1)
    return anal.cpu().numpy(), infl.cpu().numpy(), status.cpu().numpy(), nsweep.cpu().numpy()


def max_rel(c, k, a, b, pts):
    """max over the variables of |a - b| / max(|x-bar|, |x'|) on the members and the deterministic member of the points `pts`"""
    nens = c["nens"]
    x = c["gues"].reshape(11, nens, NPTS)
    a, b = a.reshape(11, nens, NPTS), b.reshape(11, nens, NPTS)
    members = list(range(k)) + [k + 1]
    worst = 0.0
    for v in range(11):
        scale = max(np.abs(x[v, k]).max(), np.abs(x[v, :k]).max())
        d = np.abs(a[v][members][:, pts] - b[v][members][:, pts])
        assert np.isfinite(d).all(), v
        worst = max(worst, d.max() / scale)
    return worst


@pytest.mark.parametrize("run_len", [2, 5, 16])
@pytest.mark.parametrize("stride", [0, NIJ1])
@pytest.mark.parametrize("k", [20, 33, 49, 50, 62])
def test_sorted_hand_over_keeps_the_analysis(k, stride, run_len):
    """Warm-started runs (sorted hand-over) against cold starts and against the oracle: k with and without the inert column on the
    line, list lengths from 0 over n < k to n > k, consecutive runs and runs up a column, run lengths 2, 5 and 16, with points
    without observations and points of status 3 inside the runs.  A point of status != 0 hands nothing on; its own (ill-conditioned)
    analysis is compared between warm and cold only through its status."""
    c, ref = case_and_ref(k)
    cold = run_gpu(c, k, 1, stride)
    warm = run_gpu(c, k, run_len, stride)
    good = np.array([p for p in range(NPTS) if p not in BAD])
    for tag, got in (("cold", cold), ("warm", warm)):
        st = got[2]
        assert (st[good] == 0).all(), (tag, st)
        assert (st[list(BAD)] != 0).all(), (tag, st)
    assert np.array_equal(cold[2], warm[2])
    e_wc = max_rel(c, k, warm[0], cold[0], good)
    e_wo = max_rel(c, k, warm[0], ref["anal"], good)
    e_co = max_rel(c, k, cold[0], ref["anal"], good)
    print(f"k={k} stride={stride} run={run_len}: warm-cold {e_wc:.2e}, warm-oracle {e_wo:.2e}, cold-oracle {e_co:.2e}; "
          f"nsweep warm {warm[3][good].mean():.3f} cold {cold[3][good].mean():.3f}")
    assert e_wc <= 1e-10 and e_wo <= 1e-10 and e_co <= 1e-10, (e_wc, e_wo, e_co)
    infl_ok = np.repeat(~np.isin(np.arange(NPTS), BAD)[None, :], 11, 0).reshape(-1)
    assert np.abs(warm[1] - ref["infl"])[infl_ok].max() <= 1e-12
    assert np.abs(cold[1] - ref["infl"])[infl_ok].max() <= 1e-12


@pytest.mark.parametrize("k,stride,run_len", [(50, NIJ1, 16), (49, 0, 5), (62, NIJ1, 5), (33, 0, 16), (20, NIJ1, 2)])
def test_two_calls_give_the_same_bytes(k, stride, run_len):
    """the rank is a function of the eigenvalues and the lane numbers alone: anal, status and nsweep of two calls are byte-identical"""
    c, _ = case_and_ref(k)
    a = run_gpu(c, k, run_len, stride)
    b = run_gpu(c, k, run_len, stride)
    assert a[0].tobytes() == b[0].tobytes()
    assert a[2].tobytes() == b[2].tobytes()
    assert a[3].tobytes() == b[3].tobytes()
    assert a[1].tobytes() == b[1].tobytes()


def prof_twin():
    """The PROF twin of the library (the only build that reads LETKF_AMD_WARM_DBG), rebuilt when a source is newer than it."""
    pkg_dir = os.path.join(ROOT, "scale-letkf_amd")
    lib = os.path.join(pkg_dir, "lib", "libletkf_amd_prof.so")
    srcs = [os.path.join(pkg_dir, "csrc", f) for f in os.listdir(os.path.join(pkg_dir, "csrc"))]
    srcs += [os.path.join(pkg_dir, "Makefile"), os.path.join(ROOT, "include", "letkf_amd.h")]
    if not os.path.exists(lib) or any(os.path.getmtime(s) > os.path.getmtime(lib) for s in srcs):
        subprocess.check_call(["make", "-j8", "-C", pkg_dir, "PROF=1"], stdout=2)
    return lib


def test_sorted_hand_over_cuts_sweeps_on_c2_mini():
    """C2-mini, runs up the columns, one build (the PROF twin), LETKF_AMD_WARM_DBG bit 4 against the default: mean nsweep over the
    warm-started points.  tools/sim_warm_order.py C2-mini 24 (the numpy model of the iteration, 264 warm points) gives 6.598 in
    lane order and 6.261 sorted: a difference of 0.337 sweeps, of which at least half (0.168) must show on the device.
    Measured on MI355X (25 344 warm points): 7.123 in lane order, 6.899 sorted, a difference of 0.224 (profiles/r06_README.md)."""
    sim_lane, sim_sorted = 6.598, 6.261
    env = dict(os.environ, LETKF_AMD_LIB=prof_twin())
    env.pop("LETKF_AMD_WARM_DBG", None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_warm_sort_run.py")], env=env, capture_output=True, text=True,
                       timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    res = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    print(res)
    assert res["anal_max_rel"] <= 1e-10, res
    assert res["nsweep_cold_sorted"] == res["nsweep_cold_lane"], res      # cold starts do not see the order
    assert res["nsweep_lane"] - res["nsweep_sorted"] >= 0.5 * (sim_lane - sim_sorted), res
