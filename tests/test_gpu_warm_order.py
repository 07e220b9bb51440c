"""Hand-over position of the warm start (csrc/letkf_wave_dev.h warm_position, LETKF_WARM_ORDER), and the apply phase of the
k = 49, 50 instantiation in all its reachable variants.

A one-wave point leaves its eigenvectors in the workspace sorted by eigenvalue with rank r at line position r ^ 1 (whole pairs of
valid ranks only).  The next point's solve starts from a column-permuted Q -- the same eigenvectors, so the analysis must stay
what the cold start gives and what the oracle gives (1e-10 * max(|x-bar|, |x'|) per variable), and two
calls must give the same bytes.  The apply phase (U = V^T B, C = D U, Out = V C on the matrix cores; profiles/r08_README.md has
the strip form of it that was measured and not kept) is compared with the oracle at the same bar."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _oracle
from _cases import DIST_ZERO_FAC_SQUARE, das_case

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NIJ1, NLEV = 3, 16
NPTS = NIJ1 * NLEV
NOBS_TOT = 700
EMPTY = (7, 22)        # points without observations ...
BAD = (13, 37)         # ... and points whose solve ends with status 3, inside the runs (consecutive runs and runs up a column)
RELAX = {"rtps": dict(relax_alpha_spread=0.8), "none": dict()}


def forced_lengths(k):
    """list length of chosen points: 1, k - 1, k, 2k, each once low and once high in the columns"""
    return {1: 1, 4: k - 1, 8: k, 11: 2 * k, 16: 2 * k, 20: k, 25: k - 1, 29: 1}


def make_case(k):
    """das_case with list lengths 0 .. 2k, the lengths 0, 1, k - 1, k and 2k at fixed points (n < k: the eigenvalue (k-1)/rho with
    multiplicity k - n), two points without observations and two ill-conditioned ones (5 observations with an error variance of
    1e-12: lambda_max / lambda_min > 1e12, status 3) placed inside the runs."""
    c = das_case(k=k, nv=11, npts=NPTS, nobs_tot=NOBS_TOT, n_mean=k, seed=8000 + k, det_run=True, infl0=1.07)
    off, idx, rdiag, rloc = c["obs_off"], c["obs_idx"], c["rdiag"], c["rloc"]
    rng = np.random.default_rng(80 + k)
    force = forced_lengths(k)
    new_idx, new_rd, new_rl, new_cnt = [], [], [], []
    for p in range(NPTS):
        if p in EMPTY:
            new_cnt.append(0)
            continue
        if p in BAD or p in force:
            n = 5 if p in BAD else force[p]
            rl = np.ones(n) if p in BAD else np.exp(-0.5 * rng.uniform(0.0, DIST_ZERO_FAC_SQUARE, size=n))
            new_idx.append(rng.choice(NOBS_TOT, size=n, replace=False).astype(np.int32))
            new_rd.append(np.full(n, 1e-12) if p in BAD else rng.choice([1.0, 9.0, 25.0], size=n) / rl)
            new_rl.append(rl)
            new_cnt.append(n)
            continue
        s = slice(off[p], off[p + 1])
        new_idx.append(idx[s])
        new_rd.append(rdiag[s])
        new_rl.append(rloc[s])
        new_cnt.append(int(off[p + 1] - off[p]))
    c["obs_off"] = np.concatenate([[0], np.cumsum(new_cnt)]).astype(np.int64)
    c["obs_idx"] = np.concatenate(new_idx).astype(np.int32)
    c["rdiag"] = np.concatenate(new_rd)
    c["rloc"] = np.concatenate(new_rl)
    c["beta"][list(EMPTY + BAD) + list(force)] = 1.0
    n = np.diff(c["obs_off"])
    assert {0, 1, k - 1, k, 2 * k} <= set(n.tolist())
    return c


_cases, _refs, _cold = {}, {}, {}


def case_and_ref(k, relax):
    if k not in _cases:
        _cases[k] = make_case(k)
    c = _cases[k]
    if (k, relax) not in _refs:
        prm = _oracle.DasParams(k=k, nv=11, det_run=1, infl_adaptive=1, relax_to_inflated_prior=1, relax_alpha=0.0,
                                relax_alpha_spread=RELAX[relax].get("relax_alpha_spread", 0.0), q_update_top=0.0, q_sprd_max=0.0,
                                iv_p=4, iv_q_first=5, iv_q_last=10, nthreads=4)
        ref = _oracle.das_points(prm, c["obs_off"], c["obs_idx"], c["rdiag"], c["rloc"], c["ensval"], c["dep"], c["beta"],
                                 c["infl"], c["gues"], c["sp"], c["sm"], c["sv"])
        assert ref["rc"] == 0
        _refs[k, relax] = ref
    return c, _refs[k, relax]


def run_gpu(c, k, relax, warm_run, warm_stride):
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
                         infl_adaptive=1, relax_to_inflated_prior=1, iv_p=4, iv_q_first=5, iv_q_last=10, status=status,
                         nsweep=nsweep, warm_run=warm_run, warm_stride=warm_stride, **RELAX[relax])
        torch.cuda.synchronize()
        assert ctx().last_path().startswith("letkf_wave_kernel") and "NW=1" in ctx().last_path(), ctx().last_path()
    finally:
        ctx().set_option(ctx().OPT_SMALL_K_TRIO, 1)
    return anal.cpu().numpy(), infl.cpu().numpy(), status.cpu().numpy(), nsweep.cpu().numpy()


def cold_run(c, k, relax, stride):
    if (k, relax, stride) not in _cold:
        _cold[k, relax, stride] = run_gpu(c, k, relax, 1, stride)
    return _cold[k, relax, stride]


def max_rel(c, k, a, b, pts, nens=None, npts=NPTS, members=None):
    """max over the variables of |a - b| / max(|x-bar|, |x'|) on the members (and the deterministic member) of the points `pts`"""
    nens = c["nens"] if nens is None else nens
    x = c["gues"].reshape(11, nens, npts)
    a, b = a.reshape(11, nens, npts), b.reshape(11, nens, npts)
    members = (list(range(k)) + [k + 1]) if members is None else members
    worst = 0.0
    for v in range(11):
        scale = max(np.abs(x[v, k]).max(), np.abs(x[v, :k]).max())
        d = np.abs(a[v][members][:, pts] - b[v][members][:, pts])
        assert np.isfinite(d).all(), v
        worst = max(worst, d.max() / scale)
    return worst


@pytest.mark.parametrize("relax", list(RELAX))
@pytest.mark.parametrize("run_len", [2, 5, 16])
@pytest.mark.parametrize("stride", [0, NIJ1])
@pytest.mark.parametrize("k", [20, 33, 49, 50, 62])
def test_pair_hand_over_keeps_the_analysis(k, stride, run_len, relax):
    """Warm-started runs against cold starts and against the oracle: k with and without the inert column on the line (odd k: the
    unpaired last rank), list lengths 0, 1, k - 1, k, 2k and others, consecutive runs and runs up a column, run lengths 2, 5 and 16,
    with points without observations and points of status 3 inside the runs, RTPS and no relaxation.  A point of status != 0 hands
    nothing on; its own (ill-conditioned) analysis is compared between warm and cold only through its status."""
    c, ref = case_and_ref(k, relax)
    cold = cold_run(c, k, relax, stride)
    warm = run_gpu(c, k, relax, run_len, stride)
    good = np.array([p for p in range(NPTS) if p not in BAD])
    for tag, got in (("cold", cold), ("warm", warm)):
        st = got[2]
        assert (st[good] == 0).all(), (tag, st)
        assert (st[list(BAD)] == 3).all(), (tag, st)
    e_wc = max_rel(c, k, warm[0], cold[0], good)
    e_wo = max_rel(c, k, warm[0], ref["anal"], good)
    e_co = max_rel(c, k, cold[0], ref["anal"], good)
    print(f"k={k} stride={stride} run={run_len} {relax}: warm-cold {e_wc:.2e}, warm-oracle {e_wo:.2e}, cold-oracle {e_co:.2e}; "
          f"nsweep warm {warm[3][good].mean():.3f} cold {cold[3][good].mean():.3f}")
    assert e_wc <= 1e-10 and e_wo <= 1e-10 and e_co <= 1e-10, (e_wc, e_wo, e_co)
    infl_ok = np.repeat(~np.isin(np.arange(NPTS), BAD)[None, :], 11, 0).reshape(-1)
    assert np.abs(warm[1] - ref["infl"])[infl_ok].max() <= 1e-12
    assert np.abs(cold[1] - ref["infl"])[infl_ok].max() <= 1e-12


@pytest.mark.parametrize("k,stride,run_len,relax", [(50, NIJ1, 16, "rtps"), (49, 0, 5, "none"), (62, NIJ1, 5, "rtps"),
                                                    (33, 0, 16, "none"), (20, NIJ1, 2, "rtps")])
def test_two_calls_give_the_same_bytes(k, stride, run_len, relax):
    """the position is a function of the eigenvalues and the lane numbers alone: anal, infl, status and nsweep of two calls are
    byte-identical"""
    c, _ = case_and_ref(k, relax)
    a = run_gpu(c, k, relax, run_len, stride)
    b = run_gpu(c, k, relax, run_len, stride)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()


def prof_twin():
    """The PROF twin of the library (the only build that reads LETKF_AMD_WARM_DBG), rebuilt when a source is newer than it."""
    pkg_dir = os.path.join(ROOT, "scale-letkf_amd")
    lib = os.path.join(pkg_dir, "lib", "libletkf_amd_prof.so")
    srcs = [os.path.join(pkg_dir, "csrc", f) for f in os.listdir(os.path.join(pkg_dir, "csrc"))]
    srcs += [os.path.join(pkg_dir, "Makefile"), os.path.join(ROOT, "include", "letkf_amd.h")]
    if not os.path.exists(lib) or any(os.path.getmtime(s) > os.path.getmtime(lib) for s in srcs):
        subprocess.check_call(["make", "-j8", "-C", pkg_dir, "PROF=1"], stdout=2)
    return lib


def test_both_positions_converge_and_agree_on_c2_mini():
    """C2-mini, runs up the columns, one build (the PROF twin), LETKF_AMD_WARM_DBG bit 5 (position = rank) against the default
    (position = rank ^ 1): both converge with status 0 everywhere and give the same analysis to 1e-10.  The sweep counts and the
    twin's time inside the iteration are printed, not asserted: they are a measurement (profiles/r08_README.md)."""
    env = dict(os.environ, LETKF_AMD_LIB=prof_twin())
    env.pop("LETKF_AMD_WARM_DBG", None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_warm_order_run.py")], env=env, capture_output=True, text=True,
                       timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    res = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    print(res)
    assert res["status_max_pair"] == 0 and res["status_max_rank"] == 0, res
    assert res["anal_max_rel"] <= 1e-10, res


# ---------------------------------------------------------------------------------------------------------------------------------
# the apply phase of the KR = 50 one-wave instantiation (k = 49, 50): U = V^T B, C = D U, Out = V C and what is made of them

APPLY_NPTS = 24
APPLY_RELAX = {"rtps": dict(relax_alpha_spread=0.95), "rtpp": dict(relax_alpha=0.7, relax_to_inflated_prior=1), "none": dict()}


@pytest.mark.parametrize("qclamp", [0.0, 0.05])
@pytest.mark.parametrize("relax", list(APPLY_RELAX))
@pytest.mark.parametrize("det", [False, True])
@pytest.mark.parametrize("k", [49, 50])
def test_apply_phase_variants_against_the_oracle(k, det, relax, qclamp):
    """k = 49 (row and eigen-column 49 are padding) and 50, with and without the deterministic member (column 1 of B), RTPS (var_a
    from U, var_g from B: eigen-columns 48, 49 sit in the narrow last tile), RTPP and no relaxation, beta in {0, 0.37, 1} across
    the points, the q clamp on and off; warm-started runs of the library's default length."""
    from _gpu import ctx, dev
    cfg = APPLY_RELAX[relax]
    c = das_case(k=k, nv=11, npts=APPLY_NPTS, nobs_tot=500, n_mean=70, seed=900 + k, det_run=det, infl0=1.07)
    c["beta"][[2, 9, 17]] = (0.0, 0.37, 1.0)
    assert {0.0, 0.37, 1.0} <= set(c["beta"].tolist())
    kw = dict(relax_to_inflated_prior=cfg.get("relax_to_inflated_prior", 0), relax_alpha=cfg.get("relax_alpha", 0.0),
              relax_alpha_spread=cfg.get("relax_alpha_spread", 0.0), q_sprd_max=qclamp, iv_p=4, iv_q_first=5, iv_q_last=10)
    prm = _oracle.DasParams(k=k, nv=11, det_run=int(det), infl_adaptive=0, q_update_top=0.0, nthreads=4, **kw)
    ref = _oracle.das_points(prm, c["obs_off"], c["obs_idx"], c["rdiag"], c["rloc"], c["ensval"], c["dep"], c["beta"], c["infl"],
                             c["gues"], c["sp"], c["sm"], c["sv"])
    assert ref["rc"] == 0
    anal = torch.full((c["gues"].size,), float("nan"), dtype=torch.float64, device="cuda")
    status = torch.full((APPLY_NPTS,), -1, dtype=torch.int32, device="cuda")
    ctx().das_points(k, 11, dev(c["obs_off"]), dev(c["obs_idx"]), dev(c["rdiag"]), dev(c["rloc"]), dev(c["ensval"]), c["kld"],
                     dev(c["dep"]), dev(c["infl"]), dev(c["gues"]), anal, c["sp"], c["sm"], c["sv"], beta=dev(c["beta"]),
                     det_run=det, status=status, **kw)
    torch.cuda.synchronize()
    assert ctx().last_path().startswith("letkf_wave_kernel<KR=50"), ctx().last_path()
    assert int(status.abs().max()) == 0, status
    members = list(range(k)) + ([k + 1] if det else [])
    err = max_rel(c, k, anal.cpu().numpy(), ref["anal"], np.arange(APPLY_NPTS), nens=c["nens"], npts=APPLY_NPTS, members=members)
    print(f"k={k} det={det} {relax} qclamp={qclamp}: max rel err vs oracle {err:.2e}")
    assert err <= 1e-10, err
