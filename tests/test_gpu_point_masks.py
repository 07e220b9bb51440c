"""GPU parity of the one-wave kernel's point loop where its per-row lane masks and its argument reads were restated
(csrc/letkf_wave_dev.h, r12: columns >= k zeroed by one mask, rows >= k by a wave-uniform test, the diagonal shifted and the trace
read while the column is in LDS, the arguments of the phases behind the eigensolve re-read from the argument segment), through
letkf_das_points_dev against the oracle at 1e-10 * max(|mean|, |x'|) per variable -- 5e-13 at the points with 1 <= n < k, as
tests/test_gpu_sparse_margin.py pins them.
  k: for every KR instantiation of the one-wave kernel (16, 20, 32, 48, 50, 64 serving k <= 62) its largest k, its smallest and an
     odd one; the padding is wrong first at k < KR and in the lanes >= k.  (KR = 16 serves k >= 1; k = 1 has no analysis -- the
     reference divides by k - 1 -- so its smallest k here is 2.)
  n: 0, 1, k - 1, k, 2 k and 257 (the first list that needs a second staging batch of 256), laid out so that runs of 2 and of 5
     points, consecutive and strided (warm_stride), walk through every length with the empty point and a status-3 point inside;
     warm against cold to 1e-10; a repeated call byte for byte.
  options: adaptive inflation on / off (the trace is read from the diagonal; the updated inflation is compared too), the
     deterministic member on / off, RTPS / RTPP / no relaxation -- all twelve at k = 50, 49 and 20, one of them in turn elsewhere.
  the other arguments the phases behind the eigensolve re-read (MORE): a variable-localisation class that leaves two variables
     out, RELAX_TO_INFLATED_PRIOR with an inflation that differs from variable to variable, the q-spread clamp (a cap that binds at 14 of the 20 points), and the RTPS
     factor and sweep count reported -- under RTPS and RTPP at k = 50 and 33."""
import itertools

import numpy as np
import pytest
import torch

import _oracle
from _cases import das_case

pytestmark = pytest.mark.gpu

NV = 11
NPTS = 20          # 4 columns of 5 points under warm_stride = 4
STRIDE = 4
BAD = 9            # the status-3 point: second of its consecutive run of 2 and of 5, third of its column
KS = [16, 2, 9, 20, 17, 19, 32, 21, 27, 48, 33, 41, 50, 49, 62, 51, 57]
OPTIONS = list(itertools.product((False, True), (False, True), ("rtps", "rtpp", "none")))   # (adaptive, det_run, relaxation)
MORE = dict(var_mask=0b11101101111, relax_to_inflated_prior=1, q_sprd_max=0.02)
RUNS = [("run2", 2, 0), ("run5", 5, 0), ("col2", 2, STRIDE), ("col5", 5, STRIDE)]


def lengths(k):
    ls = [0, 1, k - 1, k, 2 * k, 257]
    want = np.array([ls[(p + p // STRIDE) % 6] for p in range(NPTS)], dtype=np.int64)
    want[BAD] = k
    return want


def case(k, det_run, seed):
    c = das_case(k=k, nv=NV, npts=NPTS, nobs_tot=300, n_mean=257, seed=seed, det_run=det_run, vary_n=False, infl0=1.05)
    want = lengths(k)
    off = np.zeros(NPTS + 1, dtype=np.int64)
    np.cumsum(want, out=off[1:])
    keep = np.concatenate([np.arange(c["obs_off"][p], c["obs_off"][p] + want[p]) for p in range(NPTS)]).astype(np.int64)
    for key in ("obs_idx", "rdiag", "rloc"):
        c[key] = np.ascontiguousarray(c[key][keep])
    c["obs_off"] = off
    c["beta"][:] = 1.0
    # Y^T R^-1 Y of rank <= k - 1 and of order 1e12 against (k - 1) / rho: LETKF_ST_ILLCOND whatever the members are -- 1e4 past the
    # threshold 1 / sqrt(eps), and below 2^53, where the shift would vanish from the sums altogether
    c["rdiag"][off[BAD]:off[BAD + 1]] *= 1e-12
    return c


def relax(kind):
    return dict(relax_alpha=0.7 if kind == "rtpp" else 0.0, relax_alpha_spread=0.95 if kind == "rtps" else 0.0)


def oracle(c, k, adaptive, det_run, kind, more):
    opt = dict(relax_to_inflated_prior=0, q_sprd_max=0.0, var_mask=(1 << NV) - 1)
    opt.update(more)
    prm = _oracle.DasParams(k=k, nv=NV, det_run=int(det_run), infl_adaptive=int(adaptive), q_update_top=0.0, iv_p=4,
                            iv_q_first=5, iv_q_last=10, nthreads=4, **opt, **relax(kind))
    ref = _oracle.das_points(prm, c["obs_off"], c["obs_idx"], c["rdiag"], c["rloc"], c["ensval"], c["dep"], c["beta"],
                             c["infl"], c["gues"], c["sp"], c["sm"], c["sv"], want_rtps=True)
    assert ref["rc"] == 0
    return ref["anal"].reshape(NV, c["nens"], NPTS), ref["infl"].reshape(NV, NPTS), ref["rtps"].reshape(NV, NPTS)


def run(c, k, adaptive, det_run, kind, warm_run, warm_stride=0, more={}):
    from _gpu import ctx, dev
    anal = torch.full((c["gues"].size,), float("nan"), dtype=torch.float64, device="cuda")
    status = torch.full((NPTS,), -1, dtype=torch.int32, device="cuda")
    infl = dev(c["infl"].copy())
    rtps = torch.full((NV * NPTS,), float("nan"), dtype=torch.float64, device="cuda")
    nsweep = torch.full((NPTS,), -1, dtype=torch.int32, device="cuda")
    ctx().set_option(ctx().OPT_SMALL_K_TRIO, 0)    # (k <= 20: the one-wave kernel, not three points per wave)
    try:
        ctx().das_points(k, NV, dev(c["obs_off"]), dev(c["obs_idx"]), dev(c["rdiag"]), dev(c["rloc"]), dev(c["ensval"]),
                         c["kld"], dev(c["dep"]), infl, dev(c["gues"]), anal, c["sp"], c["sm"], c["sv"], beta=dev(c["beta"]),
                         det_run=det_run, infl_adaptive=adaptive, status=status, warm_run=warm_run, warm_stride=warm_stride,
                         rtps_infl_out=rtps, nsweep=nsweep, **more, **relax(kind))
        torch.cuda.synchronize()
    finally:
        ctx().set_option(ctx().OPT_SMALL_K_TRIO, 1)
    assert ctx().last_path().startswith("letkf_wave_kernel"), ctx().last_path()
    n = np.diff(c["obs_off"])
    ns = nsweep.cpu().numpy()
    assert ((ns > 0) == (n > 0)).all(), ns                       # a solve where there are observations, and only there
    return (anal.cpu().numpy().reshape(NV, c["nens"], NPTS), status.cpu().numpy(), infl.cpu().numpy().reshape(NV, NPTS),
            rtps.cpu().numpy().reshape(NV, NPTS))


def members(a, k, det_run):
    """the slots the path writes: members 0 .. k - 1 and, with a deterministic run, slot k + 1 (slot k, the mean, is not written)"""
    return np.concatenate([a[:, :k], a[:, k + 1:k + 2]], axis=1) if det_run else a[:, :k]


def rel(a, b, sc, pts, vs=range(NV)):
    """max over the variables `vs` of max |a - b| / scale, over the points `pts`"""
    if not pts.any():
        return 0.0
    return max(float(np.abs(a[v][:, pts] - b[v][:, pts]).max()) / sc[v] for v in vs)


def check(k, adaptive, det_run, kind, more={}):
    tag = f"k={k} adaptive={int(adaptive)} det={int(det_run)} {kind}" + (" more" if more else "")
    c = case(k, det_run, seed=12000 + k)
    vs = [v for v in range(NV) if (more.get("var_mask", -1) >> v) & 1]     # the variables of the class: the others are not written
    if more:
        c["infl"] = (c["infl"].reshape(NV, NPTS) + 0.02 * np.arange(NV)[:, None]).reshape(-1)
    x = c["gues"].reshape(NV, c["nens"], NPTS)
    sc = np.array([max(np.abs(x[v, k]).max(), np.abs(x[v, :k]).max()) for v in range(NV)])
    n = np.diff(c["obs_off"])
    want_st = np.where(np.arange(NPTS) == BAD, 3, 0)
    good = want_st == 0
    few = good & (n >= 1) & (n < k)                                  # the 5e-13 points
    rest = good & ~few
    exp_a, exp_i, exp_r = oracle(c, k, adaptive, det_run, kind, more)
    exp = members(exp_a, k, det_run)
    results = {}
    for name, warm_run, stride in [("cold", 1, 0)] + RUNS:
        a, st, infl, rtps = run(c, k, adaptive, det_run, kind, warm_run, stride, more)
        got = members(a, k, det_run)
        results[name] = got
        e_few, e_rest = rel(got, exp, sc, few, vs), rel(got, exp, sc, rest, vs)
        e_infl = float(np.abs(infl[:, good] - exp_i[:, good]).max() / np.abs(exp_i).max())
        e_rtps = float(np.abs(rtps[vs][:, good] - exp_r[vs][:, good]).max())          # (factors of order 1)
        ew = rel(got, results["cold"], sc, good, vs)
        print(f"{tag} {name}: err/scale n<k {e_few:.3e} others {e_rest:.3e} infl {e_infl:.3e} rtps {e_rtps:.3e} warm-cold {ew:.3e}")
        assert (st == want_st).all(), (tag, name, st)
        assert np.isfinite(got[vs]).all(), (tag, name)
        assert e_few <= 5e-13 and e_rest <= 1e-10, (tag, name, e_few, e_rest)
        assert e_infl <= 1e-10 and e_rtps <= 1e-10, (tag, name, e_infl, e_rtps)
        assert ew <= 1e-10, (tag, name, ew)
        if name in ("cold", "run5", "col2"):
            again, _, infl2, _ = run(c, k, adaptive, det_run, kind, warm_run, stride, more)
            assert members(again, k, det_run).tobytes() == got.tobytes() and infl2.tobytes() == infl.tobytes(), (tag, name)


@pytest.mark.parametrize("k", KS)
def test_every_k_of_every_instantiation(k):
    adaptive, det_run, kind = OPTIONS[KS.index(k) % len(OPTIONS)]
    check(k, adaptive, det_run, kind)


@pytest.mark.parametrize("adaptive,det_run,kind", OPTIONS)
@pytest.mark.parametrize("k", [50, 49, 20])
def test_every_option_at_the_production_k(k, adaptive, det_run, kind):
    check(k, adaptive, det_run, kind)


@pytest.mark.parametrize("kind", ["rtps", "rtpp"])
@pytest.mark.parametrize("k", [50, 33])
def test_the_other_arguments_the_phases_re_read(k, kind):
    check(k, True, True, kind, MORE)
