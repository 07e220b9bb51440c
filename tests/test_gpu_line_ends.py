"""GPU parity at the two ends of the Jacobi line (jacobi_split, csrc/letkf_jacobi_dev.h).  The slot without a left partner and the
slot without a right one keep their norms and scales through DPP moves that leave their destination alone; where those ends sit
depends on k alone (S = ceil(k / 2) slots, an odd k with one inert zero column at the far end).  So: every ensemble size that
moves an end inside a one-wave instantiation of the register kernel -- k = 33, 34, 49, 50 and the smallest and largest k of every
other KR (16: 2 .. 16, 20: 17 .. 20, 32: 21 .. 32, 48: 33 .. 48, 50: 49 .. 50, 64: 51 .. 62) -- with local lists of n = 0, 1, k - 1,
k and 200 observations (n < k: the eigenvalue (k - 1) / rho with multiplicity k - n, 45-degree rotations inside the cluster, at
the ends of the line too), cold (runs of 1), warm-started (runs of 16) and strided runs, through letkf_das_points_dev and
letkf_core_batch_dev against the oracle.  Tolerances as tests/test_gpu_das.py and tests/test_gpu_core_batch.py write them:
1e-10 * max(|mean|, |x'|) on the analysis, 1e-11 on T / Pa / w-bar, 1e-12 on the inflation; and the warm and the cold
analysis of the same points agree to 1e-10 (the warm-start product reads the previous point's eigenvectors from the workspace: a
wrong layout there shows at once)."""
import numpy as np
import pytest
import torch

import _oracle
from _cases import core_case, das_case, relerr

pytestmark = pytest.mark.gpu

KS = [2, 3, 15, 16, 17, 19, 20, 21, 31, 32, 33, 34, 47, 48, 49, 50, 51, 61, 62]
NPTS = 40          # a multiple of the strided run's stride, 8 points of every list length


def list_lengths(k):
    return [0, 1, k - 1, k, 200]


def das_case_with_lengths(k, seed):
    """das_case with every local list cut to one of the five lengths, in turn along the points (so that a warm run walks through
    all of them: a point with n < k follows one with n = 200 and the other way round)"""
    c = das_case(k=k, nv=11, npts=NPTS, nobs_tot=400, n_mean=200, seed=seed, det_run=True, vary_n=False, infl0=1.07)
    want = np.array([list_lengths(k)[p % 5] for p in range(NPTS)], dtype=np.int64)
    off = np.zeros(NPTS + 1, dtype=np.int64)
    np.cumsum(want, out=off[1:])
    keep = np.concatenate([np.arange(c["obs_off"][p], c["obs_off"][p] + want[p]) for p in range(NPTS)]).astype(np.int64)
    for key in ("obs_idx", "rdiag", "rloc"):
        c[key] = np.ascontiguousarray(c[key][keep])
    c["obs_off"] = off
    c["beta"][:] = 1.0
    c["beta"][7::11] = 0.37
    return c


def run_das(c, k, warm_run, warm_stride=0, want_trans=False):
    from _gpu import ctx, dev
    anal = torch.full((c["gues"].size,), float("nan"), dtype=torch.float64, device="cuda")
    infl = dev(c["infl"])
    status = torch.full((NPTS,), -1, dtype=torch.int32, device="cuda")
    trans = torch.zeros(NPTS, k * k, dtype=torch.float64, device="cuda") if want_trans else None
    transm = torch.zeros(NPTS, k, dtype=torch.float64, device="cuda") if want_trans else None
    ctx().das_points(k, 11, dev(c["obs_off"]), dev(c["obs_idx"]), dev(c["rdiag"]), dev(c["rloc"]), dev(c["ensval"]), c["kld"],
                     dev(c["dep"]), infl, dev(c["gues"]), anal, c["sp"], c["sm"], c["sv"], beta=dev(c["beta"]), det_run=True,
                     infl_adaptive=1, relax_to_inflated_prior=1, relax_alpha_spread=0.8, iv_p=4, iv_q_first=5, iv_q_last=10,
                     trans_out=trans, transm_out=transm, status=status, warm_run=warm_run, warm_stride=warm_stride)
    torch.cuda.synchronize()
    return (anal.cpu().numpy(), infl.cpu().numpy(), status.cpu().numpy(), trans.cpu().numpy() if want_trans else None,
            transm.cpu().numpy() if want_trans else None)


def check_das(c, ref, k, got, tag):
    anal, infl, status, trans, transm = got
    assert (status == 0).all(), (tag, status)
    nens = c["nens"]
    g = anal.reshape(11, nens, NPTS)
    e = ref["anal"].reshape(11, nens, NPTS)
    x = c["gues"].reshape(11, nens, NPTS)
    members = list(range(k)) + [k + 1]
    for v in range(11):
        scale = max(np.abs(x[v, k]).max(), np.abs(x[v, :k]).max())
        err = np.abs(g[v, members] - e[v, members]).max()
        print(f"k={k} {tag} v={v} err/scale={err / scale:.3e}")
        assert np.isfinite(g[v, members]).all(), (tag, v)
        assert err <= 1e-10 * scale, (tag, v, err, scale)
    assert np.abs(infl - ref["infl"]).max() <= 1e-12, tag
    for p in range(NPTS if trans is not None else 0):
        den = np.abs(ref["trans"][p]).max()
        assert np.abs(trans[p] - ref["trans"][p]).max() <= 1e-11 * den, (tag, p)
        assert np.abs(transm[p] - ref["transm"][p]).max() <= 1e-11 * max(1.0, np.abs(ref["transm"][p]).max()), (tag, p)


@pytest.mark.parametrize("k", KS)
def test_das_points_line_ends(k):
    """letkf_das_points_dev on the one-wave register kernel (k <= 20: the three-points-per-wave kernel switched off, and on), every
    list length, runs of 1, runs of 16 and strided runs, against the oracle; warm against cold to 1e-10; and once more with T and
    w-bar requested (the kernel's instantiation with the k x k outputs), warm-started."""
    from _gpu import ctx
    c = das_case_with_lengths(k, seed=7000 + k)
    prm = _oracle.DasParams(k=k, nv=11, det_run=1, infl_adaptive=1, relax_to_inflated_prior=1, relax_alpha=0.0,
                            relax_alpha_spread=0.8, q_update_top=0.0, q_sprd_max=0.0, iv_p=4, iv_q_first=5, iv_q_last=10,
                            nthreads=4)
    ref = _oracle.das_points(prm, c["obs_off"], c["obs_idx"], c["rdiag"], c["rloc"], c["ensval"], c["dep"], c["beta"],
                             c["infl"], c["gues"], c["sp"], c["sm"], c["sv"], want_trans=True)
    assert ref["rc"] == 0
    for trio in ((0, 1) if k <= 20 else (1,)):
        ctx().set_option(ctx().OPT_SMALL_K_TRIO, trio)
        try:
            res = {}
            for tag, warm_run, stride in (("cold", 1, 0), ("warm16", 16, 0), ("stride8", 0, 8)):
                res[tag] = run_das(c, k, warm_run, stride)
                want = "letkf_trio_kernel" if (trio and k <= 20) else "letkf_wave_kernel"
                assert ctx().last_path().startswith(want), ctx().last_path()
                check_das(c, ref, k, res[tag], f"trio={trio} {tag}")
        finally:
            ctx().set_option(ctx().OPT_SMALL_K_TRIO, 1)
        if trio:
            got = run_das(c, k, 16, 0, want_trans=True)
            assert ctx().last_path().startswith("letkf_wave_kernel"), ctx().last_path()
            check_das(c, ref, k, got, "warm16 + T")
        x = c["gues"].reshape(11, c["nens"], NPTS)
        for tag in ("warm16", "stride8"):
            a, b = res["cold"][0].reshape(x.shape), res[tag][0].reshape(x.shape)
            for v in range(11):
                scale = max(np.abs(x[v, k]).max(), np.abs(x[v, :k]).max())
                assert np.abs(a[v, :k] - b[v, :k]).max() <= 1e-10 * scale, (trio, tag, v)


@pytest.mark.parametrize("k", KS)
def test_core_batch_line_ends(k):
    """letkf_core_batch_dev (dense hdxb; T, Pa, w-bar and the deterministic member's weights out) for the same ensemble sizes and
    list lengths, 1e-11 as tests/test_gpu_core_batch.py"""
    from _gpu import ctx, dev
    nobs, reps = 200, 3
    lens = list_lengths(k) * reps
    nb = len(lens)
    nobsl = np.array(lens, dtype=np.int32)
    rng = np.random.default_rng(8000 + k)
    H = np.zeros((nb, k, nobs))
    rd = np.zeros((nb, nobs)); rl = np.zeros((nb, nobs)); dp = np.zeros((nb, nobs)); dd = np.zeros((nb, nobs))
    infl = rng.uniform(1.0, 1.3, size=nb)
    exp = []
    for b in range(nb):
        c = core_case(k, int(nobsl[b]), seed=8100 + 31 * k + b, nobs=nobs, rdiag_wloc=True, infl=float(infl[b]), with_det=True)
        H[b] = c["hdxb"].T
        rd[b], rl[b], dp[b], dd[b] = c["rdiag"], c["rloc"], c["dep"], c["depd"]
        exp.append(_oracle.letkf_core("oracle", k, nobs, int(nobsl[b]), c["hdxb"], c["rdiag"], c["rloc"], c["dep"],
                                      float(infl[b]), rdiag_wloc=True, infl_update=True, depd=c["depd"], want_transmd=True))
    d_infl = dev(infl)
    trans = torch.zeros(nb, k * k, dtype=torch.float64, device="cuda")
    pao = torch.zeros_like(trans)
    transm = torch.zeros(nb, k, dtype=torch.float64, device="cuda")
    transmd = torch.zeros_like(transm)
    status = torch.full((nb,), -1, dtype=torch.int32, device="cuda")
    nsweep = torch.zeros(nb, dtype=torch.int32, device="cuda")
    ctx().core_batch(k, nobs, dev(nobsl), dev(H), dev(rd), dev(rl), dev(dp), d_infl, trans, transm=transm, pao=pao,
                     depd=dev(dd), transmd=transmd, rdiag_wloc=True, infl_update=True, status=status, nsweep=nsweep)
    torch.cuda.synchronize()
    assert status.cpu().numpy().tolist() == [0] * nb
    T = trans.cpu().numpy(); P = pao.cpu().numpy(); W = transm.cpu().numpy(); WD = transmd.cpu().numpy()
    I = d_infl.cpu().numpy()
    for b in range(nb):
        e = exp[b]
        et, ep = relerr(T[b].reshape(k, k).T, e["trans"]), relerr(P[b].reshape(k, k).T, e["pao"])
        print(f"k={k} n={nobsl[b]} T {et:.3e} Pa {ep:.3e}")
        assert et <= 1e-11, (b, nobsl[b])
        assert ep <= 1e-11, (b, nobsl[b])
        assert np.abs(W[b] - e["transm"]).max() <= 1e-11 * max(1.0, np.abs(e["transm"]).max()), (b, nobsl[b])
        assert np.abs(WD[b] - e["transmd"]).max() <= 1e-11 * max(1.0, np.abs(e["transmd"]).max()), (b, nobsl[b])
        assert abs(I[b] - e["parm_infl"]) <= 1e-12, (b, nobsl[b])
    assert int(nsweep.max()) < 30
