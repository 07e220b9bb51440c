"""GPU parity of the one-wave Jacobi with its rotation tests decided on the upper dwords of g2 and ab (csrc/letkf_rot_rule.h:
rotate above 2^-100, stop at 2^-80, early stop at 2^-54 of the squared cosine) and one vote per step pair, through
letkf_das_points_dev against the oracle at 1e-10 * max(|mean|, |x'|) per variable.
  k = 33, 49, 50, 62 (an odd k with its inert zero column, both ends of KR = 48 / 50 / 64); local lists of 0, 1, k - 1, k, 2 k and 4 k
  observations, arranged so that consecutive runs and column runs (warm_stride) of 2, 5 and 16 points all walk through every
  length, the empty point inside; warm against cold to 1e-10; a repeated call byte for byte.
  Observation-space perturbations scaled by 1e-6 (G is the identity up to 1e-12: every squared cosine sits round the three
  thresholds), by 1e+3 (far above them) and by 1e+6 (every point with observations ill-conditioned: status 3, compared through the
  status as tests/test_gpu_warm_order.py does); two identical members (an exact cluster: g2 = ab to rounding, h = 0); every point with
  n < k (the eigenvalue (k - 1) / rho with multiplicity k - n: 45-degree rotations at noise-level cosines), which keeps the 5e-13
  that tests/test_gpu_sparse_margin.py pins for such points; and a NaN row in the list of one point inside a run: that point
  reports a status, the next one is its cold-start result bit for bit, the points of the other runs are untouched, and the call
  returns."""
import numpy as np
import pytest
import torch

import _oracle
from _cases import das_case
from _degenerate import twin_state

pytestmark = pytest.mark.gpu

NV = 11
NPTS = 96          # 6 columns of 16 points under warm_stride = 6
STRIDE = 6         # column runs: points p, p + 6, ..., 16 of them


def lengths(k, npts=NPTS, sparse=False):
    ls = [1, 2, k // 2, k - 2, k - 1, k // 3] if sparse else [0, 1, k - 1, k, 2 * k, 4 * k]
    # along consecutive points and along a column (p, p + STRIDE, ...) alike every length comes by
    return np.array([ls[(p + p // STRIDE) % 6] for p in range(npts)], dtype=np.int64)


def case(k, seed, sparse=False, ens_scale=1.0, twins=False):
    c = das_case(k=k, nv=NV, npts=NPTS, nobs_tot=4 * k + 40, n_mean=4 * k, seed=seed, det_run=False, vary_n=False, infl0=1.05)
    want = lengths(k, sparse=sparse)
    off = np.zeros(NPTS + 1, dtype=np.int64)
    np.cumsum(want, out=off[1:])
    keep = np.concatenate([np.arange(c["obs_off"][p], c["obs_off"][p] + want[p]) for p in range(NPTS)]).astype(np.int64)
    for key in ("obs_idx", "rdiag", "rloc"):
        c[key] = np.ascontiguousarray(c[key][keep])
    c["obs_off"] = off
    c["beta"][:] = 1.0
    if twins:
        twin_state(c, ens_too=True)
    c["ensval"][:, :k] *= ens_scale
    return c


def oracle(c, k):
    prm = _oracle.DasParams(k=k, nv=NV, det_run=0, infl_adaptive=0, relax_to_inflated_prior=0, relax_alpha=0.0,
                            relax_alpha_spread=0.95, q_update_top=0.0, q_sprd_max=0.0, iv_p=4, iv_q_first=5, iv_q_last=10,
                            nthreads=4)
    ref = _oracle.das_points(prm, c["obs_off"], c["obs_idx"], c["rdiag"], c["rloc"], c["ensval"], c["dep"], c["beta"],
                             c["infl"], c["gues"], c["sp"], c["sm"], c["sv"])
    assert ref["rc"] == 0
    return ref["anal"].reshape(NV, c["nens"], NPTS)[:, :k]


def run(c, k, warm_run, warm_stride=0):
    from _gpu import ctx, dev
    anal = torch.full((c["gues"].size,), float("nan"), dtype=torch.float64, device="cuda")
    status = torch.full((NPTS,), -1, dtype=torch.int32, device="cuda")
    ctx().das_points(k, NV, dev(c["obs_off"]), dev(c["obs_idx"]), dev(c["rdiag"]), dev(c["rloc"]), dev(c["ensval"]), c["kld"],
                     dev(c["dep"]), dev(c["infl"]), dev(c["gues"]), anal, c["sp"], c["sm"], c["sv"], beta=dev(c["beta"]),
                     relax_alpha_spread=0.95, status=status, warm_run=warm_run, warm_stride=warm_stride)
    torch.cuda.synchronize()
    assert ctx().last_path().startswith("letkf_wave_kernel"), ctx().last_path()
    return anal.cpu().numpy().reshape(NV, c["nens"], NPTS)[:, :k], status.cpu().numpy()


def scales(c, k):
    x = c["gues"].reshape(NV, c["nens"], NPTS)
    return np.array([max(np.abs(x[v, k]).max(), np.abs(x[v, :k]).max()) for v in range(NV)])


def rel(a, b, sc, pts=slice(None)):
    """max over variables of max |a - b| / scale, over the points `pts`"""
    return max(float(np.abs(a[v][:, pts] - b[v][:, pts]).max()) / sc[v] for v in range(NV))


RUNS = [("run2", 2, 0), ("run5", 5, 0), ("run16", 16, 0), ("col2", 2, STRIDE), ("col5", 5, STRIDE), ("col16", 16, STRIDE)]


def check_all_runs(c, k, bound, tag, illcond=False):
    """cold, repeated, and the six warm runs against the oracle (`bound`), warm against cold (1e-10).  illcond: every point with
    observations owes LETKF_ST_ILLCOND (3); as in tests/test_gpu_warm_order.py such a point is compared through its status alone
    -- the oracle treats its spectrum as the reference does, the library reports it -- and its analysis must be finite and repeat."""
    exp, sc = oracle(c, k), scales(c, k)
    want_st = np.where(np.diff(c["obs_off"]) > 0, 3, 0) if illcond else np.zeros(NPTS, dtype=np.int64)
    good = want_st == 0
    cold, st = run(c, k, 1)
    assert (st == want_st).all(), (tag, st)
    e = rel(cold, exp, sc, good)
    print(f"{tag} k={k} cold err/scale={e:.3e}" + (f" (status 3 points: {rel(cold, exp, sc, ~good):.3e})" if illcond else ""))
    assert np.isfinite(cold).all() and e <= bound, (tag, e)
    again, _ = run(c, k, 1)
    assert cold.tobytes() == again.tobytes(), tag
    for name, warm_run, stride in RUNS:
        got, st = run(c, k, warm_run, stride)
        assert (st == want_st).all(), (tag, name, st)
        e, ew = rel(got, exp, sc, good), rel(got, cold, sc, good)
        print(f"{tag} k={k} {name} err/scale={e:.3e} warm-cold={ew:.3e}")
        assert np.isfinite(got).all() and e <= bound, (tag, name, e)
        assert ew <= 1e-10, (tag, name, ew)
        if name in ("run16", "col5"):
            again, _ = run(c, k, warm_run, stride)
            assert got.tobytes() == again.tobytes(), (tag, name)


@pytest.mark.parametrize("k", [33, 49, 50, 62])
def test_every_list_length_in_consecutive_and_column_runs(k):
    check_all_runs(case(k, seed=11000 + k), k, 1e-10, "lengths")


@pytest.mark.parametrize("k", [33, 50])
@pytest.mark.parametrize("ens_scale", [1e-6, 1e3, 1e6])
def test_cosines_near_and_far_from_the_thresholds(k, ens_scale):
    """1e-6: G is the identity up to 1e-12, every squared cosine sits round the three thresholds.  1e+3: far above them, and the
    spectrum still inside 1 / sqrt(eps).  1e+6: Y^T R^-1 Y (rank k - 1: the perturbations are centred) against (k - 1) / rho spans
    1e10 and more, so every point with observations is LETKF_ST_ILLCOND -- in the library before the integer tests as well, where
    these points sat 1.2 (k = 33) and 0.99 (k = 50) of the scale from the oracle exactly as they do now: checked through the status."""
    check_all_runs(case(k, seed=11100 + k, ens_scale=ens_scale), k, 1e-10, f"scale{ens_scale:g}", illcond=ens_scale > 1e5)


@pytest.mark.parametrize("k", [33, 50])
def test_two_identical_members(k):
    check_all_runs(case(k, seed=11200 + k, twins=True), k, 1e-10, "twins")


@pytest.mark.parametrize("k", [33, 50])
def test_fewer_observations_than_members_at_every_point(k):
    check_all_runs(case(k, seed=11300 + k, sparse=True), k, 5e-13, "sparse")


@pytest.mark.parametrize("k", [33, 50])
@pytest.mark.parametrize("warm_run,stride", [(16, 0), (16, STRIDE)])
def test_a_nan_row_inside_a_run(k, warm_run, stride):
    c = case(k, seed=11400 + k)
    clean, st0 = run(c, k, warm_run, stride)
    cold, _ = run(c, k, 1)
    assert (st0 == 0).all()
    # one more row of the observation table, NaN in every member, listed by ONE point in the middle of a run
    step = stride if stride else 1
    bad = 38 if stride else 37           # the seventh point of column 2's run (38 = 2 + 6 * 6) / the sixth of the run 32 .. 47
    nxt = bad + step
    assert lengths(k)[bad] > 0 and lengths(k)[nxt] > 0
    row = c["ensval"].shape[0]
    c["ensval"] = np.ascontiguousarray(np.vstack([c["ensval"], np.full((1, c["kld"]), np.nan)]))
    c["dep"] = np.append(c["dep"], 0.5)
    at = int(c["obs_off"][bad + 1])
    c["obs_idx"] = np.insert(c["obs_idx"], at, row).astype(np.int32)
    c["rdiag"] = np.insert(c["rdiag"], at, 4.0)
    c["rloc"] = np.insert(c["rloc"], at, 0.8)
    c["obs_off"] = c["obs_off"].copy()
    c["obs_off"][bad + 1:] += 1
    got, st = run(c, k, warm_run, stride)                    # (the call returns)
    assert st[bad] != 0, st
    others = np.arange(NPTS) != bad
    assert (st[others] == 0).all(), st
    # the point after it was started cold: the bits of the cold run.  The points behind that one in the run are started from
    # another solve of it than before: the same to rounding; the points of every other run: the bits of the call without the row
    assert np.ascontiguousarray(got[:, :, nxt]).tobytes() == np.ascontiguousarray(cold[:, :, nxt]).tobytes()
    assert rel(got, clean, scales(c, k), others) <= 1e-10
    pos = np.arange(NPTS)
    same_run = (pos % stride == bad % stride) if stride else (pos // 16 == bad // 16)
    assert np.ascontiguousarray(got[:, :, ~same_run]).tobytes() == np.ascontiguousarray(clean[:, :, ~same_run]).tobytes()
