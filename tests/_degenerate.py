"""Seeded generators of the degenerate inputs a radar assimilation produces: observation-space rows that are exactly zero,
exact copies or multiples of one another or exactly low rank, state variables without any spread, and point orders that put
every such class at every position of a three-point wave and of a warm-start run.  Plain numpy, no GPU: shared by
tests/golden/make_degenerate_truth.py, tests/test_degenerate_cpu.py and tests/test_gpu_degenerate.py.

Where the classes come from (the reference's own pre-processing): every member and observation without rain is set to the one
floor value MIN_RADAR_REF_DBZ + LOW_REF_SHIFT (scale/letkf/letkf_obs.f90:279-291), and a reflectivity observation passes QC
with as few as MIN_RADAR_REF_MEMBER_OBSREF = 1 members above the threshold (:384-412), so obsda%ensval(:, n) holds k - m
bit-identical entries.  The ensemble mean is removed AFTER the rows are built, so the zeros and the equalities are exact."""
import numpy as np

from _cases import DIST_ZERO_FAC_SQUARE, das_case

FLOOR = 5.0                      # MIN_RADAR_REF_DBZ + LOW_REF_SHIFT of a typical set-up: the value of every member without rain
OBS_CLASSES = ["all_zero", "zero_rows", "dup_rows", "rank1", "rank3", "floored", "one_rainy", "twin_members", "benign"]
STATE_CLASSES = ["zero_var", "zero_spread", "q_mean_zero", "twin_state"]
ERR_DBZ = 2.5                    # observation error of a reflectivity (dBZ), at the small end: cond(A) up to a few hundred


def _rain(rng, size):
    """reflectivity of raining members: floor + U(1, 40) dBZ"""
    return FLOOR + rng.uniform(1.0, 40.0, size=size)


def _center(y):
    return y - y.mean(axis=1, keepdims=True)


def twin_pairs(k):
    """the member pairs of `twin_members` / `twin_state`: two pairs where the ensemble has four members, else one"""
    return [(0, k - 1), (1, k // 2)] if k >= 5 else [(0, k - 1)]


def all_zero(n, k, rng):
    """no member rains at any local observation: every member sits on the floor (letkf_obs.f90:279-291), Y = 0 exactly.  A
    whole localisation volume of clear-air observations; with infl_update the reference's adaptive inflation then divides by
    parm(2) = 0 (common/common_letkf.f90:230-257)."""
    return _center(np.full((n, k), FLOOR))


def zero_rows(n, k, rng):
    """about 60 % of the rows clear air (exact zeros, as all_zero), the others ordinary observations"""
    y = rng.standard_normal((n, k)) * 3.0 + 20.0
    y[rng.uniform(size=n) < 0.6] = FLOOR
    if n:
        y[0] = FLOOR
    return _center(y)


def dup_rows(n, k, rng):
    """n rows drawn with repetition from n / 4 distinct ones: the same radar gate reached through several reports, or members
    that rain at neighbouring gates with the same value (rows bit-identical)"""
    base = rng.standard_normal((max(1, n // 4), k)) * 3.0
    return _center(base[rng.integers(0, base.shape[0], size=n)])


def _low_rank(n, k, rng, r):
    f = rng.uniform(0.5, 2.0, size=(n, r))
    g = rng.standard_normal((r, k)) * 3.0
    return _center(f @ g)


def rank1(n, k, rng):
    """F @ G with one ensemble pattern G: every observation sees the same pattern scaled (one rain cell, letkf_obs.f90:384-412
    with many observations of it)"""
    return _low_rank(n, k, rng, 1)


def rank3(n, k, rng):
    """F @ G with three ensemble patterns, n >> 3: an exact Lanczos breakdown after three steps"""
    return _low_rank(n, k, rng, 3)


def floored(n, k, rng):
    """per row a random 1 .. k / 3 members off the floor, the others bit-identical (letkf_obs.f90:279-291, :384-412)"""
    y = np.full((n, k), FLOOR)
    for i in range(n):
        m = rng.integers(1, max(1, k // 3) + 1)
        y[i, rng.choice(k, size=m, replace=False)] = _rain(rng, m)
    return _center(y)


def one_rainy(n, k, rng):
    """in every row the same single member off the floor (MIN_RADAR_REF_MEMBER_OBSREF = 1, letkf_obs.f90:384-412): the rows are
    multiples of e_i - 1/k, Y has rank one and k - 1 bit-identical columns"""
    y = np.full((n, k), FLOOR)
    y[:, rng.integers(0, k)] = _rain(rng, n)
    return _center(y)


def twin_members(n, k, rng):
    """two pairs of members with identical columns (members started from the same analysis that have not diverged at these
    gates)"""
    y = rng.standard_normal((n, k)) * 3.0
    for a, b in twin_pairs(k):
        y[:, b] = y[:, a]
    return _center(y)


def benign(n, k, rng):
    """the control: Gaussian rows of the same size"""
    return _center(rng.standard_normal((n, k)) * 3.0)


GENERATORS = dict(all_zero=all_zero, zero_rows=zero_rows, dup_rows=dup_rows, rank1=rank1, rank3=rank3, floored=floored,
                  one_rainy=one_rainy, twin_members=twin_members, benign=benign)


def obs_rows(cls, n, k, rng):
    y = GENERATORS[cls](n, k, rng)
    assert y.shape == (n, k)
    return y


def core_problem(cls, k, n, seed, nobs=None, infl=1.05):
    """One letkf_core problem of an observation class, laid out as _cases.core_case: hdxb (nobs, k) Fortran-ordered with poison
    behind row n, rdiag with the localisation folded in (rdiag_wloc), dep, depd."""
    rng = np.random.default_rng([seed, k, n, OBS_CLASSES.index(cls)])
    nobs = max(n, 1) if nobs is None else nobs
    y = obs_rows(cls, n, k, rng)
    rloc = np.exp(-0.5 * rng.uniform(0.0, DIST_ZERO_FAC_SQUARE, size=n))
    rdiag = ERR_DBZ ** 2 / rloc
    if cls == "dup_rows" and n >= 2:               # copies at the same rdiag (first half) and at different ones
        _, first = np.unique(y, axis=0, return_index=True)
        for f in first:
            same = np.flatnonzero((y == y[f]).all(axis=1))
            same = same[same < n // 2]
            rdiag[same] = rdiag[f]
            rloc[same] = rloc[f]
    dep = rng.standard_normal(n) * ERR_DBZ
    depd = rng.standard_normal(n) * ERR_DBZ
    hdxb = np.full((nobs, k), 1.0e30, order="F")
    hdxb[:n] = y
    pad = lambda v: np.concatenate([v, np.full(nobs - n, 1.0e30)])
    return dict(cls=cls, k=k, n=n, nobs=nobs, hdxb=hdxb, rdiag=pad(rdiag), rloc=pad(rloc), dep=pad(dep), depd=pad(depd),
                infl=float(infl), rdiag_wloc=True)


# the stored truth's case list: (class, k, n); two n per k (n < k and n > k) up to k = 64, three classes and one n at k = 100, 144
TRUTH_K = [3, 9, 16, 20, 33, 50, 64, 100, 144]
TRUTH_K100_CLASSES = ["all_zero", "one_rainy", "floored"]
TRUTH_SEED = 20261


def truth_n(k):
    return [max(1, k // 2), 3 * k] if k < 100 else [150 if k == 100 else 200]


def truth_cases():
    out = []
    for k in TRUTH_K:
        for cls in (OBS_CLASSES if k < 100 else TRUTH_K100_CLASSES):
            for n in truth_n(k):
                out.append((cls, k, n))
    return out


def truth_name(cls, k, n):
    return f"{cls}/k{k}_n{n}"


def truth_problem(cls, k, n):
    return core_problem(cls, k, n, TRUTH_SEED, nobs=n + 3)


def pack_store(d):
    """{name: float array} as three arrays (a zip member per entry would cost more than most entries hold)"""
    names = sorted(d)
    sizes = [np.asarray(d[n]).size for n in names]
    return dict(entries=np.array(names), offs=np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64),
                data=np.concatenate([np.asarray(d[n], dtype=np.float64).ravel() for n in names]))


def load_store(z):
    """the inverse of pack_store: {name: 1-D float array}"""
    offs, data = z["offs"], z["data"]
    return {str(n): data[offs[i]:offs[i + 1]] for i, n in enumerate(z["entries"])}


def tri(a):
    """the upper triangle of a symmetric k x k matrix, row by row (T and Pa are stored so: half the file)"""
    return a[np.triu_indices(a.shape[0])]


# ---------------------------------------------------------------------------------------------------------------------
# the loop body
def arrangement(nclass, positions, npts):
    """A class per point, so that every class sits at every position: `positions` is a list of integer arrays (npts), one per
    notion of position (p % 3 in a three-point wave, the index inside a warm-start run, ...).  Greedy: each point takes the
    class that its positions have seen least.  coverage() says whether every (class, position) pair occurs."""
    seen = [np.zeros((nclass, int(pos.max()) + 1), dtype=np.int64) for pos in positions]
    order = np.empty(npts, dtype=np.int64)
    for p in range(npts):
        cost = sum(s[:, pos[p]] * 1000 for s, pos in zip(seen, positions)) + sum(s.sum(axis=1) for s in seen)
        c = int(np.argmin(cost))
        order[p] = c
        for s, pos in zip(seen, positions):
            s[c, pos[p]] += 1
    return order


def coverage(order, nclass, positions):
    return all(len({(int(c), int(q)) for c, q in zip(order, pos)}) == nclass * (int(pos.max()) + 1) for pos in positions)


def run_positions(npts, run_len, warm_stride):
    """[slot in a three-point wave, position in a warm-start run] of every point, for runs of run_len points (consecutive, or
    warm_stride apart: include/letkf_amd.h warm_run, warm_stride).  Run number r holds the points (a, b), a in
    [c * run_len, (c + 1) * run_len), of column b = p % stride, r = c * stride + b; the three-points-per-wave kernel
    (letkf_trio.hip) gives a wave three consecutive runs and walks them in step, so a point's slot is r % 3 -- p % 3 only for
    runs of one point."""
    p = np.arange(npts)
    s = max(int(warm_stride), 1)
    a, b = p // s, p % s
    rid = (a // run_len) * s + b
    return [rid % 3, a % run_len]


TRIO_RUN_CAP = 4        # letkf_launch_shape.h launch_shape: on a batch too small to give every resident wave two units of three runs
#                         (P * 2 * resident waves * 4 points: tens of thousands) the kernel shortens the runs to four points
ARRANGEMENTS = {        # name -> (warm_run passed, run length it gives, stride: 0 consecutive / "nij1")
    # warm_run = 0, the library's default, means runs of UP TO 16: 16 from 64 points per wave slot of the GPU on, shorter below
    # (letkf_launch_shape.h launch_shape), one on a test-sized batch.  So the default's length is asked for by its number.
    "run16": (16, 16, 0),
    "off": (1, 1, 0),
    "stride": (4, 4, "nij1"),
    "run4": (4, 4, 0),
}


def das_degenerate(k, nv, seed, det, arr="run4", npts=None, n_lo=None, n_hi=None, state=True, grow=1.35, trio=False):
    """das_case with the observation table rebuilt from the classes -- one block of rows per class -- and the points' lists
    drawn from their class's block: point p has class OBS_CLASSES[order[p]] by arrangement(), n < k at even visits of a class
    and n > k at odd ones; the n = 0 and beta = 0 points das_case scatters are kept.  On top: a run of four consecutive points
    with bit-identical lists (the warm start is already the solution), a degenerate point between two benign ones and the
    reverse.  state: the state classes applied (apply_state).  Returns the case with `order`, `warm_run`, `warm_stride`,
    `cls_of_point` (-1: n = 0) and `state_cls`.  trio: the case is for the three-points-per-wave kernel, whose runs are at most
    TRIO_RUN_CAP points on such a batch whatever warm_run asks."""
    warm_run, run_len, stride = ARRANGEMENTS[arr]
    if trio:
        run_len = min(run_len, TRIO_RUN_CAP)
    nc = len(OBS_CLASSES)
    nij1 = 0
    if stride == "nij1":
        nij1 = 15
        npts = nij1 * run_len * 2
    npts = npts or int(nc * max(run_len, 3) * grow) + 24
    npts += (-npts) % 3
    n_lo = n_lo or max(2, k // 2)
    n_hi = n_hi or (3 * k if k <= 64 else k + k // 4)
    block = n_hi + 8
    c = das_case(k=k, nv=nv, npts=npts, nobs_tot=block * nc, n_mean=n_lo, seed=seed, det_run=det, infl0=1.07)
    rng = np.random.default_rng([seed, k, 77])
    # hand-placed neighbourhoods at the end of the batch: degenerate between benign and the reverse, then identical points
    B, Z, O = OBS_CLASSES.index("benign"), OBS_CLASSES.index("all_zero"), OBS_CLASSES.index("one_rainy")
    tail = [] if nij1 else [B, Z, B, O, B, O, O, B, B, B, B]
    nfree = npts - len(tail)
    keep = np.diff(c["obs_off"]) == 0                     # das_case's n = 0 points stay
    keep[nfree:] = False
    c["beta"][nfree:] = 1.0
    # every class at every position, counted over the points that are solved (n > 0, beta != 0)
    solved = np.flatnonzero(~keep & (c["beta"] != 0.0) & (np.arange(npts) < nfree))
    pos = [q[solved] for q in run_positions(npts, run_len, nij1)]
    order = np.arange(npts) % nc
    order[solved] = arrangement(nc, pos, solved.size)
    if not coverage(order[solved], nc, pos):              # too few solved points at some position: a larger batch
        assert grow < 3.0, "arrangement does not cover every (class, position)"
        return das_degenerate(k, nv, seed, det, arr, None, n_lo, n_hi, state, grow * 1.25, trio)
    order[nfree:] = tail
    # the observation table
    ens = c["ensval"]
    for ci, cls in enumerate(OBS_CLASSES):
        ens[ci * block:(ci + 1) * block, :k] = obs_rows(cls, block, k, rng)
    c["dep"] = rng.standard_normal(block * nc) * ERR_DBZ
    visits = np.zeros(nc, dtype=np.int64)
    counts = np.zeros(npts, dtype=np.int64)
    lists = []
    for p in range(npts):
        if keep[p]:
            lists.append(np.zeros(0, dtype=np.int32))
            continue
        ci = int(order[p])
        n = (n_lo, n_hi)[visits[ci] % 2] + int(rng.integers(0, 4))
        visits[ci] += 1
        idx = ci * block + rng.choice(block, size=n, replace=False)
        if OBS_CLASSES[ci] in ("benign", "zero_rows") and visits[ci] % 3 == 0:   # a mixed list: a few rows of the next class
            nx = (ci + 1) % nc
            idx[:n // 3] = nx * block + rng.choice(block, size=n // 3, replace=False)
        lists.append(idx.astype(np.int32))
    if not nij1:                                          # four bit-identical consecutive points
        for p in range(npts - 3, npts):
            lists[p] = lists[npts - 4].copy()
            order[p] = order[npts - 4]
    counts[:] = [len(l) for l in lists]
    off = np.zeros(npts + 1, dtype=np.int64)
    np.cumsum(counts, out=off[1:])
    c["obs_off"], c["obs_idx"] = off, np.concatenate(lists).astype(np.int32)
    rloc = np.exp(-0.5 * rng.uniform(0.0, DIST_ZERO_FAC_SQUARE, size=int(off[-1])))
    if not nij1:                                          # ... their weights too
        a, b = off[npts - 4], off[npts - 3]
        for p in range(npts - 3, npts):
            rloc[off[p]:off[p + 1]] = rloc[a:b]
    c["rloc"], c["rdiag"] = rloc, ERR_DBZ ** 2 / rloc
    c["order"], c["warm_run"], c["warm_stride"], c["run_len"] = order, warm_run, nij1, run_len
    c["cls_of_point"] = np.where(counts > 0, order, -1)
    c["infl"] = c["infl"] * (1.0 + 0.02 * np.arange(c["infl"].size) / c["infl"].size)
    c["state_cls"] = apply_state(c, rng) if state else {}
    return c


def apply_state(c, rng):
    """The state classes on das_case's state, in place.  Hydrometeor variables are identically zero in every member over most of
    the grid: the else branch of weight_RTPS (scale/letkf/letkf_tools.f90:1990-1999) and the 0 / 0 of the Q_SPRD_MAX clamp
    (:500-513).
      zero_var     perturbations, mean and deterministic member exactly 0: the last two variables at two thirds of the points,
                   iv_q_first (the clamped variable) at every fifth point
      zero_spread  perturbations 0, mean != 0 (the deterministic member keeps its own value): variable 2 at every fourth
                   point, the variable before the zero_var pair at every other point
      q_mean_zero  iv_q_first's mean exactly 0 under non-zero perturbations, at points that have observations, beta != 0 and a
                   list that is not all zeros.  Only there is the reference's own answer decided by its inputs: the clamp
                   divides by the ANALYSIS mean, which at a point without increment is the rounding noise of the perturbations'
                   sum, of either sign.
    Returns {class: bool (nv, npts)}."""
    k, nv, npts, nens = c["k"], c["nv"], c["npts"], c["nens"]
    x = c["gues"].reshape(nv, nens, npts)
    p = np.arange(npts)
    zv = np.zeros((nv, npts), bool)
    zs = np.zeros((nv, npts), bool)
    qz = np.zeros((nv, npts), bool)
    zv[nv - 1, p % 3 != 0] = True
    zv[nv - 2, p % 3 != 1] = True
    zv[5, p % 5 == 2] = True
    zs[2, p % 4 == 1] = True
    zs[nv - 3, p % 2 == 0] = True
    live = (c["cls_of_point"] >= 0) & ~y_is_zero(c) & (c["beta"] != 0.0)
    qz[5, live & (p % 5 == 0) & ~zv[5]] = True
    for v in range(nv):
        x[v][:, zv[v]] = 0.0
        x[v][:k, zs[v]] = 0.0
        x[v][k, qz[v]] = 0.0
    return dict(zero_var=zv, zero_spread=zs, q_mean_zero=qz)


def twin_state(c, ens_too=True):
    """two members identical in every variable (and, ens_too, in every row of the observation table), the mean removed again
    afterwards so that the twins stay bit-identical; in place"""
    k, nv, npts, nens = c["k"], c["nv"], c["npts"], c["nens"]
    x = c["gues"].reshape(nv, nens, npts)
    a, b = twin_pairs(k)[0]
    x[:, b] = x[:, a]
    x[:, :k] -= x[:, :k].mean(axis=1, keepdims=True)
    if ens_too:
        e = c["ensval"]
        e[:, b] = e[:, a]
        e[:, :k] -= e[:, :k].mean(axis=1, keepdims=True)
    return a, b


# ---------------------------------------------------------------------------------------------------------------------
# comparing with the stored answers
def kk_error(got, store, nm, key):
    """max-norm relative error of a k x k output against its stored answer: whole (upper triangle) where it is stored whole,
    else through the probes and the diagonal in the norm of test_oracle_golden.check_against_golden"""
    from _cases import probes
    k = got.shape[0]
    if f"{nm}/{key}" in store:
        want = store[f"{nm}/{key}"]
        return float(np.abs(tri(got) - want).max() / np.abs(want).max())
    scale = float(store[f"{nm}/{key}_absmax"][0])
    e1 = np.abs(got @ probes(k) - store[f"{nm}/{key}_probe"].reshape(k, 4)).max() / (scale * np.sqrt(k))
    e2 = np.abs(np.diag(got) - store[f"{nm}/{key}_diag"]).max() / scale
    return float(max(e1, e2))


def vec_error(got, want):
    """w-bar: relative to max(1, |w|), as tests/test_gpu_core_batch.py"""
    return float(np.abs(got - want).max() / max(1.0, np.abs(want).max()))


def core_errors(r, store, nm):
    """(T, Pa, w, w_d) errors of one letkf_core answer r (trans, pao column-major k x k; both symmetric)"""
    return (kk_error(r["trans"], store, nm, "trans"), kk_error(r["pao"], store, nm, "pao"),
            vec_error(r["transm"], store[nm + "/transm"]), vec_error(r["transmd"], store[nm + "/transmd"]))


def inputs_sha(c):
    from _cases import array_sha
    n = c["n"]
    return array_sha(c["hdxb"][:n], c["rdiag"][:n], c["rloc"][:n], c["dep"][:n], c["depd"][:n], np.array([c["infl"]]))


# ---------------------------------------------------------------------------------------------------------------------
# metamorphic relations of the loop body: pairs of cases whose analyses are the same (up to a permutation of the members)
META_CFG = dict(relax_alpha_spread=0.9)        # RTPS; no adaptive inflation, whose estimate does count the rows of a list


def _lists(c):
    off = c["obs_off"]
    return [(c["obs_idx"][off[p]:off[p + 1]], c["rdiag"][off[p]:off[p + 1]], c["rloc"][off[p]:off[p + 1]])
            for p in range(c["npts"])]


def _with_lists(c, lists):
    d = dict(c)
    off = np.zeros(c["npts"] + 1, dtype=np.int64)
    np.cumsum([len(l[0]) for l in lists], out=off[1:])
    d["obs_off"] = off
    d["obs_idx"] = np.concatenate([l[0] for l in lists]).astype(np.int32)
    d["rdiag"] = np.concatenate([l[1] for l in lists]).astype(np.float64)
    d["rloc"] = np.concatenate([l[2] for l in lists]).astype(np.float64)
    return d


def meta_pairs(c, seed=5):
    """[(name, case a, case b, perm)]: the analysis of b is the analysis of a, with the members of b in the order perm of a's
    (perm None: the same order)."""
    k, nv, nens, npts = c["k"], c["nv"], c["nens"], c["npts"]
    rng = np.random.default_rng(seed)
    ens = c["ensval"]
    zero = ~ens[:, :k].any(axis=1)
    out = []
    # deleting the exact-zero rows of a list changes nothing (they add nothing to Y^T R^-1 Y nor to Y^T R^-1 d)
    dropped = [tuple(v[~zero[i]] for v in (i, rd, rl)) for i, rd, rl in _lists(c)]
    assert sum(len(l[0]) for l in dropped) < c["obs_idx"].size
    out.append(("drop_zero_rows", c, _with_lists(c, dropped), None))
    # m copies of a row at rdiag are one copy at rdiag / m
    m = 3
    out.append(("copies", c, _with_lists(c, [(np.repeat(i, m), np.repeat(rd * m, m), np.repeat(rl, m))
                                             for i, rd, rl in _lists(c)]), None))
    # the order of a local list does not matter
    perms = [rng.permutation(len(i)) for i, _, _ in _lists(c)]
    out.append(("permute_lists", c, _with_lists(c, [(i[q], rd[q], rl[q]) for (i, rd, rl), q in zip(_lists(c), perms)]), None))
    # permuting the members permutes the analysis members
    perm = rng.permutation(k)
    d = dict(c)
    d["ensval"] = ens.copy()
    d["ensval"][:, :k] = ens[:, perm]
    x = c["gues"].reshape(nv, nens, npts).copy()
    x[:, :k] = x[:, perm]
    d["gues"] = x.reshape(-1)
    out.append(("permute_members", c, d, perm))
    return out


def meta_error(c, anal_a, anal_b, perm, det):
    """worst |a - b| / scale over the variables (scale as the loop body's bar: max(|mean|, |perturbation|) per variable)"""
    k, nv, nens, npts = c["k"], c["nv"], c["nens"], c["npts"]
    a, b = anal_a.reshape(nv, nens, npts), anal_b.reshape(nv, nens, npts)
    x = c["gues"].reshape(nv, nens, npts)
    worst = 0.0
    for v in range(nv):
        scale = max(np.abs(x[v, k]).max(), np.abs(x[v, :k]).max())
        ea = a[v, :k] if perm is None else a[v, perm]
        err = np.abs(ea - b[v, :k]).max()
        if det:
            err = max(err, np.abs(a[v, k + 1] - b[v, k + 1]).max())
        assert np.isfinite(err), v
        worst = max(worst, err / scale if scale > 0 else float(err > 0))
    return worst


def twin_error(c, anal, pair):
    """worst |member a - member b| / scale of a case whose members a and b are twins (twin_state)"""
    k, nv, nens, npts = c["k"], c["nv"], c["nens"], c["npts"]
    a = anal.reshape(nv, nens, npts)
    x = c["gues"].reshape(nv, nens, npts)
    worst = 0.0
    for v in range(nv):
        scale = max(np.abs(x[v, k]).max(), np.abs(x[v, :k]).max())
        err = np.abs(a[v, pair[0]] - a[v, pair[1]]).max()
        assert np.isfinite(err), v
        worst = max(worst, err / scale)
    return worst


def y_is_zero(c):
    """the points of a loop-body case whose local rows are all exactly zero (n > 0): the reference's adaptive inflation gives NaN
    there (common/common_letkf.f90:230-257)"""
    zero = ~c["ensval"][:, :c["k"]].any(axis=1)
    off = c["obs_off"]
    return np.array([off[p + 1] > off[p] and zero[c["obs_idx"][off[p]:off[p + 1]]].all() for p in range(c["npts"])])
