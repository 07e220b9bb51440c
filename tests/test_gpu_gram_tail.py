"""GPU parity of the one-wave kernel's Gram where its tile loop no longer selects per step (csrc/letkf_wave_dev.h TRIM, r13): a
step past the end of a batch is fetched unclamped from padding entries the stage phase leaves behind the batch, the narrow member
block of KR = 50 / 20 goes into the sums unmasked and is cleaned up once per point, and the row offsets of the full blocks are
constants.  What can go wrong is a value that must not be read reaching a sum, so everything the call must not read is NaN:
  rows:   every row of the observation table that no local list names (row 0 is named: the padding of the loop as it was reads it,
          and the parent twin below must get through), and every slot of a row behind the members -- kld = k + 3 with NaN in the
          slots the call does not use (slot k too without a deterministic member); then the same case again with the tightest kld
          the ABI allows (k + 1, k without det_run) and the table's LAST row in every other list: a lane that reads past its row
          there reads past the table.  The two runs must agree byte for byte.
  k:      50, 49, 20, 19, 17 -- the narrow block with 2, 1, 4, 3, 1 members -- and 48, 33, 62, 51, whose last block feeds the
          matrix cores and keeps its select.
  n:      1, 3, 4, 5, 8, 11, 12, 13, 255, 256, 257, 260, 2 k + 1: every n mod 4, every step count mod 3 (the steps in flight),
          and a second batch of one observation behind a full first one (stale staging entries behind its end).
  runs:   cold, and warm runs of 2 and 5 points; RTPS and RTPP; with det_run and adaptive inflation (trace, r, r_det) and without.
  routes: lists through letkf_das_points_dev; for k = 50 and 49 also the fused search and the list-free route of
          letkf_das_columns_dev, which feed the same loop from their own staging code, on a column case poisoned the same way.
Against the oracle at 1e-10 * max(|mean|, |x'|) per variable, 5e-13 at the points with 1 <= n < k (tests/test_gpu_sparse_margin.py
pins them); status as the oracle's.  Where a parent twin of the library lies beside it (lib/libletkf_amd_ref.so, tools/
ab_build_ref.sh) every output -- analysis, status, sweeps, inflation, RTPS factor -- must be the twin's byte for byte."""
import functools
import hashlib
import json
import os
import subprocess
import sys
from unittest import mock

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
if __name__ == "__main__":                                             # (the twin's child process: see the last test)
    sys.path.insert(0, HERE)
    sys.path.insert(0, ROOT)

import _colspace
from _argspace import members
import _oracle
import _search
from _cases import DIST_ZERO_FAC_SQUARE, das_case

pytestmark = pytest.mark.gpu

NV = 11
NPTS = 26
NOBS = 300
NBAD = 20                                    # rows that no list names
K_NARROW = [50, 49, 20, 19, 17]
K_SELECT = [48, 33, 62, 51]
KS = K_NARROW + K_SELECT
CONFIGS = ["plain", "det_adaptive"]
WARM = [("cold", 1), ("run2", 2), ("run5", 5)]
TWIN = os.path.join(ROOT, "scale-letkf_amd", "lib", "libletkf_amd_ref.so")


def config(k, name):
    """(adaptive, det_run, relaxation): RTPS and RTPP alternate with k, and each k gets the other one in its second config"""
    kinds = ("rtps", "rtpp") if KS.index(k) % 2 == 0 else ("rtpp", "rtps")
    return (False, False, kinds[0]) if name == "plain" else (True, True, kinds[1])


def relax(kind):
    return dict(relax_alpha=0.7 if kind == "rtpp" else 0.0, relax_alpha_spread=0.95 if kind == "rtps" else 0.0)


def lengths(k):
    ns = [1, 3, 4, 5, 8, 11, 12, 13, 255, 256, 257, 260, 2 * k + 1]
    return np.array([ns[p] if p < 13 else ns[(5 * p) % 13] for p in range(NPTS)], dtype=np.int64)   # (other neighbours the second time)


@functools.lru_cache(maxsize=None)
def list_case(k, det_run):
    c = das_case(k=k, nv=NV, npts=NPTS, nobs_tot=NOBS, n_mean=1, seed=13000 + k, det_run=det_run, vary_n=False, infl0=1.05)
    rng = np.random.default_rng(13500 + k)
    last = NOBS - 1
    named = np.concatenate(([0], 1 + rng.choice(NOBS - 2, NOBS - 2 - NBAD, replace=False), [last]))
    want = lengths(k)
    off = np.zeros(NPTS + 1, dtype=np.int64)
    np.cumsum(want, out=off[1:])
    idx = np.empty(off[-1], dtype=np.int32)
    for p in range(NPTS):
        rows = rng.choice(named, size=want[p], replace=False)
        if p % 2 and last not in rows:
            rows[rng.integers(want[p])] = last
        idx[off[p]:off[p + 1]] = rows
    rloc = np.exp(-0.5 * rng.uniform(0.0, DIST_ZERO_FAC_SQUARE, size=idx.size))
    err = rng.choice([1.0, 3.0, 5.0], size=NOBS)
    c.update(obs_off=off, obs_idx=idx, rloc=rloc, rdiag=err[idx] ** 2 / rloc)
    c["beta"][:] = 1.0
    c["unnamed"] = np.setdiff1d(np.arange(NOBS), idx)
    assert 0 in idx and last in idx and c["unnamed"].size >= NBAD
    return c


def poisoned_table(ens, k, kld, det_run, unnamed):
    """the table with leading dimension kld: members 0 .. k - 1 (and slot k with det_run) of the named rows, NaN everywhere else"""
    t = np.full((ens.shape[0], kld), np.nan)
    used = k + int(det_run)
    t[:, :used] = ens[:, :used]
    t[unnamed] = np.nan
    return np.ascontiguousarray(t)


def klds(k, det_run):
    return [("wide", k + 3), ("tight", k + int(det_run))]


@functools.lru_cache(maxsize=None)
def list_oracle(k, cfg):
    adaptive, det_run, kind = config(k, cfg)
    c = list_case(k, det_run)
    prm = _oracle.DasParams(k=k, nv=NV, det_run=int(det_run), infl_adaptive=int(adaptive), relax_to_inflated_prior=0, q_update_top=0.0,
                            q_sprd_max=0.0, iv_p=4, iv_q_first=5, iv_q_last=10, nthreads=4, **relax(kind))
    ref = _oracle.das_points(prm, c["obs_off"], c["obs_idx"], c["rdiag"], c["rloc"], c["ensval"], c["dep"], c["beta"], c["infl"],
                             c["gues"], c["sp"], c["sm"], c["sv"], want_rtps=True)
    assert ref["rc"] == 0
    return (ref["anal"].reshape(NV, c["nens"], NPTS), ref["status"], ref["infl"].reshape(NV, NPTS), ref["rtps"].reshape(NV, NPTS))


def run_lists(k, cfg, kld, warm_run):
    import torch
    from _gpu import ctx, dev
    adaptive, det_run, kind = config(k, cfg)
    c = list_case(k, det_run)
    tab = poisoned_table(c["ensval"].reshape(NOBS, c["kld"]), k, kld, det_run, c["unnamed"])
    anal = torch.full((c["gues"].size,), float("nan"), dtype=torch.float64, device="cuda")
    status = torch.full((NPTS,), -1, dtype=torch.int32, device="cuda")
    nsweep = torch.full((NPTS,), -1, dtype=torch.int32, device="cuda")
    infl = dev(c["infl"].copy())
    rtps = torch.full((NV * NPTS,), float("nan"), dtype=torch.float64, device="cuda")
    ctx().set_option(ctx().OPT_SMALL_K_TRIO, 0)    # (k <= 20: the one-wave kernel, not three points per wave)
    try:
        ctx().das_points(k, NV, dev(c["obs_off"]), dev(c["obs_idx"]), dev(c["rdiag"]), dev(c["rloc"]), dev(tab), kld, dev(c["dep"]),
                         infl, dev(c["gues"]), anal, c["sp"], c["sm"], c["sv"], beta=dev(c["beta"]), det_run=det_run,
                         infl_adaptive=adaptive, status=status, nsweep=nsweep, rtps_infl_out=rtps, warm_run=warm_run, **relax(kind))
        torch.cuda.synchronize()
    finally:
        ctx().set_option(ctx().OPT_SMALL_K_TRIO, 1)
    assert ctx().last_path().startswith("letkf_wave_kernel"), ctx().last_path()
    a = anal.cpu().numpy().reshape(NV, c["nens"], NPTS)
    mem = members(k, det_run)
    return dict(anal=np.ascontiguousarray(a[:, mem]), status=status.cpu().numpy(), nsweep=nsweep.cpu().numpy(),
                infl=infl.cpu().numpy().reshape(NV, NPTS), rtps=rtps.cpu().numpy().reshape(NV, NPTS))


def scales(gues, k, nens, npts):
    x = gues.reshape(NV, nens, npts)
    return np.array([max(np.abs(x[v, k]).max(), np.abs(x[v, :k]).max()) for v in range(NV)])


def worst(got, exp, sc, pts):
    """max over the variables of max |got - exp| / scale, over the points `pts`"""
    return max(float(np.abs(got[v][:, pts] - exp[v][:, pts]).max()) / sc[v] for v in range(NV)) if pts.any() else 0.0


def same(a, b):
    return all(a[f].tobytes() == b[f].tobytes() for f in a)


@pytest.mark.parametrize("cfg", CONFIGS)
@pytest.mark.parametrize("k", KS)
def test_lists_with_everything_unread_poisoned(k, cfg):
    adaptive, det_run, kind = config(k, cfg)
    c = list_case(k, det_run)
    exp_a, exp_st, exp_i, exp_r = list_oracle(k, cfg)
    exp = exp_a[:, members(k, det_run)]
    sc = scales(c["gues"], k, c["nens"], NPTS)
    n = np.diff(c["obs_off"])
    few = (n >= 1) & (n < k)                                          # the 5e-13 points
    assert (exp_st == 0).all() and few.any() and (~few).any()
    for name, warm_run in WARM:
        res = {kn: run_lists(k, cfg, kld, warm_run) for kn, kld in klds(k, det_run)}
        got = res["wide"]
        e_few, e_rest = worst(got["anal"], exp, sc, few), worst(got["anal"], exp, sc, ~few)
        e_infl = float(np.abs(got["infl"] - exp_i).max() / np.abs(exp_i).max())
        e_rtps = float(np.abs(got["rtps"] - exp_r).max())             # (factors of order 1)
        print(f"k={k} {cfg} {kind} {name}: err/scale n<k {e_few:.3e} others {e_rest:.3e} infl {e_infl:.3e} rtps {e_rtps:.3e} "
              f"sweeps {got['nsweep'].min()}..{got['nsweep'].max()}")
        assert np.array_equal(got["status"], exp_st), (name, got["status"])
        assert (got["nsweep"] > 0).all(), (name, got["nsweep"])
        assert np.isfinite(got["anal"]).all(), name
        assert e_few <= 5e-13 and e_rest <= 1e-10, (name, e_few, e_rest)
        assert e_infl <= 1e-10 and e_rtps <= 1e-10, (name, e_infl, e_rtps)
        assert same(got, res["tight"]), name                          # nothing behind the members of a row reaches a sum


# ---- the routes that stage their own entries: the fused search and the column survivors

SEARCH_KS = [50, 49]
SEARCH_CFG = dict(infl_adaptive=1, relax_alpha_spread=0.95)
NIJ1, NLEV = 12, 3


@functools.lru_cache(maxsize=None)
def search_case(k):
    """tests/_colspace.py's column case at k (its routes name k = 50 only), the oracle's lists and its answer"""
    row = (k, NV, "free", {"surv": 1}, "all", [_colspace.FREE, "NW=1"], [])

    def dense(seed, nobs_per_ctype, **kw):                             # 3.5 times the observations: lists of 150 to 350
        return _search.build_case(seed, nobs_per_ctype=tuple(7 * n // 2 for n in nobs_per_ctype), **kw)
    with mock.patch.dict(_colspace.COL_ROUTES, {"gram_tail": row}), mock.patch.object(_colspace, "build_case", dense):
        c = _colspace.col_case("gram_tail", 13700 + k, det=True, nij1=NIJ1, nlev=NLEV)
    c["beta"][:] = 1.0
    lists = _colspace.oracle_lists(c)
    ref = _colspace.oracle_class(c, SEARCH_CFG, 0, lists, c["beta"], c["infl"])
    c["unnamed"] = np.setdiff1d(np.arange(1, c["tc"]["nobs"]), lists[1])   # (row 0 stays: the module's docstring)
    return c, lists, ref


def run_search(k, route, kld):
    import torch
    from _gpu import ctx, dev
    from _search import device_struct
    c, lists, _ = search_case(k)
    npts, nens = c["npts"], c["nens"]
    tab = poisoned_table(c["ensval"], k, kld, True, c["unnamed"])
    t, keep = device_struct(c["tc"], "cuda")
    anal = torch.full((c["gues"].size,), float("nan"), dtype=torch.float64, device="cuda")
    status = torch.full((npts,), -1, dtype=torch.int32, device="cuda")
    nsweep = torch.full((npts,), -1, dtype=torch.int32, device="cuda")
    nobs = torch.full((npts,), -1, dtype=torch.int32, device="cuda")
    infl = dev(c["infl"].copy())
    rtps = torch.full((NV * npts,), float("nan"), dtype=torch.float64, device="cuda")
    kw = dict(beta=dev(c["beta"]), det_run=True, infl_adaptive=True, relax_alpha_spread=0.95, status=status, nsweep=nsweep,
              rtps_infl_out=rtps, nobs_out=nobs)
    cx = ctx()
    if route == "fused":
        pts = [dev(x) for x in (np.tile(c["rig"], NLEV), np.tile(c["rjg"], NLEV), c["rlev"], c["rz"])]
        cx.das_points(k, NV, None, None, None, None, dev(tab), kld, dev(c["dep"]), infl, dev(c["gues"]), anal, 1, npts, npts * nens,
                      fused=(t, *pts), warm_run=5, **kw)
        torch.cuda.synchronize()
    else:
        cx.set_option(cx.OPT_COLUMN_SURVIVORS, 1)
        try:
            cx.das_columns(k, NV, t, NIJ1, NLEV, dev(c["rig"]), dev(c["rjg"]), dev(c["rlev"]), dev(c["rz"]), dev(tab), kld,
                           dev(c["dep"]), infl, dev(c["gues"]), anal, 1, npts, npts * nens, list_bytes=1 << 30, **kw)
            torch.cuda.synchronize()
        finally:
            cx.set_option(cx.OPT_COLUMN_SURVIVORS, 2)
    assert "FUSED" in cx.last_path() and "NW=1" in cx.last_path(), cx.last_path()
    a = anal.cpu().numpy().reshape(NV, nens, npts)
    return dict(anal=np.ascontiguousarray(a[:, members(k, True)]), status=status.cpu().numpy(), nsweep=nsweep.cpu().numpy(),
                nobs=nobs.cpu().numpy(), infl=infl.cpu().numpy(), rtps=rtps.cpu().numpy())


@pytest.mark.parametrize("route", ["fused", "columns"])
@pytest.mark.parametrize("k", SEARCH_KS)
def test_search_routes_with_everything_unread_poisoned(k, route):
    c, lists, ref = search_case(k)
    npts, nens = c["npts"], c["nens"]
    n = np.diff(lists[0])
    ok = ~lists[4]                                                     # (tied sort keys: none without MAX_NOBS_PER_GRID)
    assert ok.all() and c["unnamed"].size > 0
    # the staging buffer is flushed at more than 192 entries and holds 256: lists on both sides, and of every length mod 4
    assert n.max() > 256 and n.min() < 192 and len(set((n % 4).tolist())) == 4, n
    exp = ref["anal"].reshape(NV, nens, npts)[:, members(k, True)]
    sc = scales(c["gues"], k, nens, npts)
    few = (n >= 1) & (n < k)
    res = {kn: run_search(k, route, kld) for kn, kld in klds(k, True)}
    got = res["wide"]
    e_few, e_rest = worst(got["anal"], exp, sc, few), worst(got["anal"], exp, sc, ~few)
    e_infl = float(np.abs(got["infl"] - ref["infl"]).max() / np.abs(ref["infl"]).max())
    e_rtps = float(np.abs(got["rtps"] - ref["rtps"]).max())
    print(f"k={k} {route}: n {n.min()}..{n.max()} err/scale n<k {e_few:.3e} others {e_rest:.3e} infl {e_infl:.3e} rtps {e_rtps:.3e}")
    assert np.array_equal(got["nobs"], n)
    assert np.array_equal(got["status"], ref["status"]), got["status"]
    assert np.isfinite(got["anal"]).all()
    assert e_few <= 5e-13 and e_rest <= 1e-10, (e_few, e_rest)
    assert e_infl <= 1e-10 and e_rtps <= 1e-10, (e_infl, e_rtps)
    assert same(got, res["tight"])


# ---- the parent twin

def digests():
    """{case: SHA-256 of every output} of every run above, with the library this process loaded"""
    out = {}

    def put(tag, r):
        h = hashlib.sha256()
        for f in sorted(r):
            h.update(r[f].tobytes())
        out[tag] = h.hexdigest()
    for k in KS:
        for cfg in CONFIGS:
            for kn, kld in klds(k, config(k, cfg)[1]):
                for name, warm_run in WARM:
                    put(f"lists k={k} {cfg} {kn} {name}", run_lists(k, cfg, kld, warm_run))
    for k in SEARCH_KS:
        for route in ("fused", "columns"):
            for kn, kld in klds(k, True):
                put(f"{route} k={k} {kn}", run_search(k, route, kld))
    return out


def test_every_output_is_the_parent_twins():
    if not os.path.exists(TWIN):
        pytest.skip("no parent twin beside the library (tools/ab_build_ref.sh builds one)")
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=dict(os.environ, LETKF_AMD_LIB=TWIN), capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    theirs = json.loads(r.stdout.strip().splitlines()[-1])
    ours = digests()
    assert sorted(ours) == sorted(theirs)
    differ = [tag for tag in ours if ours[tag] != theirs[tag]]
    print(f"{len(ours)} runs compared with the parent twin, {len(differ)} differ")
    assert not differ, differ


if __name__ == "__main__":
    from __graft_entry__ import load_package
    assert load_package().LIB_PATH == TWIN, load_package().LIB_PATH
    print(json.dumps(digests()))
