"""Every route that evaluates obs_local's shared device functions (csrc/letkf_search_dev.h: cell_rect, row_span,
horizontal_nd, vertical_obs_coord, the survivor entry) on the six-type table of tests/_search_types.py, whose types reach every
branch of them: a merged pair with height and ln(dat) localisation, the rain-base mode, no vertical localisation,
varloc = 1e-300 and varloc < tiny (skipped).  1500 more rows of type 0 lie within two cells of column 0, in a thin layer: at the
levels within its vertical cut-off that column accepts more of the merged group than the per-point kernel's candidate cache
(512) and the limited column kernel's survivor buffer (576) hold, so the multi-sweep fall-backs run beside the LDS paths.

  letkf_obs_search_dev            no limit: the oracle's lists, entry for entry (weights to rtol 1e-13);
                                  with a limit: the oracle's selection (same rows, weights to rtol 1e-13), criteria 1 and 3;
  letkf_obs_search_columns_dev    with a limit, by the LDS kernel, by rings (criterion 1) and by rings of the general key
                                  (criterion 3): the per-point kernel's rows and weights, to the last bit;
  letkf_das_columns_dev           the list-free route (survivor kernel + the loop body's column-survivor mode) against the lists:
                                  nobs_out and the analysis bit for bit;
  letkf_das_points_fused_dev      against search-then-solve, as tests/test_gpu_fused.py.

Shapes: 5 columns x 2 levels and 1 column x 65 levels (a level loop that crosses 64).  The limits (100 for the merged group, 5
for the rain-base type, 12 for the 1e-300 type, none for the type without vertical localisation) were chosen with the oracle's
unlimited counts: at 5 x 2 the groups' counts are 43 .. 1580, 0 .. 14 and 12 .. 27, at 1 x 65 they are 58 .. 1584, 0 .. 18 and
11 .. 30, so every case has (point, group) pairs at the limit (18 and 156) and below it (9 and 19).  The draws are continuous:
the oracle reports no selection between equal keys, which every limited case asserts for all its points."""
import functools

import numpy as np
import pytest
import torch

import _search
from _search_types import I_ORG, J_ORG, NLAT, NLON, types_case

pytestmark = pytest.mark.gpu

SHAPES = [(5, 2), (1, 65)]
NOBS = (500, 400, 300, 200, 400, 200)
DENSE = (1500, 20.0, 20.0, 2.0, 1000.0, 1500.0)      # rows, centre, radius (cells), layer (m) of the cluster of type 0
MAX_NOBS = (100, 0, 5, 0, 12, 0)                     # per type; the master's rules a group
AT_LIMIT = {(5, 2): 15, (1, 65): 150}                # fewer (point, group) pairs at / below the limit than the oracle counted
BELOW_LIMIT = {(5, 2): 5, (1, 65): 15}
CACHE_CAP = 512                                      # kCacheCap of letkf_search.hip


@functools.lru_cache(maxsize=None)
def setup(nij1, nlev):
    rng = np.random.default_rng(100 * nij1 + nlev)
    case = types_case(rng, NOBS, dense=DENSE)
    rig = I_ORG + rng.uniform(0.5, NLON - 0.5, nij1)
    rjg = J_ORG + rng.uniform(0.5, NLAT - 0.5, nij1)
    rig[0], rjg[0] = I_ORG + 20.3, J_ORG + 19.6      # column 0 stands in the cluster
    rlev = rng.uniform(2.5e4, 1.0e5, nij1 * nlev)
    rz = rng.uniform(0.0, 12000.0, nij1 * nlev)
    return case, rig, rjg, rlev, rz


def table(nij1, nlev, limited, criterion=1):
    """The shape's case with its limits and criterion set (a copy: the cached case stays as it was built)."""
    case, *_ = setup(nij1, nlev)
    case = dict(case, arr=dict(case["arr"]), scal=dict(case["scal"], criterion=criterion))
    if limited:
        case["arr"]["max_nobs"] = np.array(MAX_NOBS, dtype=np.int32)
    return case


@functools.lru_cache(maxsize=None)
def oracle(nij1, nlev, limited, criterion=1):
    """The oracle's obs_local for every point of the shape: (off, idx, rdiag, rloc); no selection between equal keys."""
    _, rig, rjg, rlev, rz = setup(nij1, nlev)
    h, alive = _search.host_struct(table(nij1, nlev, limited, criterion))
    off, idx, rd, rl, tied = _search.oracle_csr(h, np.tile(rig, nlev), np.tile(rjg, nlev), rlev, rz)
    assert not tied.any()
    return off, idx, rd, rl


def group_counts(case, off, idx):
    """[npts, ngroup] entries of every point's list per group."""
    which = np.searchsorted(case["ctype_rows"], idx, side="right") - 1
    group_of = np.zeros(case["scal"]["nctype"], dtype=np.int64)
    for g, members in enumerate(case["groups"]):
        group_of[members] = g
    out = np.zeros((len(off) - 1, len(case["groups"])), dtype=np.int64)
    np.add.at(out, (np.repeat(np.arange(len(off) - 1), np.diff(off)), group_of[which]), 1)
    return out


def assert_limit_binds_and_not(case, shape, off, idx):
    nmax = np.array([MAX_NOBS[g[0]] for g in case["groups"]])
    cnt = group_counts(case, off, idx)[:, nmax > 0]
    assert (cnt <= nmax[nmax > 0]).all()
    at, below = int((cnt == nmax[nmax > 0]).sum()), int(((cnt > 0) & (cnt < nmax[nmax > 0])).sum())
    print(f"{shape}: {at} (point, group) pairs at the limit, {below} below it")
    assert at > AT_LIMIT[shape] and below > BELOW_LIMIT[shape]


def point_search(case, nij1, nlev):
    from _gpu import ctx, dev
    _, rig, rjg, rlev, rz = setup(nij1, nlev)
    t, keep = _search.device_struct(case, "cuda")
    out = ctx().obs_search(t, dev(np.tile(rig, nlev)), dev(np.tile(rjg, nlev)), dev(rlev), dev(rz))
    torch.cuda.synchronize()
    return [x.cpu().numpy() for x in out]


@pytest.mark.parametrize("nij1,nlev", SHAPES)
def test_point_search_without_a_limit_gives_the_oracle_lists(nij1, nlev):
    case = table(nij1, nlev, False)
    off, idx, rd, rl = oracle(nij1, nlev, False)
    o1, i1, d1, l1 = point_search(case, nij1, nlev)
    assert np.array_equal(o1, off) and np.array_equal(i1, idx)
    np.testing.assert_allclose(d1, rd, rtol=1e-13, atol=0)
    np.testing.assert_allclose(l1, rl, rtol=1e-13, atol=0)
    cnt = group_counts(case, off, idx)
    assert (cnt[:, :4].max(axis=0) > 0).all() and cnt[:, 4].max() == 0   # every type but the skipped one contributes
    assert cnt[:, 0].max() > 1500


@pytest.mark.parametrize("criterion", [1, 3])
@pytest.mark.parametrize("nij1,nlev", SHAPES)
def test_point_search_with_a_limit_gives_the_oracle_selection(nij1, nlev, criterion):
    case = table(nij1, nlev, True, criterion)
    off, idx, rd, rl = oracle(nij1, nlev, True, criterion)
    o1, i1, d1, l1 = point_search(case, nij1, nlev)
    assert np.array_equal(o1, off)
    for pt in range(nij1 * nlev):
        s = slice(off[pt], off[pt + 1])
        a, b = np.argsort(i1[s]), np.argsort(idx[s])
        assert np.array_equal(i1[s][a], idx[s][b]), pt           # same SET (the order is implementation-defined)
        np.testing.assert_allclose(d1[s][a], rd[s][b], rtol=1e-13, atol=0)
        np.testing.assert_allclose(l1[s][a], rl[s][b], rtol=1e-13, atol=0)
    assert_limit_binds_and_not(case, (nij1, nlev), off, idx)
    # both selection paths of the kernel: a limited group's accepted candidates fit the LDS cache and are more than the limit
    # (select from the cache) / do not fit it (multi-sweep radix select)
    free = group_counts(case, *oracle(nij1, nlev, False)[:2])
    nmax = np.array([MAX_NOBS[g[0]] for g in case["groups"]])
    lim = nmax > 0
    assert ((free[:, lim] > nmax[lim]) & (free[:, lim] <= CACHE_CAP)).any() and (free[:, lim] > CACHE_CAP).any()


@pytest.mark.parametrize("route", ["lds", "rings", "rings-error-criterion"])
@pytest.mark.parametrize("nij1,nlev", SHAPES)
def test_column_search_with_a_limit_gives_the_point_search_selection(nij1, nlev, route):
    from _gpu import ctx, dev
    criterion = 3 if route == "rings-error-criterion" else 1
    case = table(nij1, nlev, True, criterion)
    _, rig, rjg, rlev, rz = setup(nij1, nlev)
    oracle(nij1, nlev, True, criterion)                          # (asserts: no selection between equal keys at any point)
    o1, i1, d1, l1 = point_search(case, nij1, nlev)
    t, keep = _search.device_struct(case, "cuda")
    c = ctx()
    c.set_option(c.OPT_LIMITED_RINGS, 0 if route == "lds" else 1)
    try:
        out = c.obs_search_columns(t, nij1, nlev, dev(rig), dev(rjg), dev(rlev), dev(rz))
        torch.cuda.synchronize()
    finally:
        c.set_option(c.OPT_LIMITED_RINGS, 2)
    o2, i2, d2, l2 = (x.cpu().numpy() for x in out)
    assert np.array_equal(o1, o2)
    for pt in range(nij1 * nlev):
        s = slice(o1[pt], o1[pt + 1])
        e1 = sorted(zip(i1[s].tolist(), d1[s].tolist(), l1[s].tolist()))
        e2 = sorted(zip(i2[s].tolist(), d2[s].tolist(), l2[s].tolist()))
        assert e1 == e2, pt                                      # same rows, weights to the last bit
    assert_limit_binds_and_not(case, (nij1, nlev), o2, i2)


def _ensemble(case, k, nv, npts, seed):
    rng = np.random.default_rng(seed)
    nobs, nens = case["nobs"], k + 1
    ens = rng.standard_normal((nobs, k)) * 2.0
    ens -= ens.mean(axis=1, keepdims=True)
    dep = rng.standard_normal(nobs) * 3.0
    gues = rng.standard_normal((nv, nens, npts))
    gues[:, :k] -= gues[:, :k].mean(axis=1, keepdims=True)      # perturbations in slots 0..k-1, the mean in slot k
    gues[:, k] = 10.0 + rng.standard_normal((nv, npts))
    return np.ascontiguousarray(ens.reshape(-1)), dep, np.ascontiguousarray(gues.reshape(-1)), nens


@pytest.mark.parametrize("nij1,nlev", SHAPES)
def test_list_free_route_equals_the_lists(nij1, nlev):
    """LETKF_OPT_COLUMN_SURVIVORS = 1 (letkf_survivors_kernel writes the survivor entries, the loop body's mode 3 reads them)
    against = 0 (the lists of the column search, one slab of all levels: the same runs up the columns)."""
    from _gpu import ctx, dev
    case = table(nij1, nlev, False)
    _, rig, rjg, rlev, rz = setup(nij1, nlev)
    off = oracle(nij1, nlev, False)[0]
    t, keep = _search.device_struct(case, "cuda")
    k, nv, npts = 16, 11, nij1 * nlev
    ens, dep, gues, nens = _ensemble(case, k, nv, npts, 5 + nlev)
    c = ctx()
    g_ens, g_dep, g_gues = dev(ens), dev(dep), dev(gues)
    coords = [dev(x) for x in (rig, rjg, rlev, rz)]
    res = {}
    for survivors in (1, 0):
        anal = torch.full((gues.size,), float("nan"), dtype=torch.float64, device="cuda")
        infl = torch.ones(npts * nv, dtype=torch.float64, device="cuda")
        st = torch.full((npts,), -1, dtype=torch.int32, device="cuda")
        nobs_out = torch.full((npts,), -5, dtype=torch.int32, device="cuda")
        c.set_option(c.OPT_COLUMN_SURVIVORS, survivors)
        c.set_option(c.OPT_SMALL_K_TRIO, 0)      # (k <= 20: the list route of the SAME kernel, not three points per wave)
        try:
            c.das_columns(k, nv, t, nij1, nlev, *coords, g_ens, k, g_dep, infl, g_gues, anal, 1, npts, npts * nens,
                          list_bytes=1 << 34, nobs_out=nobs_out, relax_alpha_spread=0.9, status=st)
            torch.cuda.synchronize()
        finally:
            c.set_option(c.OPT_COLUMN_SURVIVORS, 2)
            c.set_option(c.OPT_SMALL_K_TRIO, 1)
        assert ("FUSED" in c.last_path()) == (survivors == 1), c.last_path()
        assert int(st.abs().max()) == 0
        res[survivors] = (nobs_out, anal.view(nv, nens, npts)[:, :k])
    assert np.array_equal(res[1][0].cpu().numpy(), np.diff(off))
    assert torch.equal(res[1][0], res[0][0])
    assert torch.equal(res[1][1], res[0][1])


@pytest.mark.parametrize("nij1,nlev", SHAPES)
def test_fused_search_equals_search_then_solve(nij1, nlev):
    from _gpu import ctx, dev
    case = table(nij1, nlev, False)
    _, rig, rjg, rlev, rz = setup(nij1, nlev)
    t, keep = _search.device_struct(case, "cuda")
    k, nv, npts = 16, 11, nij1 * nlev
    ens, dep, gues, nens = _ensemble(case, k, nv, npts, 9 + nlev)
    c = ctx()
    pts = [dev(x) for x in (np.tile(rig, nlev), np.tile(rjg, nlev), rlev, rz)]
    off, idx, rd, rl = c.obs_search(t, *pts)
    assert np.array_equal(off.cpu().numpy(), oracle(nij1, nlev, False)[0])
    out = {}
    for mode in ("lists", "fused"):
        anal = torch.full((gues.size,), float("nan"), dtype=torch.float64, device="cuda")
        infl = torch.full((npts * nv,), 1.03, dtype=torch.float64, device="cuda")
        st = torch.full((npts,), -1, dtype=torch.int32, device="cuda")
        nob = torch.full((npts,), -1, dtype=torch.int32, device="cuda")
        kw = dict(status=st, iv_p=4, iv_q_first=5, iv_q_last=10, warm_run=5, relax_alpha_spread=0.95)
        if mode == "lists":
            c.set_option(c.OPT_SMALL_K_TRIO, 0)  # (k <= 20: the list route of the SAME kernel, not three points per wave)
            try:
                c.das_points(k, nv, off, idx, rd, rl, dev(ens), k, dev(dep), infl, dev(gues), anal, 1, npts, npts * nens, **kw)
            finally:
                c.set_option(c.OPT_SMALL_K_TRIO, 1)
        else:
            c.das_points(k, nv, None, None, None, None, dev(ens), k, dev(dep), infl, dev(gues), anal, 1, npts, npts * nens,
                         fused=(t, *pts), nobs_out=nob, **kw)
        torch.cuda.synchronize()
        out[mode] = (anal.view(nv, nens, npts)[:, :k], st, nob)
    (m0, s0, _), (m1, s1, n1) = out["lists"], out["fused"]
    assert int(s0.abs().max()) == 0 and int(s1.abs().max()) == 0
    counts = (off[1:] - off[:-1]).to(torch.int32)
    assert torch.equal(n1, counts) and int(counts.min()) > 0 and int(counts.max()) > 1500
    assert torch.equal(m0, m1)                                   # every point has observations: bit for bit
