"""letkf_das_interp_dev (include/letkf_amd_interp.h): letkf_core on every s-th column, T and w-bar interpolated bilinearly, the
loop body's rules at every point.  Expected values come from nothing of that code: obs_local and letkf_core of the oracle at
the coarse points, the blend and the fine-point rules in numpy (tests/_interp.py).  Members and the deterministic member within
1e-10 max(|mean|, |x'|) per variable, rtps_infl_out within 1e-10 relative.  The base grid is 7 x 5 x 3: nx - 1 divisible by 2 and 3
but not 4, ny - 1 by 2 and 4 but not 3."""
import numpy as np
import pytest
import torch

import _interp as I

pytestmark = pytest.mark.gpu
RTPS = dict(relax_alpha_spread=0.95)


def call(c, sx, sy, cfg, beta=None, mask=0, ws_bytes=0, inplace=False, ensval=None, want_nobs=True, **extra):
    """one call on the case; (anal (nv, nens, npts), rtps (nv, npts), status, nobs_coarse, path)"""
    from _gpu import ctx, dev
    from _search import device_struct
    cx = ctx()
    d = torch.device("cuda:0")
    t, keep = device_struct(c["tc"], d)
    k, nv, npts, nens = c["k"], c["nv"], c["npts"], c["nens"]
    gues = dev(c["gues"].reshape(-1))
    anal = gues if inplace else torch.full_like(gues, float("nan"))
    status = torch.full((npts,), -1, dtype=torch.int32, device=d)
    rtps = torch.full((npts * nv,), float("nan"), dtype=torch.float64, device=d)
    ix, iy, pts = I.coarse_points(c, sx, sy)
    nobs = torch.full((len(pts),), -7, dtype=torch.int32, device=d) if want_nobs else None
    cx.das_interp(k, nv, t, c["nx"], c["ny"], c["nlev"], sx, sy, dev(c["rig"]), dev(c["rjg"]), dev(c["rlev"]), dev(c["rz"]),
                  dev(c["ensval"] if ensval is None else ensval), c["kld"], dev(c["dep"]), dev(c["infl"]), gues, anal, 1, npts,
                  npts * nens, ws_bytes=ws_bytes, nobs_coarse=nobs, beta=None if beta is None else dev(beta), status=status,
                  rtps_infl_out=rtps, var_mask=mask, iv_q_last=min(10, nv - 1), **cfg, **extra)
    torch.cuda.synchronize()
    return (anal.cpu().numpy().reshape(nv, nens, npts), rtps.cpu().numpy().reshape(nv, npts), status.cpu().numpy(),
            None if nobs is None else nobs.cpu().numpy(), cx.last_path())


def check(c, got, exp, cfg, mask=0):
    k, nv = c["k"], c["nv"]
    anal, rtps, status, nobs, path = got
    x = c["gues"]
    assert "letkf_interp_apply_kernel" in path, path
    assert (status == 0).all(), status
    if nobs is not None:
        assert np.array_equal(nobs, exp["ncoarse"])
    members = list(range(k)) + ([k + 1] if cfg.get("det_run") else [])
    for v in range(nv):
        if mask and not (mask >> v) & 1:
            assert np.isnan(anal[v]).all() and np.isnan(rtps[v]).all(), v      # outside the class: untouched
            continue
        scale = max(np.abs(x[v, k]).max(), np.abs(x[v, :k]).max())
        err = np.abs(anal[v, members] - exp["anal"][v, members]).max()
        print(f"v={v} err/scale={err / scale:.3e}")
        assert err <= 1e-10 * scale, (v, err / scale)
        rerr = np.abs(rtps[v] / exp["rtps"][v] - 1.0).max()
        assert rerr <= 1e-10, (v, rerr)
    assert np.isnan(anal[:, k]).all()                  # the mean slot is not the loop body's to write
    if not cfg.get("det_run"):
        assert np.isnan(anal[:, k + 1]).all()


@pytest.mark.parametrize("sx,sy", [(2, 2), (3, 2), (4, 4), (8, 8)])
def test_strides_on_the_base_grid(sx, sy):
    c = I.tile_case(50)
    exp = I.expected(c, RTPS, sx, sy)
    if (sx, sy) == (8, 8):
        assert list(exp["ix"]) == [0, 6] and list(exp["iy"]) == [0, 4]      # the ends only
    assert (exp["ncoarse"] == 0).any() and (exp["ncoarse"] > I.LIMITS[0]).any()
    check(c, call(c, sx, sy, RTPS), exp, RTPS)


@pytest.mark.parametrize("s", [2, 8])
def test_a_line_of_columns(s):
    c = I.tile_case(50, nx=1, ny=5)
    check(c, call(c, s, s, RTPS), I.expected(c, RTPS, s, s), RTPS)


@pytest.mark.parametrize("k", [3, 20, 50, 63, 100, 128])
def test_ensemble_sizes(k):
    """the k-tail of the matrix instruction (3, 50, 63, 100), the solver routes behind the coarse solves (one wave to 62, two to
    100, staged beyond) and the LDS maximum (128)"""
    c = I.tile_case(k)
    got = call(c, 2, 2, RTPS)
    route = "NW=1" if k <= 62 else "NW=2" if k <= 100 else "staged:"
    assert route in got[4], got[4]
    check(c, got, I.expected(c, RTPS, 2, 2), RTPS)


def test_five_variables_and_a_class_mask():
    c = I.tile_case(20, nv=5)
    mask = 0b10110
    check(c, call(c, 2, 2, RTPS, mask=mask), I.expected(c, RTPS, 2, 2, mask=mask), RTPS, mask=mask)


def _beta(c):
    """zeros and tapers; coarse point (2, 2, level 1) of stride (2, 2) has beta = 0, its neighbours beta > 0"""
    rng = np.random.default_rng(3)
    b = np.ones(c["npts"])
    b[rng.integers(0, c["npts"], 12)] = 0.0
    b[rng.integers(0, c["npts"], 12)] = 0.37
    p = 2 + c["nx"] * 2 + c["nij1"] * 1
    b[[p - 1, p + 1, p - c["nx"], p + c["nx"]]] = [1.0, 0.6, 1.0, 0.8]
    b[p] = 0.0
    return b


@pytest.mark.parametrize("name,cfg,opt", [
    ("rtpp", dict(relax_alpha=0.7), {}),
    ("none", dict(), {}),
    ("det", dict(relax_alpha_spread=0.95, det_run=1), {}),
    ("inflated_prior", dict(relax_alpha_spread=0.95, relax_to_inflated_prior=1), {}),
    ("inflated_prior_rtpp", dict(relax_alpha=0.7, relax_to_inflated_prior=1), {}),
    ("beta", dict(relax_alpha_spread=0.95, det_run=1), dict(beta=True)),
    ("q_update_top", dict(relax_alpha_spread=0.95, q_update_top=5.0e4, det_run=1), {}),
    ("q_sprd_max", dict(relax_alpha_spread=0.95, q_sprd_max=0.01), {}),
    ("in_place", dict(relax_alpha_spread=0.95, det_run=1), dict(inplace=True)),
])
def test_rules(name, cfg, opt):
    c = I.tile_case(50)
    beta = _beta(c) if opt.get("beta") else None
    exp = I.expected(c, cfg, 2, 2, beta=beta)
    k = c["k"]
    if name == "q_update_top":
        top = c["gues"][4, k] < 5.0e4
        assert top.any() and not top.all()                     # cuts through the levels
    if name == "q_sprd_max":
        free = I.expected(c, RTPS, 2, 2)
        assert not np.array_equal(free["anal"][5, :k], exp["anal"][5, :k])       # the clamp is active
    got = call(c, 2, 2, cfg, beta=beta, inplace=bool(opt.get("inplace")))
    if opt.get("inplace"):
        anal = got[0].copy()
        assert np.array_equal(anal[:, k], c["gues"][:, k])     # in place: the mean stays where it was
        anal[:, k] = np.nan
        got = (anal,) + got[1:]
    check(c, got, exp, cfg)


def test_stride_one_equals_das_columns():
    """every point a coarse point: the route's own kernels (no shortcut) against letkf_das_columns_dev on the same inputs"""
    from _gpu import ctx, dev
    from _search import device_struct
    c = I.tile_case(50)
    cfg = dict(relax_alpha_spread=0.95, det_run=1, q_sprd_max=0.01)
    beta = _beta(c)
    anal, rtps, status, nobs, path = call(c, 1, 1, cfg, beta=beta)
    assert path.startswith("interp:") and "letkf_interp_apply_kernel" in path, path
    cx = ctx()
    d = torch.device("cuda:0")
    t, keep = device_struct(c["tc"], d)
    k, nv, npts, nens = c["k"], c["nv"], c["npts"], c["nens"]
    a0 = torch.full((c["gues"].size,), float("nan"), dtype=torch.float64, device=d)
    r0 = torch.full((npts * nv,), float("nan"), dtype=torch.float64, device=d)
    s0 = torch.full((npts,), -1, dtype=torch.int32, device=d)
    n0 = torch.full((npts,), -7, dtype=torch.int32, device=d)
    cx.das_columns(k, nv, t, c["nij1"], c["nlev"], dev(c["rig"]), dev(c["rjg"]), dev(c["rlev"]), dev(c["rz"]), dev(c["ensval"]),
                   c["kld"], dev(c["dep"]), dev(c["infl"]), dev(c["gues"].reshape(-1)), a0, 1, npts, npts * nens, nobs_out=n0,
                   beta=dev(beta), status=s0, rtps_infl_out=r0, **cfg)
    torch.cuda.synchronize()
    assert "interp" not in cx.last_path()
    assert int(s0.abs().max()) == 0 and (status == 0).all()
    n0 = n0.cpu().numpy()
    assert np.array_equal(nobs[beta != 0.0], n0[beta != 0.0])       # (the entry reports 0 where beta = 0; a coarse point is searched anyway)
    ref = a0.cpu().numpy().reshape(nv, nens, npts)
    x = c["gues"]
    for v in range(nv):
        scale = max(np.abs(x[v, k]).max(), np.abs(x[v, :k]).max())
        err = np.abs(anal[v, list(range(k)) + [k + 1]] - ref[v, list(range(k)) + [k + 1]]).max()
        print(f"v={v} err/scale={err / scale:.3e}")
        assert err <= 1e-10 * scale, (v, err / scale)
    assert np.abs(rtps.reshape(-1) / r0.cpu().numpy() - 1.0).max() <= 1e-10


def test_slab_cut_and_repetition_change_no_bit():
    c = I.tile_case(50)
    cfg = dict(relax_alpha_spread=0.95, det_run=1)
    one = call(c, 2, 2, cfg)
    again = call(c, 2, 2, cfg)
    levels = call(c, 2, 2, cfg, ws_bytes=1)                     # one level per slab
    for other in (again, levels):
        for a, b in zip(one[:4], other[:4]):
            assert np.array_equal(a, b, equal_nan=True)


def test_a_nan_row_stays_within_the_cells_that_use_it():
    c = I.tile_case(50)
    ix, iy, pts = I.coarse_points(c, 2, 2)
    lists = I.coarse_lists(c, pts)
    holders = {}
    for p, (idx, _, _) in lists.items():
        for r in idx:
            holders.setdefault(int(r), set()).add(p)
    row = min((r for r, h in holders.items() if len(h) <= 4), key=lambda r: (len(holders[r]), r))
    hold = holders[row]
    assert 0 < len(hold) < len(pts)
    ens = c["ensval"].copy()
    ens[row, 1] = np.nan
    clean = call(c, 2, 2, RTPS)
    dirty = call(c, 2, 2, RTPS, ensval=ens)
    nx, ny, nlev, k = c["nx"], c["ny"], c["nlev"], c["k"]
    affected = np.zeros(c["npts"], bool)
    for lev in range(nlev):
        for j in range(ny):
            for i in range(nx):
                affected[i + nx * j + nx * ny * lev] = any(q in hold for _, q in I.corners_of(c, ix, iy, i, j, lev))
    assert affected.any() and not affected.all()
    same = ~affected
    assert np.array_equal(clean[0][:, :, same], dirty[0][:, :, same], equal_nan=True)
    assert np.array_equal(clean[1][:, same], dirty[1][:, same], equal_nan=True)
    assert not np.array_equal(clean[0][:, :k, affected], dirty[0][:, :k, affected])
    assert np.array_equal(dirty[2] != 0, affected), (dirty[2], affected)
    assert (clean[2] == 0).all()


@pytest.mark.parametrize("what", ["infl_adaptive", "trans_out", "transm_out", "pa_out", "nsweep", "stride_0", "stride_9", "k_129",
                                  "npts"])
def test_refusals_write_nothing(what):
    from _gpu import pkg
    d = torch.device("cuda:0")
    c = I.tile_case(129, nlev=1) if what == "k_129" else I.tile_case(50)
    buf = lambda n, dt=torch.float64: torch.zeros(n, dtype=dt, device=d)
    extra, sx, sy = {}, 2, 2
    if what == "infl_adaptive":
        extra = dict(infl_adaptive=True)
    elif what in ("trans_out", "pa_out"):
        extra = {what: buf(c["npts"] * c["k"] ** 2)}
    elif what == "transm_out":
        extra = {what: buf(c["npts"] * c["k"])}
    elif what == "nsweep":
        extra = dict(nsweep=buf(c["npts"], torch.int32))
    elif what == "stride_0":
        sx = 0
    elif what == "stride_9":
        sy = 9
    elif what == "npts":
        extra = dict(npts=c["npts"] - 1)
    with pytest.raises(pkg.LetkfError, match="letkf_amd error -1:"):
        call_refused(c, sx, sy, extra)


def call_refused(c, sx, sy, extra):
    from _gpu import ctx, dev
    from _search import device_struct
    cx = ctx()
    d = torch.device("cuda:0")
    t, keep = device_struct(c["tc"], d)
    k, nv, npts, nens = c["k"], c["nv"], c["npts"], c["nens"]
    anal = torch.full((c["gues"].size,), -3.25, dtype=torch.float64, device=d)
    status = torch.full((npts,), -1, dtype=torch.int32, device=d)
    try:
        cx.das_interp(k, nv, t, c["nx"], c["ny"], c["nlev"], sx, sy, dev(c["rig"]), dev(c["rjg"]), dev(c["rlev"]), dev(c["rz"]),
                      dev(c["ensval"]), c["kld"], dev(c["dep"]), dev(c["infl"]), dev(c["gues"].reshape(-1)), anal, 1, npts,
                      npts * nens, status=status, relax_alpha_spread=0.95, **extra)
    finally:
        torch.cuda.synchronize()
        assert bool((anal == -3.25).all()) and bool((status == -1).all())
        for v in extra.values():
            if torch.is_tensor(v):
                assert int(v.count_nonzero()) == 0
