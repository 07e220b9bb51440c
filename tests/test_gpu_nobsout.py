"""letkf_das_columns_nobs_dev (include/letkf_amd_nobsout.h): das_letkf's main loop with the NOBS_OUT diagnostics.  One small domain
where every branch occurs -- 7 x 5 columns, 5 levels; a merged radar pair (ref + re0, type 22) limited to 12, a surface type
limited to 3, an unlimited upper-air type (tests/_search.py); observations east of ri = 30 only, so that the western columns have
no local observation, the middle ones fewer than the limits and the eastern ones more; beta = 0 at a few points and in one whole
column; a list workspace that makes three uneven slabs of levels.  The analysis is letkf_das_columns_dev's to the last bit, the
diagnostics are letkf_obs_search_columns_dev's at beta /= 0 and zero at beta = 0."""
import functools

import numpy as np
import pytest
import torch

from _search import DIST_ZERO_FAC, build_case, device_struct

pytestmark = pytest.mark.gpu

NX, NY, NLEV, NV = 7, 5, 5, 11
NIJ1, NPTS = NX * NY, NX * NY * NLEV
LIMITS = (12, 12, 0, 3)
ELM_U, TYP = [9, 10, 3, 14], [22, 22, 1, 3]          # ref, re0 (PHARAD), T (ADPUPA), ps (ADPSFC)
PAD = 64
SW = dict(infl_adaptive=True, relax_alpha_spread=0.95)


@functools.lru_cache(None)
def domain(criterion, limited):
    """the search case and the columns, numpy"""
    case = build_case(77, max_nobs=LIMITS if limited else (0, 0, 0, 0), criterion=criterion, npts=NIJ1, obs_east_of=30.0)
    s = case["scal"]
    x = s["i_org"] + np.array([0.5, 6.0, 12.0, 18.0, 24.0, 30.0, 36.0])
    y = s["j_org"] + np.array([2.0, 9.0, 16.0, 23.0, 30.0])
    rng = np.random.default_rng(5)
    rig, rjg = np.tile(x, NY), np.repeat(y, NX)
    rlev, rz = rng.uniform(2.5e4, 1.0e5, NPTS), rng.uniform(0.0, 12000.0, NPTS)
    beta = np.ones(NPTS)
    beta[[40, 41, 99, NPTS - 1]] = 0.0
    beta[np.arange(NLEV) * NIJ1 + 26] = 0.0                       # a whole column (x = 36: above the limits)
    return case, rig, rjg, rlev, rz, beta


@functools.lru_cache(None)
def state(k):
    """ensval, dep, gues for an ensemble of k, numpy"""
    nobs = int(domain(1, True)[0]["ctype_rows"][-1])
    rng = np.random.default_rng(100 + k)
    nens = k + 1
    ens = rng.standard_normal((nobs, k)) * 2.0
    ens -= ens.mean(axis=1, keepdims=True)
    dep = rng.standard_normal(nobs) * 3.0
    gv = rng.standard_normal((NV, nens, NPTS))
    gv[:, :k] -= gv[:, :k].mean(axis=1, keepdims=True)
    gv[:, k] = 10.0 + rng.standard_normal((NV, NPTS))
    return ens.reshape(-1), dep, gv.reshape(-1), nens


def canary(n, dtype, fill):
    """(whole buffer, the n elements in its middle)"""
    full = torch.full((n + 2 * PAD,), fill, dtype=dtype, device="cuda")
    return full, full[PAD:PAD + n]


def untouched(full, fill):
    edge = torch.cat([full[:PAD], full[-PAD:]])
    return bool(torch.isnan(edge).all()) if fill != fill else bool((edge == fill).all())


def bits(t):
    return t.contiguous().view(torch.int64) if t.dtype == torch.float64 else t


class Run:
    """one call's outputs, each inside canaries"""
    SPEC = (("anal", torch.float64, float("nan")), ("infl", torch.float64, 1.03), ("status", torch.int32, -1),
            ("rtps", torch.float64, -3.0), ("nobs_out", torch.int32, -7))

    def __init__(self, k, nens):
        size = dict(anal=NV * nens * NPTS, infl=NPTS * NV, status=NPTS, rtps=NPTS * NV, nobs_out=NPTS)
        self.full, self.fill = {}, {}
        for name, dtype, fill in self.SPEC:
            self.full[name], view = canary(size[name], dtype, fill)
            self.fill[name] = fill
            setattr(self, name, view)

    def diag(self, nctype=4):
        self.full["nobs_ctype"], self.nobs_ctype = canary(NPTS * nctype, torch.int32, -9)
        self.full["cutd_ctype"], self.cutd_ctype = canary(NPTS * nctype, torch.float64, -5.0)
        self.fill.update(nobs_ctype=-9, cutd_ctype=-5.0)
        return self

    def canaries_hold(self):
        return all(untouched(self.full[n], self.fill[n]) for n in self.full)

    def pristine(self):
        """nothing written at all (infl is INOUT: its initial value)"""
        return all(untouched(self.full[n], self.fill[n]) and
                   (bool(torch.isnan(getattr(self, n)).all()) if self.fill[n] != self.fill[n] else bool((getattr(self, n) == self.fill[n]).all()))
                   for n in self.full)


class Setup:
    def __init__(self, k, criterion, limited):
        from _gpu import ctx, dev
        self.c = ctx()
        self.k = k
        self.case, rig, rjg, rlev, rz, beta = domain(criterion, limited)
        self.t, self.keep = device_struct(self.case, "cuda")
        ens, dep, gues, self.nens = state(k)
        self.rig, self.rjg, self.rlev, self.rz, self.beta = dev(rig), dev(rjg), dev(rlev), dev(rz), dev(beta)
        self.ens, self.dep, self.gues = dev(ens), dev(dep), dev(gues)
        self.beta_np = beta

    def args(self, r, list_bytes, beta=True):
        return ((self.k, NV, self.t, NIJ1, NLEV, self.rig, self.rjg, self.rlev, self.rz, self.ens, self.k, self.dep, r.infl, self.gues, r.anal,
                 1, NPTS, NPTS * self.nens),
                dict(list_bytes=list_bytes, nobs_out=r.nobs_out, beta=self.beta if beta else None, status=r.status, rtps_infl_out=r.rtps, **SW))

    def old(self, list_bytes, beta=True):
        r = Run(self.k, self.nens)
        a, kw = self.args(r, list_bytes, beta)
        self.c.das_columns(*a, **kw)
        torch.cuda.synchronize()
        return r, self.c.last_path()

    def new(self, list_bytes, beta=True, nobs=True, cutd=True):
        r = Run(self.k, self.nens).diag()
        a, kw = self.args(r, list_bytes, beta)
        self.c.das_columns_nobs(*a, nobs_ctype=r.nobs_ctype if nobs else None, cutd_ctype=r.cutd_ctype if cutd else None, **kw)
        torch.cuda.synchronize()
        return r, self.c.last_path()

    def search(self):
        """(list offsets, nobs_ctype, cutd_ctype) of letkf_obs_search_columns_dev"""
        n = torch.full((NPTS, 4), -9, dtype=torch.int32, device="cuda")
        cu = torch.full((NPTS, 4), -5.0, dtype=torch.float64, device="cuda")
        off = self.c.obs_search_columns(self.t, NIJ1, NLEV, self.rig, self.rjg, self.rlev, self.rz, nobs_ctype=n, cutd_ctype=cu)[0]
        torch.cuda.synchronize()
        return off, n, cu


def slabs(off, list_bytes):
    """the slabs of levels letkf_das_columns_dev makes: greedy, 20 B per list entry"""
    lev = off.cpu().numpy()[::NIJ1]
    out, l0 = [], 0
    while l0 < NLEV:
        l1 = l0 + 1
        while l1 < NLEV and (lev[l1 + 1] - lev[l0]) * 20 <= list_bytes:
            l1 += 1
        out.append(l1 - l0)
        l0 = l1
    return out


def three_slabs(off):
    """a list workspace for three uneven slabs"""
    lev = off.cpu().numpy()[::NIJ1]
    list_bytes = 20 * int(max(lev[2] - lev[0], lev[4] - lev[2]))
    got = slabs(off, list_bytes)
    assert len(got) >= 3 and len(set(got)) > 1, got
    return list_bytes


def options(c, **kw):
    class Guard:
        def __enter__(self):
            for o, v in kw.items():
                c.set_option(getattr(c, o), v)

        def __exit__(self, *exc):
            for o in kw:
                c.set_option(getattr(c, o), {"OPT_LIMITED_RINGS": 2, "OPT_COLUMN_SURVIVORS": 2}[o])
    return Guard()


def check(s, r_old, r_new, off, n_ref, c_ref, nobs=True, cutd=True, beta=True):
    # 1. the analysis is the old entry's
    for name in ("anal", "status", "infl", "rtps", "nobs_out"):
        assert torch.equal(bits(getattr(r_old, name)), bits(getattr(r_new, name))), name
    assert int(r_new.status.abs().max()) == 0
    live = torch.from_numpy(s.beta_np != 0.0).cuda() if beta else torch.ones(NPTS, dtype=torch.bool, device="cuda")
    counts = (off[1:] - off[:-1]).to(torch.int32)
    assert torch.equal(r_new.nobs_out, torch.where(live, counts, torch.zeros_like(counts)))
    # 2. the diagnostics are the search's where beta /= 0, zero elsewhere
    n_new, c_new = r_new.nobs_ctype.view(NPTS, 4), r_new.cutd_ctype.view(NPTS, 4)
    if nobs:
        assert torch.equal(n_new[live], n_ref[live]) and not bool(n_new[~live].any())
        assert torch.equal(n_new.sum(dim=1).to(torch.int32), r_new.nobs_out)        # 3. the row sums
    else:
        assert bool((n_new == -9).all())
    if cutd:
        assert torch.equal(bits(c_new[live]), bits(c_ref[live])) and not bool(c_new[~live].any())
    else:
        assert bool((c_new == -5.0).all())
    assert r_old.canaries_hold() and r_new.canaries_hold()                          # 4.


@pytest.mark.parametrize("rings", [0, 1])
@pytest.mark.parametrize("criterion", [1, 2, 3])
@pytest.mark.parametrize("k", [10, 50, 64])
def test_limited_tables_on_every_kernel_criterion_and_search_route(k, criterion, rings):
    s = Setup(k, criterion, True)
    with options(s.c, OPT_LIMITED_RINGS=rings):
        off, n_ref, c_ref = s.search()
        lb = three_slabs(off)
        r_old, p_old = s.old(lb)
        r_new, p_new = s.new(lb)
    assert p_new == p_old
    check(s, r_old, r_new, off, n_ref, c_ref)
    # the domain has what its docstring says: points without observations, below and above the limits, and cut-offs that moved
    n = n_ref.cpu().numpy()
    tot = n.sum(axis=1)
    assert (tot == 0).sum() >= NLEV * NY and (n[:, 0] == 12).sum() > 20 and ((n[:, 0] > 0) & (n[:, 0] < 12)).sum() > 3
    assert (n[:, 3] == 3).sum() > 20 and not n[:, 1].any() and n[:, 2].max() > 12
    cu = c_ref.cpu().numpy()
    default = np.where(criterion == 1, np.array([4000.0, 0.0, 6000.0, 8000.0]) * DIST_ZERO_FAC, 0.0)
    lim = [0, 1, 3]                                                                 # the types of the limited groups
    assert (cu[tot == 0][:, lim] == default[lim]).all()                             # trivial points carry the defaults
    assert (cu[n[:, 0] == 12, 0] != default[0]).any() and (cu[:, 1] == 0.0).all()
    # (the unlimited group's master: the default from the column kernel; the ring kernel writes no cut-off for such a group and
    # leaves the initial 0 -- the search's own difference between its routes, which this entry passes on as it is)
    assert (cu[:, 2] == (default[2] if rings == 0 else 0.0)).all() or (cu[:, 2] == default[2]).all()


@pytest.mark.parametrize("survivors", [0, 1])
@pytest.mark.parametrize("k", [10, 50])
def test_unlimited_tables_on_the_list_route_and_the_list_free_route(k, survivors):
    s = Setup(k, 1, False)
    with options(s.c, OPT_COLUMN_SURVIVORS=survivors):
        off, n_ref, c_ref = s.search()
        lb = three_slabs(off)
        r_old, p_old = s.old(lb)
        r_new, p_new = s.new(lb)
    assert ("FUSED" in p_new) == (survivors == 1) and p_new == p_old, (p_new, p_old)
    check(s, r_old, r_new, off, n_ref, c_ref)
    cu = r_new.cutd_ctype.view(NPTS, 4).cpu().numpy()
    live = s.beta_np != 0.0
    assert (cu[live] == np.array([4000.0, 0.0, 6000.0, 8000.0]) * DIST_ZERO_FAC).all()
    assert r_new.nobs_ctype.view(NPTS, 4)[:, 1].max() > 0                           # without a limit re0 counts for itself


@pytest.mark.parametrize("criterion", [2, 3])
def test_unlimited_tables_have_no_cutoff_under_the_other_criteria(criterion):
    s = Setup(10, criterion, False)
    off, n_ref, c_ref = s.search()
    r_old, _ = s.old(0)
    r_new, _ = s.new(0)
    check(s, r_old, r_new, off, n_ref, c_ref)
    assert not bool(r_new.cutd_ctype.any())


@pytest.mark.parametrize("limited,survivors", [(True, 2), (False, 0), (False, 1)])
@pytest.mark.parametrize("nobs,cutd", [(True, False), (False, True), (False, False)])
def test_either_diagnostic_may_be_null_and_without_both_the_call_is_the_old_entry(limited, survivors, nobs, cutd):
    s = Setup(10, 1, limited)
    with options(s.c, OPT_COLUMN_SURVIVORS=survivors):
        off, n_ref, c_ref = s.search()
        lb = three_slabs(off)
        r_old, p_old = s.old(lb)
        r_new, p_new = s.new(lb, nobs=nobs, cutd=cutd)
    assert p_new == p_old                                                           # 5.
    check(s, r_old, r_new, off, n_ref, c_ref, nobs=nobs, cutd=cutd)


@pytest.mark.parametrize("limited", [True, False])
def test_without_beta_no_point_is_zeroed(limited):
    s = Setup(10, 1, limited)
    off, n_ref, c_ref = s.search()
    r_old, _ = s.old(0, beta=False)
    r_new, _ = s.new(0, beta=False)
    check(s, r_old, r_new, off, n_ref, c_ref, beta=False)


def test_two_calls_give_the_same_bits():
    s = Setup(50, 1, True)
    a, _ = s.new(0)
    b, _ = s.new(0)
    for name in ("anal", "infl", "nobs_out", "nobs_ctype", "cutd_ctype"):
        assert torch.equal(bits(getattr(a, name)), bits(getattr(b, name))), name


def test_refusals_write_nothing():
    from _gpu import pkg
    s = Setup(10, 1, True)
    c = s.c

    def refused(match, mutate=None, **over):
        r = Run(s.k, s.nens).diag()
        a, kw = s.args(r, 0)
        a = list(a)
        kw.update(nobs_ctype=r.nobs_ctype, cutd_ctype=r.cutd_ctype)
        if mutate:
            mutate(a, kw, r)
        kw.update(over)
        with pytest.raises(pkg.LetkfError, match=match):
            c.das_columns_nobs(*a, **kw)
        torch.cuda.synchronize()
        assert r.pristine(), match

    # what letkf_das_columns_dev refuses
    refused("npts must be nij1", lambda a, kw, r: a.__setitem__(4, 0))
    refused("bad k", lambda a, kw, r: a.__setitem__(0, 1))
    refused("coordinate array is NULL", lambda a, kw, r: a.__setitem__(7, None))
    refused("kld too small", lambda a, kw, r: a.__setitem__(10, s.k - 1))
    refused("required device pointer", lambda a, kw, r: a.__setitem__(13, None))
    # the overlaps: a diagnostic array with nobs_out, with status, with the other one
    refused("overlaps nobs_out or args->status", lambda a, kw, r: kw.__setitem__("nobs_out", r.nobs_ctype[NPTS:2 * NPTS]))
    refused("overlaps nobs_out or args->status", lambda a, kw, r: kw.__setitem__("status", r.nobs_ctype[4 * NPTS - NPTS:]))
    refused("overlaps nobs_out or args->status", lambda a, kw, r: kw.__setitem__("nobs_out", r.cutd_ctype.view(torch.int32)[:NPTS]))
    refused("overlaps nobs_out or args->status", lambda a, kw, r: kw.__setitem__("status", r.cutd_ctype.view(torch.int32)[-NPTS:]))
    refused("nobs_ctype overlaps cutd_ctype", lambda a, kw, r: kw.__setitem__("nobs_ctype", r.cutd_ctype.view(torch.int32)[-4 * NPTS:]))
    # and the tables, which the diagnostics read
    t_bad, keep = device_struct(s.case, "cuda")
    t_bad.criterion = 4
    refused("criterion", lambda a, kw, r: a.__setitem__(2, t_bad))
