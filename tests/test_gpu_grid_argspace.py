"""The grid-side streaming entries of the C ABI (letkf_api_grid.hip: sections 4 and 7 and row f4) across their argument space,
against the numpy statement of tests/_gridspace.py (which tests/test_gridspace_helpers.py holds to the oracle without a GPU).

Every tolerance here is one of three things: bit equality (data movement, the member-order mean, the perturbations, relax_beta,
infl_init, counts, zeros, canaries); a bound derived from the count of roundings (_gridspace.spread_bound, additive_bound, the
chain length L of monit_dep's two-level reduction); or a number the project already uses for the operation (5e-14 / 1e-12 for
state_trans, 1e-15 for the exp weight).  Each tolerance check prints `worst error / bound`.

Every call that writes into a state buffer gets canary-filled buffers, the elements it must not address are compared bit for
bit afterwards, and a second identical call on a fresh upload must give identical bits.

The grids of ens_mean / to_perturbations / ens_spread are capped at 65535*16 blocks of 256 threads (2.7e8 elements): that cap
cannot be reached at a test's size and is not tried.  The caps of the five num_cu-sized grids are: relax_beta, infl_init,
additive_inflation, addinfl_weight and monit_dep each run one size at which a thread (for addinfl_weight, a wave) makes a
second trip through its stride loop."""
import ctypes as C

import numpy as np
import pytest
import torch

import _gridspace as G

pytestmark = pytest.mark.gpu
VP = C.c_void_p


@pytest.fixture(scope="module")
def env():
    from _gpu import ctx, dev, pkg
    return pkg, ctx(), dev


def num_cu():
    return torch.cuda.get_device_properties(0).multi_processor_count


def down(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def ptr(t, off=0):
    return None if t is None else VP(t.data_ptr() + off * t.element_size())


def call(env, name, *args):
    pkg, ctx, _ = env
    return getattr(pkg.lib(), name)(ctx._c, *args)


def ok(env, rc):
    assert rc == 0, (rc, env[0].lib().letkf_amd_last_error().decode())


def report(what, err, bound):
    err, bound = np.asarray(err, np.float64), np.asarray(bound, np.float64)
    ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))
    worst = float(ratio.max()) if ratio.size else 0.0
    print(f"{what}: worst error / bound {worst:.3g}")
    return worst


def twice(run):
    """run() uploads afresh, calls and returns host arrays: both runs, after asserting they agree bit for bit"""
    a, b = run(), run()
    for x, y in zip(a, b):
        assert G.same_bits(x, y)
    return a


# ------------------------------------------------------------------------------------------- mean, perturbations, spread
@pytest.mark.parametrize("k,nv,npts,name", G.ENS_CASES)
def test_mean_perturbations_spread(env, k, nv, npts, name):
    pkg, ctx, dev = env
    x = G.ens_case(k, nv, npts, filled_mean=False)
    buf, off, sp, sm, sv, mask = G.place(x, name)
    want = x.copy()
    want[:, k] = G.mean_f64(x, k)

    def mean():
        d = dev(buf)
        ctx.ens_mean(k, nv, npts, d[off:], sp, sm, sv)
        return (down(d),)
    assert G.same_bits(twice(mean)[0], G.place(want, name)[0])      # slot k the member-order sum, all else as it was

    wbuf = G.place(want, name)[0]

    def pert():
        d = dev(wbuf)
        ctx.to_perturbations(k, nv, npts, d[off:], sp, sm, sv)
        return (down(d),)
    assert G.same_bits(twice(pert)[0], G.place(G.perturbations(want, k), name)[0])
    if k < 2:
        return

    def spread():
        d, s = dev(wbuf), dev(G.canary_buffer(nv * npts + G.TAIL))
        ctx.ens_spread(k, nv, npts, d[off:], sp, sm, sv, s)
        return down(s), down(d)
    s, d = twice(spread)
    assert G.same_bits(d, wbuf) and np.all(G.bits(s[nv * npts:]) == G.CANARY)
    ref = G.spread_ld(want, k)
    err, bound = np.abs(s[:nv * npts].reshape(nv, npts) - ref).astype(np.float64), G.spread_bound(ref, k)
    assert report(f"spread k {k} nv {nv} npts {npts} {name}", err, bound) <= 1.0


def test_mean_perturbations_spread_without_points(env):
    pkg, ctx, dev = env
    d, s = dev(G.canary_buffer(G.TAIL)), dev(G.canary_buffer(G.TAIL))
    ctx.ens_mean(3, 2, 0, d, 1, 0, 0)
    ctx.to_perturbations(3, 2, 0, d, 1, 0, 0)
    ctx.ens_spread(3, 2, 0, d, 1, 0, 0, s)
    assert np.all(G.bits(down(d)) == G.CANARY) and np.all(G.bits(down(s)) == G.CANARY)


# ------------------------------------------------------------------------------------------------------- member_points
@pytest.mark.parametrize("nlev,nlon,nlat,np_,rank,nv3d,mean_slot,name", G.MP_CASES)
def test_member_points(env, nlev, nlon, nlat, np_, rank, nv3d, mean_slot, name):
    pkg, ctx, dev = env
    nxy, k = nlon * nlat, G.MP_K
    nij1 = G.nij1_of(nxy, np_, rank)
    npts, m = nij1 * nlev, (k if mean_slot else 0)
    rng = np.random.default_rng(nlev + nxy)
    field = rng.standard_normal(nv3d * nxy * nlev)
    x = G.canary_buffer(nv3d * (k + 1) * npts).reshape(nv3d, k + 1, npts)
    buf, off, sp, sm, sv, mask = G.place(x, name)

    def fwd():
        f, d = dev(field), dev(buf)
        ctx.member_points(0, nlev, nlon, nlat, nv3d, np_, rank, m, f, d[off:], nij1, sp, sm, sv)
        return down(d), down(f)
    got, f = twice(fwd)
    want = x.copy()
    want[:, m] = G.member_points_fwd(field, nlev, nxy, nv3d, np_, rank)
    assert G.same_bits(got, G.place(want, name)[0]) and G.same_bits(f, field)   # slot m; other slots and gaps: canary

    full = rng.standard_normal(x.shape)                              # every slot holds data; only slot m may travel
    fbuf = G.place(full, name)[0]
    blank = G.canary_buffer(field.size)

    def back():
        f, d = dev(blank), dev(fbuf)
        ctx.member_points(1, nlev, nlon, nlat, nv3d, np_, rank, m, f, d[off:], nij1, sp, sm, sv)
        return down(f), down(d)
    f, d = twice(back)
    assert G.same_bits(f, G.member_points_back(blank, full[:, m], nlev, nxy, nv3d, np_, rank)) and G.same_bits(d, fbuf)
    own = np.zeros(nxy, bool)
    own[rank::np_] = True
    assert np.all(G.bits(f.reshape(nv3d, nxy, nlev)[:, ~own]) == G.CANARY)


def test_member_points_of_a_rank_without_points(env):
    pkg, ctx, dev = env
    nlev, nlon, nlat, np_, rank = 31, 3, 1, 5, 4                     # np > nxy: ranks 3 and 4 own nothing
    assert G.nij1_of(nlon * nlat, np_, rank) == 0
    for direction in (0, 1):
        f, d = dev(G.canary_buffer(nlev * 3 * 2)), dev(G.canary_buffer(G.TAIL))
        ctx.member_points(direction, nlev, nlon, nlat, 2, np_, rank, 0, f, d, 0, 1, 0, 0)
        assert np.all(G.bits(down(f)) == G.CANARY) and np.all(G.bits(down(d)) == G.CANARY)


# --------------------------------------------------------------------------------------------------------- state_trans
def consts_struct(pkg, c):
    s = pkg.StateConsts()
    for f in ("rdry", "rvap", "cvdry", "pre00", "iv_q", "positive_definite_q", "positive_definite_qhyd") + G.SLOTS:
        setattr(s, f, c[f])
    for i, v in enumerate(c["tracer_cv"]):
        s.tracer_cv[i] = v
    return s


LEAD = 17


def run_state_trans(env, c, dims, v, inverse):
    pkg, ctx, dev = env
    buf = G.canary_buffer(LEAD + v.size + G.TAIL)
    buf[LEAD:LEAD + v.size] = v.reshape(-1)

    def run():
        d = dev(buf)
        ctx.state_trans(consts_struct(pkg, c), *dims, c["nv3d"], d[LEAD:], inverse=inverse)
        return (down(d),)
    out = twice(run)[0]
    assert np.all(G.bits(out[:LEAD]) == G.CANARY) and np.all(G.bits(out[LEAD + v.size:]) == G.CANARY)
    return out[LEAD:LEAD + v.size].reshape(v.shape)


@pytest.mark.parametrize("assign", G.STATE_ASSIGN)
@pytest.mark.parametrize("nq", G.STATE_NQ)
def test_state_trans(env, nq, assign):
    worst = 0.0
    for dims in G.STATE_GRIDS:
        n = dims[0] * dims[1] * dims[2]
        for cq, ch in G.CLAMPS:
            c = G.state_consts(assign, nq, cq, ch)
            nv3d = c["nv3d"]
            v = G.state_field(c, n, seed=n + nq)
            for inverse in (False, True):
                src = G.state_inverse_input(c, v) if inverse else v
                got = run_state_trans(env, c, dims, src, inverse)
                ref = G.state_trans_ld(c, src, inverse)
                wr = G.state_written(c, inverse)
                keep = [s for s in range(nv3d) if s not in wr]
                assert G.same_bits(got[keep], src[keep])                         # untouched variables
                err, bound = np.abs(got[wr] - ref[wr]).astype(np.float64), 5e-14 * np.abs(ref[wr]).astype(np.float64)
                assert np.all(err <= bound), (dims, cq, ch, inverse, float((err / bound).max()))
                worst = max(worst, float(np.where(bound > 0, err / np.where(bound > 0, bound, 1), 0).max()))
                if inverse:
                    cl = G.clamped_species(c)
                    for s in cl:
                        assert np.all(got[s][src[s] < 0] == 0.0) and G.same_bits(got[s][src[s] >= 0], src[s][src[s] >= 0])
                        assert n < 255 or (src[s] < 0).any()
                    if nq == 8 and ch:                                           # the 7th and 8th species are not hydrometeors
                        assert cl[-5:] == list(range(c["iv_q"] + 1, c["iv_q"] + 6))
                        assert n < 255 or (got[c["iv_q"] + 6:] < 0).any()
        # inverse of forward: with negative moisture kept (no clamp), and with every clamp on a state that needs none
        for cq, negative in ((0, True), (1, False)):
            c = G.state_consts(assign, nq, cq, cq)
            v = G.state_field(c, n, seed=n + nq + 1, negative=negative)
            b = run_state_trans(env, c, dims, run_state_trans(env, c, dims, v, False), True)
            held = [s for s in range(c["nv3d"]) if s in G.state_written(c, True) or s >= c["iv_q"]]
            assert np.allclose(b[held], v[held], rtol=1e-12, atol=1e-18)
    print(f"state_trans {assign} nq {nq}: worst error / bound {worst:.3g}")


# ------------------------------------------------------------------------------------------------ relax_beta, infl_init
def beta_struct(pkg, p):
    s = pkg.BetaParams()
    for f, v in p.items():
        setattr(s, f, v)
    return s


def run_relax_beta(env, p, rig, rjg, hgt):
    pkg, ctx, dev = env
    nlev, nij1 = hgt.shape
    beta = dev(G.canary_buffer(hgt.size + G.TAIL))
    ctx.relax_beta(beta_struct(pkg, p), nij1, nlev, dev(rig), dev(rjg), dev(hgt.reshape(-1)), beta)
    out = down(beta)
    assert np.all(G.bits(out[hgt.size:]) == G.CANARY)
    return out[:hgt.size].reshape(nlev, nij1)


@pytest.mark.parametrize("radar_only,bw", G.BETA_FLAGS)
@pytest.mark.parametrize("nlev", [1, 9])
def test_relax_beta(env, radar_only, bw, nlev):
    p = G.beta_params(radar_only, bw)
    for rig, rjg in (G.beta_points(p), tuple(a[:1] for a in G.beta_points(p))):      # the placed points; nij1 = 1
        hgt = G.beta_heights(p, nlev, rig.size, seed=nlev)
        z = G.zcut_of(p)
        assert (hgt == z).any() and (hgt.size < 3 or ((hgt == np.nextafter(z, np.inf)).any() and (hgt == np.nextafter(z, 0)).any()))
        want = G.relax_beta(p, rig, rjg, hgt)
        assert G.same_bits(run_relax_beta(env, p, rig, rjg, hgt), want)
        if radar_only and hgt.size >= 3:
            assert want[hgt == np.nextafter(z, np.inf)][0] == 0.0
        if bw > 0 and not radar_only and rig.size > 1:
            assert list(want[0][:4]) == [0.0, 0.0, 1.0, 1.0] and 0 < want[0][5] < 1e-12 and list(want[0][6:8]) == [0.0, 0.0]


def test_relax_beta_second_trip_of_the_stride_loop(env):
    n = num_cu() * 32 * 256 + 1000                                   # the grid is capped at num_cu*32 blocks of 256
    nlev = 8
    assert n % nlev == 0
    nij1 = n // nlev
    p = G.beta_params(1, 5000.0, nlong=2000, nlatg=1500)
    rng = np.random.default_rng(2)
    rig, rjg = rng.uniform(1.0, 2004.0, nij1), rng.uniform(1.0, 1504.0, nij1)
    hgt = rng.uniform(20.0, 19000.0, (nlev, nij1))
    want = G.relax_beta(p, rig, rjg, hgt)
    assert (want == 0).any() and (want == 1).any() and ((want > 0) & (want < 1)).any()
    assert G.same_bits(run_relax_beta(env, p, rig, rjg, hgt), want)


def run_infl_init(env, w0, mul, mn):
    pkg, ctx, dev = env
    buf = G.canary_buffer(w0.size + G.TAIL)
    buf[:w0.size] = w0
    d = dev(buf)
    ctx.infl_init(d[:w0.size], mul, mn)
    out = down(d)
    assert np.all(G.bits(out[w0.size:]) == G.CANARY)
    return out[:w0.size]


@pytest.mark.parametrize("mul,mn", G.INFL_SIGNS)
@pytest.mark.parametrize("n", [1, 257])
def test_infl_init(env, mul, mn, n):
    w0 = np.random.default_rng(n).uniform(0.7, 1.6, n)
    assert G.same_bits(run_infl_init(env, w0, mul, mn), G.infl_init(w0, mul, mn))


def test_infl_init_second_trip_of_the_stride_loop(env):
    w0 = np.random.default_rng(5).uniform(0.7, 1.6, num_cu() * 32 * 256 + 1000)
    assert G.same_bits(run_infl_init(env, w0, -1.0, 0.95), G.infl_init(w0, -1.0, 0.95))


# ------------------------------------------------------------------------------------------ additive inflation, weights
def run_additive(env, case, d, what):
    pkg, ctx, dev = env
    k, nv, npts, nij1 = d["k"], d["nv"], d["npts"], d["nij1"]
    anal, add = d["anal"], d["add"]
    w = d["weight"] if case["weight"] else None
    sh = d["ishuf"] if case["ishuf"] else None
    q2 = d["gues"][:, k] if case["qmean"] else None
    abuf, off, sp, sm, sv, mask = G.place(anal, case["layout"])
    bbuf = G.place(add, case["layout"])[0]
    if case["qmean"] in (None, "packed"):
        qbuf, qoff, q_sp, q_sv = (np.ascontiguousarray(q2).reshape(-1) if q2 is not None else None), 0, 1, npts
    else:                                                            # the mean slot of a gues buffer in a layout of its own
        qbuf, goff, q_sp, g_sm, q_sv, _ = G.place(d["gues"], case["qmean"])
        qoff = goff + k * g_sm

    def run():
        da, db = dev(abuf), dev(bbuf)
        dq = dev(qbuf) if qbuf is not None else None
        ctx.additive_inflation(k, nv, npts, nij1, da[off:], db[off:], sp, sm, sv, d["infl_add"],
                               weight=dev(w) if w is not None else None, qmean=dq[qoff:] if dq is not None else None,
                               q_sp=q_sp, q_sv=q_sv, iv_q_first=case["q"][0], iv_q_last=case["q"][1],
                               ishuf=dev(sh) if sh is not None else None)
        return down(da), down(db)
    out, b = twice(run)
    assert G.untouched(out, mask) and G.same_bits(b, bbuf)
    got = G.lift(out, anal.shape, case["layout"])
    ref, ax = G.additive_ld(anal, add, k, nij1, d["infl_add"], w, q2, *case["q"], sh)
    assert G.same_bits(got[:, k], anal[:, k])                        # the mean slot
    assert report(what, np.abs(got - ref).astype(np.float64), G.additive_bound(anal, ax)) <= 1.0
    assert not G.same_bits(got[:, :k], anal[:, :k])
    return got


@pytest.mark.parametrize("ci", range(len(G.ADD_CASES)))
def test_additive_inflation(env, ci):
    case = G.ADD_CASES[ci]
    d = G.additive_case(case["k"], 11, 15, 3, seed=ci)
    got = run_additive(env, case, d, f"additive_inflation {case}")
    if case["qmean"] and case["q"] == (11, 10):                      # no variable in the q range: as without qmean
        plain = run_additive(env, dict(case, qmean=None), d, "additive_inflation, the same without qmean")
        assert G.same_bits(got, plain)


def test_additive_inflation_second_trip_of_the_stride_loop(env):
    cap = num_cu() * 16 * 256                                        # the grid is capped at num_cu*16 blocks of 256
    k, nv, nij1 = 6, 11, 100
    nlev = cap // (k * nv * nij1) + 1
    assert cap < nlev * nij1 * k * nv < cap + k * nv * nij1 + 1
    d = G.additive_case(k, nv, nij1, nlev, seed=77)
    run_additive(env, dict(weight=1, qmean="packed", ishuf=1, layout="point", k=k, q=(5, 10)), d, "additive_inflation, long")


def test_additive_inflation_without_points(env):
    pkg, ctx, dev = env
    a, b = dev(G.canary_buffer(G.TAIL)), dev(G.canary_buffer(G.TAIL))
    ctx.additive_inflation(6, 11, 0, 15, a, b, 1, 0, 0, 0.3)
    assert np.all(G.bits(down(a)) == G.CANARY)


def run_weight(env, c):
    pkg, ctx, dev = env
    nij1, nob = len(c["rig"]), len(c["ob_ri"])
    out = dev(G.canary_buffer(nij1 + G.TAIL))
    ri, rj = dev(c["rig"]), dev(c["rjg"])
    oi, oj = (dev(c["ob_ri"]), dev(c["ob_rj"])) if nob else (None, None)
    ok(env, call(env, "letkf_addinfl_weight_dev", nij1, ptr(ri), ptr(rj), nob, ptr(oi), ptr(oj), c["dx"], c["dy"], c["hori_loc"],
                 ptr(out)))
    got = down(out)
    assert np.all(G.bits(got[nij1:]) == G.CANARY)
    return got[:nij1]


def check_weight(what, got, ref):
    assert np.array_equal(got == 0.0, ref == 0)                      # zeros exact, and nowhere else
    r = ref.astype(np.float64)
    assert report(what, np.abs(got - ref).astype(np.float64), 1e-15 * r) <= 1.0


@pytest.mark.parametrize("nob", G.WEIGHT_NOB)
@pytest.mark.parametrize("nij1", G.WEIGHT_NIJ1)
def test_addinfl_weight(env, nij1, nob):
    c = G.weight_case(nij1, nob, seed=nob + nij1)
    got = run_weight(env, c)
    assert G.same_bits(got, run_weight(env, c))
    d = G.addinfl_weight_d(c["rig"], c["rjg"], c["ob_ri"], c["ob_rj"], c["dx"], c["dy"], c["hori_loc"])
    check_weight(f"addinfl_weight nij1 {nij1} nob {nob}", got, G.addinfl_weight_ld(d))
    if nob == 0:
        assert not got.any()
    else:
        assert got[c["on_obs"]] == 1.0                               # an observation exactly on the grid point
    if nob >= 63 and nij1 > 1:
        assert (got == 0).any() and ((got > 0) & (got < 0.01)).any()


def test_addinfl_weight_second_trip_of_the_stride_loop(env):
    nij1 = num_cu() * 64 + 5                                         # one wave per point on at most num_cu*16 blocks of 4 waves
    c = G.weight_case(nij1, 3, seed=11)
    c["rig"][-1], c["rjg"][-1] = c["ob_ri"][0] + 1.0, c["ob_rj"][0]    # a point of the second trip a quarter length from an obs
    got = run_weight(env, c)
    d = G.addinfl_weight_d(c["rig"], c["rjg"], c["ob_ri"], c["ob_rj"], c["dx"], c["dy"], c["hori_loc"])
    check_weight(f"addinfl_weight nij1 {nij1} nob 3", got, G.addinfl_weight_ld(d))
    tail = got[num_cu() * 64:]                                       # the points of the second trip
    assert got[c["on_obs"]] == 1.0 and (got == 0).any() and tail.size == 5 and tail[-1] > 0.9


def test_addinfl_weight_at_the_cut_off(env):
    h, t_eq, t_far = G.cutoff_construction()
    c = dict(rig=np.array([t_eq, t_far, 0.0]), rjg=np.zeros(3), ob_ri=np.array([0.0, 1000.0]), ob_rj=np.array([0.0, 1000.0]),
             dx=1.0, dy=1.0, hori_loc=h)
    d = G.addinfl_weight_d(c["rig"], c["rjg"], c["ob_ri"], c["ob_rj"], 1.0, 1.0, h)
    assert d[0] == G.CUT2 and d[1] == np.nextafter(G.CUT2, np.inf) and d[2] == 0.0     # the statement lands where meant
    got = run_weight(env, c)
    assert got[1] == 0.0 and got[2] == 1.0 and got[0] > 0.0
    check_weight("addinfl_weight at the cut-off", got, G.addinfl_weight_ld(d))


# ------------------------------------------------------------------------------------------------------------ monit_dep
def run_monit(env, table, elm, dep, qc):
    pkg, ctx, dev = env
    nid, nn = len(table), len(elm)
    nobs = dev(G.canary_buffer(nid + G.TAIL, np.int32))
    bias, rmse = dev(G.canary_buffer(nid + G.TAIL)), dev(G.canary_buffer(nid + G.TAIL))
    e, d, q = (dev(elm), dev(dep), dev(qc)) if nn else (None, None, None)
    ok(env, call(env, "letkf_monit_dep_dev", nid, table.ctypes.data_as(VP), nn, ptr(e), ptr(d), ptr(q), ptr(nobs), ptr(bias),
                 ptr(rmse)))
    n, b, r = down(nobs), down(bias), down(rmse)
    assert np.all(n[nid:] == G.ICANARY) and np.all(G.bits(b[nid:]) == G.CANARY) and np.all(G.bits(r[nid:]) == G.CANARY)
    return n[:nid], b[:nid], r[:nid]


def check_monit(what, got, table, elm, dep, qc):
    """counts exact, undef where nothing counted; |bias - ref| <= L u mean|d| and |mean square - ref| <= L u mean d^2, L the
    longest chain of additions (the division is paid for by the two additions to zero that open a thread's run and the final
    pass; the squares enter by fused multiply-add and cost no rounding of their own).  rmse is the root of the mean square:
    the root halves the relative error of its argument and adds one rounding, so |rmse - ref| <= (L/2 + 1) u rmse."""
    n, b, r = got
    r_n, r_b, r_ms, r_abs = G.monit_dep_ld(table, elm, dep, qc)
    assert np.array_equal(n, r_n)
    has = r_n > 0
    assert np.all(b[~has] == G.UNDEF) and np.all(r[~has] == G.UNDEF)
    L = G.monit_chain(len(elm), 4 * num_cu())
    rr = np.sqrt(r_ms[has])
    w1 = report(f"{what} bias (L {L})", np.abs(b[has] - r_b[has]).astype(np.float64), (L * G.U * r_abs[has]).astype(np.float64))
    w2 = report(f"{what} rmse (L {L})", np.abs(r[has] - rr).astype(np.float64), ((L / 2 + 1) * G.U * rr).astype(np.float64))
    assert w1 <= 1.0 and w2 <= 1.0
    return r_n


@pytest.mark.parametrize("kind", ["offset", "zero"])
@pytest.mark.parametrize("size", ["one", "n255", "n257", "per257", "ragged"])
@pytest.mark.parametrize("nid", [1, 16, 32])
def test_monit_dep(env, nid, size, kind):
    nblk = 4 * num_cu()
    nn = G.monit_sizes(num_cu())[size]
    if size == "per257":
        assert -(-nn // nblk) == 257
    if size == "ragged":
        per = -(-nn // nblk)
        assert (nblk - 1) * per > nn                                 # the last blocks start behind the data
    table, elm, dep, qc = G.monit_case(nid, nn, kind, seed=nid + nn)
    got = run_monit(env, table, elm, dep, qc)
    for a, b in zip(got, run_monit(env, table, elm, dep, qc)):
        assert G.same_bits(a, b)
    r_n = check_monit(f"monit_dep nid {nid} nn {nn} {kind}", got, table, elm, dep, qc)
    if nid >= 16 and nn > 1000:                                      # the table lists 3074 and 4004: nothing lands there
        assert r_n[3] == 0 and r_n[9] == 0 and r_n[2] > 0 and r_n[8] > 0
        assert got[1][3] == G.UNDEF and got[2][9] == G.UNDEF
        folded = (qc == 0) & ((elm == G.ID_T) | (elm == G.ID_TV))
        assert r_n[2] == int(folded.sum()) and ((elm == G.ID_TV) & (qc == 0)).any()
    # rows whose id the table lacks have no effect on any slot: rejecting them changes no bit
    e = np.where(elm == G.ID_TV, G.ID_T, elm)
    e = np.where(e == G.ID_RE0, G.ID_REF, e)
    lacking = ~np.isin(e, table)
    if nn > 1000:
        assert (lacking & (qc == 0)).any()
    for a, b in zip(got, run_monit(env, table, elm, dep, np.where(lacking, 5, qc).astype(np.int32))):
        assert G.same_bits(a, b)


@pytest.mark.parametrize("nid", [1, 16])
def test_monit_dep_rejected_rows(env, nid):
    """NaN and +-Inf departures on rejected rows: the statistics stay finite and keep the bits of the call that has finite
    values on those rows (the same rows, so the same partition over blocks and threads); all rows rejected: all undef"""
    nn = 3 * 4 * num_cu() - 5
    table, elm, dep, qc = G.monit_case(nid, nn, "zero", seed=9)
    clean = run_monit(env, table, elm, dep, qc)
    bad = dep.copy()
    rej = np.flatnonzero(qc != 0)
    bad[rej] = np.resize(np.array([np.nan, np.inf, -np.inf]), rej.size)
    assert rej.size > 100
    got = run_monit(env, table, elm, bad, qc)
    assert np.isfinite(got[1]).all() and np.isfinite(got[2]).all()
    for a, b in zip(got, clean):
        assert G.same_bits(a, b)
    check_monit(f"monit_dep nid {nid}, NaN / Inf on rejected rows", got, table, elm, dep, qc)
    n, b, r = run_monit(env, table, elm, bad, np.full(nn, 5, np.int32))
    assert not n.any() and np.all(b == G.UNDEF) and np.all(r == G.UNDEF)


# ------------------------------------------------------------------------------------------------------------- refusals
N_R = dict(k=3, nv=2, npts=5, nlev=3, nlon=2, nlat=2, nv3d=11)


def canary_dev(dev, n, dtype=np.float64):
    return dev(G.canary_buffer(n, dtype))


def refusal_case(env, entry):
    """(argument names in the entry's order, valid arguments, the device buffers the call could write).  Every device buffer
    holds canaries: a refused call reads and writes none of them."""
    pkg, ctx, dev = env
    k, nv, npts = N_R["k"], N_R["nv"], N_R["npts"]
    state = canary_dev(dev, nv * (k + 1) * npts)
    strides = dict(sp=1, sm=npts, sv=npts * (k + 1))
    if entry in ("letkf_ens_mean_dev", "letkf_ens_to_perturbations_dev"):
        return ["k", "nv", "npts", "x", "sp", "sm", "sv"], dict(k=k, nv=nv, npts=npts, x=state, **strides), [state]
    if entry == "letkf_ens_spread_dev":
        s = canary_dev(dev, nv * npts)
        return (["k", "nv", "npts", "x", "sp", "sm", "sv", "sprd"], dict(k=k, nv=nv, npts=npts, x=state, sprd=s, **strides),
                [state, s])
    if entry == "letkf_state_trans_dev":
        c = consts_struct(pkg, G.state_consts("scale", 6))
        v = canary_dev(dev, 14 * 12)                                 # room for the 14 variables one case asks for
        return (["c", "nlev", "nlon", "nlat", "nv3d", "v3dg", "inverse"],
                dict(c=c, nlev=3, nlon=2, nlat=2, nv3d=11, v3dg=v, inverse=0), [v])
    if entry == "letkf_member_points_dev":
        f, x = canary_dev(dev, 2 * 12), canary_dev(dev, 2 * 3 * 6)    # nxy 4, np 2: nij1 2, npts 6
        return (["dir", "nlev", "nlon", "nlat", "nv3d", "np", "rank", "m", "v3dg", "x", "nij1", "sp", "sm", "sv"],
                dict(dir=0, nlev=3, nlon=2, nlat=2, nv3d=2, np=2, rank=1, m=1, v3dg=f, x=x, nij1=2, sp=1, sm=6, sv=18), [f, x])
    if entry == "letkf_relax_beta_dev":
        p = beta_struct(pkg, G.beta_params(1, 5000.0))
        a = [canary_dev(dev, 4), canary_dev(dev, 4), canary_dev(dev, 12), canary_dev(dev, 12)]
        return (["p", "nij1", "nlev", "rig", "rjg", "hgt", "beta"],
                dict(p=p, nij1=4, nlev=3, rig=a[0], rjg=a[1], hgt=a[2], beta=a[3]), [a[3]])
    if entry == "letkf_infl_init_dev":
        w = canary_dev(dev, 7)
        return ["n", "work3d", "infl_mul", "infl_mul_min"], dict(n=7, work3d=w, infl_mul=1.1, infl_mul_min=0.0), [w]
    if entry == "letkf_additive_inflation_dev":
        add = canary_dev(dev, nv * (k + 1) * 6)
        anal = canary_dev(dev, nv * (k + 1) * 6)
        return (["k", "nv", "npts", "nij1", "anal", "add", "sp", "sm", "sv", "infl_add", "weight", "qmean", "q_sp", "q_sv",
                 "iv_q_first", "iv_q_last", "ishuf"],
                dict(k=k, nv=nv, npts=6, nij1=3, anal=anal, add=add, sp=1, sm=6, sv=6 * (k + 1), infl_add=0.3, weight=None,
                     qmean=None, q_sp=0, q_sv=0, iv_q_first=5, iv_q_last=10, ishuf=None), [anal])
    if entry == "letkf_addinfl_weight_dev":
        a = [canary_dev(dev, 4) for _ in range(5)]
        return (["nij1", "rig", "rjg", "nob", "ob_ri", "ob_rj", "dx", "dy", "hori_loc", "weight"],
                dict(nij1=4, rig=a[0], rjg=a[1], nob=4, ob_ri=a[2], ob_rj=a[3], dx=1000.0, dy=1000.0, hori_loc=4000.0,
                     weight=a[4]), [a[4]])
    if entry == "letkf_monit_dep_dev":
        outs = [canary_dev(dev, 32, np.int32), canary_dev(dev, 32), canary_dev(dev, 32)]
        ins = [canary_dev(dev, 9, np.int32), canary_dev(dev, 9), canary_dev(dev, 9, np.int32)]
        return (["nid", "elem_uid", "nn", "elm", "dep", "qc", "nobs", "bias", "rmse"],
                dict(nid=16, elem_uid=G.ELEM_UID.copy(), nn=9, elm=ins[0], dep=ins[1], qc=ins[2], nobs=outs[0], bias=outs[1],
                     rmse=outs[2]), outs)
    raise ValueError(entry)


def null(*names):
    return [(f"{n} NULL", {n: None}) for n in names]


SLOT_CASES = [(f"{s} = {name}", {"c." + s: bad}) for s in G.SLOTS for name, bad in (("-1", -1), ("nv3d", 11))]
REFUSALS = {
    "letkf_ens_mean_dev": null("x") + [("k 0", dict(k=0)), ("nv 0", dict(nv=0)), ("npts -1", dict(npts=-1))],
    "letkf_ens_to_perturbations_dev": null("x") + [("k 0", dict(k=0)), ("nv 0", dict(nv=0)), ("npts -1", dict(npts=-1))],
    "letkf_ens_spread_dev": null("x", "sprd") + [("k 1", dict(k=1)), ("nv 0", dict(nv=0)), ("npts -1", dict(npts=-1))],
    "letkf_state_trans_dev": null("c", "v3dg") + [("nlev 0", dict(nlev=0)), ("nlon 0", dict(nlon=0)), ("nlat 0", dict(nlat=0)),
                                                  ("nv3d 0", dict(nv3d=0)), ("iv_q -1", {"c.iv_q": -1}),
                                                  ("iv_q = nv3d", {"c.iv_q": 11}),
                                                  ("nine moisture species", dict(nv3d=14))] + SLOT_CASES,
    "letkf_member_points_dev": null("v3dg", "x") + [("nlev 0", dict(nlev=0)), ("nlon 0", dict(nlon=0, nij1=0)),
                                                    ("nlat 0", dict(nlat=0, nij1=0)), ("nv3d 0", dict(nv3d=0)),
                                                    ("nlev -1", dict(nlev=-1)), ("nv3d -1", dict(nv3d=-1)),
                                                    ("np 0", dict(np=0)), ("rank = np", dict(rank=2)), ("rank -1", dict(rank=-1)),
                                                    ("m -1", dict(m=-1)), ("nij1 one more", dict(nij1=3)),
                                                    ("nij1 one less", dict(nij1=1)), ("nij1 -1", dict(nij1=-1))],
    "letkf_relax_beta_dev": null("p", "rig", "rjg", "hgt", "beta") + [("nij1 -1", dict(nij1=-1)), ("nlev 0", dict(nlev=0))],
    "letkf_infl_init_dev": null("work3d") + [("n -1", dict(n=-1))],
    "letkf_additive_inflation_dev": null("anal", "add") + [("k 0", dict(k=0)), ("nv 0", dict(nv=0)), ("npts -1", dict(npts=-1)),
                                                           ("nij1 0", dict(nij1=0)), ("npts % nij1", dict(nij1=4))],
    "letkf_addinfl_weight_dev": null("rig", "rjg", "weight", "ob_ri", "ob_rj") + [
        ("nij1 -1", dict(nij1=-1)), ("nob -1", dict(nob=-1)), ("hori_loc 0", dict(hori_loc=0.0)),
        ("hori_loc -1", dict(hori_loc=-1.0)), ("hori_loc NaN", dict(hori_loc=float("nan")))],
    "letkf_monit_dep_dev": null("elem_uid", "elm", "dep", "qc", "nobs", "bias", "rmse") + [
        ("nid 0", dict(nid=0)), ("nid 33", dict(nid=33)), ("nn -1", dict(nn=-1))],
}


# the text letkf_amd_last_error() must hold after a refusal: the entry's usual one, and the cases with a reason of their own
_SLOT, _DIM, _ARR = "outside [0, nv3d)", "must be at least 1", "an observation array is NULL"
WHY = {
    "letkf_ens_mean_dev": ("bad argument", {}),
    "letkf_ens_to_perturbations_dev": ("bad argument", {}),
    "letkf_ens_spread_dev": ("bad argument", {}),
    "letkf_state_trans_dev": ("bad argument", dict({w: _SLOT for w, _ in SLOT_CASES}, **{
        "iv_q -1": "moisture range", "iv_q = nv3d": "moisture range", "nine moisture species": "moisture range"})),
    "letkf_member_points_dev": ("bad argument", {"nlev 0": _DIM, "nlon 0": _DIM, "nlat 0": _DIM, "nv3d 0": _DIM, "nlev -1": _DIM,
                                                 "nv3d -1": _DIM, "nij1 one more": "cyclic share", "nij1 one less": "cyclic share"}),
    "letkf_relax_beta_dev": ("a point array is NULL", {w: "params is NULL or bad nij1 / nlev" for w in ("p NULL", "nij1 -1", "nlev 0")}),
    "letkf_infl_init_dev": ("negative size", {"work3d NULL": "work3d is NULL"}),
    "letkf_additive_inflation_dev": ("bad argument", {"npts % nij1": "npts must be nij1 * nlev"}),
    "letkf_addinfl_weight_dev": ("bad argument", {f"{n} NULL": "a pointer is NULL" for n in ("rig", "rjg", "weight", "ob_ri", "ob_rj")}),
    "letkf_monit_dep_dev": ("bad element table / outputs", {"elm NULL": _ARR, "dep NULL": _ARR, "qc NULL": _ARR}),
}


def plant_error(env, entry):
    """a refusal of another entry, with a text of its own, just before the call under test: the error text is the thread's and
    an accepted call leaves it alone, so without this a stale text could pass for the new one"""
    pkg, ctx, _ = env
    if entry == "letkf_infl_init_dev":
        rc, text = pkg.lib().letkf_relax_beta_dev(ctx._c, None, 0, 1, None, None, None, None), "params is NULL"
    else:
        rc, text = pkg.lib().letkf_infl_init_dev(ctx._c, -1, None, 1.0, 0.0), "negative size"
    assert rc == G.E_INVALID and text in pkg.lib().letkf_amd_last_error().decode()
    return text


def refusal_call(env, entry, change):
    pkg, ctx, dev = env
    names, args, outs = refusal_case(env, entry)
    args = dict(args)
    for key, val in change.items():
        if key.startswith("c."):
            setattr(args["c"], key[2:], val)
        else:
            args[key] = val

    def conv(a):
        if isinstance(a, torch.Tensor):
            return ptr(a)
        if isinstance(a, np.ndarray):
            return a.ctypes.data_as(VP)
        if isinstance(a, C.Structure):
            return C.byref(a)
        return a
    rc = call(env, entry, *[conv(args[n]) for n in names])
    torch.cuda.synchronize()
    return rc, outs


def check_refusals(env, entry, what, change):
    pkg = env[0]
    if what == "valid":                                              # the unchanged call is accepted: the refusals are not
        rc, _ = refusal_call(env, entry, {})                          # this test's own mistake
        assert rc == 0, pkg.lib().letkf_amd_last_error().decode()
        return
    planted = plant_error(env, entry)
    rc, outs = refusal_call(env, entry, change)
    why = WHY[entry][1].get(what, WHY[entry][0])
    text = pkg.lib().letkf_amd_last_error().decode()
    assert rc == G.E_INVALID and why in text and planted not in text, (entry, what, rc, text)
    for t in outs:
        want = G.CANARY if t.dtype == torch.float64 else G.ICANARY
        assert np.all(G.bits(t.cpu().numpy()) == want), (entry, what)


def _params(entry):
    return [pytest.param(w, c, id=w) for w, c in [("valid", {})] + REFUSALS[entry]]


@pytest.mark.parametrize("what,change", _params("letkf_ens_mean_dev"))
def test_ens_mean_refuses(env, what, change):
    check_refusals(env, "letkf_ens_mean_dev", what, change)


@pytest.mark.parametrize("what,change", _params("letkf_ens_to_perturbations_dev"))
def test_ens_to_perturbations_refuses(env, what, change):
    check_refusals(env, "letkf_ens_to_perturbations_dev", what, change)


@pytest.mark.parametrize("what,change", _params("letkf_ens_spread_dev"))
def test_ens_spread_refuses(env, what, change):
    check_refusals(env, "letkf_ens_spread_dev", what, change)


@pytest.mark.parametrize("what,change", _params("letkf_state_trans_dev"))
def test_state_trans_refuses(env, what, change):
    check_refusals(env, "letkf_state_trans_dev", what, change)


@pytest.mark.parametrize("what,change", _params("letkf_member_points_dev"))
def test_member_points_refuses(env, what, change):
    check_refusals(env, "letkf_member_points_dev", what, change)


@pytest.mark.parametrize("what,change", _params("letkf_relax_beta_dev"))
def test_relax_beta_refuses(env, what, change):
    check_refusals(env, "letkf_relax_beta_dev", what, change)


@pytest.mark.parametrize("what,change", _params("letkf_infl_init_dev"))
def test_infl_init_refuses(env, what, change):
    check_refusals(env, "letkf_infl_init_dev", what, change)


@pytest.mark.parametrize("what,change", _params("letkf_additive_inflation_dev"))
def test_additive_inflation_refuses(env, what, change):
    check_refusals(env, "letkf_additive_inflation_dev", what, change)


@pytest.mark.parametrize("what,change", _params("letkf_addinfl_weight_dev"))
def test_addinfl_weight_refuses(env, what, change):
    check_refusals(env, "letkf_addinfl_weight_dev", what, change)


@pytest.mark.parametrize("what,change", _params("letkf_monit_dep_dev"))
def test_monit_dep_refuses(env, what, change):
    check_refusals(env, "letkf_monit_dep_dev", what, change)
