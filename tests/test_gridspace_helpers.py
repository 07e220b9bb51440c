"""tests/_gridspace.py against the oracle's C functions, on the cases tests/test_gpu_grid_argspace.py runs on the device (the
second-trip sizes of relax_beta, infl_init, additive_inflation and addinfl_weight apart: the same functions at up to two million
elements): the numpy statement of the ten grid-side
streaming operations and the layout helpers.  No GPU.

Bit for bit: data movement, the member-order mean, the perturbations, relax_beta, infl_init, counts.  Everything else within the
bound _gridspace derives for it (the oracle is a float64 program with the reference's operation order, so it owes the
longdouble statement the same roundings the device does)."""
import ctypes as C

import numpy as np
import pytest

import _gridspace as G
import _oracle
from __graft_entry__ import load_package

pkg = load_package()
c_i32p = C.POINTER(C.c_int32)
I64, I32 = C.c_int64, C.c_int


def dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def ip(a):
    return a.ctypes.data_as(c_i32p)


class OrcBeta(C.Structure):                      # orc_beta_params (oracle/letkf_oracle.h)
    _fields_ = [("radar_only", C.c_int), ("radar_zmax", C.c_double), ("vert_local_radar", C.c_double),
                ("boundary_buffer_width", C.c_double), ("dx", C.c_double), ("dy", C.c_double), ("ihalo", C.c_int),
                ("jhalo", C.c_int), ("nlong", C.c_int), ("nlatg", C.c_int)]


def consts_struct(c):
    s = pkg.StateConsts()
    for f in ("rdry", "rvap", "cvdry", "pre00", "iv_q", "positive_definite_q", "positive_definite_qhyd") + G.SLOTS:
        setattr(s, f, c[f])
    for i, v in enumerate(c["tracer_cv"]):
        s.tracer_cv[i] = v
    return s


# ------------------------------------------------------------------------------------------------------------------ layouts
@pytest.mark.parametrize("name", G.LAYOUTS)
@pytest.mark.parametrize("shape", [(1, 2, 1), (11, 51, 257), (3, 4, 0), (2, 1, 5)])
def test_layout_round_trip_and_mask(name, shape):
    nv, nens, npts = shape
    x = np.random.default_rng(3).standard_normal(shape)
    buf, off, sp, sm, sv, mask = G.place(x, name)
    assert int(mask.sum()) == nv * nens * npts                    # no two elements share an address
    assert G.same_bits(G.lift(buf, shape, name), x)
    assert G.untouched(buf, mask) and not mask[buf.size - G.TAIL:].any()
    if npts:
        assert buf[off + (npts - 1) * sp + (nens - 1) * sm + (nv - 1) * sv] == x[-1, -1, -1]
    if name == "view":
        assert off == 17 and not mask[:17].any()
    if name == "padded" and npts:
        assert sm == npts + 3 and sv == sm * nens + 5
    if name == "member":
        assert (sv, sm, sp) == (1, nv, nens * nv)
    if name == "var_mid":
        assert (sp, sv, sm) == (1, npts, npts * nv)


# ------------------------------------------------------------------------------------------- mean, perturbations, spread
@pytest.mark.parametrize("k,nv,npts,name", G.ENS_CASES)
def test_mean_perturbations_spread_against_the_oracle(k, nv, npts, name):
    o = _oracle.oracle()
    x = G.ens_case(k, nv, npts, filled_mean=False)
    buf, off, sp, sm, sv, mask = G.place(x, name)
    o.orc_ensmean(I32(k), I32(nv), I64(npts), dp(buf[off:]), I64(sp), I64(sm), I64(sv))
    want = x.copy()
    want[:, k] = G.mean_f64(x, k)
    assert G.same_bits(buf, G.place(want, name)[0])
    ld = G.mean_ld(x, k)                                          # k - 1 additions and a division
    assert np.all(np.abs(want[:, k] - ld) <= k * G.U * np.abs(x[:, :k]).sum(axis=1) / k)
    o.orc_to_perturbations(I32(k), I32(nv), I64(npts), dp(buf[off:]), I64(sp), I64(sm), I64(sv))
    assert G.same_bits(buf, G.place(G.perturbations(want, k), name)[0])
    if k >= 2:
        buf = G.place(want, name)[0]
        sprd = G.canary_buffer(nv * npts + G.TAIL)
        o.orc_ens_spread(I32(k), I32(nv), I64(npts), dp(buf[off:]), I64(sp), I64(sm), I64(sv), dp(sprd))
        ref = G.spread_ld(want, k)
        err = np.abs(sprd[:nv * npts].reshape(nv, npts) - ref).astype(np.float64)
        assert np.all(err <= G.spread_bound(ref, k)), (err / G.spread_bound(ref, k)).max()
        assert np.all(ref < 2e-2 * np.abs(want[:, k])) and np.all(G.bits(sprd[nv * npts:]) == G.CANARY)


# ------------------------------------------------------------------------------------------------------- member_points
@pytest.mark.parametrize("nlev,nlon,nlat,np_,rank,nv3d,mean_slot,name", G.MP_CASES)
def test_member_points_against_the_oracle(nlev, nlon, nlat, np_, rank, nv3d, mean_slot, name):
    o = _oracle.oracle()
    nxy, k = nlon * nlat, G.MP_K
    nij1 = G.nij1_of(nxy, np_, rank)
    npts, m = nij1 * nlev, (k if mean_slot else 0)
    field = np.random.default_rng(nlev + nxy).standard_normal(nv3d * nxy * nlev)
    x = G.canary_buffer(nv3d * (k + 1) * npts).reshape(nv3d, k + 1, npts)
    buf, off, sp, sm, sv, mask = G.place(x, name)
    o.orc_member_points(I32(0), I32(nlev), I32(nlon), I32(nlat), I32(nv3d), I32(np_), I32(rank), I32(m), dp(field),
                        dp(buf[off:]), I64(nij1), I64(sp), I64(sm), I64(sv))
    want = x.copy()
    want[:, m] = G.member_points_fwd(field, nlev, nxy, nv3d, np_, rank)
    assert G.same_bits(buf, G.place(want, name)[0])
    back = G.canary_buffer(field.size)
    o.orc_member_points(I32(1), I32(nlev), I32(nlon), I32(nlat), I32(nv3d), I32(np_), I32(rank), I32(m), dp(back),
                        dp(buf[off:]), I64(nij1), I64(sp), I64(sm), I64(sv))
    assert G.same_bits(back, G.member_points_back(G.canary_buffer(field.size), want[:, m], nlev, nxy, nv3d, np_, rank))
    own = np.zeros(nxy, bool)
    own[rank::np_] = True
    b = back.reshape(nv3d, nxy, nlev)
    assert G.same_bits(b[:, own], field.reshape(nv3d, nxy, nlev)[:, own]) and np.all(G.bits(b[:, ~own]) == G.CANARY)


def test_member_points_shares():
    got = sorted({G.nij1_of(c[1] * c[2], c[3], c[4]) for c in G.MP_CASES})
    assert got == [1, 31, 32, 33, 100]
    assert sorted({c[0] for c in G.MP_CASES}) == [1, 31, 32, 33, 65]
    assert G.nij1_of(3, 5, 4) == 0 and G.nij1_of(3, 5, 2) == 1


# --------------------------------------------------------------------------------------------------------- state_trans
@pytest.mark.parametrize("assign", G.STATE_ASSIGN)
@pytest.mark.parametrize("nq", G.STATE_NQ)
def test_state_trans_against_the_oracle(nq, assign):
    o = _oracle.oracle()
    for nlev, nlon, nlat in G.STATE_GRIDS:
        n = nlev * nlon * nlat
        for cq, ch in G.CLAMPS:
            c = G.state_consts(assign, nq, cq, ch)
            cs, nv3d = consts_struct(c), c["nv3d"]
            v = G.state_field(c, n, seed=n + nq)
            for inverse in (0, 1):
                src = G.state_inverse_input(c, v) if inverse else v
                got = src.copy()
                o.orc_state_trans(C.byref(cs), I32(nlev), I32(nlon), I32(nlat), I32(nv3d), dp(got), I32(inverse))
                ref = G.state_trans_ld(c, src, bool(inverse))
                wr = G.state_written(c, bool(inverse))
                keep = [s for s in range(nv3d) if s not in wr]
                assert G.same_bits(got[keep], src[keep])
                assert np.all(np.abs(got[wr] - ref[wr]) <= 5e-14 * np.abs(ref[wr]))
                if inverse:
                    for s in G.clamped_species(c):
                        assert np.all(got[s][src[s] < 0] == 0.0) and (n < 255 or (src[s] < 0).any())
    # eight species: POSITIVE_DEFINITE_QHYD clamps the five after iv_q and leaves the 7th and 8th alone
    if nq == 8:
        assert G.clamped_species(G.state_consts(assign, nq, 0, 1)) == [c["iv_q"] + i for i in range(1, 6)]


def test_state_trans_round_trip_statement():
    c = G.state_consts("disjoint", 6)
    v = G.state_field(c, 255, seed=1)
    f = G.state_trans_ld(c, v, False).astype(np.float64)
    b = G.state_trans_ld(c, f, True).astype(np.float64)
    keep = [s for s in range(c["nv3d"]) if s not in G.state_written(c, False)]       # the analysis slots held no state
    assert np.allclose(b[keep], v[keep], rtol=1e-12, atol=1e-18)


# ------------------------------------------------------------------------------------------------ relax_beta, infl_init
@pytest.mark.parametrize("radar_only,bw", G.BETA_FLAGS)
@pytest.mark.parametrize("nlev", [1, 9])
def test_relax_beta_against_the_oracle(radar_only, bw, nlev):
    o = _oracle.oracle()
    p = G.beta_params(radar_only, bw)
    bp = OrcBeta(radar_only, p["radar_zmax"], p["vert_local_radar"], bw, p["dx"], p["dy"], p["ihalo"], p["jhalo"],
                 p["nlong"], p["nlatg"])
    for rig, rjg in (G.beta_points(p), tuple(a[:1] for a in G.beta_points(p))):
        hgt = G.beta_heights(p, nlev, rig.size, seed=nlev)
        want = G.relax_beta(p, rig, rjg, hgt)
        got = np.array([[o.orc_relax_beta(C.byref(bp), C.c_double(rig[i]), C.c_double(rjg[i]), C.c_double(hgt[l, i]))
                         for i in range(rig.size)] for l in range(nlev)])
        assert G.same_bits(got, want)
        z = G.zcut_of(p)
        if radar_only:                                             # at the cut itself the point is still updated
            assert np.all(want[hgt > z] == 0.0) and (hgt == z).any()
            assert bw > 0 or np.all(want[hgt <= z] == 1.0)
    if bw > 0 and not radar_only:
        full = G.relax_beta(p, *G.beta_points(p), np.zeros((1, 16)))[0]
        assert list(full[:4]) == [0.0, 0.0, 1.0, 1.0] and 0 < 1.0 - full[4] < 1e-15 and 0 < full[5] < 1e-12
        assert list(full[6:8]) == [0.0, 0.0]
        assert list(full[8:]) == [1.0, 0.0, 1.0, 0.0, 0.5, 0.25, 0.125, 0.0]


@pytest.mark.parametrize("mul,mn", G.INFL_SIGNS)
@pytest.mark.parametrize("n", [1, 257])
def test_infl_init_against_the_oracle(mul, mn, n):
    w0 = np.random.default_rng(n).uniform(0.7, 1.6, n)
    got = w0.copy()
    _oracle.oracle().orc_infl_init(I64(n), dp(got), C.c_double(mul), C.c_double(mn))
    assert G.same_bits(got, G.infl_init(w0, mul, mn))


# ------------------------------------------------------------------------------------------ additive inflation, weights
def additive_inputs(case, d):
    """(logical anal / add, weight, qmean [nv, npts] or None, ishuf or None) of one ADD_CASES entry"""
    w = d["weight"] if case["weight"] else None
    q = d["gues"][:, d["k"]] if case["qmean"] else None
    return d["anal"], d["add"], w, q, (d["ishuf"] if case["ishuf"] else None)


@pytest.mark.parametrize("ci", range(len(G.ADD_CASES)))
def test_additive_inflation_against_the_oracle(ci):
    case = G.ADD_CASES[ci]
    d = G.additive_case(case["k"], 11, 15, 3, seed=ci)
    k, nv, npts, nij1 = d["k"], d["nv"], d["npts"], d["nij1"]
    anal, add, w, q, sh = additive_inputs(case, d)
    ref, ax = G.additive_ld(anal, add, k, nij1, d["infl_add"], w, q, *case["q"], sh)
    abuf, off, sp, sm, sv, mask = G.place(anal, case["layout"])
    bbuf = G.place(add, case["layout"])[0]
    qa = np.ascontiguousarray(q) if q is not None else None
    _oracle.oracle().orc_additive_inflation(I32(k), I32(nv), I64(npts), I64(nij1), dp(abuf[off:]), dp(bbuf[off:]), I64(sp),
                                            I64(sm), I64(sv), C.c_double(d["infl_add"]), dp(w) if w is not None else None,
                                            dp(qa) if qa is not None else None, I64(1), I64(npts), I32(case["q"][0]),
                                            I32(case["q"][1]), ip(sh) if sh is not None else None)
    got = G.lift(abuf, anal.shape, case["layout"])
    assert np.all(np.abs(got - ref) <= G.additive_bound(anal, ax))
    assert G.same_bits(got[:, k], anal[:, k]) and G.untouched(abuf, mask) and not G.same_bits(got[:, :k], anal[:, :k])


@pytest.mark.parametrize("nob", G.WEIGHT_NOB)
@pytest.mark.parametrize("nij1", G.WEIGHT_NIJ1)
def test_addinfl_weight_against_the_oracle(nij1, nob):
    c = G.weight_case(nij1, nob, seed=nob + nij1)
    d = G.addinfl_weight_d(c["rig"], c["rjg"], c["ob_ri"], c["ob_rj"], c["dx"], c["dy"], c["hori_loc"])
    ref = G.addinfl_weight_ld(d)
    got = np.full(nij1, -5.0)
    _oracle.oracle().orc_addinfl_weight(I64(nij1), dp(c["rig"]), dp(c["rjg"]), I64(nob), dp(c["ob_ri"]), dp(c["ob_rj"]),
                                        C.c_double(c["dx"]), C.c_double(c["dy"]), C.c_double(c["hori_loc"]), dp(got))
    assert np.all(np.abs(got - ref) <= 1e-15 * ref) and np.array_equal(got == 0.0, ref == 0)
    if nob == 0:
        assert not got.any()
    else:
        assert got[c["on_obs"]] == 1.0
    if nob >= 63 and nij1 > 1:
        assert (got == 0).any() and ((got > 0) & (got < 0.01)).any()


def test_the_cut_off_construction_lands_on_the_cut_off():
    h, t_eq, t_far = G.cutoff_construction()
    rig, rjg = np.array([t_eq, t_far, 0.0]), np.zeros(3)
    ob = np.array([0.0, 1000.0])
    d = G.addinfl_weight_d(rig, rjg, ob, ob.copy(), 1.0, 1.0, h)
    assert d[0] == G.CUT2 and d[1] == np.nextafter(G.CUT2, np.inf) and d[2] == 0.0
    w = G.addinfl_weight_ld(d)
    assert w[1] == 0 and w[2] == 1 and abs(float(w[0]) - np.exp(-0.5 * G.CUT2)) < 1e-18
    got = np.full(3, -5.0)
    _oracle.oracle().orc_addinfl_weight(I64(3), dp(rig), dp(rjg), I64(2), dp(ob), dp(ob.copy()), C.c_double(1.0),
                                        C.c_double(1.0), C.c_double(h), dp(got))
    assert got[1] == 0.0 and got[2] == 1.0 and abs(got[0] - float(w[0])) <= 1e-15 * float(w[0])


# ------------------------------------------------------------------------------------------------------------ monit_dep
def orc_monit(table, elm, dep, qc):
    nid = len(table)
    nobs, bias, rmse = np.zeros(nid, np.int32), np.zeros(nid), np.zeros(nid)
    _oracle.oracle().orc_monit_dep(I32(nid), ip(table), I64(len(elm)), ip(elm), dp(dep), ip(qc), ip(nobs), dp(bias), dp(rmse))
    return nobs, bias, rmse


@pytest.mark.parametrize("kind", ["offset", "zero"])
@pytest.mark.parametrize("size", ["one", "n255", "n257", "per257", "ragged"])
@pytest.mark.parametrize("nid", [1, 16, 32])
def test_monit_dep_against_the_oracle(nid, size, kind):
    nn = G.monit_sizes(256)[size]
    table, elm, dep, qc = G.monit_case(nid, nn, kind, seed=nid + nn)
    nobs, bias, rmse = orc_monit(table, elm, dep, qc)
    r_n, r_b, r_ms, r_abs = G.monit_dep_ld(table, elm, dep, qc)
    assert np.array_equal(nobs, r_n)
    has = r_n > 0
    assert np.all(bias[~has] == G.UNDEF) and np.all(rmse[~has] == G.UNDEF)
    # the oracle adds one row after the other: nn - 1 additions and the division for the bias; for the mean square one more,
    # the squares being rounded on their own; the root halves the relative error of its argument and adds one rounding
    assert np.all(np.abs(bias[has] - r_b[has]) <= nn * G.U * r_abs[has])
    assert np.all(np.abs(rmse[has] - np.sqrt(r_ms[has])) <= ((nn + 1) / 2 + 1) * G.U * np.sqrt(r_ms[has]))
    if nid >= 16 and nn > 1000:
        assert nobs[3] == 0 and nobs[9] == 0 and nobs[2] > 0 and nobs[8] > 0          # Tv under T, RE0 under REF
        assert int(nobs.sum()) < int((qc == 0).sum())                                  # ids no table lists count nowhere


def test_monit_chain_lengths():
    assert G.monit_chain(1, 1024) == 1 + 8 + 1024 and G.monit_chain(257 * 1024 - 100, 1024) == 2 + 8 + 1024
    assert G.monit_chain(0, 1024) == 8 + 1024
