"""The numpy statement of the departure monitor (tests/_monit.py) against things its author did not write, and the fixture's
distance from every comparison.  No GPU, no library."""
import ctypes as C

import numpy as np
import pytest

import _monit as M
import _obsope as O
import _oracle


@pytest.fixture(scope="module", params=[8, 70])
def case(request):
    return M.case(request.param)


def _both_steps(case, **kw):
    mcfg = M.default_mcfg(**kw)
    s1 = M.monit(case["cfg"], mcfg, case, case["hist"][0], 1, None)
    s2 = M.monit(case["cfg"], mcfg, case, case["hist"][1], 2, s1["rec"])
    return s1, s2


def test_no_fixture_row_is_near_a_comparison(case):
    """no row of either state within 1e-6 relative of a comparison it takes, METHOD_REF_CALC 2 and 3, with and without the time
    range: the cap on excluded rows is zero"""
    for method in (2, 3):
        cfg = dict(case["cfg"], method_ref_calc=method)
        for tr in (0.0, M.T_RANGE):
            mcfg = M.default_mcfg(t_range=tr)
            for hist in case["hist"]:
                st = M.monit(cfg, mcfg, case, hist, 1, None)
                near = np.nonzero(st["dist"] < 1e-6)[0]
                assert near.size == 0, (method, tr, near.tolist(), st["dist"][near].tolist())


def test_the_fixture_covers_what_it_claims(case):
    s1, s2 = _both_steps(case)
    g = case["g"]
    assert 150 <= case["nrow"] <= 260
    tags = {}
    for n, r in enumerate(case["rows"]):
        tags.setdefault(r["tag"], []).append(n)
        assert g["ihalo"] + 0.5 <= r["ri"] - case["cfg"]["ri_off"] < g["ihalo"] + g["nlon"] + 0.5
        assert g["jhalo"] + 0.5 <= r["rj"] - case["cfg"]["rj_off"] < g["jhalo"] + g["nlat"] + 0.5
    qcs = set(s1["qc"].tolist())
    assert {0, O.QC_PS_TER, O.QC_OUT_VHI, O.QC_OUT_VLO, O.QC_OTYPE} <= qcs, qcs
    good_elm = {int(case["rows"][n]["elm"]) for n in np.nonzero(s1["qc"] == 0)[0]}
    assert {O.ID_U, O.ID_V, O.ID_T, O.ID_TV, O.ID_Q, O.ID_RH, O.ID_PS, O.ID_REF, O.ID_REF_ZERO, O.ID_VR} <= good_elm
    assert len(tags["halo"]) >= 16 and all(s1["qc"][n] in (0, O.QC_PS_TER) for n in tags["halo"])
    # good at step 1 and bad at step 2, and the reverse
    assert ((s1["qc"] == 0) & (s2["qc"] != 0)).sum() >= 1 and ((s1["qc"] != 0) & (s2["qc"] == 0)).sum() >= 1
    # the merge rule shows: a row bad at step 1 keeps its qc although step 2 finds it good
    assert (s2["rec"]["qc"] != s2["qc"]).any() and (s2["rec"]["qc"][s1["qc"] == 0] == s2["qc"][s1["qc"] == 0]).all()
    out = np.abs(np.array([r["dif"] for r in case["rows"]])) > M.T_RANGE
    assert 0.1 < out.mean() < 0.3


def test_a_wrong_edge_fill_shows_in_the_halo_and_stagger_rows(case):
    """the rows tagged halo / stagger read a lateral halo column: with the halo left unwritten (NaN) their H(x) is NaN"""
    st = case["gues"]
    v3, v2, _, _ = M.state_to_history(st["state"], st["topo"], st["cz"], st["ztop"], case["g"], 0)
    for n, r in enumerate(case["rows"]):
        if r["tag"] in ("halo", "stagger"):
            o = O.operator(case["cfg"], case["g"], v3, v2, r, tuple(case["rotc"][n]))
            assert o["qc"] != 0 or np.isnan(o["val"]), (n, r["tag"], o)


def test_height_is_cz_over_flat_ground_and_the_halos_repeat(case):
    g, st = case["g"], case["gues"]
    v3, v2, w3, w2 = M.state_to_history(st["state"], np.zeros_like(st["topo"]), st["cz"], st["ztop"], g, 15)
    kh, ih, jh = g["khalo"], g["ihalo"], g["jhalo"]
    assert w3.all() and w2.all()
    assert np.array_equal(v3[O.V_HGT, jh:-jh, ih:-ih, kh:-kh], np.broadcast_to(st["cz"], (g["nlat"], g["nlon"], g["nlev"])))
    for h in range(kh):                                                   # the vertical halo repeats
        assert np.array_equal(v3[..., h], v3[..., kh]) and np.array_equal(v3[..., -1 - h], v3[..., -1 - kh])
    inner3, inner2 = v3[:, jh:-jh, ih:-ih, :], v2[:, jh:-jh, ih:-ih]
    assert np.array_equal(v3, np.pad(inner3, ((0, 0), (jh, jh), (ih, ih), (0, 0)), mode="edge"))
    assert np.array_equal(v2, np.pad(inner2, ((0, 0), (jh, jh), (ih, ih)), mode="edge"))
    assert np.array_equal(v2[O.V2_TOPO], v3[O.V_HGT, :, :, kh]) and not v3[O.V_RH].any() and not v2[O.V2_RAIN].any()
    # a side whose bit is clear is not written, a corner needs both of its sides
    _, _, m3, m2 = M.state_to_history(st["state"], st["topo"], st["cz"], st["ztop"], g, M.WEST | M.SOUTH)
    assert m2[0, :jh + g["nlat"], :ih + g["nlon"]].all() and not m2[0, jh + g["nlat"]:, :].any() and not m2[0, :, ih + g["nlon"]:].any()
    assert np.array_equal(m3[:, :, :, 0], np.broadcast_to(m2[0], m3[:, :, :, 0].shape))


def test_an_affine_state_gives_the_affine_function_and_the_departures_follow():
    """stggrd = 0, T and Q affine in (i, j, z) over flat ground: H(x) is that function at the row's coordinates"""
    g = O.make_grid(8)
    st = M.make_state(g, 5)
    nj, ni, nk = g["nlat"], g["nlon"], g["nlev"]
    topo = np.zeros((nj, ni))
    jj, ii, _ = np.meshgrid(np.arange(nj), np.arange(ni), np.arange(nk), indexing="ij")
    z = np.broadcast_to(st["cz"], (nj, ni, nk))
    s = st["state"].copy()
    s[O.V_P] = 1.0e5 * np.exp(-z / 8000.0)                               # log p linear in z: the level search is exact
    fT = lambda i, j, zz: 300.0 + 0.5 * i - 0.25 * j - 6.5e-3 * zz
    fQ = lambda i, j, zz: 0.01 + 1e-4 * i + 2e-4 * j - 1e-6 * zz
    s[O.V_T], s[O.V_Q] = fT(ii, jj, z), fQ(ii, jj, z)
    v3, v2, _, _ = M.state_to_history(s, topo, st["cz"], st["ztop"], g, 15)
    cfg = O.default_cfg(stggrd=0)
    rng = np.random.default_rng(3)
    for elm, fn in ((O.ID_T, fT), (O.ID_Q, fQ)):
        for _ in range(6):
            ril, rjl = rng.uniform(3.0, 7.0), rng.uniform(3.0, 5.0)       # between interior columns
            zz = rng.uniform(st["cz"][0], st["cz"][-1])
            # z is piecewise linear in the level coordinate and log p linear in z: a target pressure names its height
            row = dict(elm=elm, typ=1, lev=1.0e5 * np.exp(-zz / 8000.0), ri=ril + cfg["ri_off"], rj=rjl + cfg["rj_off"], lon=0.0,
                       lat=0.0, radar=None, dat=1.5, dif=0.0)
            want = fn(ril - 1 - g["ihalo"], rjl - 1 - g["jhalo"], zz)
            o = O.operator(cfg, g, v3, v2, row)
            assert o["qc"] == 0 and abs(o["val"] - want) <= 1e-10 * abs(want), (o, want)
            case = dict(g=g, rows=[row], nrow=1, set=np.array([1], dtype=np.int32), idx=np.array([1], dtype=np.int32),
                        rotc=np.array([[1.0, 0.0]]))
            m = M.monit(cfg, M.default_mcfg(), case, (v3[None], v2[None]), 1, None)
            assert m["qc"][0] == 0 and abs(m["dep"][0] - (1.5 - want)) <= 1e-10 * abs(want)


def test_the_statistics_agree_with_the_oracles_monit_dep(case):
    for st in _both_steps(case) + _both_steps(case, t_range=M.T_RANGE, departure_stat_radar=0):
        nid, nn = len(M.ELEM_UID), len(st["qc"])
        nobs, bias, rmse = np.zeros(nid, dtype=np.int32), np.zeros(nid), np.zeros(nid)
        p = lambda a, t: a.ctypes.data_as(C.POINTER(t))
        elm, dep, qc = (np.ascontiguousarray(st["elm"], dtype=np.int32), np.ascontiguousarray(st["dep"]),
                        np.ascontiguousarray(st["qc"], dtype=np.int32))
        _oracle.oracle().orc_monit_dep(C.c_int(nid), p(M.ELEM_UID, C.c_int32), C.c_int64(nn), p(elm, C.c_int32), p(dep, C.c_double),
                                       p(qc, C.c_int32), p(nobs, C.c_int32), p(bias, C.c_double), p(rmse, C.c_double))
        assert np.array_equal(nobs, st["nobs"]) and nobs.sum() == (st["qc"] == 0).sum()
        assert np.allclose(bias, st["bias"], rtol=1e-13, atol=0) and np.allclose(rmse, st["rmse"], rtol=1e-13, atol=0)


def test_monit_print_has_the_references_shape():
    nobs = np.array([3, 0] + [1] * 14, dtype=np.int32)
    lines = M.monit_print(nobs, np.full(16, -1.2346e-3), np.full(16, 12.5), M.monit_type(M.ELEM_UID, True, False))
    assert lines[0] == "=" * (6 + 12 * 7) and lines[2] == "-" * (6 + 12 * 7) and lines[6] == lines[0]
    assert lines[1] == " " * 6 + "".join(n.rjust(12) for n in ("  U", "  V", "  T", "  Q", " PS", "REF", " Vr"))
    assert lines[3].startswith("BIAS  " + "  -1.235E-03" + "         N/A")
    assert lines[4].startswith("RMSE  " + "   1.250E+01") and lines[5].startswith("NUMBER" + "           3" + "           0")
    assert len(M.monit_print(nobs, nobs * 1.0, nobs * 1.0, M.monit_type(M.ELEM_UID, False, False))[0]) == 6 + 12 * 5
