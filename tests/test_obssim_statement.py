"""The CPU statement of obssim_cal (tests/_obssim.py) anchored without a device: integer coordinates make itpl_3d a pass-through;
on interior levels the statement is bitwise what _obsope.operator gives for an observation row placed on the grid point (the two
share the point physics, not the control flow: the operator searches its level, the statement is handed it); no fixture point
lies close to a comparison; the record index formula against a literal loop in write_grd_mpi's order; PS in the 2-D list."""
import math

import numpy as np
import pytest

import _obsope as ope
import _obssim as sim


def test_itpl_3d_at_integer_coordinates_is_the_fields_own_value():
    case = sim.make_case("8x5x3")
    g = case["g"]
    for v in (ope.V_T, ope.V_QR, ope.V_U):
        f = case["v3"][0, v]
        for j in range(g["nlath"]):
            for i in range(g["nlonh"]):
                for k in range(g["nlevh"]):
                    got, _ = ope.itpl_3d(f, float(k + 1), float(i + 1), float(j + 1))
                    assert got == f[j, i, k]                                       # (-0.0 == 0.0: the sign of zero aside)
                    assert got.hex() == float(f[j, i, k]).hex() or f[j, i, k] == 0.0


@pytest.mark.parametrize("name", ["8x5x3", "70x5x3"])
@pytest.mark.parametrize("stggrd", [0, 1])
def test_statement_equals_the_row_operator_on_grid_points(name, stggrd):
    case = sim.make_case(name)
    g = case["g"]
    cfg = sim.default_cfg(stggrd=stggrd)
    vars3 = (ope.ID_REF, ope.ID_VR, ope.ID_U, ope.ID_V, ope.ID_T, ope.ID_TV, ope.ID_Q, ope.ID_RH)
    st = sim.cached_statement(name, cfg, vars3, ())
    ocfg = ope.default_cfg(stggrd=stggrd, radar_zmax=math.inf, ri_off=0.0, rj_off=0.0)
    n = ncol = 0
    for s in range(sim.NSTATE):
        v3, v2 = case["v3"][s], case["v2"][s]
        for j in range(g["nlat"]):
            for i in range(g["nlon"]):
                # (the operator's level search looks at all four corner columns of CEILING(ri), CEILING(rj), the three of weight 0
                # included: a terrain column among them raises its lowest level)
                if any((j - dj, i - di) in case["terrain_cols"] for dj in (0, 1) for di in (0, 1)) or (j, i) == case["on_radar"]:
                    continue
                ncol += 1
                jj, ii = j + g["jhalo"], i + g["ihalo"]
                for k in range(1, g["nlev"] - 1):                                   # levels 2 .. nlev - 1
                    kk = k + g["khalo"]
                    for m, elm in enumerate(vars3):
                        radar = elm in sim.RADAR_IDS
                        row = dict(elm=elm, typ=1, lev=float(v3[ope.V_HGT if radar else ope.V_P, jj, ii, kk]), ri=float(ii + 1),
                                   rj=float(jj + 1), lon=float(case["lon"][j, i]), lat=float(case["lat"][j, i]),
                                   radar=case["radar"] if radar else None)
                        o = ope.operator(ocfg, g, v3, v2, row, tuple(float(x) for x in case["rotc"][j, i]))
                        assert o["qc"] == 0, (s, j, i, k, elm, o)
                        assert float(o["val"]).hex() == float(st["val3"][s, m, j, i, k]).hex(), (s, j, i, k, elm)
                        n += 1
    assert ncol == sim.NSTATE * (g["nlat"] * g["nlon"] - 6 - 1) and n == ncol * (g["nlev"] - 2) * len(vars3)


@pytest.mark.parametrize("name", list(sim.GRIDS))
def test_no_fixture_point_is_close_to_a_comparison(name):
    worst = math.inf
    for method in (1, 2, 3):
        for stg in (0, 1):
            st = sim.cached_statement(name, sim.default_cfg(method_ref_calc=method, stggrd=stg))
            worst = min(worst, st["dist"])
    print(name, "closest comparison", worst)
    assert worst > 1e-6


def test_rec_index_formula_is_write_grd_mpis_record_order():
    ns, n3, n2, nlev, nlat, nlon = 2, 3, 2, 4, 3, 5
    rng = np.random.default_rng(3)
    val3, val2 = rng.normal(size=(ns, n3, nlat, nlon, nlev)), rng.normal(size=(ns, n2, nlat, nlon))
    nrec = n3 * nlev + n2
    flat = np.zeros(ns * nrec * nlat * nlon, dtype=np.float32)
    for step in range(1, ns + 1):                                                  # obsope_tools.f90:1181-1204
        irec = (nlev * n3 + n2) * (step - 1)
        for n in range(n3):
            for k in range(nlev):
                irec += 1
                flat[(irec - 1) * nlat * nlon:irec * nlat * nlon] = val3[step - 1, n, :, :, k].astype(np.float32).ravel()
        for n in range(n2):
            irec += 1
            flat[(irec - 1) * nlat * nlon:irec * nlat * nlon] = val2[step - 1, n].astype(np.float32).ravel()
    rec = sim.records(val3, val2)
    assert np.array_equal(rec.ravel(), flat)
    for s, n, k, j, i in ((0, 0, 0, 0, 0), (1, 2, 3, 2, 4), (1, 1, 2, 1, 3)):
        assert flat[sim.rec_index(s, n * nlev + k, j, i, nrec, nlat, nlon)] == np.float32(val3[s, n, j, i, k])
    for s, n, j, i in ((0, 0, 0, 0), (1, 1, 2, 4)):
        assert flat[sim.rec_index(s, n3 * nlev + n, j, i, nrec, nlat, nlon)] == np.float32(val2[s, n, j, i])


def test_ps_in_the_2d_list_is_undef_at_a_realistic_threshold_and_a_value_at_1e4():
    case = sim.make_case("8x5x3")
    lo = sim.statement(case, sim.default_cfg(ps_adjust_thres=100.0), (), (ope.ID_PS,))
    hi = sim.statement(case, sim.default_cfg(ps_adjust_thres=1.0e4), (), (ope.ID_PS,))
    assert (lo["val2"] == ope.UNDEF).all() and (lo["kind2"] == "undef").all()
    assert (hi["kind2"] == "ps").all() and (hi["val2"] > 5.0e4).all() and (hi["val2"] < 1.1e5).all()
    g = case["g"]
    j, i = 1, 2
    want = ope.prsadj(case["v2"][0, ope.V2_PS, j + 2, i + 2], float(1 + g["khalo"]) - case["v2"][0, ope.V2_TOPO, j + 2, i + 2],
                      case["v2"][0, ope.V2_T2M, j + 2, i + 2], case["v2"][0, ope.V2_Q2M, j + 2, i + 2])
    assert hi["val2"][0, 0, j, i] == want
