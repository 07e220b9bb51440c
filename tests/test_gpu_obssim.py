"""letkf_obssim_dev against the numpy statement of tests/_obssim.py on the seeded grids (two states each): (8, 5, 3) and
(70, 5, 3) with halos 2 (partial waves, a row of 350 lanes, more than 64 levels), (64, 4, 2) (every wave full), (1, 1, 1), and
(8, 5, 3) without horizontal halo under stggrd = 1 (the clamped edge reads).  The lists hold every element Trans_XtoY and
Trans_XtoY_radar serve, the pseudo-RH id, PS in both lists and a radar id in the 2-D list; one column lies exactly on the radar.

Tolerances are the operator's (derived, not tuned: the docstring of tests/test_gpu_obsope.py), carried by tests/_obssim.py:
  Tv; U, V under rotc or stggrd    64 eps sum |w v| of the interpolations behind the value (+ 4 ulp of the rotation)
  PS                               the same bound through prsadj by its derivative, + 64 ulp
  dBZ                              1e-11 absolute
  Vr                               1e-9 (|u| + |v| + |w| + wt); every column but the one ON the radar is at least 0.5 degrees from it
  exact ("pass", "undef", "lowref")  T, Q, RH, and U, V with rotc NULL and stggrd = 0 (the field's own value); undef;
                                   MIN_RADAR_REF_DBZ + LOW_REF_SHIFT: bit for bit
The terrain columns of the fixtures hold -9.99e33 in their two lowest levels and the reference runs its physics on those numbers:
pass-through elements are compared there exactly, radar elements are excluded there -- 2 columns x 2 levels per radar variable and
state, counted -- and nothing else is.  tests/test_obssim_statement.py asserts that no point is within 1e-6 of a comparison.
"""
import math

import numpy as np
import pytest
import torch

import _obsope as O
import _obssim as S

pytestmark = pytest.mark.gpu

CONFIGS_8 = [dict(method_ref_calc=m, use_terminal_velocity=tv, stggrd=s) for m in (1, 2, 3) for tv in (0, 1) for s in (0, 1)]
OTHER = ([("70x5x3", kw) for kw in (dict(method_ref_calc=2, use_terminal_velocity=1, stggrd=0), dict(method_ref_calc=3, use_terminal_velocity=0, stggrd=1))] +
         [("64x4x2", kw) for kw in (dict(method_ref_calc=1, use_terminal_velocity=1, stggrd=1), dict(method_ref_calc=3, use_terminal_velocity=1, stggrd=0))] +
         [("1x1x1", kw) for kw in (dict(method_ref_calc=2, use_terminal_velocity=1, stggrd=0), dict(method_ref_calc=2, use_terminal_velocity=0, stggrd=1))] +
         [("8x5x3-nohalo", kw) for kw in (dict(method_ref_calc=2, use_terminal_velocity=1, stggrd=1), dict(method_ref_calc=3, use_terminal_velocity=0, stggrd=1))])
N_RADAR_3 = sum(1 for e in S.VARS3 if e in S.RADAR_IDS)


@pytest.fixture(scope="module")
def env():
    from _gpu import ctx, pkg
    return pkg, ctx(), torch.device("cuda:0")


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64 if a.dtype == np.float64 else np.int32)


def ident(v):
    return "-".join(f"{k[0]}{x}" for k, x in v.items()) if isinstance(v, dict) else str(v)


@pytest.mark.parametrize("name,kw", [("8x5x3", kw) for kw in CONFIGS_8] + OTHER, ids=ident)
def test_obssim_matches_the_statement(env, name, kw):
    pkg, ctx, dev = env
    case, cfg = S.make_case(name), S.default_cfg(**kw)
    st = S.cached_statement(name, cfg)
    got = S.DeviceCase(pkg, case, cfg, S.VARS3, S.VARS2, dev).run(ctx)
    bad, worst, excluded = S.compare(got["v3"], got["v2"], st)
    print(f"{name} {kw}: worst error / tolerance {worst}, excluded {excluded}")
    assert excluded == case["nterrain"] * S.NSTATE * N_RADAR_3 and (case["nterrain"] == 4 or name == "1x1x1")
    assert bad == []
    # rec is the float of it at the stated index, for every state
    assert np.array_equal(bits(got["rec"]), bits(S.records(got["v3"], got["v2"])))
    g = case["g"]
    nrec = len(S.VARS3) * g["nlev"] + len(S.VARS2)
    flat = got["rec"].ravel()
    for s, n, k, j, i in ((0, 0, 0, 0, 0), (1, 4, g["nlev"] - 1, g["nlat"] - 1, g["nlon"] - 1)):
        assert flat[S.rec_index(s, n * g["nlev"] + k, j, i, nrec, g["nlat"], g["nlon"])] == np.float32(got["v3"][s, n, j, i, k])


@pytest.mark.parametrize("stggrd", [0, 1])
def test_pass_through_values_are_the_input_fields_bits(env, stggrd):
    pkg, ctx, dev = env
    case, cfg = S.make_case("8x5x3"), S.default_cfg(stggrd=stggrd, min_radar_ref_dbz=60.0)
    g = case["g"]
    vars3 = (O.ID_T, O.ID_Q, O.ID_RH, O.ID_U, O.ID_V, O.ID_REF, 1234)
    got = S.DeviceCase(pkg, case, cfg, vars3, (O.ID_T,), dev, rotc=False).run(ctx)
    inner = lambda v: np.transpose(case["v3"][:, v, 2:2 + g["nlat"], 2:2 + g["nlon"], 2:2 + g["nlev"]], (0, 1, 2, 3))
    for n, v in ((0, O.V_T), (1, O.V_Q), (2, O.V_RH)) + (((3, O.V_U), (4, O.V_V)) if stggrd == 0 else ()):
        assert np.array_equal(bits(got["v3"][:, n]), bits(inner(v) + 0.0)), n          # (+ 0.0: the sum's sign of zero)
    assert np.array_equal(bits(got["v2"][:, 0]), bits(inner(O.V_T)[..., 0] + 0.0))
    assert np.array_equal(bits(got["v3"][:, 6]), bits(np.full(got["v3"][:, 6].shape, O.UNDEF)))
    # MIN_RADAR_REF_DBZ = 60: every reflectivity is below it and stores the constant, but for the column on the radar (undef)
    ref = got["v3"][:, 5].copy()
    jr, ir = case["on_radar"]
    assert np.array_equal(bits(ref[:, jr, ir]), bits(np.full(ref[:, jr, ir].shape, O.UNDEF)))
    ref[:, jr, ir] = 55.0
    assert np.array_equal(bits(ref), bits(np.full(ref.shape, 55.0)))


def test_round_single_is_the_float_of_the_double_run_and_undef_is_floats_undef(env):
    pkg, ctx, dev = env
    case, cfg = S.make_case("8x5x3"), S.default_cfg(method_ref_calc=3, stggrd=1)
    d = S.DeviceCase(pkg, case, cfg, S.VARS3, S.VARS2, dev, round_single=0).run(ctx)
    r = S.DeviceCase(pkg, case, cfg, S.VARS3, S.VARS2, dev, round_single=1).run(ctx)
    with np.errstate(over="ignore"):
        for n in ("v3", "v2"):
            assert np.array_equal(bits(r[n]), bits(d[n].astype(np.float32).astype(np.float64)))
    assert np.array_equal(bits(r["rec"]), bits(d["rec"]))
    assert (r["v3"] == float(np.float32(O.UNDEF))).any() and not (r["v3"] == O.UNDEF).any()


@pytest.mark.parametrize("name", ["8x5x3", "70x5x3"])
def test_each_output_alone_gives_the_values_of_all_three_together(env, name):
    pkg, ctx, dev = env
    case, cfg = S.make_case(name), S.default_cfg(stggrd=1)
    dc = S.DeviceCase(pkg, case, cfg, S.VARS3, S.VARS2, dev)
    all3 = dc.run(ctx)
    for want in (("v3",), ("v2",), ("rec",), ("v3", "rec")):
        one = dc.run(ctx, want=want)
        for n in ("v3", "v2", "rec"):
            assert (one[n] is None) == (n not in want)
            if n in want:
                assert np.array_equal(bits(one[n]), bits(all3[n])), (want, n)
    # a list of one kind only: rec without a 3-D list, and without a 2-D list
    only2 = S.DeviceCase(pkg, case, cfg, (), S.VARS2, dev).run(ctx, want=("v2", "rec"))
    assert np.array_equal(bits(only2["v2"]), bits(all3["v2"])) and np.array_equal(bits(only2["rec"]), bits(all3["v2"].astype(np.float32)))
    only3 = S.DeviceCase(pkg, case, cfg, S.VARS3, (), dev).run(ctx, want=("v3", "rec"))
    assert np.array_equal(bits(only3["v3"]), bits(all3["v3"]))
    assert np.array_equal(bits(only3["rec"]), bits(S.records(all3["v3"], all3["v2"][:, :0])))


def test_two_states_in_one_call_equal_two_calls_and_two_calls_give_the_same_bits(env):
    pkg, ctx, dev = env
    case, cfg = S.make_case("70x5x3"), S.default_cfg(method_ref_calc=3)
    dc = S.DeviceCase(pkg, case, cfg, S.VARS3, S.VARS2, dev)
    a, b = dc.run(ctx), dc.run(ctx)
    for n in ("v3", "v2", "rec"):
        assert np.array_equal(bits(a[n]), bits(b[n]))
    for s in range(S.NSTATE):
        one = S.DeviceCase(pkg, case, cfg, S.VARS3, S.VARS2, dev, states=(s, 1)).run(ctx)
        for n in ("v3", "v2", "rec"):
            assert np.array_equal(bits(one[n][0]), bits(a[n][s])), (s, n)


@pytest.mark.parametrize("name", ["8x5x3", "70x5x3"])
def test_the_row_operator_on_the_grid_points_agrees(env, name):
    """The device cross-check: letkf_obsope_dev, tested on its own, on one member with observation rows placed on the interior-level
    grid points (lev = hgt, the point's lon / lat / rotc, radar_zmax = inf) against letkf_obssim_dev, within the derived tolerances."""
    pkg, ctx, dev = env
    case, cfg = S.make_case(name), S.default_cfg(method_ref_calc=2, stggrd=1)
    g = case["g"]
    vars3 = (O.ID_REF, O.ID_VR)
    st = S.cached_statement(name, cfg, vars3, ())
    sim = S.DeviceCase(pkg, case, cfg, vars3, (), dev, states=(0, 1)).run(ctx, want=("v3",))["v3"][0]
    rows, where = {n: [] for n in ("elm", "typ", "lev", "ri", "rj", "lon", "lat")}, []
    rotc = []
    for j in range(g["nlat"]):
        for i in range(g["nlon"]):
            if any((j - dj, i - di) in case["terrain_cols"] for dj in (0, 1) for di in (0, 1)) or (j, i) == case["on_radar"]:
                continue
            for k in range(1, g["nlev"] - 1):
                for n, elm in enumerate(vars3):
                    for key, v in (("elm", elm), ("typ", 1), ("lev", case["v3"][0, O.V_HGT, j + 2, i + 2, k + 2]), ("ri", i + 3.0),
                                   ("rj", j + 3.0), ("lon", case["lon"][j, i]), ("lat", case["lat"][j, i])):
                        rows[key].append(v)
                    rotc.append(case["rotc"][j, i])
                    where.append((n, j, i, k))
    nrow = len(where)
    ocase = dict(g=g, v3=case["v3"][:1], v2=case["v2"][:1], nmem=1, nrow=nrow, off=np.array([0, nrow], dtype=np.int64),
                 files=dict(elm=np.array(rows["elm"], dtype=np.int32), typ=np.array(rows["typ"], dtype=np.int32),
                            **{n: np.array(rows[n], dtype=np.float64) for n in ("lev", "ri", "rj", "lon", "lat")}),
                 set=np.ones(nrow, dtype=np.int32), idx=np.arange(1, nrow + 1, dtype=np.int32), rotc=np.array(rotc),
                 file_radar=np.array([0], dtype=np.int32), radars=np.array([S.RADAR]))
    ocfg = O.default_cfg(method_ref_calc=2, stggrd=1, radar_zmax=math.inf, ri_off=0.0, rj_off=0.0,
                         **{n: cfg[n] for n in ("use_terminal_velocity", "min_radar_ref_dbz", "low_ref_shift", "ps_adjust_thres")})
    val, qc = O.DeviceCase(pkg, ocase, ocfg, dev).run(ctx)
    assert not qc.any()
    worst = 0.0
    for r, (n, j, i, k) in enumerate(where):
        kind, tol = st["kind3"][0, n, j, i, k], st["tol3"][0, n, j, i, k]
        err = abs(val[r, 0] - sim[n, j, i, k])
        assert err == 0.0 if kind in S.EXACT_KINDS else err <= tol, (n, j, i, k, kind, val[r, 0], sim[n, j, i, k], tol)
        worst = max(worst, err / tol if tol > 0 else 0.0)
    print(f"{name}: {nrow} rows, worst |operator - obssim| / tolerance {worst}")
