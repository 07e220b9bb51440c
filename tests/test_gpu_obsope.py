"""letkf_obsope_dev against the numpy statement of tests/_obsope.py on the seeded fixtures (about 300 obsda rows x 3 members,
nlev = 8 and nlev = 70): every element of both formats, the qc paths, terrain, exact bounds, the domain's edges, the three
reflectivity methods with and without terminal velocity, stggrd 0 and 1.

Tolerances (derived, not tuned; tests/_obsope.py operator() computes them per row and member):
  qc                      equal everywhere
  U, V, T, Tv, Q, RH      64 eps sum |w_c v_c| of the interpolations behind the value (an 8-term sum of triple products)
  PS                      the same bound on the four 2-D interpolations, carried through prsadj by its derivative, + 64 ulp
  dBZ                     1e-11 absolute: ~100 eps relative in ref is 4.34 * 100 eps ~ 1e-13; the margin of 100 is for pow and
                          log10 differences between libm and the device
  Vr                      1e-9 (|u| + |v| + |w| + wt).  Every radar row of the fixtures is at least 0.1 degrees from its radar:
                          a few-ulp difference in cosd is amplified by 1 / sin(theta) <= 600 into ~5e-13 rad of the arc and
                          ~1.5e-10 rad of the elevation; the azimuth's error is of the order of eps.  If a row exceeds the
                          tolerance the restatement or the kernel is wrong: the tolerance stays.
  exact values            0.0 where qc stopped before Trans_XtoY*, undef, MIN_RADAR_REF_DBZ + LOW_REF_SHIFT: bit for bit
tests/test_obsope_statement.py asserts that no row of these fixtures is within 1e-6 of a comparison, so none is excluded.
"""
import numpy as np
import pytest
import torch

import _obsope as O

pytestmark = pytest.mark.gpu

CONFIGS_8 = [dict(method_ref_calc=m, use_terminal_velocity=tv, stggrd=s) for m in (1, 2, 3) for tv in (0, 1) for s in (0, 1)]
CONFIGS_70 = [dict(method_ref_calc=2, use_terminal_velocity=1, stggrd=0), dict(method_ref_calc=3, use_terminal_velocity=0, stggrd=1)]
_CASES = {}


def case_of(nlev):
    if nlev not in _CASES:
        _CASES[nlev] = O.make_case(nlev)
    return _CASES[nlev]


@pytest.fixture(scope="module")
def env():
    from _gpu import ctx, pkg
    return pkg, ctx(), torch.device("cuda:0")


def bits(a):
    return np.ascontiguousarray(a).view(np.int64)


@pytest.mark.parametrize("nlev,kw", [(8, kw) for kw in CONFIGS_8] + [(70, kw) for kw in CONFIGS_70],
                         ids=lambda v: "-".join(f"{k[0]}{x}" for k, x in v.items()) if isinstance(v, dict) else str(v))
def test_operator_matches_the_statement(env, nlev, kw):
    pkg, ctx, dev = env
    case, cfg = case_of(nlev), O.default_cfg(**kw)
    st = O.statement(case, cfg)
    val, qc = O.DeviceCase(pkg, case, cfg, dev).run(ctx)
    kinds = st["kind"]
    worst = {}
    for kind in ("interp", "ps", "dbz", "vr"):
        sel = kinds == kind
        if sel.any():
            worst[kind] = float(np.max(np.abs(val - st["val"])[sel] / np.maximum(st["tol"][sel], 1e-300)))
    print(f"nlev {nlev} {kw}: worst error / tolerance {worst}, qc mismatches {int((qc != st['qc']).sum())}")
    assert O.compare(val, qc, st) == []


def test_two_calls_give_the_same_bits(env):
    pkg, ctx, dev = env
    case, cfg = case_of(8), O.default_cfg(method_ref_calc=3)
    dc = O.DeviceCase(pkg, case, cfg, dev)
    v1, q1 = dc.run(ctx)
    v2, q2 = dc.run(ctx)
    assert np.array_equal(bits(v1), bits(v2)) and np.array_equal(q1, q2)


def test_member_by_member_calls_give_the_bits_and_qc_of_one_call(env):
    pkg, ctx, dev = env
    case, cfg = case_of(8), O.default_cfg(method_ref_calc=2)
    k, nrow = case["nmem"], case["nrow"]
    v_all, q_all = O.DeviceCase(pkg, case, cfg, dev).run(ctx)
    ens = torch.zeros((nrow, k), dtype=torch.float64, device=dev)
    qc = torch.zeros(nrow, dtype=torch.int32, device=dev)
    for m in range(k):
        O.DeviceCase(pkg, case, cfg, dev, members=(m, 1)).run(ctx, kld=k, m0=m, qc=qc, ensval=ens)
    assert np.array_equal(bits(ens.cpu().numpy()), bits(v_all))
    assert np.array_equal(qc.cpu().numpy(), q_all)


def test_nothing_outside_the_slots_and_the_row_range_is_written(env):
    pkg, ctx, dev = env
    case, cfg = case_of(8), O.default_cfg()
    k, nrow = case["nmem"], case["nrow"]
    canary = -1.2345e300
    v_all, q_all = O.DeviceCase(pkg, case, cfg, dev).run(ctx)
    row0, nrows, m0, kld = 17, 101, 2, k + 4
    qc0 = torch.full((nrow,), 7, dtype=torch.int32, device=dev)
    got, qc = O.DeviceCase(pkg, case, cfg, dev).run(ctx, kld=kld, m0=m0, row0=row0, nrows=nrows, qc=qc0, canary=canary)
    want = np.full((nrow, kld), canary)
    want[row0:row0 + nrows, m0:m0 + k] = v_all[row0:row0 + nrows]
    assert np.array_equal(bits(got), bits(want))
    want_qc = np.full(nrow, 7, dtype=np.int32)
    want_qc[row0:row0 + nrows] = np.maximum(7, q_all[row0:row0 + nrows])         # qc is INOUT: merged by maximum
    assert np.array_equal(qc, want_qc)


def test_a_nan_at_zero_weight_corners_and_in_the_lowest_halo_level_reaches_no_output(env):
    """The rows on integer ri, rj and an exact level bound put all their weight on one column (and, at the lower bound, on one
    level).  NaN goes into level index 0 of every column (a halo level no weight reaches), into the other three corner columns
    of those rows and into the level below an exact lower bound -- in every variable but the two the level scan reads in all four
    columns.  Those rows keep the bits of the clean run; what other rows make of the NaNs is not looked at."""
    pkg, ctx, dev = env
    case, cfg = case_of(8), O.default_cfg(method_ref_calc=2)
    g = case["g"]
    v_clean, q_clean = O.DeviceCase(pkg, case, cfg, dev).run(ctx)
    v3 = case["v3"].copy()
    others = [v for v in range(O.NV3DD) if v not in (O.V_P, O.V_HGT)]
    v3[..., 0] = np.nan
    exact_rows, lower = [], 0
    for n, row in enumerate(case["rows"]):
        if row["tag"] != "exact":
            continue
        exact_rows.append(n)
        i, j = int(row["ri"] - cfg["ri_off"]) - 1, int(row["rj"] - cfg["rj_off"]) - 1     # 0-based column that carries the weight
        for v in others:
            v3[:, v, j - 1, i, :] = v3[:, v, j, i - 1, :] = v3[:, v, j - 1, i - 1, :] = np.nan
        col = case["v3"][0, O.V_HGT if row["radar"] else O.V_P, j, i]
        k = int(np.nonzero(col == row["lev"])[0][0])
        if k == g["khalo"] + (2 if (i, j) in O.TERRAIN_COLS else 0):                       # exact lower bound: weight 0 on k - 1
            for v in others:
                v3[0, v, j, i, k - 1] = np.nan
            lower += 1
    assert len(exact_rows) == 12 and lower == 6
    val, qc = O.DeviceCase(pkg, dict(case, v3=v3), cfg, dev).run(ctx)
    assert np.isfinite(v_clean[exact_rows, 0]).all() and (q_clean[exact_rows] < 90).all()
    assert np.array_equal(bits(val[exact_rows, 0]), bits(v_clean[exact_rows, 0]))           # (the levels were placed with member 0)
    assert np.array_equal(qc[exact_rows], q_clean[exact_rows])
