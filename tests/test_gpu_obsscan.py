"""letkf_obsscan_dev against the numpy statement of obsope_cal's first scan (tests/_obsscan.py): every integer output bit for bit
-- rank, slot and own per file row, set / idx / qc per list row, bsn and bsna -- on the edges of the domain, of every subdomain
and of every slot, on files that do not run, on one bucket that holds 70 001 rows (stability across blocks and sort tiles) and on
10 800 buckets that are nearly all empty."""
import ctypes as C

import numpy as np
import pytest
import torch

import _obsscan as S

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env():
    from _gpu import ctx, pkg
    return pkg, ctx(), torch.device("cuda:0")


def run(env, case, myrank_d=0):
    pkg, ctx, dev = env
    p, f, o, out, keep = S.raw_call(pkg, case, dev, myrank_d)
    rc = pkg.obsscan_lib().letkf_obsscan_dev(ctx._c, C.byref(p), C.byref(f), C.byref(o))
    assert rc == 0, pkg.lib().letkf_amd_last_error()
    torch.cuda.synchronize()
    n, nlist = int(case["off"][-1]), S.list_rows(case)
    for name, length in (("set", nlist), ("idx", nlist), ("qc", nlist), ("rank", n), ("slot", n), ("own", n)):
        assert bool((out[name][length:] == S.CANARY).all()), name            # nothing past the end
    return S.host(out, case)


@pytest.mark.parametrize("tint", [600.0, 0.3])
@pytest.mark.parametrize("flags", [(1, 1, 1), (1, 0, 1), (0, 0, 0)])
def test_edges_of_domain_subdomains_and_slots(env, tint, flags):
    case = S.edge_case(file_rows=(0, 7, 300), run=list(flags), slots=(1, 3, 2, tint))
    assert case["off"][-1] >= S.edge_rows_needed()
    S.assert_same_bits(run(env, case, myrank_d=4), S.scan(case, myrank_d=4))


def test_obsda_run_null_is_all_true(env):
    case = S.edge_case(file_rows=(0, 7, 300), run=None)
    want = S.scan(dict(case, run=[1, 1, 1]), myrank_d=0)
    S.assert_same_bits(run(env, case), want)


def test_files_that_run_between_files_that_do_not(env):
    case = S.edge_case(file_rows=(150, 0, 7, 150), run=[0, 1, 1, 0])
    S.assert_same_bits(run(env, case), S.scan(case, myrank_d=0))


def test_zero_rows_in_total(env):
    pkg, ctx, dev = env
    case = S.edge_case(file_rows=(0, 0, 0))
    S.assert_same_bits(run(env, case), S.scan(case, myrank_d=0))
    # ... and with the device arrays NULL
    p, f, o, out, keep = S.raw_call(pkg, case, dev)
    f.ri = f.rj = p.dif = None
    for name in ("set", "idx", "qc", "rank", "slot", "own"):
        setattr(o, name, None)
    assert pkg.obsscan_lib().letkf_obsscan_dev(ctx._c, C.byref(p), C.byref(f), C.byref(o)) == 0, pkg.lib().letkf_amd_last_error()
    assert not out["bsn"].any() and not out["bsna"].any()


@pytest.mark.parametrize("one_bucket", [True, False])
def test_70001_rows_in_one_bucket_and_over_all_30(env, one_bucket):
    layout, slots = ((3, 5, 2, 2, 1, 1), (1, 1, 1, 600.0)) if one_bucket else ((3, 5, 2, 2, 3, 2), (1, 3, 2, 600.0))
    case = S.spread_case(70001, layout, slots, one_bucket, file_rows=(30000, 0, 40001))
    want = S.scan(case, myrank_d=0)
    if one_bucket:
        assert want["bsn"][0, 0] == 70001
    else:
        assert want["bsn"].size == 30 and (want["bsn"][:, :4] > 0).all() and want["bsn"][0, 4] > 0
    S.assert_same_bits(run(env, case), want)


def test_10800_buckets_most_of_them_empty(env):
    layout, slots = (4, 3, 1, 2, 40, 30), (3, 9, 5, 60.0)
    case = S.spread_case(5000, layout, slots, False, seed=13, file_rows=(1, 4999))
    want = S.scan(case, myrank_d=1199)
    assert want["bsn"].size == 10800 and (want["bsn"] == 0).sum() > 5800
    S.assert_same_bits(run(env, case, myrank_d=1199), want)


def test_two_calls_give_equal_bits(env):
    case = S.spread_case(70001, S.LAYOUT, S.SLOTS, False, seed=3)
    a, b = run(env, case), run(env, case)
    S.assert_same_bits(a, b)


def test_the_python_entry_and_the_host_helpers(env):
    pkg, ctx, dev = env
    case = S.edge_case(file_rows=(0, 7, 300), run=[1, 0, 1])
    want = S.scan(case, myrank_d=2)
    p, f, o, out, keep = S.raw_call(pkg, case, dev)
    got = ctx.obsscan(f, keep[1]["dif"], case["layout"], case["slots"], obsda_run=case["run"], myrank_d=2)
    torch.cuda.synchronize()
    S.assert_same_bits({k: (v if isinstance(v, np.ndarray) else v.cpu().numpy()) for k, v in got.items()}, want)
    s0, s1, base, tint = case["slots"]
    for ip in range(6):
        for islot in [0] + list(range(s0, s1 + 3)):
            assert pkg.obsscan_rows(got["bsna"], s0, ip, islot) == S.rows_of(want["bsna"], s0, ip, islot)
    lb, ub = pkg.obsscan_slot_bounds(s0, s1, base, 0.3)
    for s in range(s0, s1 + 1):                                              # obsope_tools.f90:317-318
        assert lb[s - s0] == (float(s - base) - 0.5) * 0.3 and ub[s - s0] == (float(s - base) + 0.5) * 0.3
    for bad, word in (((got["bsna"], s0, 6, 0), "ip"), ((got["bsna"], s0, 0, s1 + 3), "islot"), ((got["bsna"], 0, 0, 0), "slot_start")):
        with pytest.raises(pkg.LetkfError, match=word):
            pkg.obsscan_rows(*bad)
    with pytest.raises(pkg.LetkfError, match="slot_tinterval"):
        pkg.obsscan_slot_bounds(1, 3, 2, float("nan"))
