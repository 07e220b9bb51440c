"""The numpy statement of obsope_cal's first scan (tests/_obsscan.py) without a device: the vectorised scan() against the literal
row-by-row transcription of the reference's loops on small inputs, and the properties the lists and tables must have."""
import numpy as np
import pytest

import _obsscan as S

CASES = {
    "edges": lambda: S.edge_case(),
    "edges T=0.3": lambda: S.edge_case(slots=(1, 3, 2, 0.3)),
    "run 1 0 1": lambda: S.edge_case(file_rows=(40, 7, 300), run=[1, 0, 1]),
    "run 0 0 0": lambda: S.edge_case(run=[0, 0, 0]),
    "no rows": lambda: S.edge_case(file_rows=(0, 0)),
    "one bucket": lambda: S.spread_case(500, (3, 5, 2, 2, 1, 1), (1, 1, 1, 600.0), True),
    "all buckets": lambda: S.spread_case(2000, S.LAYOUT, S.SLOTS, False, file_rows=(900, 0, 1100)),
    "slots 4..9": lambda: S.spread_case(700, (7, 4, 0, 3, 2, 5), (4, 9, 6, 37.5), False),
}


@pytest.fixture(scope="module", params=list(CASES))
def both(request):
    case = CASES[request.param]()
    return case, S.scan(case), S.scan_literal(case)


def test_the_vectorised_statement_is_the_literal_one(both):
    case, got, want = both
    S.assert_same_bits(got, want)


def test_the_lists_are_a_permutation_of_the_running_files_rows(both):
    case, st, _ = both
    off, run = case["off"], case.get("run")
    want = sorted((f + 1, r + 1) for f in range(len(off) - 1) if run is None or run[f] for r in range(int(off[f + 1] - off[f])))
    assert sorted(zip(st["set"].tolist(), st["idx"].tolist())) == want
    assert len(st["qc"]) == len(want) == S.list_rows(case)


def test_bsna_is_the_running_sum_of_bsn_across_subdomains(both):
    case, st, _ = both
    flat = np.concatenate([[0], np.cumsum(st["bsn"].reshape(-1))])
    nb = st["bsn"].shape[1]
    for ip in range(st["bsn"].shape[0]):
        assert np.array_equal(st["bsna"][ip], flat[ip * nb:ip * nb + nb + 1]), ip
    assert st["bsna"][-1, -1] == S.list_rows(case)
    assert st["bsn"][1:, -1].sum() == 0              # outside the domain: booked under subdomain 0 only


def test_every_bucket_holds_its_own_rows_in_file_then_row_order(both):
    case, st, _ = both
    s0 = case["slots"][0]
    off = case["off"]
    for ip in range(st["bsn"].shape[0]):
        for islot in range(s0, s0 + st["bsn"].shape[1]):
            first, count = S.rows_of(st["bsna"], s0, ip, islot)
            assert count == st["bsn"][ip, islot - s0]
            pairs = list(zip(st["set"][first:first + count].tolist(), st["idx"][first:first + count].tolist()))
            assert pairs == sorted(pairs), (ip, islot)
            flat = np.array([off[f - 1] + r - 1 for f, r in pairs], dtype=np.int64)
            assert np.all(st["slot"][flat] == islot), (ip, islot)
            assert np.all(np.maximum(st["rank"][flat], 0) == ip), (ip, islot)
            want_qc = 0 if islot <= case["slots"][1] else S.IQC_TIME if islot == case["slots"][1] + 1 else S.IQC_OUT_H
            assert np.all(st["qc"][first:first + count] == want_qc), (ip, islot)
        first, count = S.rows_of(st["bsna"], s0, ip, 0)
        assert (first, count) == (st["bsna"][ip, 0], st["bsn"][ip].sum())


def test_the_edge_case_reaches_every_bucket_kind_and_every_rank():
    case = S.edge_case()
    assert case["off"][-1] >= S.edge_rows_needed()
    st = S.scan(case)
    assert set(st["rank"].tolist()) == set(range(-1, 6))
    assert set(st["slot"].tolist()) == {1, 2, 3, 4, 5}
    assert np.isnan(case["ri"]).any() and np.isinf(case["rj"]).any() and np.isnan(case["dif"]).any()


def test_slot_edges_round_as_the_ceiling_formula_says():
    """dif = (s - base - 0.5) * T belongs to slot s - 1's upper end... unless the division rounds across: whatever it does, the
    statement is the formula evaluated in double, and at T = 600 the edges are exact"""
    slots = (1, 3, 2, 600.0)
    dif = np.array([-900.0, np.nextafter(-900.0, np.inf), -300.0, np.nextafter(-300.0, np.inf), 900.0, np.nextafter(900.0, np.inf)])
    assert S.slot_of(dif, np.zeros(6, dtype=np.int32), slots).tolist() == [4, 1, 1, 2, 3, 4]
