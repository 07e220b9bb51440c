"""tools/sim_warm_order.py, the "pair" hand-over (sorted by eigenvalue, then rank r at line position r ^ 1): the order is a
permutation of the line, columns without an eigenvector stay last, only whole pairs of valid ranks swap (the last valid rank of
an odd count keeps its position), and the "sorted" order is what it was."""
import importlib.util
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def sim():
    spec = importlib.util.spec_from_file_location("sim_warm_order", os.path.join(ROOT, "tools", "sim_warm_order.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def lines(k):
    """(lam, valid) of a line of (k + 1) & ~1 columns: all k valid (odd k: the inert zero column somewhere on the line), a tie,
    and a line that lost further columns (zero columns at several positions)."""
    ncol = (k + 1) & ~1
    rng = np.random.default_rng(100 + k)
    for nzero in (ncol - k, ncol - k + 1, ncol - k + 2, ncol - 1):
        if nzero >= ncol:
            continue
        lam = rng.uniform(1.0, 50.0, size=ncol)
        lam[rng.choice(ncol, size=nzero, replace=False)] = 0.0
        nz = np.flatnonzero(lam > 0.0)
        if len(nz) >= 3:
            lam[nz[2]] = lam[nz[0]]                      # a tie: broken by position
        yield lam, lam > 0.0


@pytest.mark.parametrize("k", [3, 20, 49, 50])
def test_pair_hand_over_is_a_permutation_with_invalid_columns_last(sim, k):
    for lam, valid in lines(k):
        ncol, nvalid = len(lam), int(valid.sum())
        srt = sim.hand_over_order(lam, valid, "sorted")
        par = sim.hand_over_order(lam, valid, "pair")
        assert np.array_equal(sim.hand_over_order(lam, valid, "sit"), np.arange(ncol))
        for order in (srt, par):
            assert sorted(order.tolist()) == list(range(ncol))
            assert valid[order[:nvalid]].all() and not valid[order[nvalid:]].any()
        # sorted: eigenvalue descending, ties by position
        key = [(-lam[c], c) for c in srt[:nvalid]]
        assert key == sorted(key)
        assert np.array_equal(srt[nvalid:], np.sort(srt[nvalid:]))
        # pair: rank r sits at r ^ 1 where both ranks of the pair are valid, else at r
        for r in range(ncol):
            pos = r ^ 1 if max(r, r ^ 1) < nvalid else r
            assert par[pos] == srt[r], (k, nvalid, r)
        if nvalid % 2:
            assert par[nvalid - 1] == srt[nvalid - 1]
        assert np.array_equal(par[nvalid:], srt[nvalid:])


def test_hand_over_reorders_columns_only(sim):
    rng = np.random.default_rng(5)
    G = rng.standard_normal((7, 8))
    G[:, 3] = 0.0
    cols = {}
    for mode in sim.MODES:
        Q = sim.hand_over(G.copy(), mode)
        assert Q.shape == G.shape
        zero = 3 if mode == "sit" else 7
        assert not Q[:, zero].any() and np.allclose(np.delete((Q * Q).sum(0), zero), 1.0)
        cols[mode] = sorted(map(tuple, np.round(Q.T, 12)))
    assert cols["sit"] == cols["sorted"] == cols["pair"]
