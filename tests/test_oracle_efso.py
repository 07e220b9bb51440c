"""CPU checks of the numpy restatement of das_efso (tests/_efso.py, scale/letkf/letkf_tools.f90:1158-1302) on the
oracle's obs_local lists (tests/_search.py:oracle_csr): the point-by-point loop equals the dense matrix form."""
import numpy as np
import pytest

import _efso
from _search import build_case, host_struct, oracle_csr


@pytest.mark.parametrize("k,nterm,term", [(5, 3, [0, 0, 1, 2, -1, -1, 1]), (3, 1, [0, -1, 0]), (8, 4, [3, 2, 1, 0, 3])])
def test_loop_equals_dense_form(k, nterm, term):
    case = build_case(41, nobs_per_ctype=(300, 100, 120, 60), npts=40)
    h, keep = host_struct(case)
    p = case["pts"]
    off, idx, rd, rl, _ = oracle_csr(h, p["ri"], p["rj"], p["rlev"], p["rz"])
    assert off[-1] > 200
    rng = np.random.default_rng(k)
    nv = len(term)
    fcst, fcer, ya, _ = _efso.inputs(rng, 40, k, nv, case["nobs"])
    loop, scale = _efso.efso_loop(off, idx, rd, rl, ya, fcst, fcer, term, nterm)
    dense = _efso.efso_dense(off, idx, rd, rl, ya, fcst, fcer, term, nterm)
    assert np.abs(loop).max() > 0
    assert _efso.within(loop, dense, scale, 1e-13) < 1e-13


def test_var_mask_splits_the_sum():
    """two variable classes with the same lists add up to one call over all variables"""
    case = build_case(42, nobs_per_ctype=(200, 50, 80, 40), npts=30)
    h, keep = host_struct(case)
    p = case["pts"]
    off, idx, rd, rl, _ = oracle_csr(h, p["ri"], p["rj"], p["rlev"], p["rz"])
    term = [0, 1, 1, 2, 0, -1]
    fcst, fcer, ya, _ = _efso.inputs(np.random.default_rng(3), 30, 6, 6, case["nobs"])
    full, scale = _efso.efso_loop(off, idx, rd, rl, ya, fcst, fcer, term, 3)
    a, _ = _efso.efso_loop(off, idx, rd, rl, ya, fcst, fcer, term, 3, var_mask=0b000111)
    b, _ = _efso.efso_loop(off, idx, rd, rl, ya, fcst, fcer, term, 3, var_mask=0b111000, djdy=a)
    assert _efso.within(b, full, scale, 1e-13) < 1e-13
