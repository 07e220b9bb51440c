"""The C restatement against the reference's own Fortran (letkf_core, mtx_eigen): the reference's answers were computed by
its routines compiled into oracle/_ref and are stored in tests/golden/reference_checks.npz (tests/golden/make_golden.py),
the inputs come from tests/_cases.py."""
import os

import numpy as np
import pytest

import _oracle
from _cases import (REF_CORE_MODES, REF_CORE_SHAPES, REF_EIGEN_SIZES, array_sha, case_sha, ref_core_inputs,
                    ref_core_name, ref_eigen_input, relerr)


@pytest.fixture(scope="module")
def ref():
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_checks.npz"))


@pytest.mark.parametrize("k,n", REF_CORE_SHAPES)
@pytest.mark.parametrize("wloc,iu,det", REF_CORE_MODES)
def test_letkf_core(ref, k, n, wloc, iu, det):
    c = ref_core_inputs(k, n, wloc, det)
    nm = ref_core_name(k, n, wloc, iu, det)
    assert case_sha(c) == bytes(ref[nm + "/sha"]).hex(), "input generator drifted from the committed fixture"
    kw = dict(rdiag_wloc=wloc, infl_update=iu, depd=c["depd"], want_transmd=det)
    b = _oracle.letkf_core("oracle", k, c["nobs"], n, c["hdxb"], c["rdiag"], c["rloc"], c["dep"], c["infl"], **kw)
    for key in ("trans", "pao", "transm"):
        assert relerr(b[key], ref[f"{nm}/{key}"]) <= 1e-13, key
    if det:
        assert relerr(b["transmd"], ref[nm + "/transmd"]) <= 1e-13
    assert abs(float(ref[nm + "/parm_infl"][0]) - b["parm_infl"]) <= 1e-14


@pytest.mark.parametrize("n", REF_EIGEN_SIZES)
def test_mtx_eigen(ref, n):
    a = ref_eigen_input(n)
    assert np.array_equal(array_sha(a), ref[f"eigen/n{n}/sha"]), "input generator drifted from the committed fixture"
    w1, v1, nr1 = ref[f"eigen/n{n}/w"], ref[f"eigen/n{n}/v"], int(ref[f"eigen/n{n}/nr"][0])
    w2, v2, nr2, rc = _oracle.mtx_eigen("oracle", a)
    assert rc == 0 and nr1 == nr2 == n
    assert np.all(np.diff(w1) <= 0), "descending order (common/common_mtx.f90:93-96)"
    assert relerr(w2, w1) <= 1e-14
    assert relerr(v2, v1) <= 1e-12
