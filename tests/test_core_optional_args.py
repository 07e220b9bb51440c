"""The letkf_core boundary under every presence pattern of its OPTIONAL arguments (common/common_letkf.f90:52-68): transm,
pao, depd, transmd, rdiag_wloc and infl_update, each present or absent, at nobsl = 0, 1, k - 1, k and 200.  Every output
starts as a sentinel, so "not written" and "written" differ.  What the reference does with transmd (the oracle follows it):
  - transmd present and nobsl == 0: zeros, whether depd is given or not (:97-99);
  - transmd present, depd absent, nobsl > 0: untouched (:188);
  - depd present, transmd absent: nothing is written for it.
The CPU test pins these rules on the oracle; the GPU tests hold the host entry (letkf_core_c) and the batch entry
(letkf_core_batch_dev) to the oracle, pattern by pattern."""
import itertools

import numpy as np
import pytest

import _oracle
from _cases import core_case, relerr

KS = (2, 20, 50, 64, 100, 144)
SENT = -12345.678                      # what an output element holds when the call does not write it
TOL = 1e-11
NAMES = ("transm", "pao", "depd", "transmd", "rdiag_wloc", "infl_update")
PATTERNS = list(itertools.product((False, True), repeat=len(NAMES)))


def nobsl_list(k):
    return sorted({0, 1, k - 1, k, 200})


def pattern_id(p):
    return "".join(n[0:2] if on else "__" for n, on in zip(NAMES, p))


def inputs(k, n, nobs):
    return core_case(k, n, seed=7000 + 13 * k + n, nobs=nobs, rdiag_wloc=True, infl=1.06, with_det=True)


def oracle_core(k, n, c, p, fill=SENT):
    transm, pao, depd, transmd, wloc, iu = p
    return _oracle.letkf_core("oracle", k, c["nobs"], n, c["hdxb"], c["rdiag"], c["rloc"], c["dep"], c["infl"],
                              want_transm=transm, want_pao=pao, rdiag_wloc=True if wloc else None,
                              infl_update=True if iu else None, depd=c["depd"] if depd else None,
                              want_transmd=transmd, fill=fill, transmd_without_depd=True)


def check(got, exp, k, p, n, what):
    """got against the oracle's answer, sentinels included (an element the oracle leaves must be left, and vice versa)"""
    transm, pao, depd, transmd, wloc, iu = p
    ctx = (what, pattern_id(p), k, n)
    assert relerr(got["trans"], exp["trans"]) <= TOL, ctx
    if transm:
        assert np.abs(got["transm"] - exp["transm"]).max() <= TOL * max(1.0, np.abs(exp["transm"]).max()), ctx
    if pao:
        assert relerr(got["pao"], exp["pao"]) <= TOL, ctx
    if transmd:
        e = exp["transmd"]
        if depd and n > 0:
            assert np.abs(got["transmd"] - e).max() <= TOL * max(1.0, np.abs(e).max()), ctx
        else:
            assert np.array_equal(got["transmd"], e), (ctx, got["transmd"][:4], e[:4])
    assert abs(got["parm_infl"] - exp["parm_infl"]) <= 1e-12, ctx


@pytest.mark.parametrize("k", KS)
def test_oracle_transmd_rules(k):
    """The expectation itself, on the CPU: the oracle's transmd under the three rules, and depd without transmd changing
    nothing (every output bit for bit what the same call without depd gives)."""
    for n in nobsl_list(k):
        c = inputs(k, n, max(n, 1) + 3)
        for p in PATTERNS:
            transm, pao, depd, transmd, wloc, iu = p
            r = oracle_core(k, n, c, p)
            assert r["rc"] == 0
            if transmd and n == 0:
                assert (r["transmd"] == 0.0).all(), (pattern_id(p), n)
            elif transmd and not depd:
                assert (r["transmd"] == SENT).all(), (pattern_id(p), n)
            elif transmd:
                assert np.isfinite(r["transmd"]).all() and (r["transmd"] != SENT).any()
            if depd and not transmd:
                q = oracle_core(k, n, c, (transm, pao, False, False, wloc, iu))
                for key in ("trans", "transm", "pao"):
                    if r[key] is not None:
                        assert np.array_equal(r[key], q[key]), (key, pattern_id(p), n)
                assert r["parm_infl"] == q["parm_infl"]
            # outputs the call does not take stay out of it; the ones it takes are written
            assert (r["trans"] != SENT).all()
            if transm:
                assert (r["transm"] != SENT).all()
            if pao:
                assert (r["pao"] != SENT).all()


@pytest.mark.gpu
@pytest.mark.parametrize("k", KS)
def test_host_entry_every_optional_pattern(k):
    """letkf_core_c (the Fortran shim's entry) against the oracle, all 64 presence patterns x the nobsl values."""
    from _gpu import pkg
    for n in nobsl_list(k):
        c = inputs(k, n, max(n, 1) + 3)
        for p in PATTERNS:
            transm, pao, depd, transmd, wloc, iu = p
            exp = oracle_core(k, n, c, p)
            got = pkg.letkf_core_host(k, c["nobs"], n, c["hdxb"], c["rdiag"], c["rloc"], c["dep"], c["infl"],
                                      want_transm=transm, want_pao=pao, rdiag_wloc=True if wloc else None,
                                      infl_update=True if iu else None, depd=c["depd"] if depd else None,
                                      want_transmd=transmd, fill=SENT, transmd_without_depd=True)
            assert got["status"] in (0, 3), (pattern_id(p), n, got["status"])
            check(got, exp, k, p, n, "letkf_core_c")


@pytest.mark.gpu
@pytest.mark.parametrize("k", KS)
def test_batch_entry_every_optional_pattern(k):
    """letkf_core_batch_dev: one batch per presence pattern holding every nobsl value (absent rdiag_wloc / infl_update
    are 0, as in the reference's defaults, :84-87); every output buffer starts as the sentinel."""
    import torch
    from _gpu import ctx, dev
    ns = nobsl_list(k)
    nb, nobs = len(ns), max(ns) + 3
    cases = [inputs(k, n, nobs) for n in ns]
    H = np.stack([c["hdxb"].T for c in cases])           # (k, nobs) C-order == column-major (nobs, k)
    rd, rl, dp, dd = (np.stack([c[key] for c in cases]) for key in ("rdiag", "rloc", "dep", "depd"))
    d_in = [dev(a) for a in (np.array(ns, dtype=np.int32), H, rd, rl, dp, dd)]
    for p in PATTERNS:
        transm, pao, depd, transmd, wloc, iu = p
        full = lambda *shape: torch.full(shape, SENT, dtype=torch.float64, device="cuda")
        trans, t_m, t_pa, t_md = full(nb, k * k), full(nb, k), full(nb, k * k), full(nb, k)
        infl = dev(np.array([c["infl"] for c in cases]))
        status = torch.full((nb,), -1, dtype=torch.int32, device="cuda")
        ctx().core_batch(k, nobs, d_in[0], d_in[1], d_in[2], d_in[3], d_in[4], infl, trans,
                         transm=t_m if transm else None, pao=t_pa if pao else None, depd=d_in[5] if depd else None,
                         transmd=t_md if transmd else None, rdiag_wloc=wloc, infl_update=iu, status=status)
        torch.cuda.synchronize()
        st = status.cpu().numpy()
        T, W, P, WD, I = (x.cpu().numpy() for x in (trans, t_m, t_pa, t_md, infl))
        for b, n in enumerate(ns):
            assert st[b] in (0, 3), (pattern_id(p), n, st[b])
            exp = oracle_core(k, n, cases[b], p)
            got = dict(trans=T[b].reshape(k, k).T, transm=W[b], pao=P[b].reshape(k, k).T, transmd=WD[b], parm_infl=I[b])
            check(got, exp, k, p, n, "letkf_core_batch_dev")
