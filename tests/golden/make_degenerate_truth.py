#!/usr/bin/env python3
"""Generate tests/golden/degenerate_truth.npz and tests/golden/degenerate_reference.npz: for the observation classes of
tests/_degenerate.py (truth_cases()) a high-precision solution of letkf_core's equations, and what the reference's own letkf_core
answers on the same inputs (two files, 0.68 MB and 0.40 MB: one file of both would be 1.07 MB, above the 1 MiB this repository
allows a newly committed file).

The truth is computed with mpmath at 50 digits straight from the equations, with rdiag holding the localised error variance:

    A = Y^T R^-1 Y + (k - 1) / rho I,   Pa = A^-1,   w = Pa Y^T R^-1 d,   w_d = Pa Y^T R^-1 d_det,   T = sqrt(k - 1) A^(-1/2)

through the symmetric eigen-decomposition of A in that precision (any orthonormal basis of a degenerate eigenspace gives the same
Pa and T).  Stored as FP64: the upper triangles of T and Pa for k <= 50, their products with _cases.probes(k) and their diagonals
for k >= 64, w, w_d, cond(A) and an array_sha of the inputs.

The reference's answers (trans, pao, transm, transmd, and parm_infl with infl_update) come from oracle/_ref through
tests/_oracle.py and are stored the same way (triangles for k <= 20, probes and diagonals above); only numbers are stored.
Needs mpmath, and the compiled reference for the second half (without it the stored reference answers are carried over):

    make -C oracle ref && python tests/golden/make_degenerate_truth.py [k ...]
"""
import multiprocessing
import os
import resource
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from _cases import probes  # noqa: E402
from _degenerate import inputs_sha, load_store, pack_store, truth_cases, truth_name, truth_problem, tri  # noqa: E402

DIGITS = 50
PROBE_FROM = 64        # k x k outputs of k >= 64 are stored through probes
REF_FULL_TO = 20       # the reference's k x k answers are stored whole up to k = 20


def truth(c):
    """(T, Pa, w, w_d, cond) of one problem, FP64 copies of the 50-digit solution"""
    import mpmath as mp
    mp.mp.dps = DIGITS
    k, n = c["k"], c["n"]
    y = [[mp.mpf(float(v)) for v in row] for row in c["hdxb"][:n]]
    rinv = [1 / mp.mpf(float(v)) for v in c["rdiag"][:n]]
    a = mp.zeros(k, k)
    for i in range(k):
        for j in range(i, k):
            s = mp.fsum(y[r][i] * rinv[r] * y[r][j] for r in range(n))
            a[i, j] = s
            a[j, i] = s
    shift = mp.mpf(k - 1) / mp.mpf(c["infl"])
    for i in range(k):
        a[i, i] += shift
    ev, q = mp.eigsy(a)
    assert min(ev) > 0
    cond = float(max(ev) / min(ev))
    qi = q * mp.diag([1 / e for e in ev])
    qs = q * mp.diag([mp.sqrt(mp.mpf(k - 1) / e) for e in ev])
    qt = q.T
    pa = qi * qt
    t = qs * qt
    out = []
    for d in (c["dep"], c["depd"]):
        rhs = mp.matrix([mp.fsum(y[r][i] * rinv[r] * mp.mpf(float(d[r])) for r in range(n)) for i in range(k)])
        out.append(np.array([float(v) for v in pa * rhs]))
    f = lambda m: np.array([[float(m[i, j]) for j in range(k)] for i in range(k)])
    return f(t), f(pa), out[0], out[1], cond


def pack(out, nm, key, m, full):
    if full:
        out[f"{nm}/{key}"] = tri(m)
    else:
        k = m.shape[0]
        out[f"{nm}/{key}_probe"] = (m @ probes(k)).ravel()
        out[f"{nm}/{key}_diag"] = np.diag(m).copy()
        out[f"{nm}/{key}_absmax"] = np.array([np.abs(m).max()])


def one(case):
    cls, k, n = case
    t0 = time.time()
    c = truth_problem(cls, k, n)
    nm = truth_name(cls, k, n)
    T, Pa, w, wd, cond = truth(c)
    out = {nm + "/sha": inputs_sha(c).astype(np.float64), nm + "/cond": np.array([cond]), nm + "/transm": w, nm + "/transmd": wd}
    pack(out, nm, "trans", T, k < PROBE_FROM)
    pack(out, nm, "pao", Pa, k < PROBE_FROM)
    print(f"{nm}: cond {cond:.3g}, {time.time() - t0:.1f} s", flush=True)
    return out


def reference(case):
    import _oracle
    cls, k, n = case
    c = truth_problem(cls, k, n)
    nm = "ref/" + truth_name(cls, k, n)
    r = _oracle.letkf_core("ref", k, c["nobs"], n, c["hdxb"], c["rdiag"], c["rloc"], c["dep"], c["infl"], rdiag_wloc=True,
                           infl_update=True, depd=c["depd"], want_transmd=True)
    out = {nm + "/transm": r["transm"], nm + "/transmd": r["transmd"], nm + "/parm_infl": np.array([r["parm_infl"]])}
    pack(out, nm, "trans", r["trans"], k <= REF_FULL_TO)
    pack(out, nm, "pao", r["pao"], k <= REF_FULL_TO)
    return out


def main():
    import _oracle
    resource.setrlimit(resource.RLIMIT_STACK, (resource.RLIM_INFINITY, resource.RLIM_INFINITY))
    path = os.path.join(HERE, "degenerate_truth.npz")
    ref_path = os.path.join(HERE, "degenerate_reference.npz")
    ks = [int(a) for a in sys.argv[1:]]
    old = load_store(np.load(path)) if os.path.exists(path) else {}
    cases = truth_cases()
    todo = [c for c in cases if not ks or c[1] in ks]
    out = {}
    with multiprocessing.Pool(min(8, os.cpu_count() or 1)) as pool:
        for d in pool.imap_unordered(one, sorted(todo, key=lambda c: -c[1])):
            out.update(d)
    names = [truth_name(*c) for c in cases]
    for nm in names:                                    # cases not regenerated in this run are carried over
        for key, v in old.items():
            if key.startswith(nm + "/") and not key.startswith("ref/") and key not in out:
                out[key] = v
    np.savez_compressed(path, names=np.array(names), **pack_store(out))
    print("wrote", path, os.path.getsize(path) / 1e6, "MB")
    if _oracle.ref() is not None:
        ref = {}
        for c in cases:
            ref.update(reference(c))
            ref["ref/" + truth_name(*c) + "/sha"] = out[truth_name(*c) + "/sha"]
        np.savez_compressed(ref_path, names=np.array(names), **pack_store(ref))
        print("wrote", ref_path, os.path.getsize(ref_path) / 1e6, "MB")
    else:
        print("oracle/_ref not built:", ref_path, "is left as it is")


if __name__ == "__main__":
    main()
