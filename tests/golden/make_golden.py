#!/usr/bin/env python3
"""Generate the golden fixtures from the REFERENCE's own routines (compiled by oracle/Makefile into oracle/_ref).
Needs the reference tree + amdflang, i.e. it only runs in the build container; the fixtures it writes are data
(inputs' SHA-256 + expected outputs):

  tests/golden/letkf_core_golden.npz   letkf_core (common/common_letkf.f90:52) on the covering case matrix in
                                       tests/_cases.py:golden_case_list()
  tests/golden/reference_checks.npz    letkf_core, mtx_eigen (common/common_mtx.f90) and QUICKSELECT_arg /
                                       QUICKSELECT_desc_arg (common/common_sort.f90:341,404) on the inputs of
                                       tests/test_oracle_vs_ref.py and tests/test_oracle_search.py (tests/_cases.py REF_*)

    make -C oracle ref && python tests/golden/make_golden.py [core] [checks]
"""
import ctypes as C
import os
import sys
import resource

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from _cases import (REF_CORE_MODES, REF_CORE_SHAPES, REF_EIGEN_SIZES, array_sha, case_sha,  # noqa: E402
                    golden_case_list, golden_inputs, probes, ref_core_inputs, ref_core_name, ref_eigen_input,
                    ref_select_inputs)
import _oracle  # noqa: E402


def core_golden():
    out = {}
    names = []
    for c in golden_case_list():
        inp = golden_inputs(c)
        r = _oracle.letkf_core("ref", c["k"], inp["nobs"], c["n"], inp["hdxb"], inp["rdiag"], inp["rloc"],
                               inp["dep"], inp["infl"], want_transm=c["transm"], want_pao=c["pao"],
                               rdiag_wloc=c["rdiag_wloc"], infl_update=c["infl_update"], depd=inp["depd"],
                               want_transmd=c["det"])
        nm = c["name"]
        names.append(nm)
        out[nm + "/sha"] = np.frombuffer(bytes.fromhex(case_sha(inp)), dtype=np.uint8)
        out[nm + "/parm_infl"] = np.array([r["parm_infl"]])
        k = c["k"]
        big = k > 100
        pr = probes(k)
        for key in ("trans", "pao"):
            if r[key] is None:
                continue
            if big:
                out[f"{nm}/{key}_probe"] = r[key] @ pr
                out[f"{nm}/{key}_diag"] = np.diag(r[key]).copy()
                out[f"{nm}/{key}_absmax"] = np.array([np.abs(r[key]).max()])
            else:
                out[f"{nm}/{key}"] = r[key]
        for key in ("transm", "transmd"):
            if r[key] is not None:
                out[f"{nm}/{key}"] = r[key]
        print(f"{nm}: ok", flush=True)
    out["names"] = np.array(names)
    return out


def reference_checks():
    out = {}
    for k, n in REF_CORE_SHAPES:
        for wloc, iu, det in REF_CORE_MODES:
            c = ref_core_inputs(k, n, wloc, det)
            r = _oracle.letkf_core("ref", k, c["nobs"], n, c["hdxb"], c["rdiag"], c["rloc"], c["dep"], c["infl"],
                                   rdiag_wloc=wloc, infl_update=iu, depd=c["depd"], want_transmd=det)
            nm = ref_core_name(k, n, wloc, iu, det)
            out[nm + "/sha"] = np.frombuffer(bytes.fromhex(case_sha(c)), dtype=np.uint8)
            for key in ("trans", "pao", "transm", "transmd"):
                if r[key] is not None:
                    out[f"{nm}/{key}"] = r[key]
            out[nm + "/parm_infl"] = np.array([r["parm_infl"]])
    for n in REF_EIGEN_SIZES:
        a = ref_eigen_input(n)
        w, v, nr, _ = _oracle.mtx_eigen("ref", a)
        out[f"eigen/n{n}/sha"] = array_sha(a)
        out[f"eigen/n{n}/w"], out[f"eigen/n{n}/v"], out[f"eigen/n{n}/nr"] = w, v, np.array([nr])
    ref = _oracle.ref()
    for desc in (0, 1):
        for n, K, a, x in ref_select_inputs():
            x_ref = (x + 1).astype(np.int32)      # Fortran indices
            ref.ref_quickselect_arg(C.c_int(a.size), a.ctypes.data_as(C.POINTER(C.c_double)), C.c_int(n),
                                    x_ref.ctypes.data_as(C.POINTER(C.c_int)), C.c_int(1), C.c_int(n), C.c_int(K),
                                    C.c_int(desc))
            nm = f"select/d{desc}_n{n}_K{K}"
            out[nm + "/sha"] = array_sha(a, x)
            out[nm + "/first"] = np.sort(x_ref[:K] - 1).astype(np.int32)   # the K selected (their order is the routine's)
    return out


def main():
    # the reference keeps all workspace in automatic arrays: k=1000 needs a big stack
    resource.setrlimit(resource.RLIMIT_STACK, (resource.RLIM_INFINITY, resource.RLIM_INFINITY))
    if _oracle.ref() is None:
        sys.exit("oracle/_ref/libletkf_ref.so missing: run `make -C oracle ref` where the reference tree exists")
    which = sys.argv[1:] or ["core", "checks"]
    for w, fname, make in (("core", "letkf_core_golden.npz", core_golden),
                           ("checks", "reference_checks.npz", reference_checks)):
        if w in which:
            path = os.path.join(HERE, fname)
            np.savez_compressed(path, **make())
            print("wrote", path, os.path.getsize(path) / 1e6, "MB")


if __name__ == "__main__":
    main()
