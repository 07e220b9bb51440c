"""das_efso from a Fortran host on the device: scale-letkf_amd/fortran/letkf_tools_amd.f90 `das_efso_amd` (das_efso,
scale/letkf/letkf_tools.f90:1158-1302), called by fortran/efso_driver.f90 for two variable-localisation classes that
accumulate into one djdy, against the numpy restatement tests/_efso.py on the oracle's obs_local lists."""
import os
import struct
import subprocess
import tempfile

import numpy as np
import pytest

import _efso
from __graft_entry__ import PKG_DIR, load_package
from _search import build_case, host_struct, oracle_csr

FDIR = os.path.join(PKG_DIR, "fortran")
DRIVER = os.path.join(FDIR, "build", "efso_driver")
HAVE_FC = os.path.exists("/opt/rocm/bin/amdflang")


def build_fortran():
    load_package().build()
    subprocess.check_call(["make", "-C", FDIR], stdout=subprocess.DEVNULL)


@pytest.mark.skipif(not HAVE_FC, reason="amdflang not present")
def test_das_efso_amd_compiles_and_links():
    build_fortran()
    assert os.path.exists(DRIVER)


@pytest.mark.gpu
@pytest.mark.skipif(not HAVE_FC, reason="amdflang not present")
@pytest.mark.parametrize("k,nterm,kld_pad", [(10, 3, 0), (50, 4, 3)])
def test_das_efso_amd_from_fortran_matches_numpy(k, nterm, kld_pad):
    build_fortran()
    nij1, nlev = 60, 4
    case = build_case(81, npts=nij1)
    arr, scal, pts = case["arr"], case["scal"], case["pts"]
    nobs, nctype = case["nobs"], scal["nctype"]
    npts = nij1 * nlev
    rng = np.random.default_rng(k)
    rlev = rng.uniform(2.5e4, 1.0e5, npts)
    rz = rng.uniform(0.0, 12000.0, npts)
    h, keep = host_struct(case)
    off, idx, rd, rl, _ = oracle_csr(h, np.tile(pts["ri"], nlev), np.tile(pts["rj"], nlev), rlev, rz)
    assert off[-1] > 20 * npts
    nv = 7
    term1 = [1, 1, 0, 2, nterm, 3 if nterm >= 3 else 0, 2]      # Fortran: 1-based terms, 0 = none
    term0 = [t - 1 for t in term1]
    mask1, mask2 = 0b0010011, 0b1101100
    kld = k + kld_pad
    fcst, fcer, ya, dep = _efso.inputs(rng, npts, k, nv, nobs)
    exp, _ = _efso.efso_loop(off, idx, rd, rl, ya, fcst, fcer, term0, nterm, var_mask=mask1)
    exp, _ = _efso.efso_loop(off, idx, rd, rl, ya, fcst, fcer, term0, nterm, var_mask=mask2, djdy=exp)
    scale = (_efso.efso_loop(off, idx, rd, rl, ya, fcst, fcer, term0, nterm, var_mask=mask1)[1]
             + _efso.efso_loop(off, idx, rd, rl, ya, fcst, fcer, term0, nterm, var_mask=mask2)[1])
    tab = np.zeros((nobs, kld))
    tab[:, :k] = ya
    f, _, e, _ = _efso.ref_layout(fcst, fcer)
    with tempfile.TemporaryDirectory() as d:
        fin, fout = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
        with open(fin, "wb") as fh:
            hdr = [nctype, scal["ngroup"], scal["criterion"], scal["nlon"], scal["nlat"], nij1, nlev, k, nv, nterm, nobs, kld,
                   arr["ac_ext"].size, mask1, mask2, arr["group_member"].size]
            fh.write(struct.pack("<16i", *hdr))
            fh.write(struct.pack("<5d", scal["dx"], scal["dy"], scal["i_org"], scal["j_org"], scal["rain_base"]))
            w = lambda a, dt: fh.write(np.ascontiguousarray(a, dtype=dt).tobytes())
            for a in (arr["group_start"], arr["group_member"], arr["vmode"], arr["max_nobs"], arr["ngrd_i"], arr["ngrd_j"],
                      arr["ngrdsch_i"], arr["ngrdsch_j"], arr["ngrdext_i"], arr["ngrdext_j"], term1):
                w(a, "<i4")
            w(arr["ac_off"], "<i8")
            w(arr["ac_ext"], "<i4")
            for a in (arr["hori_loc"], arr["vert_loc"], arr["varloc"], arr["ob_ri"], arr["ob_rj"], arr["ob_lev"], arr["ob_dat"],
                      arr["ob_err"], pts["ri"], pts["rj"], rlev, rz, f, e, tab, dep):
                w(a, "<f8")
        r = subprocess.run([DRIVER, fin, fout], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        raw = np.fromfile(fout, dtype="<f8")
    assert raw.size == 2 * nobs * nterm
    djdy = raw[:nobs * nterm].reshape(nobs, nterm)          # djdy(nterm, nobs), column-major
    obsense = raw[nobs * nterm:].reshape(nobs, nterm)
    assert np.abs(exp).max() > 0
    assert _efso.within(djdy, exp, scale) < 1e-12
    assert np.array_equal(obsense, djdy * dep[:, None])
