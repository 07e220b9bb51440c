"""das_efso with localisation advection from a Fortran host: scale-letkf_amd/fortran/letkf_tools_amd.f90 `das_efso_amd` with
its optional wind arguments (das_efso's advection branch, scale/letkf/letkf_tools.f90:1225-1229), called by
fortran/efso_locadv_driver.f90 for two variable-localisation classes that accumulate into one djdy.  With the arguments
(and a rate > 0) it gives the bits of Context.efso_locadv + Context.efso_search; without them, or at rate 0, those of
Context.efso_columns."""
import os
import struct
import subprocess
import tempfile

import numpy as np
import pytest

import _efso
import _efso_locadv as la
from __graft_entry__ import PKG_DIR, load_package
from _search import build_case

FDIR = os.path.join(PKG_DIR, "fortran")
DRIVER = os.path.join(FDIR, "build", "efso_locadv_driver")
HAVE_FC = os.path.exists("/opt/rocm/bin/amdflang")


def build_fortran():
    load_package().build()
    subprocess.check_call(["make", "-C", FDIR], stdout=subprocess.DEVNULL)


@pytest.mark.skipif(not HAVE_FC, reason="amdflang not present")
def test_efso_locadv_driver_compiles_and_links():
    build_fortran()
    assert os.path.exists(DRIVER)


def run_driver(case, nij1, nlev, k, nv, nterm, term1, kld, mask1, mask2, rlev, rz, fcst, fcer, tab, dep, winds, mode, rate, eft):
    arr, scal, pts = case["arr"], case["scal"], case["pts"]
    nobs = case["nobs"]
    f, _, e, _ = _efso.ref_layout(fcst, fcer)
    with tempfile.TemporaryDirectory() as d:
        fin, fout = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
        with open(fin, "wb") as fh:
            hdr = [scal["nctype"], scal["ngroup"], scal["criterion"], scal["nlon"], scal["nlat"], nij1, nlev, k, nv, nterm, nobs,
                   kld, arr["ac_ext"].size, mask1, mask2, arr["group_member"].size, mode]
            fh.write(struct.pack("<17i", *hdr))
            fh.write(struct.pack("<7d", scal["dx"], scal["dy"], scal["i_org"], scal["j_org"], scal["rain_base"], rate, eft))
            w = lambda a, dt: fh.write(np.ascontiguousarray(a, dtype=dt).tobytes())
            for a in (arr["group_start"], arr["group_member"], arr["vmode"], arr["max_nobs"], arr["ngrd_i"], arr["ngrd_j"],
                      arr["ngrdsch_i"], arr["ngrdsch_j"], arr["ngrdext_i"], arr["ngrdext_j"], term1):
                w(a, "<i4")
            w(arr["ac_off"], "<i8")
            w(arr["ac_ext"], "<i4")
            for a in (arr["hori_loc"], arr["vert_loc"], arr["varloc"], arr["ob_ri"], arr["ob_rj"], arr["ob_lev"], arr["ob_dat"],
                      arr["ob_err"], pts["ri"], pts["rj"], rlev, rz, f, e, tab, dep, *winds):
                w(a, "<f8")
        r = subprocess.run([DRIVER, fin, fout], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        raw = np.fromfile(fout, dtype="<f8")
    assert raw.size == 2 * nobs * nterm
    return raw[:nobs * nterm].reshape(nobs, nterm), raw[nobs * nterm:].reshape(nobs, nterm)


@pytest.mark.gpu
@pytest.mark.skipif(not HAVE_FC, reason="amdflang not present")
@pytest.mark.parametrize("k,nterm,kld_pad", [(10, 3, 0), (50, 4, 3)])
def test_das_efso_amd_with_advection_matches_the_c_route(k, nterm, kld_pad):
    import torch
    from _gpu import ctx, dev
    from _search import device_struct
    build_fortran()
    nij1, nlev = 60, 4
    case = build_case(91, npts=nij1)
    pts, nobs = case["pts"], case["nobs"]
    npts = nij1 * nlev
    rng = np.random.default_rng(k)
    rlev = rng.uniform(2.5e4, 1.0e5, npts)
    rz = rng.uniform(0.0, 12000.0, npts)
    nv = 7
    term1 = [1, 1, 0, 2, nterm, 3 if nterm >= 3 else 0, 2]      # Fortran: 1-based terms, 0 = none
    term0 = [t - 1 for t in term1]
    mask1, mask2 = 0b0010011, 0b1101100
    kld = k + kld_pad
    fcst, fcer, ya, dep = _efso.inputs(rng, npts, k, nv, nobs)
    tab = np.zeros((nobs, kld))
    tab[:, :k] = ya
    winds = la.shear_winds(rng, nij1, nlev, noise=2.0)
    rate, eft = 0.5, 0.1
    c = ctx()
    t, keep = device_struct(case, "cuda")
    f, fs, e, es = _efso.ref_layout(fcst, fcer)
    ri, rj = c.efso_locadv(dev(pts["ri"]), dev(pts["rj"]), nlev, *(dev(x) for x in winds), rate, eft, case["scal"]["dx"],
                           case["scal"]["dy"])
    dj = torch.zeros(nobs * nterm, dtype=torch.float64, device="cuda")
    for m in (mask1, mask2):
        c.efso_search(k, nv, term0, nterm, t, ri, rj, dev(rlev), dev(rz), dev(tab.ravel()), kld, nobs, dev(f), *fs, dev(e), *es,
                      dj, var_mask=m)
    dj_col = torch.zeros(nobs * nterm, dtype=torch.float64, device="cuda")
    for m in (mask1, mask2):
        c.efso_columns(k, nv, term0, nterm, t, nij1, nlev, dev(pts["ri"]), dev(pts["rj"]), dev(rlev), dev(rz), dev(tab.ravel()),
                       kld, nobs, dev(f), *fs, dev(e), *es, dj_col, var_mask=m)
    torch.cuda.synchronize()
    want = dj.cpu().numpy().reshape(nobs, nterm)
    want_col = dj_col.cpu().numpy().reshape(nobs, nterm)
    assert np.abs(want).max() > 0 and not np.array_equal(want, want_col)
    args = (case, nij1, nlev, k, nv, nterm, term1, kld, mask1, mask2, rlev, rz, fcst, fcer, tab, dep, winds)
    djdy, obsense = run_driver(*args, mode=1, rate=rate, eft=eft)
    assert np.array_equal(djdy.view(np.int64), want.view(np.int64))
    assert np.array_equal(obsense, djdy * dep[:, None])
    for mode, r in ((0, rate), (1, 0.0)):         # without the arguments, and with them at rate 0: today's column call
        djdy, obsense = run_driver(*args, mode=mode, rate=r, eft=eft)
        assert np.array_equal(djdy.view(np.int64), want_col.view(np.int64)), (mode, r)
        assert np.array_equal(obsense, djdy * dep[:, None])
