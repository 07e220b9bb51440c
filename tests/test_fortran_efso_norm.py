"""EFSO from the forecast fields to the impact table from a Fortran host: fortran/efso_tools_amd.f90 (efso_norm_amd,
print_obsense_amd) around das_efso_amd, called by fortran/efso_norm_driver.f90.  The driver's normed fields, obsense and
tables equal Context.efso_norm / efso_columns / efso_obsense / efso_summary bit for bit, and its printed table is
Python's formatting of the same table (tests/_efso_norm.py table_lines)."""
import os
import struct
import subprocess
import tempfile

import numpy as np
import pytest

import _efso_norm as en
from __graft_entry__ import PKG_DIR, load_package
from _search import build_case

FDIR = os.path.join(PKG_DIR, "fortran")
DRIVER = os.path.join(FDIR, "build", "efso_norm_driver")
HAVE_FC = os.path.exists("/opt/rocm/bin/amdflang")
ELEM_UID = [2819, 2820, 3073, 3330, 3331, 14593]
ELEM_NAMES = ["U", "V", "T", "Q", "RH", "PS"]
TYPE_NAMES = ["ADPUPA", "AIRCAR", "AIRCFT", "SATWND"]


def build_fortran():
    load_package().build()
    subprocess.check_call(["make", "-C", FDIR], stdout=subprocess.DEVNULL)


@pytest.mark.skipif(not HAVE_FC, reason="amdflang not present")
def test_efso_norm_driver_compiles_and_links():
    build_fortran()
    assert os.path.exists(DRIVER)
    src = open(os.path.join(FDIR, "efso_tools_amd.f90")).read()
    assert "SUBROUTINE efso_norm_amd" in src and "SUBROUTINE print_obsense_amd" in src


def make_case(seed, nij1, nlev, k, nv, nterm):
    sc = build_case(seed, npts=nij1)
    nobs = sc["nobs"]
    npts = nij1 * nlev
    rng = np.random.default_rng(seed)
    fcst = rng.standard_normal((npts, k, nv)) * rng.uniform(0.5, 5.0, nv) + rng.uniform(-10.0, 300.0, nv)
    prof = 1.0e5 * np.exp(-np.linspace(0.0, 2.5, nlev))[:, None] * rng.uniform(0.97, 1.03, nij1)[None, :]
    fcst[:, :, 4] = prof.ravel()[:, None] + 50.0 * rng.standard_normal((npts, k))
    x3 = [rng.standard_normal((npts, nv)) * s for s in (3.0, 3.0, 2.0)]
    term = [0, 0, -1, 1, -1, 2, -1, -1, -1, -1, -1][:nv]
    if nterm == 4:
        term[6] = 3
    return dict(sc=sc, nobs=nobs, rng=rng, fcst=fcst, x3=x3, term=term, rlev=rng.uniform(2.5e4, 1.0e5, npts),
                rz=rng.uniform(0.0, 12000.0, npts), ya=rng.standard_normal((nobs, k)), dep=rng.standard_normal(nobs),
                wg1=rng.uniform(0.8, 1.2, nij1), lon=rng.uniform(0.0, 360.0, nij1), lat=rng.uniform(-90.0, 90.0, nij1),
                elm=rng.choice(ELEM_UID + [9999], nobs).astype(np.int32),
                typ=rng.integers(0, len(TYPE_NAMES) + 3, nobs).astype(np.int32),
                olat=rng.choice([-20.0, 20.0, -50.0, 0.0, 35.0], nobs))


def run_driver(c, nij1, nlev, k, nv, nterm, tar, wmoist, box, mode, latbound):
    sc, nobs = c["sc"], c["nobs"]
    arr, scal, pts = sc["arr"], sc["scal"], sc["pts"]
    npts = nij1 * nlev
    f3 = lambda a: np.ascontiguousarray(a.reshape(nlev, nij1, -1).transpose(2, 0, 1))    # (p, v) -> (v, lev, ij)
    with tempfile.TemporaryDirectory() as d:
        fin, fout = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
        with open(fin, "wb") as fh:
            hdr = [scal["nctype"], scal["ngroup"], scal["criterion"], scal["nlon"], scal["nlat"], nij1, nlev, k, nv, nterm, nobs,
                   arr["ac_ext"].size, arr["group_member"].size, len(ELEM_UID), len(TYPE_NAMES), tar[0], tar[1], mode]
            fh.write(struct.pack("<18i", *hdr))
            fh.write(struct.pack("<11d", scal["dx"], scal["dy"], scal["i_org"], scal["j_org"], scal["rain_base"], wmoist, *box,
                                 latbound))
            w = lambda a, dt: fh.write(np.ascontiguousarray(a, dtype=dt).tobytes())
            for a in (arr["group_start"], arr["group_member"], arr["vmode"], arr["max_nobs"], arr["ngrd_i"], arr["ngrd_j"],
                      arr["ngrdsch_i"], arr["ngrdsch_j"], arr["ngrdext_i"], arr["ngrdext_j"], [t + 1 for t in c["term"]]):
                w(a, "<i4")
            w(arr["ac_off"], "<i8")
            w(arr["ac_ext"], "<i4")
            fcst3d = np.ascontiguousarray(c["fcst"].transpose(2, 1, 0))        # (v, m, p): fcst3d(nij1, nlev, member, nv3d)
            for a in (arr["hori_loc"], arr["vert_loc"], arr["varloc"], arr["ob_ri"], arr["ob_rj"], arr["ob_lev"], arr["ob_dat"],
                      arr["ob_err"], pts["ri"], pts["rj"], c["rlev"], c["rz"], fcst3d, *(f3(x) for x in c["x3"]), c["wg1"],
                      c["lon"], c["lat"], c["ya"], c["dep"], c["olat"]):
                w(a, "<f8")
            for a in (c["elm"], c["typ"], ELEM_UID):
                w(a, "<i4")
            fh.write("".join(f"{n:<6s}" for n in TYPE_NAMES).encode() + "".join(f"{n:<3s}" for n in ELEM_NAMES).encode())
        r = subprocess.run([DRIVER, fin, fout], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        raw = open(fout, "rb").read()
    nid, ntp = len(ELEM_UID), len(TYPE_NAMES) + 1
    nf, ne, no, ns = npts * k * nv, npts * nv, nobs * nterm, nid * ntp * 3 * nterm
    dbl = np.frombuffer(raw[:8 * (nf + ne + no + ns)], dtype="<f8")
    ints = np.frombuffer(raw[8 * (nf + ne + no + ns):], dtype="<i4")
    assert ints.size == nid * ntp * 3 + ns
    fo = dbl[:nf].reshape(nv, k, npts).transpose(2, 1, 0)
    eo = dbl[nf:nf + ne].reshape(nv, npts).T
    ob = dbl[nf + ne:nf + ne + no].reshape(nobs, nterm)
    ssum = dbl[nf + ne + no:].reshape(nterm, 3, ntp, nid)                   # sumsense(nid, nobtype+1, 3, nterm)
    cnt = ints[:nid * ntp * 3].reshape(3, ntp, nid)
    neg = ints[nid * ntp * 3:].reshape(nterm, 3, ntp, nid)
    return fo, eo, ob, cnt, ssum, neg, r.stdout.splitlines()


@pytest.mark.gpu
@pytest.mark.skipif(not HAVE_FC, reason="amdflang not present")
@pytest.mark.parametrize("k,nterm,mode,tar,wmoist", [(10, 3, 1, (1, 64), 1.0), (50, 4, 0, (2, 3), 0.0)])
def test_driver_matches_the_c_route_and_prints_the_table(k, nterm, mode, tar, wmoist):
    import torch
    from _gpu import ctx, dev
    from _search import device_struct
    build_fortran()
    nij1, nlev, nv = 60, 4, 11
    box, latbound = (60.0, 300.0, -60.0, 75.0), 20.0
    c = make_case(k + nterm, nij1, nlev, k, nv, nterm)
    nobs, npts = c["nobs"], nij1 * nlev
    fo, eo, ob, cnt, ssum, neg, out = run_driver(c, nij1, nlev, k, nv, nterm, tar, wmoist, box, mode, latbound)
    # the same chain through the Python binding
    cx = ctx()
    prm = pkg_params(k, nv, tar, wmoist, box)
    f, e = dev(c["fcst"].transpose(2, 1, 0).ravel()), torch.zeros(npts * nv, dtype=torch.float64, device="cuda")
    xs = [dev(x.T.ravel()) for x in c["x3"]]
    kw = dict(wg1=dev(c["wg1"]), lon=dev(c["lon"]), lat=dev(c["lat"])) if mode == 1 else {}
    cx.efso_norm(prm, nij1, nlev, f, 1, npts, npts * k, e, 1, npts, xf=xs[0], xg=xs[1], xa=xs[2], **kw)
    t, keep = device_struct(c["sc"], "cuda")
    dj = torch.zeros(nobs * nterm, dtype=torch.float64, device="cuda")
    pts = c["sc"]["pts"]
    cx.efso_columns(k, nv, c["term"], nterm, t, nij1, nlev, dev(pts["ri"]), dev(pts["rj"]), dev(c["rlev"]), dev(c["rz"]),
                    dev(c["ya"].ravel()), k, nobs, f, 1, npts, npts * k, e, 1, npts, dj)
    obs = torch.empty_like(dj)
    cx.efso_obsense(nterm, dj, dev(c["dep"]), obs)
    cc, cs, cn = cx.efso_summary(nterm, obs, dev(c["elm"]), dev(c["typ"]), dev(c["olat"]), ELEM_UID, len(TYPE_NAMES), latbound)
    torch.cuda.synchronize()
    bits = lambda a: np.ascontiguousarray(a).view(np.int64)
    assert np.array_equal(bits(fo), bits(f.cpu().numpy().reshape(nv, k, npts).transpose(2, 1, 0)))
    assert np.array_equal(bits(eo), bits(e.cpu().numpy().reshape(nv, npts).T))
    assert np.array_equal(bits(ob), bits(obs.cpu().numpy().reshape(nobs, nterm))) and np.abs(ob).max() > 0
    assert np.array_equal(cnt, cc.cpu().numpy()) and np.array_equal(neg, cn.cpu().numpy())
    assert np.array_equal(bits(ssum), bits(cs.cpu().numpy()))
    lines = en.table_lines(cnt, ssum, neg, nobs, TYPE_NAMES, ELEM_NAMES)
    assert len(lines) > 6 and out[-len(lines):] == lines


def pkg_params(k, nv, tar, wmoist, box):
    p = load_package().EfsoNormParams()
    p.k, p.nv, p.iv_u, p.iv_v, p.iv_t, p.iv_q, p.iv_p = k, nv, 0, 1, 3, 5, 4
    p.tar_minlev, p.tar_maxlev = tar
    p.cp, p.tref, p.hvap, p.wmoist = en.CP, en.TREF, en.HVAP, wmoist
    p.tar_minlon, p.tar_maxlon, p.tar_minlat, p.tar_maxlat = box
    return p
