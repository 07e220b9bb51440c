"""EFSO's forecast-error norm and impact summary on the device (include/letkf_amd.h section 13): letkf_efso_norm_dev bit for
bit against the numpy restatement tests/_efso_norm.py over k, nv, strides, layer weights, target regions, the moist term
and the fcer assembly; argument errors with outputs untouched; the chain norm -> letkf_efso_columns_dev ->
letkf_efso_obsense_dev -> letkf_efso_summary_dev against the same chain fed with numpy-normed inputs; the summary bit for
bit against print_obsense's sequential loop."""
import numpy as np
import pytest
import torch

import _efso_norm as en
from __graft_entry__ import load_package

pytestmark = pytest.mark.gpu
pkg = load_package()

IV, IV_P = (0, 1, 3, 5), 4
BOX = (90.0, 270.0, -30.0, 60.0)
ELEM_UID = [2819, 2820, 3073, 3330, 3331, 14593, 4001]


def _ctx():
    from _gpu import ctx
    return ctx()


def _d(a, dt=None):
    from _gpu import dev
    return dev(a, dt)


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def params(k, nv, tar=(1, 64), wmoist=1.0, box=BOX, iv=IV, iv_p=IV_P):
    p = pkg.EfsoNormParams()
    p.k, p.nv = k, nv
    p.iv_u, p.iv_v, p.iv_t, p.iv_q = iv
    p.iv_p = iv_p
    p.tar_minlev, p.tar_maxlev = tar
    p.cp, p.tref, p.hvap, p.wmoist = en.CP, en.TREF, en.HVAP, wmoist
    p.tar_minlon, p.tar_maxlon, p.tar_minlat, p.tar_maxlat = box
    return p


def case(seed, nij1, nlev, k, nv):
    rng = np.random.default_rng(seed)
    fcst = rng.standard_normal((nij1 * nlev, k, nv)) * rng.uniform(0.5, 5.0, nv) + rng.uniform(-10.0, 300.0, nv)
    prof = 1.0e5 * np.exp(-np.linspace(0.0, 2.5, nlev))[:, None] * rng.uniform(0.97, 1.03, nij1)[None, :]
    fcst[:, :, IV_P] = prof.ravel()[:, None] + 50.0 * rng.standard_normal((nij1 * nlev, k))
    fcer = rng.standard_normal((nij1 * nlev, nv)) * 0.1
    return rng, fcst, fcer


def pack(fcst, fcer, layout):
    """device arrays and strides: 'point' = gues3d's order (p fastest), 'member' = members fastest, (p, v) for fcer"""
    npts, k, nv = fcst.shape
    if layout == "point":
        return (_d(fcst.transpose(2, 1, 0).ravel()), (1, npts, npts * k), _d(fcer.T.ravel()), (1, npts))
    return (_d(fcst.transpose(0, 2, 1).ravel()), (nv * k, 1, k), _d(fcer.ravel()), (nv, 1))


def unpack(f, e, shape, layout):
    npts, k, nv = shape
    f, e = f.cpu().numpy(), e.cpu().numpy()
    if layout == "point":
        return f.reshape(nv, k, npts).transpose(2, 1, 0), e.reshape(nv, npts).T
    return f.reshape(npts, nv, k).transpose(0, 2, 1), e.reshape(npts, nv)


def run_norm(fcst, fcer, nij1, prm, layout="point", wlev=None, wg1=None, lon=None, lat=None, x3=None, fmean=False):
    f, fs, e, es = pack(fcst, fcer if fcer is not None else np.zeros(fcst.shape[::2]), layout)
    nlev = fcst.shape[0] // nij1
    fm = torch.full((fcst.shape[0] * fcst.shape[2],), np.nan, dtype=torch.float64, device="cuda") if fmean else None
    xs = [None] * 3
    if x3 is not None:
        xs = [pack(fcst, x, layout)[2] for x in x3]
    dv = lambda a: None if a is None else _d(a)
    _ctx().efso_norm(prm, nij1, nlev, f, *fs, e, *es, fmean=fm, xf=xs[0], xg=xs[1], xa=xs[2], wlev=dv(wlev), wg1=dv(wg1),
                     lon=dv(lon), lat=dv(lat))
    torch.cuda.synchronize()
    fo, eo = unpack(f, e, fcst.shape, layout)
    return fo, eo, (fm.cpu().numpy().reshape(fcst.shape[2], -1).T if fmean else None)


def check(fcst, fcer, nij1, layout="point", tar=(1, 64), wmoist=1.0, wlev=None, wg1=None, lon=None, lat=None, x3=None,
          fmean=False):
    npts, k, nv = fcst.shape
    got = run_norm(fcst, fcer, nij1, params(k, nv, tar, wmoist), layout, wlev, wg1, lon, lat, x3, fmean)
    xf, xg, xa = x3 if x3 is not None else (None, None, None)
    fo, eo, mean, bad = en.norm(fcst, fcer, nij1, IV, IV_P, tar, wlev, wg1, lon, lat, BOX, xf, xg, xa, wmoist=wmoist)
    assert not bad.any()
    assert np.array_equal(_bits(got[0]), _bits(fo)), np.abs(got[0] - fo).max()
    assert np.array_equal(_bits(got[1]), _bits(eo)), np.abs(got[1] - eo).max()
    if fmean:
        assert np.array_equal(_bits(got[2]), _bits(mean))
    return fo, eo


@pytest.mark.parametrize("k", [2, 3, 20, 50, 100, 320])
@pytest.mark.parametrize("nv", [11, 7])
@pytest.mark.parametrize("layout", ["point", "member"])
def test_norm_matches_the_restatement(k, nv, layout):
    nij1, nlev = (37, 5) if k <= 100 else (13, 4)
    rng, fcst, fcer = case(k * 31 + nv, nij1, nlev, k, nv)
    wg1 = rng.uniform(0.5, 1.5, nij1)
    fo, _ = check(fcst, fcer, nij1, layout, wg1=wg1, fmean=True)
    assert np.abs(fo[:, :, [0, 1, 3, 5]]).min() > 0 and np.all(fo[:, :, [2, 4, 6]] == 0)


@pytest.mark.parametrize("k", [20, 100])
@pytest.mark.parametrize("opt", ["wlev", "wg1", "box", "empty_box", "levels", "empty_levels", "dry", "assembly",
                                 "assembly_box_member", "nlev1"])
def test_norm_options(k, opt):
    nij1, nlev, nv = 41, 6, 11
    rng, fcst, fcer = case(sum(map(ord, opt)) + k, nij1, nlev if opt != "nlev1" else 1, k, nv)
    kw = {}
    lon, lat = rng.uniform(0.0, 360.0, nij1), rng.uniform(-90.0, 90.0, nij1)
    lon[0], lat[1], lon[2] = BOX[0], BOX[3], BOX[1]          # on the box's edges: inside
    if opt == "wlev":
        kw["wlev"] = rng.uniform(0.0, 0.3, fcst.shape[0])
    elif opt == "wg1":
        kw["wg1"] = rng.uniform(0.0, 2.0, nij1)
    elif opt in ("box", "assembly_box_member"):
        kw["lon"], kw["lat"] = lon, lat
    elif opt == "empty_box":
        kw["lon"], kw["lat"] = np.full(nij1, 10.0), lat
    elif opt == "levels":
        kw["tar"] = (2, 4)
    elif opt == "empty_levels":
        kw["tar"] = (7, 9)
    elif opt == "dry":
        kw["wmoist"] = 0.0
    if opt.startswith("assembly"):
        kw["x3"] = tuple(rng.standard_normal((fcst.shape[0], nv)) * s for s in (3.0, 3.0, 2.0))
        fcer = None
    layout = "member" if opt == "assembly_box_member" else "point"
    fo, eo = check(fcst, fcer, nij1, layout, **kw)
    if opt.startswith("empty"):
        assert not np.any(fo) and not np.any(eo)
    else:
        assert np.any(fo) and np.any(eo)


def test_norm_repeats_bit_for_bit():
    nij1, nlev, k, nv = 200, 10, 50, 11
    rng, fcst, fcer = case(7, nij1, nlev, k, nv)
    prm = params(k, nv)
    a = run_norm(fcst, fcer, nij1, prm, wg1=np.full(nij1, 0.9))
    b = run_norm(fcst, fcer, nij1, prm, wg1=np.full(nij1, 0.9))
    assert np.array_equal(_bits(a[0]), _bits(b[0])) and np.array_equal(_bits(a[1]), _bits(b[1]))


def test_norm_argument_errors_leave_the_outputs_untouched():
    nij1, nlev, k, nv = 17, 4, 5, 11
    rng, fcst, fcer = case(9, nij1, nlev, k, nv)
    f, fs, e, es = pack(fcst, fcer, "point")
    x = _d(fcer.T.ravel())
    f0, e0 = f.clone(), e.clone()
    fm = torch.full((nij1 * nlev * nv,), 7.0, dtype=torch.float64, device="cuda")
    c = _ctx()

    def call(prm, n1=nij1, nl=nlev, **kw):
        with pytest.raises(pkg.LetkfError, match="error -1"):
            c.efso_norm(prm, n1, nl, f, *fs, e, *es, fmean=fm, **kw)
        torch.cuda.synchronize()
        assert torch.equal(f, f0) and torch.equal(e, e0) and bool((fm == 7.0).all())

    call(params(1, nv))
    call(params(k, 0))
    call(params(k, 33))
    call(params(k, nv, iv=(0, 1, 11, 5)))
    call(params(k, nv, iv=(-1, 1, 3, 5)))
    call(params(k, nv, iv_p=11))
    call(params(k, nv, tar=(4, 3)))
    call(params(k, nv), xf=x)
    call(params(k, nv), xf=x, xg=x)
    call(params(k, nv), lon=x)
    call(params(k, nv), n1=0)
    call(params(k, nv), nl=0)
    bad = params(k, nv)
    bad.cp = 0.0
    call(bad)
    bad = params(k, nv, wmoist=-1.0)
    call(bad)
    with pytest.raises(pkg.LetkfError, match="error -1"):
        c.efso_norm(params(k, nv), nij1, nlev, None, *fs, e, *es)
    # a column whose pressure increases with level: rejected, nothing written
    fc2 = fcst.copy()
    col = fc2[np.arange(nlev) * nij1 + 5, :, IV_P]
    fc2[np.arange(nlev) * nij1 + 5, :, IV_P] = col[::-1]
    f2, _, _, _ = pack(fc2, fcer, "point")
    f20 = f2.clone()
    with pytest.raises(pkg.LetkfError, match="1 column"):
        c.efso_norm(params(k, nv), nij1, nlev, f2, *fs, e, *es, fmean=fm)
    torch.cuda.synchronize()
    assert torch.equal(f2, f20) and torch.equal(e, e0) and bool((fm == 7.0).all())
    # with wlev given, the pressure is not looked at
    c.efso_norm(params(k, nv, iv_p=-1), nij1, nlev, f2, *fs, e, *es, wlev=_d(np.full(nij1 * nlev, 0.25)))
    torch.cuda.synchronize()


def summary_rows(rng, nobs, nterm, nobtype, latbound=20.0):
    elm = rng.choice(ELEM_UID + [9999, -1], nobs).astype(np.int32)
    typ = rng.integers(-1, nobtype + 3, nobs).astype(np.int32)
    lat = rng.choice([latbound, -latbound, np.nextafter(latbound, 99), np.nextafter(-latbound, -99), 0.0, 45.0, -45.0], nobs)
    qc = rng.choice([0, 0, 0, 1], nobs).astype(np.int32)
    obsense = rng.standard_normal((nobs, nterm)) * 10.0 ** rng.uniform(-3, 3, (nobs, 1))
    obsense[rng.random((nobs, nterm)) < 0.1] = 0.0
    return obsense, elm, typ, lat, qc


def run_summary(obsense, elm, typ, lat, nobtype, latbound=20.0, qc=None, elem_uid=ELEM_UID):
    nterm = obsense.shape[1]
    nobs = obsense.shape[0]
    d = lambda a, dt=None: _d(a, dt) if nobs else None
    cnt, s, neg = _ctx().efso_summary(nterm, d(obsense.ravel()), d(elm), d(typ), d(lat), elem_uid, nobtype, latbound,
                                      qc=None if qc is None else d(qc), nobs=nobs)
    torch.cuda.synchronize()
    return cnt.cpu().numpy(), s.cpu().numpy(), neg.cpu().numpy()


@pytest.mark.parametrize("nterm", [1, 2, 3, 4])
@pytest.mark.parametrize("nobs", [0, 1, 5000])
def test_summary_matches_the_sequential_loop(nterm, nobs):
    rng = np.random.default_rng(nterm * 7 + nobs)
    nobtype = 6
    obsense, elm, typ, lat, qc = summary_rows(rng, nobs, nterm, nobtype)
    for q in (None, qc):
        got = run_summary(obsense, elm, typ, lat, nobtype, 20.0, q)
        want = en.summary_loops(obsense, elm, typ, lat, ELEM_UID, nobtype, 20.0, q)
        assert np.array_equal(got[0], want[0])
        assert np.array_equal(_bits(got[1]), _bits(want[1]))
        assert np.array_equal(got[2], want[2])
    if nobs == 0:
        assert not got[0].any() and not got[1].any() and not got[2].any()


def test_summary_argument_errors():
    rng = np.random.default_rng(3)
    obsense, elm, typ, lat, qc = summary_rows(rng, 50, 2, 4)
    c = _ctx()
    outs = (torch.full((3, 5, 7), 5, dtype=torch.int32, device="cuda"), torch.full((2, 3, 5, 7), 5.0, dtype=torch.float64,
                                                                                     device="cuda"),
            torch.full((2, 3, 5, 7), 5, dtype=torch.int32, device="cuda"))
    ob, e, t, la = _d(obsense.ravel()), _d(elm), _d(typ), _d(lat)
    for kw in (dict(nterm=0), dict(nterm=5), dict(nobtype=0), dict(elem_uid=[]), dict(elem_uid=list(range(1, 34))),
               dict(latbound=float("nan")), dict(elm=None)):
        a = dict(nterm=2, obsense=ob, elm=e, typ=t, lat=la, elem_uid=ELEM_UID, nobtype=4, latbound=20.0)
        a.update(kw)
        with pytest.raises(pkg.LetkfError, match="error -1"):
            c.efso_summary(a["nterm"], a["obsense"], a["elm"], a["typ"], a["lat"], a["elem_uid"], a["nobtype"], a["latbound"],
                           nobs=50, outs=outs)
    torch.cuda.synchronize()
    assert bool((outs[0] == 5).all()) and bool((outs[1] == 5.0).all()) and bool((outs[2] == 5).all())


@pytest.mark.parametrize("k,nterm", [(10, 3), (50, 4)])
def test_chain_norm_efso_obsense_summary(k, nterm):
    from _search import build_case, device_struct
    nij1, nlev, nv = 60, 4, 11
    sc = build_case(91, npts=nij1)
    pts, nobs = sc["pts"], sc["nobs"]
    npts = nij1 * nlev
    rng, fcst, _ = case(k + 5, nij1, nlev, k, nv)
    rlev = rng.uniform(2.5e4, 1.0e5, npts)
    rz = rng.uniform(0.0, 12000.0, npts)
    x3 = tuple(rng.standard_normal((npts, nv)) * s for s in (3.0, 3.0, 2.0))
    term = [0, 0, -1, 1, -1, 2, -1, -1, -1, -1, -1]
    if nterm == 4:
        term[6] = 3
    ya = rng.standard_normal((nobs, k))
    dep = rng.standard_normal(nobs)
    t, keep = device_struct(sc, "cuda")
    elm = rng.choice(ELEM_UID, nobs).astype(np.int32)
    typ = rng.integers(1, 6, nobs).astype(np.int32)
    lat = rng.uniform(-60.0, 60.0, nobs)
    wg1 = rng.uniform(0.8, 1.2, nij1)
    # (a) the device norm
    prm = params(k, nv)
    f, fs, e, es = pack(fcst, np.zeros((npts, nv)), "point")
    xs = [pack(fcst, x, "point")[2] for x in x3]
    c = _ctx()
    c.efso_norm(prm, nij1, nlev, f, *fs, e, *es, xf=xs[0], xg=xs[1], xa=xs[2], wg1=_d(wg1))
    # (b) numpy's
    fo, eo, _, _ = en.norm(fcst, None, nij1, IV, IV_P, wg1=wg1, xf=x3[0], xg=x3[1], xa=x3[2])
    fn, _, en_, _ = pack(fo, eo, "point")
    out = []
    for ff, ee in ((f, e), (fn, en_)):
        dj = torch.zeros(nobs * nterm, dtype=torch.float64, device="cuda")
        c.efso_columns(k, nv, term, nterm, t, nij1, nlev, _d(pts["ri"]), _d(pts["rj"]), _d(rlev), _d(rz), _d(ya.ravel()), k,
                       nobs, ff, *fs, ee, *es, dj)
        ob = torch.empty_like(dj)
        c.efso_obsense(nterm, dj, _d(dep), ob)
        cnt, s, neg = c.efso_summary(nterm, ob, _d(elm), _d(typ), _d(lat), ELEM_UID, 4)
        torch.cuda.synchronize()
        out.append((dj.cpu().numpy(), ob.cpu().numpy(), cnt.cpu().numpy(), s.cpu().numpy(), neg.cpu().numpy()))
    (dja, oba, ca, sa, na), (djb, obb, cb, sb, nb) = out
    assert np.abs(dja).max() > 0
    assert np.array_equal(_bits(dja), _bits(djb)) and np.array_equal(_bits(oba), _bits(obb))
    assert np.array_equal(ca, cb) and np.array_equal(_bits(sa), _bits(sb)) and np.array_equal(na, nb)
    want = en.summary_loops(oba.reshape(nobs, nterm), elm, typ, lat, ELEM_UID, 4)
    assert np.array_equal(ca, want[0]) and np.array_equal(_bits(sa), _bits(want[1])) and np.array_equal(na, want[2])
