"""The entries of include/letkf_amd_h08.h against the numpy restatement of tests/_h08.py, on the fixtures
tests/test_h08_statement.py pins: the 12 x 10 domain of tests/test_gpu_obsope_chain.py with 2 .. 130 levels and 1 .. 17 members.

Everything is compared bit for bit except the zenith angle, which goes through six library calls that the device and numpy
implement separately.  Its bound is measured, not fixed: on the statement test's 400 points between 1 and 89 degrees the device's
worst error against the 50-digit value may be at most four times the restatement's worst error against the same value
(test_the_zenith_angle_against_fifty_digits prints both).  In the profile tests, whose points are not those 400, the device and
the restatement may then differ by five times that worst error: four for the one, one for the other."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import _h08 as H
from _argspace import CANARY, canary_buffer
from test_h08_statement import zenith_errors, zenith_points

pytestmark = pytest.mark.gpu
H08_SET = 2
CAN = -7.25e77


@pytest.fixture(scope="module")
def env():
    from _gpu import ctx, pkg
    return pkg, ctx()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def same(got, want):
    """the same bits; a NaN where and only where the other has one (a NaN's payload is the arithmetic unit's own)"""
    if got.shape != want.shape or not np.array_equal(np.isnan(got), np.isnan(want)):
        return False
    fin = ~np.isnan(want)
    return np.array_equal(bits(got)[fin], bits(want)[fin])


def params_of(pkg, p, **kw):
    d = dict(p)
    d.update(kw)
    return pkg.h08_params(**d)


def fields_of(pkg, g, nmem, t3, t2, strides, nv2dd=H.NV2DD, nv3dd=H.NV3DD):
    f = pkg.ObsopeFields()
    for n in ("nlev", "nlon", "nlat", "khalo", "ihalo", "jhalo"):
        setattr(f, n, g[n])
    f.nv3dd, f.nv2dd, f.nmem, f.m0 = nv3dd, nv2dd, nmem, 0
    f.v3d, f.v2d = C.c_void_p(t3.data_ptr()), C.c_void_p(t2.data_ptr())
    for n, v in strides.items():
        setattr(f, n, v)
    return f


@functools.lru_cache(None)
def zenith_bound():
    """the restatement's worst error against the 50-digit value on the statement test's points, degrees"""
    lon, lat = zenith_points()
    return float(zenith_errors(H.zenith(lon, lat, H.params()), lon, lat).max())


def run_profiles(env, case, p, prof_list, layout="ref", rotc=True):
    """one call on the host case; the outputs as numpy, with the elements behind them checked to be untouched"""
    pkg, ctx = env
    g, nmem, nlev, nsel = case["g"], case["nmem"], case["g"]["nlev"], len(prof_list)
    o3 = o2 = 0
    if layout == "ref":
        a3, a2, st = case["v3"], case["v2"], H.reference_strides(g)
    elif layout == "perm":
        a3, a2, st = H.permuted(case, "kjmiv", "ijvm")
    else:
        a3, a2, st, o3, o2 = H.padded(case, canary_buffer)
    t3, t2 = dev(a3).reshape(-1), dev(a2).reshape(-1)
    f = fields_of(pkg, g, nmem, t3[o3:], t2[o2:], st)
    tail = 7
    out = dict(lev3=torch.full((nmem * nsel * 5 * nlev + tail,), CAN, dtype=torch.float64, device="cuda"),
               sfc=torch.full((nmem * nsel * 8 + tail,), CAN, dtype=torch.float64, device="cuda"),
               cloud=torch.full((nmem * nsel * 3 * (nlev - 1) + tail,), CAN, dtype=torch.float64, device="cuda"),
               pflag=torch.full((nsel + tail,), -77, dtype=torch.int32, device="cuda"))
    ctx.h08_profiles(params_of(pkg, p), f, nsel, dev(prof_list), dev(case["ri"]), dev(case["rj"]), dev(case["lon"]), dev(case["lat"]),
                     dev(case["rotc"]) if rotc else None, out=out)
    torch.cuda.synchronize()
    h = {k: v.cpu().numpy() for k, v in out.items()}
    for k in ("lev3", "sfc", "cloud"):
        assert np.all(h[k][-tail:] == CAN), k
    assert np.all(h["pflag"][-tail:] == -77)
    res = dict(lev3=h["lev3"][:-tail].reshape(nmem, nsel, 5, nlev), sfc=h["sfc"][:-tail].reshape(nmem, nsel, 8),
               pflag=h["pflag"][:-tail])
    if p["rttov_units"]:
        res["cloud"] = h["cloud"][:-tail].reshape(nmem, nsel, 3, nlev - 1)
    else:
        assert np.all(h["cloud"] == CAN)                         # not written without rttov_units
        res["cloud"] = None
    return res


def check_profiles(got, want):
    assert np.array_equal(got["pflag"], want["pflag"])
    assert same(got["lev3"], want["lev3"]), "lev3"
    assert same(got["sfc"][..., :7], want["sfc"][..., :7]), "sfc"
    if want["cloud"] is not None:
        assert same(got["cloud"], want["cloud"]), "cloud"
    ok = want["pflag"] == 0
    assert np.all(got["sfc"][:, ~ok, 7] == H.UNDEF)
    dz = np.abs(got["sfc"][:, ok, 7] - want["sfc"][:, ok, 7])
    assert dz.max() <= 5.0 * zenith_bound(), (dz.max(), zenith_bound())
    assert np.all(got["sfc"][:, ok, 7] == got["sfc"][:1, ok, 7])   # the same for every member


# ------------------------------------------------------------------------------------------------------------ the records
@pytest.mark.parametrize("big_endian", [False, True])
@pytest.mark.parametrize("nprof", [0, 1, 63, 64, 65, 1000])
def test_decode_and_encode_are_the_restatement(env, nprof, big_endian):
    pkg, ctx = env
    cols = H.file_cols(nprof, 40 + nprof)
    if nprof:
        cols["elm"][0], cols["typ"][0], cols["dat"][:3] = 8799, -4, [np.nan, 3.0e38 * 10, -0.0]      # rounding, NaN, overflow
    obserr = 1.5 + 0.25 * np.arange(H.NCH)
    image = H.encode(cols, big_endian)
    assert pkg.h08_bytes(nprof) == image.size == 64 * nprof and pkg.h08_count(image.size) == nprof
    bad = image.copy()
    nwrong = 0
    for q in range(0, nprof, 7):                                 # wrong markers: counted, decoded all the same
        bad[64 * q + (60 if q % 2 else 0)] ^= 0x10
        nwrong += 1
    want, nbad = H.decode(bad, obserr, big_endian)
    assert nbad == nwrong
    t = dev(bad) if nprof else torch.empty(0, dtype=torch.uint8, device="cuda")
    got = ctx.h08_decode(t, obserr, big_endian=big_endian, check=True)
    torch.cuda.synchronize()
    assert got["nbad"] == nwrong
    for k in pkg.OBSFILE_COLUMNS:
        g = got[k].cpu().numpy()
        assert g.dtype == want[k].dtype
        assert np.array_equal(g, want[k]) if g.dtype == np.int32 else same(g, want[k]), k
    # NULL columns: only what is asked for is written, and no count without check
    part = ctx.h08_decode(t, obserr, big_endian=big_endian, want=("dat", "lev"))
    assert part["nbad"] is None and part["elm"] is None and same(part["dat"].cpu().numpy(), want["dat"])
    # encode: the image bit for bit, from the columns the decoder gave and from the raw doubles
    for src in (cols, want):
        img = ctx.h08_encode({k: dev(v) for k, v in src.items()}, big_endian=big_endian, nprof=nprof)
        torch.cuda.synchronize()
        assert np.array_equal(img.cpu().numpy(), H.encode(src, big_endian))
    if nprof:
        with pytest.raises(pkg.LetkfError):
            pkg.h08_count(image.size - 4)


# ---------------------------------------------------------------------------------------------------------- the selection
def obsda_rows(nprof, seed, order="file", other=60):
    """set / idx of an obsda table: every row of the Himawari-8 file (file 2) but those of a few profiles, between rows of files 1
    and 3 that name the same idx values"""
    rng = np.random.default_rng(seed)
    skip = set(rng.choice(nprof, size=max(1, nprof // 5), replace=False).tolist()) if nprof > 2 else set()
    idx8 = np.array([fp * H.NCH + c + 1 for fp in range(nprof) if fp not in skip for c in range(H.NCH)], dtype=np.int32)
    set_ = np.concatenate([np.full(other // 2, 1), np.full(idx8.size, H08_SET), np.full(other - other // 2, 3)]).astype(np.int32)
    idx = np.concatenate([rng.integers(1, nprof * H.NCH + 1, other // 2), idx8, rng.integers(1, nprof * H.NCH + 1, other - other // 2)])
    idx = idx.astype(np.int32)
    if order == "shuffled":
        perm = rng.permutation(set_.size)
        set_, idx = set_[perm], idx[perm]
    return set_, idx


@pytest.mark.parametrize("order", ["file", "shuffled"])
@pytest.mark.parametrize("nprof", [1, 40, 700])
def test_select_is_the_restatement(env, nprof, order):
    pkg, ctx = env
    set_, idx = obsda_rows(nprof, 9 + nprof, order)
    idx[:3] = [0, -5, nprof * H.NCH + 1]                          # outside the file: name no profile
    set_[:3] = H08_SET
    n = set_.size
    for row0, nrows, hs in ((0, n, H08_SET), (n // 3, n // 2, H08_SET), (0, n, 1), (0, n, 3), (0, n, 5), (5, 0, H08_SET)):
        wl, ws, wn = H.select(set_, idx, row0, nrows, hs, nprof)
        pl, slot, nsel = ctx.h08_select(dev(set_), dev(idx), hs, nprof, row0=row0, nrows=nrows)
        torch.cuda.synchronize()
        assert nsel == wn
        assert np.array_equal(slot.cpu().numpy(), ws)
        pl = pl.cpu().numpy()
        assert np.array_equal(pl[:nsel], wl) and np.all(pl[nsel:] == -1)       # the rest is not written
    # twice the same bits
    a = ctx.h08_select(dev(set_), dev(idx), H08_SET, nprof)
    b = ctx.h08_select(dev(set_), dev(idx), H08_SET, nprof)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


# ----------------------------------------------------------------------------------------------------------- the profiles
SWITCHES = [dict(top_down=t, stggrd=s, rttov_units=u, cfrac_cnst=c) for t in (0, 1) for s in (0, 1) for u in (0, 1) for c in (0.1, 0.0)]


@pytest.mark.parametrize("n", range(len(H.SIZES)))
def test_profiles_are_the_restatement_at_every_size(env, n):
    nlev, nmem, seed = H.SIZES[n]
    case = H.make_case(nlev, nmem, seed)
    z = H.zenith(case["lon"], case["lat"], H.params())
    assert np.all((z > 1.0) | (np.arange(case["nprof"]) == 4))   # (the bound on the zenith angle is measured above 1 degree)
    prof_list = np.arange(case["nprof"], dtype=np.int32)
    for sw in (SWITCHES[(3 * n) % 16], SWITCHES[(3 * n + 5) % 16], SWITCHES[(3 * n + 10) % 16]):
        p = H.params(nlev=nlev, nprof_file=case["nprof"], **sw)
        rot = sw["stggrd"] == sw["top_down"]
        want = H.profiles(p, case["g"], case["v3"], case["v2"], prof_list, case["ri"], case["rj"], case["lon"], case["lat"],
                          case["rotc"] if rot else None)
        check_profiles(run_profiles(env, case, p, prof_list, rotc=rot), want)


@pytest.mark.parametrize("sw", SWITCHES)
@pytest.mark.parametrize("rot", [False, True])
def test_profiles_under_every_switch(env, sw, rot):
    case = H.make_case(3, 3, 147)
    prof_list = np.array([0, 1, 2, 3, 4, 5, 9, 17, 18, 39], dtype=np.int32)       # a subset: slots differ from file profiles
    p = H.params(nlev=3, nprof_file=case["nprof"], **sw)
    want = H.profiles(p, case["g"], case["v3"], case["v2"], prof_list, case["ri"], case["rj"], case["lon"], case["lat"],
                      case["rotc"] if rot else None)
    check_profiles(run_profiles(env, case, p, prof_list, rotc=rot), want)


@pytest.mark.parametrize("layout", ["ref", "perm", "padded"])
@pytest.mark.parametrize("size", [(65, 3, 137), (3, 17, 147)])
def test_profiles_in_other_layouts(env, size, layout):
    case = H.make_case(*size)
    prof_list = np.arange(case["nprof"], dtype=np.int32)
    p = H.params(nlev=size[0], nprof_file=case["nprof"], top_down=1, rttov_units=1, stggrd=1, ri_off=0.0)
    want = H.profiles(p, case["g"], case["v3"], case["v2"], prof_list, case["ri"], case["rj"], case["lon"], case["lat"], case["rotc"])
    check_profiles(run_profiles(env, case, p, prof_list, layout=layout), want)


def test_profiles_edge_cases(env):
    """an integer coordinate, ri = 1.0 (the clamped index 0 has weight 0 and holds a NaN), outside, NaN, q below qmin, the
    sub-satellite point, offsets of a subdomain, and a NaN in a zero-weight corner that must not spread"""
    case = H.make_case(5, 2, 116)
    case["v3"][:, :, 3, 5, :] = np.nan                           # profile 0 at (7.0, 5.0): corner (i - 1, j - 1) = 0-based (5, 3)
    case["v2"][:, :, 3, 5] = np.nan
    case["ri"], case["rj"] = case["ri"] + 12.0, case["rj"] + 20.0
    prof_list = np.array([0, 1, 2, 3, 4, 5, 6, 7, -1, case["nprof"]], dtype=np.int32)     # the last two: not profiles of the file
    p = H.params(nlev=5, nprof_file=case["nprof"], rttov_units=1, ri_off=12.0, rj_off=20.0)
    want = H.profiles(p, case["g"], case["v3"], case["v2"], prof_list, case["ri"], case["rj"], case["lon"], case["lat"], case["rotc"])
    assert want["pflag"].tolist() == [0, 0, 98, 98, 0, 0, 0, 0, 98, 98]
    assert np.all(np.isfinite(want["lev3"][:, 0])) and np.all(np.isfinite(want["sfc"][:, 0]))
    assert want["sfc"][0, 4, 7] == 0.0                           # the sub-satellite point: finite
    floor = p["qmin"] + p["qmin"] * 0.01
    assert np.all(want["lev3"][:, 5, 2] == floor) and np.all(want["sfc"][:, 5, 1] == floor)
    got = run_profiles(env, case, p, prof_list)
    check_profiles(got, want)
    assert got["sfc"][0, 4, 7] == 0.0


def test_the_zenith_angle_against_fifty_digits(env):
    lon, lat = zenith_points()
    n = lon.size
    case = H.make_case(2, 1, 113, nprof=n)
    case["lon"], case["lat"] = lon, lat
    case["ri"], case["rj"] = np.full(n, 6.5), np.full(n, 6.5)
    p = H.params(nlev=2, nprof_file=n)
    got = run_profiles(env, case, p, np.arange(n, dtype=np.int32))["sfc"][0, :, 7]
    e_dev, e_np = zenith_errors(got, lon, lat).max(), zenith_bound()
    print(f"zenith angle, worst error against the 50-digit value over {n} points: device {e_dev:.3e}, numpy {e_np:.3e} degrees")
    assert e_dev <= 4.0 * e_np


# --------------------------------------------------------------------------------------------------------------- the rows
def run_rows(env, p, set_, idx, slot, nsel, nmem, prof, rt, rig, rjg, kld, m0=0, qc_replace=True, state=None, row0=0, nrows=None,
             h08_set=H08_SET):
    """one call; state = (qc, ensval, lev, val2) numpy, INOUT: returns the new state"""
    pkg, ctx = env
    n = set_.size
    if state is None:
        state = (np.full(n, 90, dtype=np.int32), np.full((n, kld), CAN), np.zeros(n), np.zeros(n))
    qc, ens, lev, val2 = (dev(a) for a in state)
    btall, btclr, trans = rt
    dprof = dict(lev3=dev(prof["lev3"]), sfc=dev(prof["sfc"]), pflag=dev(prof["pflag"]))
    ctx.h08_rows(params_of(pkg, p), dev(set_), dev(idx), h08_set, dev(slot), nsel, dprof, dev(btall), dev(btclr), dev(trans), dev(rig),
                 dev(rjg), qc, ens, kld, lev, val2, nmem=nmem, m0=m0, qc_replace=qc_replace, row0=row0, nrows=nrows)
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in (qc, ens, lev, val2))


def want_rows(p, set_, idx, slot, nsel, nmem, prof, rt, rig, rjg, kld, m0=0, qc_replace=True, state=None, row0=0, nrows=None,
              h08_set=H08_SET):
    n = set_.size
    if state is None:
        state = (np.full(n, 90, dtype=np.int32), np.full((n, kld), CAN), np.zeros(n), np.zeros(n))
    qc, ens, lev, val2 = (a.copy() for a in state)
    H.rows(p, row0, n - row0 if nrows is None else nrows, set_, idx, h08_set, slot, nsel, nmem, m0, prof, *rt, rig, rjg, qc_replace, qc,
           ens, lev, val2)
    return qc, ens, lev, val2


def check_rows(got, want):
    assert np.array_equal(got[0], want[0]), "qc"
    for k, name in ((1, "ensval"), (2, "lev"), (3, "val2")):
        assert same(got[k], want[k]), name


def sliced(prof, rt, m0, nmem):
    """members m0 .. m0 + nmem - 1 of the profile arrays and of the radiative transfer's"""
    return (dict(lev3=prof["lev3"][m0:m0 + nmem], sfc=prof["sfc"][m0:m0 + nmem], pflag=prof["pflag"]),
            tuple(np.ascontiguousarray(a[m0:m0 + nmem]) for a in rt))


@pytest.mark.parametrize("n", range(len(H.SIZES)))
def test_rows_are_the_restatement_at_every_size(env, n):
    nlev, nmem, seed = H.SIZES[n]
    top_down, units = n % 2, (n // 2) % 2
    case, p, _, prof_all, _ = H.fixture(nlev, nmem, seed, top_down, units)
    set_, idx = obsda_rows(case["nprof"], seed, "shuffled")
    pl, slot, nsel = H.select(set_, idx, 0, set_.size, H08_SET, case["nprof"])
    assert 0 < nsel < case["nprof"]
    prof = H.profiles(p, case["g"], case["v3"], case["v2"], pl, case["ri"], case["rj"], case["lon"], case["lat"], case["rotc"])
    rt = H.stand_in(prof, p)
    q = dict(p, cldsky_thrs=1.0, reject_land=n % 3 == 0, finish=1, member=nmem + 1, ch_use=(1, 1, 0, 1, 1, 2, 1, 1, 1, -1), **H.BUFFER)
    kld = nmem + 2
    args = (set_, idx, slot, nsel, nmem, prof, rt, case["ri"], case["rj"], kld)
    want = want_rows(q, *args, m0=1)
    served = np.flatnonzero((set_ == H08_SET) & (idx >= 1))
    assert set(np.unique(want[0][served])) >= {0, 50, 98} and np.all(want[0][set_ != H08_SET] == 90)
    assert np.all(want[1][:, 0] == CAN) and np.all(want[1][:, -1] == CAN)      # the columns beside m0 .. m0 + nmem - 1
    check_rows(run_rows(env, q, *args, m0=1), want)
    check_rows(run_rows(env, q, *args, m0=1), want)                            # the same bits from call to call


def small_rows(nlev=3, nmem=3, seed=147, nprof_used=6):
    case, p, _, _, _ = H.fixture(nlev, nmem, seed)
    idx = np.array([fp * H.NCH + c + 1 for fp in (0, 2, 5, 9, 17, 20)[:nprof_used] for c in range(H.NCH)], dtype=np.int32)
    set_ = np.full(idx.size, H08_SET, dtype=np.int32)
    pl, slot, nsel = H.select(set_, idx, 0, set_.size, H08_SET, case["nprof"])
    prof = H.profiles(p, case["g"], case["v3"], case["v2"], pl, case["ri"], case["rj"], case["lon"], case["lat"], case["rotc"])
    return case, p, set_, idx, slot, nsel, prof, H.stand_in(prof, p)


def test_rows_under_every_ch_use_pattern(env):
    case, p, set_, idx, slot, nsel, prof, rt = small_rows(nmem=1, seed=116, nprof_used=2)
    args = (set_, idx, slot, nsel, 1, prof, rt, case["ri"], case["rj"], 1)
    for pattern in range(1 << H.NCH):
        use = tuple((pattern >> c) & 1 for c in range(H.NCH))
        q = dict(p, ch_use=use)
        want = want_rows(q, *args)
        assert np.array_equal(want[0][:H.NCH] == 0, np.array(use) == 1)
        got = run_rows(env, q, *args)
        assert np.array_equal(got[0], want[0]), pattern
    q = dict(p, ch_use=(2, -1, 0, 1, 1, 1, 1, 1, 1, 1))                        # only the value 1 uses a channel
    check_rows(run_rows(env, q, *args), want_rows(q, *args))


@pytest.mark.parametrize("reject_land", [0, 1])
@pytest.mark.parametrize("box", [False, True])
@pytest.mark.parametrize("thrs", [-5.0, 1.0])
def test_rows_land_buffer_and_sky(env, reject_land, box, thrs):
    case, p, set_, idx, slot, nsel, prof, rt = small_rows()
    q = dict(p, reject_land=reject_land, cldsky_thrs=thrs, **(H.BUFFER if box else {}))
    args = (set_, idx, slot, nsel, 3, prof, rt, case["ri"], case["rj"], 3)
    want = want_rows(q, *args)
    if thrs < 0.0:
        assert np.all(want[1][want[0] == 0] < 0.0)               # the default: every finite value is cloudy
    else:
        ok = want[1][want[0] != 98]
        assert (ok < 0.0).any() and (ok > 0.0).any()
    check_rows(run_rows(env, q, *args), want)


def test_a_coastal_profile_is_land_in_either_units(env):
    """H08_REJECT_LAND tests the interpolated mask (common_obs_scale.f90:2951): a mask of 0.7 is land, 0.3 is not, and the units the
    profiles were made in change neither"""
    case = H.make_case(3, 3, 147)
    case["ri"][6], case["rj"][6] = 8.3, 4.4                      # 0.7 of the weight on the land block's last column
    case["ri"][7], case["rj"][7] = 8.7, 4.4                      # 0.3
    prof_list = np.array([6, 7], dtype=np.int32)
    idx = np.array([fp * H.NCH + c + 1 for fp in (6, 7) for c in range(H.NCH)], dtype=np.int32)
    set_ = np.full(idx.size, H08_SET, dtype=np.int32)
    slot = np.full(case["nprof"], -1, dtype=np.int32)
    slot[6], slot[7] = 0, 1
    qcs, masks = [], []
    for units in (0, 1):
        p = H.params(nlev=3, nprof_file=case["nprof"], rttov_units=units, reject_land=1)
        want = H.profiles(p, case["g"], case["v3"], case["v2"], prof_list, case["ri"], case["rj"], case["lon"], case["lat"], case["rotc"])
        assert np.all(np.abs(want["sfc"][:, 0, 6] - 0.7) < 1e-12) and np.all(np.abs(want["sfc"][:, 1, 6] - 0.3) < 1e-12)
        got = run_profiles(env, case, p, prof_list)
        check_profiles(got, want)
        rt = H.stand_in(want, p)
        args = (set_, idx, slot, 2, 3, got, rt, case["ri"], case["rj"], 3)
        rows_w = want_rows(p, *args)
        assert rows_w[0].tolist() == [50] * H.NCH + [0] * H.NCH
        rows_g = run_rows(env, p, *args)
        check_rows(rows_g, rows_w)
        qcs.append(rows_g[0])
        masks.append(got["sfc"][..., 6])
    assert np.array_equal(qcs[0], qcs[1]) and same(masks[0], masks[1])


@pytest.mark.parametrize("qc_replace", [False, True])
@pytest.mark.parametrize("finish", [0, 1])
def test_rows_in_two_calls_are_one_call(env, qc_replace, finish):
    nlev, nmem, seed = 63, 3, 119
    case, p, set_, idx, slot, nsel, prof, rt = small_rows(nlev, nmem, seed)
    n, kld, half = set_.size, nmem + 1, nmem // 2
    q = dict(p, finish=finish, member=nmem, cldsky_thrs=1.0, **H.BUFFER)
    rng = np.random.default_rng(4)
    start = (rng.choice([0, 10, 60, 90, 99], n).astype(np.int32), np.full((n, kld), CAN), rng.standard_normal(n), rng.standard_normal(n))
    base = (set_, idx, slot, nsel)
    one = run_rows(env, q, *base, nmem, prof, rt, case["ri"], case["rj"], kld, qc_replace=qc_replace, state=start)
    check_rows(one, want_rows(q, *base, nmem, prof, rt, case["ri"], case["rj"], kld, qc_replace=qc_replace, state=start))
    pa, ra = sliced(prof, rt, 0, half)
    pb, rb = sliced(prof, rt, half, nmem - half)
    first = run_rows(env, dict(q, finish=0), *base, half, pa, ra, case["ri"], case["rj"], kld, qc_replace=qc_replace, state=start)
    both = run_rows(env, q, *base, nmem - half, pb, rb, case["ri"], case["rj"], kld, m0=half, qc_replace=False, state=first)
    check_rows(both, one)
    if qc_replace:
        assert not np.array_equal(one[0], start[0])
    else:
        assert np.all(one[0] >= start[0])


def test_rows_without_report_type_23(env):
    case, p, set_, idx, slot, nsel, prof, rt = small_rows()
    q = dict(p, use_obs23=0)
    n = set_.size
    for qc_replace in (False, True):
        start = (np.where(np.arange(n) % 2, 98, 10).astype(np.int32), np.full((n, 3), CAN), np.full(n, 1.5), np.full(n, 2.5))
        args = (set_, idx, slot, nsel, 3, prof, rt, case["ri"], case["rj"], 3)
        want = want_rows(q, *args, qc_replace=qc_replace, state=start)
        assert set(want[0].tolist()) == ({90} if qc_replace else {90, 98}) and np.all(want[1] == CAN) and np.all(want[2] == 1.5)
        check_rows(run_rows(env, q, *args, qc_replace=qc_replace, state=start), want)
        # ... and a host that made no profiles and called no radiative transfer passes NULL for what they would have given
        pkg, ctx = env
        qc = dev(start[0])
        none = dict(lev3=None, sfc=None, pflag=None)
        ctx.h08_rows(params_of(pkg, q), dev(set_), dev(idx), H08_SET, dev(slot), nsel, none, None, None, None, None, None, qc, None, 3,
                     None, None, nmem=3, qc_replace=qc_replace)
        torch.cuda.synchronize()
        assert np.array_equal(qc.cpu().numpy(), want[0])


@pytest.mark.parametrize("nlev", [8, 64, 65, 130])
@pytest.mark.parametrize("kind", ["first", "later", "nan", "nan1"])
@pytest.mark.parametrize("top_down", [0, 1])
def test_rows_ties_and_nan_weights(env, nlev, kind, top_down):
    lev3, trans, win = H.tie_fixture(nlev, kind)
    if top_down:
        lev3, trans = np.ascontiguousarray(lev3[..., ::-1]), np.ascontiguousarray(trans[..., ::-1])
    prof = dict(lev3=lev3, sfc=np.zeros((1, 1, 8)), pflag=np.zeros(1, dtype=np.int32))
    rt = (np.full((1, 1, H.NCH), 250.0), np.full((1, 1, H.NCH), 251.0), trans)
    p = H.params(nlev=nlev, nprof_file=3, top_down=top_down)
    set_, idx = np.full(H.NCH, H08_SET, dtype=np.int32), (H.NCH + 1 + np.arange(H.NCH)).astype(np.int32)      # profile 1 of 3
    slot = np.array([-1, 0, -1], dtype=np.int32)
    args = (set_, idx, slot, 1, 1, prof, rt, np.zeros(3), np.zeros(3), 1)
    want = want_rows(p, *args)
    prs = 1048576.0 - 8192.0 * np.arange(nlev)
    assert np.all(want[2] == (prs[win] + prs[win - 1]) * 0.5)
    check_rows(run_rows(env, p, *args), want)


def test_rows_of_other_files_and_unselected_profiles_stay(env):
    case, p, _, prof_all, _ = H.fixture(3, 17, 147)
    set_, idx = obsda_rows(case["nprof"], 77, "shuffled")
    n = set_.size
    third = n // 3
    pl, slot, nsel = H.select(set_, idx, third, 12, H08_SET, case["nprof"])             # the profiles a dozen rows name, no more
    prof = H.profiles(p, case["g"], case["v3"], case["v2"], pl, case["ri"], case["rj"], case["lon"], case["lat"], None)
    rt = H.stand_in(prof, p)
    rng = np.random.default_rng(8)
    start = (rng.integers(0, 99, n).astype(np.int32), canary_buffer(n * 17).reshape(n, 17), canary_buffer(n), canary_buffer(n))
    lev0 = start[2].copy()
    served = (set_ == H08_SET) & (slot[np.clip((idx - 1) // H.NCH, 0, case["nprof"] - 1)] >= 0)
    start[2][served], start[3][served] = 0.0, 0.0
    args = (set_, idx, slot, nsel, 17, prof, rt, case["ri"], case["rj"], 17)
    got = run_rows(env, p, *args, state=start)
    check_rows(got, want_rows(p, *args, state=start))
    assert 0 < nsel <= 12 and served.sum() >= 10 * nsel - 10 and (~served & (set_ == H08_SET)).sum() > 100
    assert np.array_equal(got[0][~served], start[0][~served])
    assert np.all(bits(got[1][~served]) == CANARY) and np.all(bits(got[2][~served]) == CANARY) and np.all(bits(got[3][~served]) == CANARY)
    assert not np.any(bits(got[1][served]) == CANARY) and np.all(bits(lev0) == CANARY)
    # a sub-range of the rows: the rows outside it stay, whatever they name
    sub = run_rows(env, p, *args, state=start, row0=third, nrows=third)
    inside = np.zeros(n, dtype=bool)
    inside[third:2 * third] = True
    check_rows(sub, want_rows(p, *args, state=start, row0=third, nrows=third))
    assert np.all(bits(sub[1][~inside]) == CANARY)


# ---------------------------------------------------------------------------------------------------------- the refusals
def test_refusals(env):
    pkg, ctx = env
    case, p, set_, idx, slot, nsel, prof, rt = small_rows()
    g, nmem = case["g"], case["nmem"]
    t3, t2 = dev(case["v3"]), dev(case["v2"])
    # (each in a buffer longer than any output's extent, so that an output laid on it overlaps it and nothing beside it)
    d = {k: dev(np.concatenate([case[k], np.zeros(1024)])) for k in ("ri", "rj", "lon", "lat")}
    pl = dev(np.arange(4, dtype=np.int32))

    def refused(call, word):
        with pytest.raises(pkg.LetkfError) as e:
            call()
        assert word in str(e.value), (word, str(e.value))

    def profiles(pp=None, nsel_=4, out=None, **fkw):
        f = fields_of(pkg, g, nmem, t3, t2, H.reference_strides(g))
        for k, v in fkw.items():
            setattr(f, k, v)
        return ctx.h08_profiles(params_of(pkg, p, **(pp or {})), f, nsel_, pl, d["ri"], d["rj"], d["lon"], d["lat"], None, out=out)

    profiles()                                                                           # the call itself is fine
    for fkw, word in ((dict(nlev=1), "nlev"), (dict(nlon=0), "nlon"), (dict(jhalo=-1), "halo"), (dict(nv3dd=12), "nv3dd"),
                      (dict(nv2dd=8), "nv2dd"), (dict(s3k=0), "stride"), (dict(s2m=0), "stride"), (dict(nmem=0), "nmem"),
                      (dict(v3d=None), "v3d")):
        refused(lambda: profiles(**fkw), word)
    for pp, word in ((dict(rd=0.0), "rd"), (dict(rv=np.nan), "rv"), (dict(q_ppmv=-1.0), "q_ppmv"), (dict(qmin=np.inf), "qmin"),
                     (dict(nlev=4), "nlev")):
        refused(lambda: profiles(pp), word)
    good = dict(lev3=torch.empty(nmem * 4 * 5 * 3, dtype=torch.float64, device="cuda"), sfc=torch.empty(nmem * 4 * 8, dtype=torch.float64, device="cuda"),
                cloud=None, pflag=torch.empty(4, dtype=torch.int32, device="cuda"))
    refused(lambda: profiles(dict(rttov_units=1), out=good), "cloud")
    refused(lambda: profiles(nsel_=-1, out=good), "nsel")
    refused(lambda: profiles(out=dict(good, sfc=None)), "sfc")
    refused(lambda: profiles(out=dict(good, sfc=good["lev3"])), "overlaps")
    refused(lambda: profiles(out=dict(good, pflag=pl)), "overlaps")
    refused(lambda: profiles(out=dict(good, sfc=d["ri"])), "overlaps ri")
    refused(lambda: profiles(out=dict(good, sfc=d["lat"])), "overlaps lat")
    refused(lambda: profiles(out=dict(good, lev3=t3)), "overlaps fields->v3d")
    refused(lambda: profiles(out=dict(good, sfc=t2)), "overlaps fields->v2d")
    refused(lambda: profiles(dict(nprof_file=-1)), "nprof_file")
    profiles(nsel_=0)                                                                    # zero profiles: no error

    kld = 3
    n = set_.size
    qc, ens = dev(np.zeros(n, dtype=np.int32)), dev(np.full((n, kld), CAN))
    lev, val2 = dev(np.zeros(n)), dev(np.zeros(n))
    dp = dict(lev3=dev(prof["lev3"]), sfc=dev(prof["sfc"]), pflag=dev(prof["pflag"]))
    drt = tuple(dev(a) for a in rt)

    def rows(pp=None, h08_set=H08_SET, ens_=ens, lev_=lev, **kw):
        kw = dict(dict(nmem=3, m0=0), **kw)
        return ctx.h08_rows(params_of(pkg, p, **(pp or {})), dev(set_), dev(idx), h08_set, dev(slot), nsel, dp, *drt, d["ri"], d["rj"], qc,
                            ens_, kld, lev_, val2, **kw)

    rows()
    for kw, word in ((dict(nmem=0), "nmem"), (dict(m0=1), "m0"), (dict(m0=-1), "m0"), (dict(nrows=-1), "nrows"), (dict(row0=-1), "row0")):
        refused(lambda: rows(**kw), word)
    refused(lambda: rows(h08_set=0), "h08_set")
    refused(lambda: rows(h08_set=17), "h08_set")
    refused(lambda: rows(dict(nlev=1)), "nlev")
    refused(lambda: rows(dict(finish=1, member=0)), "member")
    refused(lambda: rows(lev_=None), "lev")
    refused(lambda: rows(ens_=drt[2]), "overlaps")
    refused(lambda: rows(lev_=val2), "overlaps")
    refused(lambda: rows(lev_=d["rj"]), "overlaps rjg")
    torch.cuda.synchronize()
    assert np.all(ens.cpu().numpy() != CAN)                                              # (the good call wrote; no refused one did after it)
    rows(nrows=0)

    refused(lambda: ctx.h08_select(dev(set_), dev(idx), 0, 40), "h08_set")
    refused(lambda: ctx.h08_select(dev(set_), dev(idx), H08_SET, -1, prof_list=pl, slot_of_prof=pl), "nprof_file")
    refused(lambda: ctx.h08_select(dev(set_), dev(idx), H08_SET, 40, nrows=-2), "nrows")
    both = torch.empty(40, dtype=torch.int32, device="cuda")
    refused(lambda: ctx.h08_select(dev(set_), dev(idx), H08_SET, 40, prof_list=both, slot_of_prof=both), "overlaps")
    assert ctx.h08_select(dev(set_), dev(idx), H08_SET, 0)[2] == 0

    image = dev(H.encode(H.file_cols(3, 1), False))
    err = np.ones(H.NCH)
    refused(lambda: ctx.h08_decode(image[1:], err, nprof=2), "aligned")
    refused(lambda: ctx.h08_decode(image, err, nprof=-1, out={}), "nprof")
    refused(lambda: ctx.h08_decode(image, err, out=dict(dat=image.view(torch.float64))), "overlaps")
    cols = {k: dev(v) for k, v in H.file_cols(3, 1).items()}
    refused(lambda: ctx.h08_encode(dict(cols, lat=None)), "lat")
    refused(lambda: ctx.h08_encode(cols, out=torch.empty(200, dtype=torch.uint8, device="cuda")[1:]), "aligned")
    refused(lambda: ctx.h08_encode(cols, out=cols["dat"]), "overlaps")
    for call in (lambda: pkg.h08_count(-64), lambda: pkg.h08_count(65), lambda: pkg.h08_bytes(-1)):
        with pytest.raises(pkg.LetkfError):
            call()
    assert pkg.h08_count(0) == 0 and pkg.h08_bytes(0) == 0
