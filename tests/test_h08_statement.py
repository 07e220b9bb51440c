"""The fixtures and the numpy restatement of tests/_h08.py, pinned without a device so that no device test can hide behind them:
every seeded (member, profile, channel) has a clear weighting-function peak, the exact-tie fixtures are exactly representable,
the cloudy / land / buffer shares are where a test of those branches needs them, and the zenith angle's restatement is held to a
50-digit evaluation of the same formula."""
import numpy as np
import pytest

import _h08 as H

ZENITH_POINTS = 400


def zenith_points():
    """(lon, lat) whose zenith angle lies between 1 and 89 degrees, seeded"""
    rng = np.random.default_rng(5)
    p = H.params()
    lon, lat = p["sub_lon"] + rng.uniform(-80.0, 80.0, 4 * ZENITH_POINTS), rng.uniform(-80.0, 80.0, 4 * ZENITH_POINTS)
    z = H.zenith(lon, lat, p)
    keep = np.flatnonzero((z > 1.0) & (z < 89.0))[:ZENITH_POINTS]
    assert keep.size == ZENITH_POINTS
    return lon[keep], lat[keep]


def zenith_errors(got, lon, lat):
    """|got - the 50-digit value| per point, in degrees"""
    p = H.params()
    return np.array([abs(float(H.zenith_mp(a, b, p) - float(g))) for a, b, g in zip(lon, lat, got)])


@pytest.mark.parametrize("size", H.SIZES)
def test_every_seeded_row_has_a_clear_peak(size):
    case, p, _, prof, (btall, btclr, trans) = H.fixture(*size)
    ok = np.flatnonzero(prof["pflag"] == 0)
    assert ok.size >= case["nprof"] - 2
    worst = np.inf
    for m in range(case["nmem"]):
        for s in ok:
            for c in range(H.NCH):
                w = H.weights(prof["lev3"][m, s, 0], trans[m, s, c])
                assert np.all(np.isfinite(w)) and np.all(np.diff(trans[m, s, c]) > 0.0)       # monotone towards the top
                if w.size > 1:
                    top = np.sort(w)[-2:]
                    worst = min(worst, (top[1] - top[0]) / top[1])
                    j = H.peak(prof["lev3"][m, s, 0], trans[m, s, c])[1]
                    assert j == int(np.argmax(w)) + 1
                    if size[0] >= 63:
                        assert 1 < j < size[0] - 1, "the peak is not inside the column"
    print(f"nlev {size[0]}: smallest relative gap between the two largest weights {worst:.3e}")
    assert worst >= 1e-9


@pytest.mark.parametrize("nlev", [8, 64, 65, 130])
@pytest.mark.parametrize("kind", ["first", "later", "nan", "nan1"])
def test_the_tie_fixtures_are_exact(nlev, kind):
    lev3, trans, win = H.tie_fixture(nlev, kind)
    prs, tau = lev3[0, 0, 0], trans[0, 0, 0]
    assert np.all(prs == np.round(prs)) and np.all(np.diff(prs) == -8192.0)
    fin = np.isfinite(tau)
    assert np.all(tau[fin] * 1024.0 == np.round(tau[fin] * 1024.0)) and np.all(np.abs(tau[fin]) < 1.0)
    w = H.weights(prs, tau)
    wf = w[np.isfinite(w)]
    assert np.all(wf * 2.0 ** 23 == np.round(wf * 2.0 ** 23))                                # no weight was rounded
    if kind == "nan1":
        assert np.isnan(w[0]) and np.nanmax(w) == w[nlev - 2]
    else:
        assert (w == np.nanmax(w)).sum() == 2 and int(np.flatnonzero(w == np.nanmax(w))[0]) + 1 == win
    if kind == "nan":
        assert np.isnan(w).sum() == 2
    plev, j = H.peak(prs, tau)
    assert j == win and plev == (prs[win] + prs[win - 1]) * 0.5


@pytest.mark.parametrize("size", H.SIZES)
def test_the_branches_are_populated(size):
    case, p, _, prof, (btall, btclr, trans) = H.fixture(*size)
    ok = prof["pflag"] == 0
    cloudy = (np.abs(btall - btclr) > 1.0)[:, ok]
    land = (prof["sfc"][0, :, 6] > 0.5)[ok]
    b = H.BUFFER
    buf = ((case["ri"] <= b["bris"]) | (case["ri"] >= b["brie"]) | (case["rj"] <= b["brjs"]) | (case["rj"] >= b["brje"]))[ok]
    print(f"nlev {size[0]}: cloudy {cloudy.mean():.2f}, land {land.mean():.2f}, buffer {buf.mean():.2f}")
    assert 0.30 <= cloudy.mean() <= 0.70
    assert 0.20 <= land.mean() <= 0.40
    assert 0.10 <= buf.mean() <= 0.30
    # ... and with the reference's default threshold every finite row is cloudy
    assert np.all(np.abs(btall - btclr)[:, ok] > -5.0)
    assert (prof["pflag"] == H.QC_OUT).sum() == 2 and np.all(prof["lev3"][:, ~ok] == H.UNDEF)


def test_the_rttov_profile_has_the_floor_and_the_layers():
    case, p, _, prof, _ = H.fixture(64, 1, 152, top_down=1, rttov_units=1)
    raw = H.fixture(64, 1, 152)[3]
    floor = p["qmin"] + p["qmin"] * 0.01
    assert np.all(prof["lev3"][0, 5, 2] == floor) and prof["sfc"][0, 5, 1] == floor          # profile 5: q below qmin
    assert np.all(prof["lev3"][0, 0, 2] > 1.0)                                                # ppmv elsewhere
    assert np.array_equal(prof["lev3"][0, 0, 0], (raw["lev3"][0, 0, 0] * 0.01)[::-1])         # hPa, top down
    assert np.array_equal(prof["lev3"][0, 0, 1], raw["lev3"][0, 0, 1][::-1])
    cl = prof["cloud"][0]
    ok = prof["pflag"] == 0
    assert cl.shape == (case["nprof"], 3, 63) and np.all(cl[ok, :2] >= 0.0) and np.all((cl[ok, 2] >= 0.0) & (cl[ok, 2] <= 1.0))
    assert 0.1 < (cl[ok, 2] == 1.0).mean() < 0.9                                              # both sides of min(.., 1)
    frac = prof["sfc"][0, ok, 6]
    assert np.array_equal(frac, raw["sfc"][0, ok, 6]) and ((frac > 0.0) & (frac < 1.0)).any()   # the mask is not converted: rows tests it
    step = H.profiles(H.params(rttov_units=1, cfrac_cnst=0.0, minq=0.1), case["g"], case["v3"], case["v2"], np.arange(8, dtype=np.int32),
                      case["ri"], case["rj"], case["lon"], case["lat"], None)["cloud"]
    assert set(np.unique(step[0, [0, 1, 4, 5, 6, 7], 2])) <= {0.0, 1.0}


def test_the_zenith_restatement_against_fifty_digits():
    p = H.params()
    lon, lat = zenith_points()
    err = zenith_errors(H.zenith(lon, lat, p), lon, lat)
    print(f"zenith restatement: worst error against the 50-digit value {err.max():.3e} degrees over {lon.size} points")
    assert err.max() <= 64 * H.EPS * 90.0                # six library calls deep, each within an ulp or two, angles up to 90
    assert float(H.zenith(p["sub_lon"], 0.0, p)) == 0.0 and float(H.zenith_mp(p["sub_lon"], 0.0, p)) == 0.0


def test_the_codec_round_trips_and_counts_markers():
    cols = H.file_cols(65, 3)
    for be in (False, True):
        img = H.encode(cols, be)
        assert img.size == 64 * 65
        back, nbad = H.decode(img, cols["err"][:H.NCH], be)
        assert nbad == 0
        for k in ("elm", "typ", "lev", "err", "dif"):
            assert np.array_equal(back[k], cols[k]), k
        for k in ("lon", "lat", "dat"):
            assert np.array_equal(back[k], cols[k].astype(np.float32).astype(np.float64)), k
        wrong = img.copy()
        wrong[64 * 7] ^= 1
        wrong[64 * 9 + 60] ^= 1
        assert H.decode(wrong, cols["err"][:H.NCH], be)[1] == 2
    assert H.nint32(np.float32([2.5, -2.5, 0.49999997, np.nan, 3e9, -3e9])).tolist() == [3, -3, 0, 0, 2147483647, -2147483648]


def test_select_restatement():
    set_ = np.array([2, 1, 2, 2, 2, 3, 2], dtype=np.int32)
    idx = np.array([31, 31, 5, 10, 0, 1, 9999], dtype=np.int32)
    pl, slot, nsel = H.select(set_, idx, 0, 7, 2, 6)
    assert pl.tolist() == [0, 3] and slot.tolist() == [0, -1, -1, 1, -1, -1] and nsel == 2
    assert H.select(set_, idx, 1, 2, 2, 6)[0].tolist() == [0]
