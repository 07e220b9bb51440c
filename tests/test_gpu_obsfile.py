"""letkf_obs_decode_dev and letkf_obs_encode_dev (include/letkf_amd_obsfile.h) against the statement of tests/_obsfile.py: every
integer output and every float, compared as its bit pattern, is equal.  The one exception: the dat of a TC position row (ids
99991 / 99992) is within one float32 step of float32(statement x or y) -- the projection carries no bit-for-bit claim -- and the
tests assert that at most those rows differ.  Outputs carry a canary beyond their extent.

Encode-then-decode is the identity where the format scales nothing (radar rows, conventional rows of an id outside the SELECT
CASE); a scaled conventional row passes through x * 0.01f * 100.0f, which is not x for every float32, so those rows are compared
with the statement's round trip instead."""
import functools

import numpy as np
import pytest
import torch

import _mapproj as M
import _obsfile as O

pytestmark = pytest.mark.gpu
ROWS = (0, 1, 63, 64, 65, 257, 4099)
I32_CANARY, F64_CANARY, U8_CANARY, EXTRA = 0x5A5A5A5A, -7.25e77, 0xA5, 16
CONFIG = "BDA_d3_1km_9p_bf20"


@pytest.fixture(scope="module")
def env():
    from _gpu import ctx, pkg
    return pkg, ctx()


@pytest.fixture(scope="module")
def proj(env):
    p = M.configs()[CONFIG]
    return M.setup(p), env[0].mapproj_setup(**M.setup_args(p))


def dev_bytes(data):
    return torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).cuda()


def guarded(n, dtype):
    fill = {torch.int32: I32_CANARY, torch.float64: F64_CANARY, torch.uint8: U8_CANARY}[dtype]
    return torch.full((n + EXTRA,), fill, dtype=dtype, device="cuda")


def intact(t, n):
    fill = {torch.int32: I32_CANARY, torch.float64: F64_CANARY, torch.uint8: U8_CANARY}[t.dtype]
    return bool((t[n:] == fill).all().item())


def guarded_cols(n, names=O.COLUMNS):
    full = {k: guarded(n, torch.int32 if k in ("elm", "typ") else torch.float64) for k in names}
    return full, {k: (full[k][:n] if k in full else None) for k in O.COLUMNS}


def cols_to_dev(cols):
    return {k: torch.from_numpy(np.ascontiguousarray(cols[k])).cuda() for k in O.COLUMNS}


@functools.lru_cache(None)
def conv_case(n):
    rec = O.conv_records(n, seed=n)
    q = M.setup(M.configs()[CONFIG])
    return rec, O.decode_obs(rec, O.CONV, q), O.decode_obs(rec, O.CONV, None)


def check_columns(full, n, st, tc_exempt=True):
    torch.cuda.synchronize()
    tc = np.isin(st["elm"], (O.ID["tclon"], O.ID["tclat"]))
    for k in O.COLUMNS:
        got = full[k][:n].cpu().numpy()
        assert intact(full[k], n), k
        if k == "dat" and tc_exempt:
            assert O.same_bits(got[~tc], st[k][~tc]), k
            assert (O.ulp32_apart(got[tc], st[k][tc]) <= 1).all(), (k, got[tc], st[k][tc])
            assert O.same_bits(got[tc], got[tc].astype(np.float32).astype(np.float64))       # a widened float32
        else:
            assert O.same_bits(got, st[k]), k


@pytest.mark.parametrize("be", [False, True], ids=["le", "be"])
@pytest.mark.parametrize("n", ROWS)
def test_decode_conventional(env, proj, n, be):
    pkg, ctx = env
    rec, st, _ = conv_case(n)
    data = O.frame(rec, be)
    assert pkg.obsfile_count(O.CONV, 8, len(data)) == n and pkg.obsfile_bytes(O.CONV, 8, n) == len(data)
    img = dev_bytes(data)
    full, views = guarded_cols(n)
    res = ctx.obs_decode(img, O.CONV, big_endian=be, proj=proj[1], check=True, out=views)
    assert res["nbad"] == 0 and res["meta"] is None
    check_columns(full, n, st)
    again = ctx.obs_decode(img, O.CONV, big_endian=be, proj=proj[1])           # bitwise equal between two calls
    torch.cuda.synchronize()
    for k in O.COLUMNS:
        assert torch.equal(again[k].view(torch.uint8), full[k][:n].view(torch.uint8)), k


def test_decode_every_id_and_the_single_precision_points(env, proj):
    pkg, ctx = env
    rec, st, st_noproj = conv_case(65)
    assert set(O.ID.values()) | {O.UNKNOWN_ID} == set(st["elm"])
    rh = 5
    assert st["elm"][rh] == O.ID["rh"] and 0.0 < st["err"][rh] < O.TINY          # the denormal is kept
    res = ctx.obs_decode(dev_bytes(O.frame(rec)), O.CONV, proj=proj[1])
    torch.cuda.synchronize()
    assert res["err"][rh].item() == st["err"][rh] == float(np.float32(1e-37) * np.float32(0.01))
    # without a projection: NaN in the dat of the TC position rows, and nowhere else
    full, views = guarded_cols(65)
    ctx.obs_decode(dev_bytes(O.frame(rec)), O.CONV, proj=None, out=views)
    check_columns(full, 65, st_noproj, tc_exempt=False)
    tc = np.isin(st["elm"], (O.ID["tclon"], O.ID["tclat"]))
    assert tc.sum() >= 10 and np.isnan(full["dat"][:65].cpu().numpy()[tc]).all() and not np.isnan(st_noproj["dat"][~tc]).any()


def test_nint_halves_nan_and_saturation(env):
    pkg, ctx = env
    vals = np.array([0.5, -0.5, 2.5, -2.5, 1.5, -1.5, 0.49999997, np.nan, 3e9, -3e9, np.inf, -np.inf, 2 ** 24 + 2.0], dtype=np.float32)
    rec = O.radar_records(len(vals), 7)
    rec[:, 0] = vals
    res = ctx.obs_decode(dev_bytes(O.frame(rec, head=(0, 0, 0))), O.RADAR, nrec=7)
    torch.cuda.synchronize()
    want = [1, -1, 3, -3, 2, -2, 0, 0, O.INT_MAX, O.INT_MIN, O.INT_MAX, O.INT_MIN, 2 ** 24 + 2]
    assert res["elm"].cpu().tolist() == want == [O.nint(v) for v in vals]


@pytest.mark.parametrize("be", [False, True], ids=["le", "be"])
@pytest.mark.parametrize("nrec", [7, 8])
@pytest.mark.parametrize("n", ROWS)
def test_decode_radar(env, n, nrec, be):
    pkg, ctx = env
    rec = O.radar_records(n, nrec, seed=n)
    head = (135.523, 34.823, 120.5)
    data = O.frame(rec, be, head=head)
    assert pkg.obsfile_count(O.RADAR, nrec, len(data)) == n
    st = O.decode_obs(rec, O.RADAR)
    full, views = guarded_cols(n)
    res = ctx.obs_decode(dev_bytes(data), O.RADAR, nrec=nrec, big_endian=be, check=True, out=views)
    check_columns(full, n, st)
    assert res["nbad"] == 0
    assert O.same_bits(res["meta"], np.array(head, dtype=np.float64).astype(np.float32).astype(np.float64))
    if n:
        assert (st["typ"] == 22).all() and (nrec == 8 or (st["dif"] == 0.0).all())


def test_two_bad_markers_are_counted_and_the_rest_decoded(env):
    pkg, ctx = env
    rec = O.radar_records(300, 8, seed=3)
    words = np.frombuffer(O.frame(rec, head=(1, 2, 3)), dtype=np.uint32).copy()
    words[9 + 10 * 17] = 28                  # the first marker of row 17
    words[9 + 10 * 299 + 9] = 0              # the second marker of the last row
    res = ctx.obs_decode(dev_bytes(words.tobytes()), O.RADAR, check=True)
    torch.cuda.synchronize()
    assert res["nbad"] == 2
    st = O.decode_obs(rec, O.RADAR)
    for k in O.COLUMNS:
        assert O.same_bits(res[k].cpu().numpy(), st[k]), k


def encode_and_check(ctx, cols, fmt, nrec, be, missing, meta):
    n = len(cols["elm"])
    want = O.frame(O.encode_obs(cols, fmt, nrec, missing), be, head=meta)
    size = 4 * (O.HEAD_WORDS[fmt] + n * (nrec + 2))
    buf = guarded(size, torch.uint8)
    d = cols_to_dev(cols)
    _, nw = ctx.obs_encode(d, fmt, nrec=nrec, big_endian=be, missing=missing, meta=meta, out=buf[:size])
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    assert nw == O.count(fmt, nrec, len(want))
    assert got[:len(want)].tobytes() == want
    assert (got[len(want):] == U8_CANARY).all()          # nothing behind the survivors, nothing behind the image
    buf2 = guarded(size, torch.uint8)
    ctx.obs_encode(d, fmt, nrec=nrec, big_endian=be, missing=missing, meta=meta, out=buf2[:size])
    torch.cuda.synchronize()
    assert torch.equal(buf, buf2)
    return got[:len(want)].tobytes()


@pytest.mark.parametrize("be", [False, True], ids=["le", "be"])
@pytest.mark.parametrize("n", ROWS)
def test_encode_conventional_then_decode(env, n, be):
    pkg, ctx = env
    cols = O.columns_of(n, seed=n, fmt=O.CONV)
    data = encode_and_check(ctx, cols, O.CONV, 8, be, True, None)
    back = ctx.obs_decode(dev_bytes(data), O.CONV, big_endian=be)
    torch.cuda.synchronize()
    st = O.decode_obs(O.unframe(data, 8, be)[0], O.CONV)
    plain = cols["elm"] == O.UNKNOWN_ID
    for k in O.COLUMNS:
        got = back[k].cpu().numpy()
        assert O.same_bits(got, st[k]), k
        assert O.same_bits(got[plain], cols[k][plain]), k                   # the identity where nothing is scaled


@pytest.mark.parametrize("be", [False, True], ids=["le", "be"])
@pytest.mark.parametrize("nrec", [7, 8])
@pytest.mark.parametrize("n", ROWS)
def test_encode_radar_then_decode_is_the_identity(env, n, nrec, be):
    pkg, ctx = env
    cols = O.decode_obs(O.radar_records(n, nrec, seed=n + 1), O.RADAR)
    data = encode_and_check(ctx, cols, O.RADAR, nrec, be, True, (135.5, 34.75, 88.0))
    back = ctx.obs_decode(dev_bytes(data), O.RADAR, nrec=nrec, big_endian=be)
    torch.cuda.synchronize()
    for k in O.COLUMNS:
        assert O.same_bits(back[k].cpu().numpy(), cols[k]), k
    assert list(back["meta"]) == [135.5, 34.75, 88.0]


STEP = float(np.nextafter(np.float32(O.UNDEF), np.float32(0.0)))     # one float32 step off float32(undef)
UNDEFINED = {
    "none": [],
    "all": "all",
    "ends_and_runs": [0, 1, 599] + list(range(250, 263)) + [511, 512, 513],      # across the blocks of 256 rows
    "every_other": list(range(0, 600, 2)),
}


@pytest.mark.parametrize("fmt,nrec", [(O.CONV, 8), (O.RADAR, 7), (O.RADAR, 8)])
@pytest.mark.parametrize("which", list(UNDEFINED))
def test_encode_without_the_undefined_rows(env, which, fmt, nrec):
    pkg, ctx = env
    n = 600
    cols = O.columns_of(n, seed=11, fmt=fmt)
    gone = np.arange(n) if UNDEFINED[which] == "all" else np.array(UNDEFINED[which], dtype=np.int64)
    cols["dat"][gone] = O.UNDEF
    if which == "ends_and_runs":
        cols["dat"][300] = STEP                          # a defined value next to undef: written
        cols["dat"][301] = float(np.float32(O.UNDEF))    # float32(undef) is not undef in double: written
        assert O.defined(STEP) and O.defined(cols["dat"][301]) and not O.defined(O.UNDEF)
    meta = (135.5, 34.75, 88.0) if fmt == O.RADAR else None
    data = encode_and_check(ctx, cols, fmt, nrec, False, False, meta)
    rec = O.unframe(data, nrec, head=fmt == O.RADAR)[0]
    keep = np.setdiff1d(np.arange(n), gone)
    assert len(rec) == len(keep)
    assert O.same_bits(rec[:, 1].astype(np.float64), cols["lon"][keep])      # the survivors, in their order


def test_encode_big_endian_without_the_undefined_rows(env):
    pkg, ctx = env
    cols = O.columns_of(257, seed=5, fmt=O.CONV)
    cols["dat"][[0, 100, 256]] = O.UNDEF
    encode_and_check(ctx, cols, O.CONV, 8, True, False, None)
