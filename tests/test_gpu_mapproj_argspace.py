"""The device entries of include/letkf_amd_mapproj.h across their argument space: every refusal returns LETKF_E_INVALID with
the argument named and writes nothing, the overlap refusals, a user stream, and the Python entries with buffers of the
caller."""
import ctypes as C

import numpy as np
import pytest
import torch

import _header
import _mapproj as M

pytestmark = pytest.mark.gpu
CANARY = -777.0
N = 65
INVALID = _header.defines()["LETKF_E_INVALID"]


@pytest.fixture(scope="module")
def env():
    from _gpu import ctx, pkg
    c = ctx()
    p = M.configs()["BDA_d3_1km_9p_bf20"]
    return pkg, c, pkg.mapproj_setup(**M.setup_args(p)), p


def buffers():
    lon, lat = M.points(3, N)
    t = lambda a: torch.from_numpy(a).cuda()
    return dict(a=t(lon), b=t(lat), u=torch.full((N,), CANARY, dtype=torch.float64, device="cuda"),
                v=torch.full((N,), CANARY, dtype=torch.float64, device="cuda"),
                r=torch.full((N, 2), CANARY, dtype=torch.float64, device="cuda"))


def ptr(t, offset=0):
    return None if t is None else C.c_void_p(t.data_ptr() + offset)


def untouched(b):
    torch.cuda.synchronize()
    return all(bool((b[k] == CANARY).all()) for k in ("u", "v", "r"))


def last_error(pkg):
    return pkg.lib().letkf_amd_last_error().decode()


ROW_REFUSALS = [
    ("ctx", "ctx"), ("proj", "proj"), ("n<0", "n must"), ("a", "NULL"), ("b", "NULL"), ("u", "NULL"), ("v", "NULL"),
    ("type", "proj->type"), ("c", "proj->c"), ("dx", "proj->dx"), ("misaligned", "16-byte"),
    ("u=a", "overlaps"), ("v=b", "overlaps"), ("r~a", "overlaps"), ("u=v", "overlaps"), ("r~u", "overlaps"), ("r~v", "overlaps"),
]


@pytest.mark.parametrize("entry", ("letkf_phys2ij_dev", "letkf_ij2phys_dev"))
@pytest.mark.parametrize("what,word", ROW_REFUSALS, ids=[w for w, _ in ROW_REFUSALS])
def test_the_row_entries_refuse_and_write_nothing(env, entry, what, word):
    pkg, ctx, proj, _ = env
    f = getattr(pkg.mapproj_lib(), entry)
    b = buffers()
    big = torch.full((4 * N,), CANARY, dtype=torch.float64, device="cuda")      # for the overlaps: inputs and outputs in one buffer
    bad = pkg.Mapproj.from_buffer_copy(bytes(proj))
    a = dict(ctx=ctx._c, proj=C.addressof(proj), n=N, a=ptr(b["a"]), b=ptr(b["b"]), u=ptr(b["u"]), v=ptr(b["v"]), r=ptr(b["r"]))
    if what in ("ctx", "proj", "a", "b", "u", "v"):
        a[what] = None
    elif what == "n<0":
        a["n"] = -1
    elif what in ("type", "c", "dx"):
        setattr(bad, what, 0)
        a["proj"] = C.addressof(bad)
    elif what == "misaligned":
        a["r"] = ptr(big, 8)
    elif what == "u=a":
        a["u"] = a["a"]
    elif what == "v=b":
        a["v"] = ptr(b["b"], 8 * (N - 1))                       # one element of overlap
    elif what == "r~a":
        a["a"], a["r"] = ptr(big, 16 * N - 16), ptr(big)       # a starts on rotc's last pair
    elif what == "u=v":
        a["v"] = a["u"]
    elif what == "r~u":
        a["u"], a["r"] = ptr(big, 16), ptr(big)
    elif what == "r~v":
        a["v"], a["r"] = ptr(big), ptr(big, 8 * N - 16 + 8)   # rotc (16-byte aligned) starts inside v's last elements
    before_a, before_b = b["a"].clone(), b["b"].clone()
    rc = f(a["ctx"], a["proj"], a["n"], a["a"], a["b"], a["u"], a["v"], a["r"])
    assert rc == INVALID, (what, rc)
    assert word in last_error(pkg), (what, last_error(pkg))
    assert untouched(b) and bool((big == CANARY).all()) and torch.equal(before_a, b["a"]) and torch.equal(before_b, b["b"])


def test_zero_rows_take_null_arrays_and_rotc_is_optional(env):
    pkg, ctx, proj, _ = env
    lib = pkg.mapproj_lib()
    for f in (lib.letkf_phys2ij_dev, lib.letkf_ij2phys_dev):
        assert f(ctx._c, C.addressof(proj), 0, None, None, None, None, None) == 0
        b = buffers()
        assert f(ctx._c, C.addressof(proj), N, ptr(b["a"]), ptr(b["b"]), ptr(b["u"]), ptr(b["v"]), None) == 0
        torch.cuda.synchronize()
        assert bool((b["r"] == CANARY).all()) and not bool((b["u"] == CANARY).any())
        # n rows of longer buffers: the rows behind n stay
        b = buffers()
        assert f(ctx._c, C.addressof(proj), N - 2, ptr(b["a"]), ptr(b["b"]), ptr(b["u"]), ptr(b["v"]), ptr(b["r"])) == 0
        torch.cuda.synchronize()
        assert bool((b["u"][N - 2:] == CANARY).all()) and bool((b["v"][N - 2:] == CANARY).all()) and bool((b["r"][N - 2:] == CANARY).all())
        assert not bool((b["r"][:N - 2] == CANARY).any())


GRID_REFUSALS = [
    ("ctx", dict(ctx=None), "ctx"), ("proj", dict(proj=None), "proj"), ("nlon", dict(nlon=0), "nlon"), ("nlat", dict(nlat=-1), "nlat"),
    ("ihalo", dict(ihalo=-1), "ihalo"), ("jhalo", dict(jhalo=-2), "jhalo"), ("huge", dict(nlon=65536, nlat=32768), "2^31"),
    ("halo-huge", dict(ihalo=2 ** 31 - 2), "2^31"), ("cx1", dict(cx1=np.nan), "cx1"), ("cy1", dict(cy1=np.inf), "cy1"),
    ("all-null", dict(lon=None, lat=None, rotc=None), "all NULL"), ("lon=lat", dict(lat="lon"), "overlaps"),
    ("rotc~lon", dict(rotc="lon"), "overlaps"), ("misaligned", dict(rotc="odd"), "16-byte"),
]


@pytest.mark.parametrize("what,change,word", GRID_REFUSALS, ids=[w for w, _, _ in GRID_REFUSALS])
def test_the_grid_entry_refuses_and_writes_nothing(env, what, change, word):
    pkg, ctx, proj, p = env
    nlon, nlat = 3, 5
    out = {k: torch.full((nlat, nlon) + ((2,) if k == "rotc" else ()), CANARY, dtype=torch.float64, device="cuda") for k in ("lon", "lat", "rotc")}
    big = torch.full((64,), CANARY, dtype=torch.float64, device="cuda")
    a = dict(ctx=ctx._c, proj=C.addressof(proj), nlon=nlon, nlat=nlat, ihalo=2, jhalo=2, cx1=p["cxg1"], cy1=p["cyg1"],
             lon=ptr(out["lon"]), lat=ptr(out["lat"]), rotc=ptr(out["rotc"]))
    for k, v in change.items():
        a[k] = a["lon"] if v == "lon" else ptr(big, 8) if v == "odd" else v
    rc = pkg.mapproj_lib().letkf_mapproj_grid_dev(a["ctx"], a["proj"], a["nlon"], a["nlat"], a["ihalo"], a["jhalo"], a["cx1"], a["cy1"],
                                                  a["lon"], a["lat"], a["rotc"])
    assert rc == INVALID and word in last_error(pkg), (what, rc, last_error(pkg))
    torch.cuda.synchronize()
    assert all(bool((t == CANARY).all()) for t in out.values()) and bool((big == CANARY).all())


def test_a_user_stream_carries_the_calls(env):
    """the context on a stream of the caller's: the results are the default stream's bits, and the work is ordered on that stream
    (an event recorded behind the call completes it)"""
    pkg, ctx, proj, p = env
    lon, lat = M.points(9, 70001)
    t = lambda a: torch.from_numpy(a).cuda()
    want = ctx.phys2ij(proj, t(lon), t(lat))
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    own = pkg.Context(0, s.cuda_stream)
    try:
        dlon, dlat = t(lon), t(lat)
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            got = own.phys2ij(proj, dlon, dlat)
            back = own.ij2phys(proj, got[0], got[1])
            grid = own.mapproj_grid(proj, 3, 5, 2, 2, p["cxg1"], p["cyg1"])
            done = torch.cuda.Event()
            done.record(s)
        done.synchronize()
        for x, y in zip(got, want):
            assert torch.equal(x.view(torch.int64), y.view(torch.int64))
        assert float((back[0] - dlon).abs().max()) <= 2 * M.BOUND_DEG
        st = M.grid(M.setup(p), 3, 5, 2, 2, p["cxg1"], p["cyg1"])
        assert np.abs(grid["lon"].cpu().numpy() - st["lon"]).max() <= 2 * M.BOUND_DEG
    finally:
        torch.cuda.synchronize()
        own.close()


def test_the_python_entries_write_into_the_callers_buffers(env):
    pkg, ctx, proj, p = env
    b = buffers()
    out = ctx.phys2ij(proj, b["a"], b["b"], out=(b["u"], b["v"], b["r"]))
    assert out[0] is b["u"] and out[2] is b["r"]
    fresh = ctx.phys2ij(proj, b["a"], b["b"])
    torch.cuda.synchronize()
    for x, y in zip(out, fresh):
        assert torch.equal(x, y)
    none = ctx.phys2ij(proj, b["a"], b["b"], rotc=False)
    assert none[2] is None and torch.equal(none[0], fresh[0])
    back = ctx.ij2phys(proj, fresh[0], fresh[1], out=(b["u"], b["v"], None))
    torch.cuda.synchronize()
    assert back[2] is None and float((back[0] - b["a"]).abs().max()) <= 2 * M.BOUND_DEG
    with pytest.raises(pkg.LetkfError, match="overlaps"):
        ctx.phys2ij(proj, b["a"], b["b"], out=(b["a"], b["v"], None))
    g = ctx.mapproj_grid(proj, 3, 5, 2, 2, p["cxg1"], p["cyg1"], want=("lat",))
    assert g["lon"] is None and g["rotc"] is None and g["lat"].shape == (5, 3)
    with pytest.raises(pkg.LetkfError, match="all NULL"):
        ctx.mapproj_grid(proj, 3, 5, 2, 2, p["cxg1"], p["cyg1"], want=())
