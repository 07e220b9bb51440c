"""The producer of the observation table (include/letkf_amd.h sections 5 and 9: letkf_api_obs.hip's front half, letkf_obsprep.hip,
letkf_setobs.hip) across its argument space, against the oracle (oracle/letkf_oracle.c and tests/native/setobs_oracle.c through
tests/_obsspace.py, tests/_obsprep.py and tests/_setobs.py; tests/test_obsspace_helpers.py holds what _obsspace states itself to
the oracle without a GPU).

Every comparison is bit for bit, integers and doubles alike, with two exceptions that are not this file's: a reflectivity
converted by the device's log10 and what derives from it agree within 2 ulp of the converted dat (tests/test_gpu_setobs.py), and
the gathers, which are plain indexing, are compared with numpy indexing.  One more is stated where it is used: the sign and
payload of a NaN that arithmetic produced are not defined by IEEE 754, so the row with a NaN member must be NaN where the
oracle's is and equal in every other bit.

Every output buffer starts as canaries, what a call must not address is compared bit for bit afterwards, and a second identical
call on a fresh upload must give identical bits (`twice`).  A refusal is run only against a check that is in the code: an
unchecked bad index would reach a kernel."""
import ctypes as C

import numpy as np
import pytest
import torch

import _obsspace as S
import _setobs as SO

pytestmark = pytest.mark.gpu
VP = C.c_void_p
I32, F64 = torch.int32, torch.float64


@pytest.fixture(scope="module")
def env():
    from _gpu import ctx, dev, pkg
    return pkg, ctx(), dev


def num_cu():
    return torch.cuda.get_device_properties(0).multi_processor_count


def down(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def ptr(t):
    return None if t is None else VP(t.data_ptr())


def hp(a):
    return None if a is None else VP(a.ctypes.data)


def call(env, name, *args):
    pkg, ctx, _ = env
    return getattr(pkg.lib(), name)(ctx._c, *args)


def message(env):
    return env[0].lib().letkf_amd_last_error().decode()


def refused(env, rc, name):
    """LETKF_E_INVALID, and the message names the argument"""
    assert rc == S.E_INVALID, (rc, name, message(env))
    assert name in message(env), (name, message(env))


def twice(run):
    a, b = run(), run()
    for x, y in zip(a, b):
        assert S.same_bits(np.asarray(x), np.asarray(y))
    return a


def canaries(a):
    return bool(np.all(S.bits(a) == (S.CANARY if a.dtype == np.float64 else S.ICANARY)))


# ================================================================================================================= departure
def gpu_departure(env, prm, r):
    pkg, ctx, dev = env
    n = len(r["qc"])
    ens, qc, v2, lev = dev(r["ens"]), dev(r["qc"]), dev(r["val2"]), dev(r["lev"])
    val = dev(S.canary_buffer(n))
    prm.h08_lev, prm.h08_val2 = lev.data_ptr(), (v2.data_ptr() if prm.h08_val2 else None)
    ctx.obs_departure(prm, dev(r["elm"]), dev(r["dat"]), dev(r["err"]), ens, r["kld"], val, qc)
    return down(ens), down(val), down(qc), down(v2)


def both_departures(env, r, k, det, h08, with_v2=True, **over):
    def prm(cls):
        p = S.params(cls, k, det, h08=h08, **over)
        p.h08_val2 = 1 if (h08 and with_v2) else None        # a marker: the runners put the address in
        return p
    want = S.oracle_departure(prm(S.QcParams), r)
    got = twice(lambda: gpu_departure(env, prm(env[0].QcParams), r))
    return got, want


def check_departure(env, r, k, det, h08, **over):
    got, want = both_departures(env, r, k, det, h08, **over)
    for name, g, w in zip(("ensval", "val", "qc", "val2"), got, want):
        assert S.same_bits(g, w), name
    ens, val, qc, v2 = got
    cols = k + (1 if det else 0)
    assert S.same_bits(ens[:, cols:], r["ens"][:, cols:])                       # columns the call does not own
    skip = r["qc"] > 0
    assert S.same_bits(ens[skip], r["ens"][skip]) and canaries(val[skip]) and S.same_bits(v2[skip], r["val2"][skip])
    early = np.isin(qc, (S.QC_BAD, S.QC_REFMEM, S.QC_OTYPE)) & ~skip            # rejected before the mean
    assert canaries(val[early]) and S.same_bits(ens[early], r["ens"][early])
    return got


@pytest.mark.parametrize("h08", [0, 1])
@pytest.mark.parametrize("k,det,kld,nobs", S.KLD_CASES)
def test_departure_at_every_kld(env, k, det, kld, nobs, h08):
    """MEMBER = 320 and 1000 are rows of BASELINE's table; each route of the launch, either side of each threshold"""
    r = S.kld_rows(k, kld, nobs)
    ens, val, qc, v2 = check_departure(env, r, k, det, h08)
    live = r["qc"] <= 0
    assert {0, S.QC_GROSS, S.QC_REFMEM, S.QC_BAD} <= set(qc[live].tolist())
    assert h08 == 0 or not S.same_bits(v2, r["val2"])


@pytest.mark.parametrize("k,det,kld", [(5, True, 6), (320, False, 320), (1280, False, 1280)])
@pytest.mark.parametrize("nobs", [1, 63, 64, 65, 128])
def test_departure_tiles(env, nobs, k, det, kld):
    check_departure(env, S.dep_rows(nobs + kld, k, kld, nobs), k, det, 1)


def test_departure_second_trip(env):
    """num_cu * 16 blocks of 64 rows: the rows from num_cu * 1024 on are a block's second trip through its LDS buffer.  They are
    copies of first-trip rows chosen so that every flag the first trip produces is produced again."""
    n0, k, kld = num_cu() * 1024, 2, 3
    r = S.dep_rows(9, k, kld, n0 + 70, nan_pad=False)
    prm = S.params(S.QcParams, k, True, h08=1, min_radar_ref_member=2, min_radar_ref_member_obsref=1)
    first = S.oracle_departure(prm, r)[2][:n0]
    src = np.concatenate([np.nonzero(first == q)[0][:4] for q in np.unique(first)])
    src = np.resize(src, 70)
    for key in ("elm", "dat", "err", "ens", "qc", "lev", "val2"):
        r[key][n0:] = r[key][src]
    ens, val, qc, v2 = check_departure(env, r, k, True, 1, min_radar_ref_member=2, min_radar_ref_member_obsref=1)
    assert set(qc[n0:].tolist()) == set(qc[:n0].tolist()) and len(set(qc.tolist())) >= 6
    assert S.same_bits(ens[n0:], ens[src]) and S.same_bits(val[n0:], val[src])


@pytest.mark.parametrize("h08", [0, 1])
def test_departure_thresholds(env, h08):
    """each comparison of letkf_obs.f90:361-561 at equality and one ulp either side (tests/_obsspace.threshold_rows)"""
    r = S.threshold_rows(h08)
    ens, val, qc, v2 = check_departure(env, r, S.TK, True, h08)
    assert [(n, int(q)) for n, q, w in zip(r["name"], qc, r["want"]) if q != w] == []
    off = check_departure(env, r, S.TK, True, h08, use_radar_ref=0, use_radar_vr=0)[2]
    radar = np.isin(r["elm"], (S.ID_REF, S.ID_REF0, S.ID_VR)) & (r["qc"] <= 0)
    assert np.all(off[radar] == S.QC_OTYPE) and np.array_equal(off[~radar], r["want"][~radar])
    if h08:                                                  # val2 NULL: nothing of it is touched, nothing else changes
        got, want = both_departures(env, r, S.TK, True, 1, with_v2=False)
        assert S.same_bits(got[3], r["val2"]) and S.same_bits(got[0], ens) and np.array_equal(got[2], qc)
        assert S.same_bits(got[0], want[0]) and S.same_bits(got[1], want[1])


@pytest.mark.parametrize("k,kld", [(4, 5), (320, 321)])
def test_departure_nan_member(env, k, kld):
    """One member of one row is NaN: that row's mean, perturbations and departures are NaN, its flag stays (no comparison with a
    NaN is true) -- as the oracle's; the other 63 rows of its tile are what they are without it.  The NaN results are compared
    as NaN (sign and payload of a computed NaN are the processor's choice), every other bit exactly."""
    r = S.dep_rows(77, k, kld, 64)
    at = 17
    r["elm"][at], r["qc"][at], r["dat"][at] = S.ID_U, 0, 1.0
    clean = both_departures(env, r, k, True, 1)[0]
    r["ens"][at, 1] = np.nan
    got, want = both_departures(env, r, k, True, 1)
    others = np.arange(64) != at
    for g, w, c in zip(got, want, clean):
        assert S.same_bits(g[others], w[others]) and S.same_bits(g[others], c[others])
    assert got[2][at] == want[2][at] == 0
    for g, w in ((got[0][at], want[0][at]), (got[1][at:at + 1], want[1][at:at + 1])):
        assert np.array_equal(np.isnan(g), np.isnan(w)) and S.same_bits(g[~np.isnan(w)], w[~np.isnan(w)])
    assert np.isnan(got[0][at, :k]).all() and np.isnan(got[1][at])
    print("NaN row bit-identical to the oracle's:", S.same_bits(got[0][at], want[0][at]))


@pytest.mark.parametrize("k,det", [(320, False), (1000, True)])
def test_set_obs_at_the_benchmarked_member_counts(env, k, det):
    """set_obs_local + finish at MEMBER = 320 and 1000 (BASELINE configs[2] and [4]), a few hundred obsda rows"""
    from test_gpu_setobs import check_finish, check_local, finish_conv, run_local
    nml = SO.namelist()
    w = SO.make_world(200 + k, k=k, det_run=det, nfile_rows=(300, 200), h08=True)
    rk = w["ranks"][0]
    assert 300 < len(rk["qc"]) < 500
    o = SO.oracle_local(w, rk, nml)
    g = run_local(w, rk, nml, both=True)
    g["_set"], g["_idx"] = rk["set"], rk["idx"]
    conv_file, _, _ = check_local(w, g, o)
    check_finish(w, g["tab"], finish_conv(w, [o], 0, conv_file), conv_file)
    assert g["tab"].info().nobstotal > 100
    g["tab"].close()


# ================================================================================================================= mesh sort
def gpu_sort(env, w, r, n_cell0=None):
    pkg, ctx, dev = env
    n = len(r["qc"])
    d = {key: dev(r[key]) for key in ("ctype", "ri", "rj", "qc")}
    n_cell, key = dev(S.canary_buffer(w["ncell"] + 5, np.int32)), dev(S.canary_buffer(n + 5, np.int32))
    ns = C.c_int64(-77)
    m = S.mesh_of(pkg.Mesh, w)
    rc = call(env, "letkf_obs_mesh_sort_dev", C.byref(m), n, ptr(d["ctype"]), ptr(d["ri"]), ptr(d["rj"]), ptr(d["qc"]),
              ptr(n_cell), ptr(key), C.byref(ns))
    for name, t in d.items():
        assert S.same_bits(down(t), r[name]), name
    return rc, down(n_cell), down(key), ns.value


def check_sort(env, w, r):
    want_cell, want_key, want_ns = S.oracle_sort(w, r)
    rc, n_cell, key, ns = twice(lambda: gpu_sort(env, w, r))
    assert rc == 0, message(env)
    n = len(r["qc"])
    assert ns == want_ns and np.array_equal(n_cell[:w["ncell"]], want_cell) and canaries(n_cell[w["ncell"]:])
    assert np.array_equal(key[:n], want_key) and canaries(key[ns:])
    return n_cell, key, ns


@pytest.mark.parametrize("fix", [0, 1])
@pytest.mark.parametrize("nctype", [1, 3])
@pytest.mark.parametrize("ngrd", S.NGRD_PAIRS)
def test_mesh_sort(env, ngrd, nctype, fix):
    """rows on every cell boundary and one ulp either side, on and outside the subdomain's edges, at +-inf, NaN, 1e300 and beyond
    2^31 cells; many rows in one cell (order by row number); rejected rows with garbage ctypes interleaved; an empty type"""
    w = S.mesh_world(ngrd, nctype, fix, rank=(2, 1) if fix else (0, 0))
    r = S.mesh_rows(w)
    n_cell, key, ns = check_sort(env, w, r)
    assert n_cell[:w["ncell"]].max() >= 40 and 0 < ns < len(r["qc"])


def test_mesh_sort_second_trip(env):
    w = S.mesh_world((4, 6), 3, 1)
    n = num_cu() * 4096 + 1000
    rng = np.random.default_rng(4)
    r = dict(ctype=rng.integers(0, 3, n).astype(np.int32), ri=S.IHALO + 0.5 + rng.uniform(-1.0, S.NLON + 1.0, n),
             rj=S.JHALO + 0.5 + rng.uniform(-1.0, S.NLAT + 1.0, n), qc=np.where(rng.random(n) < 0.3, 5, 0).astype(np.int32))
    n_cell, key, ns = check_sort(env, w, r)
    assert (key[:ns] >= num_cu() * 4096).sum() > 500


# ==================================================================================================== halo plan and gathers
def gpu_plan(env, w, me, cap, n_all=None):
    pkg, ctx, dev = env
    na = dev(w["n_all"] if n_all is None else n_all)
    ac, src = dev(S.canary_buffer(w["nacx"] + 5, np.int32)), dev(S.canary_buffer(cap + 5, np.int32))
    nt = C.c_int64(-77)
    lay = S.layout_of(pkg.HaloLayout, w, me)
    rc = call(env, "letkf_obs_halo_plan_dev", C.byref(lay), ptr(na), ptr(ac), ptr(src), cap, C.byref(nt))
    assert np.array_equal(down(na), w["n_all"] if n_all is None else n_all)
    return rc, down(ac), down(src), nt.value


@pytest.mark.parametrize("fix", [0, 1])
@pytest.mark.parametrize("px,py", [(3, 2), (1, 4)])
def test_halo_plan(env, px, py, fix):
    """every rank of a 3 x 2 and a 1 x 4 world of 8 x 12 subdomains, the last rank without a row, type 1 reaching through its
    neighbour into the rank after it; the row map at a capacity of exactly nobstotal and refused, untouched, at one less"""
    w = S.plan_world(px, py, fix, empty_rank=px * py - 1)
    for me in range(px * py):
        want_ac, want_src, want_nt = S.oracle_plan(w, me, w["total"])
        for cap in (w["total"], want_nt):
            rc, ac, src, nt = twice(lambda: gpu_plan(env, w, me, cap))
            assert rc == 0 and nt == want_nt, message(env)
            assert np.array_equal(ac[:w["nacx"]], want_ac) and canaries(ac[w["nacx"]:])
            assert np.array_equal(src[:nt], want_src[:nt]) and canaries(src[nt:])
        rc, ac, src, nt = gpu_plan(env, w, me, want_nt - 1)
        refused(env, rc, "cap")
        assert nt == want_nt and canaries(src)


@pytest.mark.parametrize("ncols,nrows,nsrc", [(1, 37, 20), (7, None, 1000), (1001, 37, 20), (7, 0, 20)])
def test_gather_rows(env, ncols, nrows, nsrc):
    pkg, ctx, dev = env
    nrows = num_cu() * 4096 // 7 + 50 if nrows is None else nrows            # nrows * ncols just above the grid's first trip
    rng = np.random.default_rng(ncols)
    ld_src, ld_dst = ncols + 3, ncols + 2
    src = rng.standard_normal((nsrc, ld_src))
    row = rng.integers(0, nsrc, max(nrows, 1)).astype(np.int32)               # repeated source rows
    row[0] = nsrc - 1

    def run():
        dst, s, r = dev(S.canary_buffer(max(nrows, 1) * ld_dst + 5)), dev(src), dev(row)
        rc = call(env, "letkf_obs_gather_rows_dev", nrows, ptr(r), ncols, ptr(s), ld_src, ptr(dst), ld_dst)
        assert rc == 0 and S.same_bits(down(s), src) and np.array_equal(down(r), row)
        return (down(dst),)
    got = twice(run)[0]
    want = S.canary_buffer(got.size)
    want[:nrows * ld_dst].reshape(nrows, ld_dst)[:, :ncols] = src[row[:nrows], :ncols]
    assert S.same_bits(got, want)


@pytest.mark.parametrize("nrows", [0, 37, None])
def test_gather_i32(env, nrows):
    pkg, ctx, dev = env
    nrows = num_cu() * 4096 + 50 if nrows is None else nrows
    rng = np.random.default_rng(8)
    src = rng.integers(-9, 9, 100).astype(np.int32)
    row = rng.integers(0, 100, max(nrows, 1)).astype(np.int32)

    def run():
        dst = dev(S.canary_buffer(max(nrows, 1) + 5, np.int32))
        assert call(env, "letkf_obs_gather_i32_dev", nrows, ptr(dev(row)), ptr(dev(src)), ptr(dst)) == 0
        return (down(dst),)
    got = twice(run)[0]
    assert np.array_equal(got[:nrows], src[row[:nrows]]) and canaries(got[nrows:])


# ================================================================================================== set_obs behind one call
def copy_dev(address, dtype, n):
    from test_gpu_setobs import _np
    return _np(address, dtype, n)


@pytest.mark.parametrize("fix", [0, 1])
def test_set_obs_three_by_two_world(env, fix):
    """subdomains of 8 x 12 (ngrd_i /= ngrd_j for every type), both statements of ij_obsgrd, through the two halves"""
    from test_gpu_setobs import check_finish, check_local, finish_conv, run_local
    pkg, ctx, dev = env
    nml = SO.namelist()
    w = SO.make_world(40 + fix, px=3, py=2, nlon=8, nlat=12, k=6, det_run=True, nfile_rows=(5000, 2500))
    w["fix_ij_obsgrd"] = fix
    locs = [SO.oracle_local(w, rk, nml) for rk in w["ranks"]]
    assert np.any(locs[0]["dims"]["ngrd_i"] != locs[0]["dims"]["ngrd_j"])
    if fix:                                                  # the two statements sort differently here, or the case is idle
        w0 = dict(w, fix_ij_obsgrd=0)
        assert not np.array_equal(SO.oracle_local(w0, w["ranks"][0], nml)["n_cell"], locs[0]["n_cell"])
    gs = []
    for me, rk in enumerate(w["ranks"]):
        g = run_local(w, rk, nml, me=me)
        g["_set"], g["_idx"] = rk["set"], rk["idx"]
        conv_file, _, _ = check_local(w, g, locs[me])
        gs.append(g)
    infos = [g["tab"].info() for g in gs]
    n_all = torch.stack([dev(copy_dev(i.n_cell, I32, i.ncell)) for i in infos]).contiguous()
    recv = torch.cat([dev(copy_dev(i.sendbuf, F64, i.nsorted * i.ld_send)).view(-1, i.ld_send) for i in infos]).contiguous()
    tot_g = dev(sum(g["tab"].host()["tot_sub"] for g in gs).astype(np.int32).ravel())
    for me, g in enumerate(gs):
        ctx.set_obs_finish(g["tab"], n_all, recv, tot_g=tot_g)
        check_finish(w, g["tab"], finish_conv(w, locs, me, conv_file), conv_file)
        g["tab"].close()


def test_set_obs_second_trip(env):
    """One rank, num_cu * 4096 + 1000 radar file rows, all of them obsda rows, MEMBER 2: preprocess, row_gather, counts,
    pack_send and assemble each make a second trip through their stride loops.  The one case of this file that may take more
    than a few seconds: building the world and the oracle's side of it took 0.5 s + 0.7 s on a CPU for 1 049 768 rows."""
    from test_gpu_setobs import check_finish, check_local, finish_conv, run_local
    n = num_cu() * 4096 + 1000
    nml = SO.namelist()
    w = SO.make_world(5, k=2, det_run=True, nfile_rows=(n, 300), qc_reject=0.0)   # three of eight rows survive the QC: x kld 3
    rk = w["ranks"][0]
    assert len(rk["qc"]) >= n
    o = SO.oracle_local(w, rk, nml)
    g = run_local(w, rk, nml, both=True)
    g["_set"], g["_idx"] = rk["set"], rk["idx"]
    conv_file, _, _ = check_local(w, g, o)
    of = finish_conv(w, [o], 0, conv_file)
    check_finish(w, g["tab"], of, conv_file)
    assert of["nobstotal"] * w["kld"] > num_cu() * 4096
    g["tab"].close()


def small_world(h08=False, **kw):
    return SO.make_world(61, k=3, det_run=True, nfile_rows=(400, 300), h08=h08, **kw)


def test_ctype_merge_tot_g_and_varloc(env):
    """ctype_merge NULL = all zeros; tot_g NULL = the rank's own tot_sub, given = what was given; set_varloc shows in the tables"""
    from test_gpu_setobs import run_local
    pkg, ctx, dev = env
    nml = SO.namelist()
    w = small_world()
    rk = w["ranks"][0]
    seen = []
    for merge in (None, np.zeros(SO.NID_OBS * SO.NOBTYPE, np.int32)):
        f = w["files"]
        d = {k: dev(v) for k, v in f.items()}
        off = np.ascontiguousarray(w["off"], np.int64)
        files = pkg.ObsFileRows(nfile=2, off=off.ctypes.data, **{k: d[k].data_ptr() for k in d})
        p, keep = SO.setobs_params(pkg.SetObsParams, w, nml)
        p.ctype_merge = None if merge is None else merge.ctypes.data
        q = SO.qc_of(w)
        ens, qc, s, i = dev(rk["ensval"]), dev(rk["qc"]), dev(rk["set"]), dev(rk["idx"])
        tab = ctx.set_obs_local(p, q, files, s, i, qc, ens, w["kld"], keep=(keep, d, off, merge))
        info = tab.info()
        given = np.arange(2 * info.nctype, dtype=np.int32) + 100
        n_all, recv = dev(copy_dev(info.n_cell, I32, info.ncell)), dev(copy_dev(info.sendbuf, F64, info.nsorted * info.ld_send))
        ctx.set_obs_finish(tab, n_all, recv.view(-1, info.ld_send), tot_g=None if merge is None else dev(given))
        h = tab.host()
        assert np.array_equal(h["tot_g"], h["tot_sub"] if merge is None else given.reshape(-1, 2))
        t = tab.search_tables()
        nc = info.nctype
        assert np.array_equal(copy_dev(t.varloc, F64, nc), np.ones(nc))
        new = 0.25 + np.arange(nc) / 8.0
        tab.set_varloc(new)
        t = tab.search_tables()
        assert np.array_equal(copy_dev(t.varloc, F64, nc), new)
        seen.append((t.ngroup, copy_dev(t.group_start, I32, t.ngroup + 1), copy_dev(t.group_member, I32, nc), tab.download()))
        tab.close()
    a, b = seen
    assert a[0] == b[0] == len(a[2]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    assert all(S.same_bits(a[3][key], b[3][key]) for key in a[3])


# ================================================================================================================= refusals
def dep_args(env, n=5, k=3, kld=4):
    pkg, ctx, dev = env
    r = S.dep_rows(2, k, kld, n)
    t = dict(elm=dev(r["elm"]), dat=dev(r["dat"]), err=dev(r["err"]), ensval=dev(r["ens"]), val=dev(S.canary_buffer(n)),
             qc=dev(r["qc"]), lev=dev(r["lev"]))
    p = S.params(pkg.QcParams, k, True)
    return r, t, p


def test_refusals_departure(env):
    order = ("elm", "dat", "err", "ensval", "val", "qc")

    def run(name, nobs=5, kld=4, null=None, no_p=False, **prm):
        r, t, p = dep_args(env)
        for key, v in prm.items():
            setattr(p, key, v)
        a = {key: (None if key == null else ptr(t[key])) for key in order}
        rc = call(env, "letkf_obs_departure_dev", None if no_p else C.byref(p), nobs, a["elm"], a["dat"], a["err"], a["ensval"],
                  kld, a["val"], a["qc"])
        refused(env, rc, name)
        assert canaries(down(t["val"])) and S.same_bits(down(t["ensval"]), r["ens"]) and np.array_equal(down(t["qc"]), r["qc"])
    run("p", no_p=True)
    run("nobs", nobs=-1)
    for key in order:
        run(key, null=key)
    run("member", member=0)
    run("kld", kld=2)
    run("kld", kld=3)                                        # MEMBER = 3 with DET_RUN needs 4


def test_refusals_mesh_sort(env):
    pkg, ctx, dev = env
    w = S.mesh_world((4, 6), 3, 1)
    r = S.mesh_rows(w)
    n = len(r["qc"])
    order = ("ctype", "ri", "rj", "qc", "n_cell", "key")

    def run(name, nobs=n, null=None, no_mesh=False, no_ns=False, **mesh):
        d = {key: dev(r[key]) for key in ("ctype", "ri", "rj", "qc")}
        d["n_cell"], d["key"] = dev(S.canary_buffer(w["ncell"], np.int32)), dev(S.canary_buffer(n, np.int32))
        m = S.mesh_of(pkg.Mesh, w)
        for key, v in mesh.items():
            setattr(m, key, v)
        a = {key: (None if key == null else ptr(d[key])) for key in order}
        ns = C.c_int64(-77)
        rc = call(env, "letkf_obs_mesh_sort_dev", None if no_mesh else C.byref(m), nobs, a["ctype"], a["ri"], a["rj"], a["qc"],
                  a["n_cell"], a["key"], None if no_ns else C.byref(ns))
        refused(env, rc, name)
        assert ns.value == -77 and canaries(down(d["n_cell"])) and canaries(down(d["key"]))
    run("mesh", no_mesh=True)
    run("nsorted", no_ns=True)
    for key in order:
        run(key, null=key)
    run("nctype", nctype=0)
    run("ngrd_i", ngrd_i=None)
    run("ngrd_j", ngrd_j=None)
    run("nlon", nlon=0)
    run("nlat", nlat=0)
    run("nobs", nobs=-1)
    zero = np.array([4, 0, 1], np.int32)
    run("ngrd_i", ngrd_i=zero.ctypes.data)


@pytest.mark.parametrize("value", [-1, 3, -(1 << 31), (1 << 31) - 1])
def test_mesh_sort_refuses_a_ctype_outside_the_types(env, value):
    """found on the device, reported with the count's read-back: key and *nsorted untouched, n_cell = the counts of the other
    accepted rows (what the header says it holds), nothing outside the buffers addressed"""
    w = S.mesh_world((4, 6), 3, 1)
    r = S.mesh_rows(w)
    at = np.nonzero(r["qc"] == 0)[0][[3, -1]]
    r["ctype"][at] = value
    rc, n_cell, key, ns = twice(lambda: gpu_sort(env, w, r))
    refused(env, rc, "ctype")
    assert ns == -77 and canaries(key) and canaries(n_cell[w["ncell"]:])
    ok = dict(r, qc=r["qc"].copy())
    ok["qc"][at] = 5
    ok["ctype"] = np.where(ok["qc"] == 0, r["ctype"], 0).astype(np.int32)
    assert np.array_equal(n_cell[:w["ncell"]], S.oracle_sort(w, ok)[0])
    r["qc"][at] = 12                                         # the same rows rejected: their ctype is not read
    assert gpu_sort(env, w, r)[0] == 0


def test_refusals_halo_plan(env):
    pkg, ctx, dev = env
    w = S.plan_world(3, 2, 1)
    cap = w["total"]

    def run(name, null=None, no_lay=False, no_nt=False, cap=cap, n_all=None, **lay):
        na = dev(w["n_all"] if n_all is None else n_all)
        d = dict(n_all=na, ac_ext=dev(S.canary_buffer(w["nacx"], np.int32)), src_row=dev(S.canary_buffer(max(cap, 1), np.int32)))
        layout = S.layout_of(pkg.HaloLayout, w, 1)
        for key, v in lay.items():
            setattr(layout, key, v)
        a = {key: (None if key == null else ptr(t)) for key, t in d.items()}
        nt = C.c_int64(-77)
        rc = call(env, "letkf_obs_halo_plan_dev", None if no_lay else C.byref(layout), a["n_all"], a["ac_ext"], a["src_row"], cap,
                  None if no_nt else C.byref(nt))
        refused(env, rc, name)
        assert nt.value == -77 and canaries(down(d["ac_ext"])) and canaries(down(d["src_row"]))
    run("layout", no_lay=True)
    run("nobstotal", no_nt=True)
    for key in ("n_all", "ac_ext", "src_row"):
        run(key, null=key)
    for key in ("ngrd_i", "ngrd_j", "ngrdsch_i", "ngrdsch_j"):
        run(key, **{key: None})
    run("nctype", nctype=0)
    run("nprocs", nprocs=0)
    run("prc_num_x", prc_num_x=0)
    run("prc_num_x", prc_num_x=4)                            # 6 ranks in rows of 4
    run("myrank", myrank=-1)
    run("myrank", myrank=6)
    run("cap", cap=-1)
    neg = w["n_all"].copy()
    neg[4, 7] = -1
    run("n_all", n_all=neg)
    big = np.zeros_like(w["n_all"])
    big[0, :2] = 1 << 30                                     # a total of 2^31
    run("n_all", n_all=big)


def test_refusals_gathers(env):
    pkg, ctx, dev = env
    src, row = dev(np.arange(40.0)), dev(np.array([1, 0, 3], np.int32))
    isrc = dev(np.arange(10, dtype=np.int32))

    def rows(name, nrows=3, ncols=4, ld_src=5, ld_dst=6, null=None):
        dst = dev(S.canary_buffer(18))
        a = dict(src_row=ptr(row), src=ptr(src), dst=ptr(dst))
        a[null] = None
        rc = call(env, "letkf_obs_gather_rows_dev", nrows, a["src_row"], ncols, a["src"], ld_src, a["dst"], ld_dst)
        refused(env, rc, name)
        assert canaries(down(dst))
    rows("nrows", nrows=-1)
    rows("ncols", ncols=-1)
    for key in ("src_row", "src", "dst"):
        rows(key, null=key)
    rows("ld_src", ld_src=3)
    rows("ld_dst", ld_dst=3)

    def ints(name, nrows=3, null=None):
        dst = dev(S.canary_buffer(3, np.int32))
        a = dict(src_row=ptr(row), src=ptr(isrc), dst=ptr(dst))
        a[null] = None
        refused(env, call(env, "letkf_obs_gather_i32_dev", nrows, a["src_row"], a["src"], a["dst"]), name)
        assert canaries(down(dst))
    ints("nrows", nrows=-1)
    for key in ("src_row", "src", "dst"):
        ints(key, null=key)


def test_refusals_mesh_dims(env):
    pkg = env[0]
    ins = dict(typ_ctype=np.array([1, 8, 22], np.int32), hori_loc_ctype=np.array([4000.0, 5000.0, 2500.0]),
               obs_sort_grid_spacing=SO.namelist()["obs_sort_grid_spacing"], max_nobs_per_grid=SO.namelist()["max_nobs_per_grid"],
               obs_min_spacing=SO.namelist()["obs_min_spacing"])
    outs = ("ngrd_i", "ngrd_j", "grdspc_i", "grdspc_j", "ngrdsch_i", "ngrdsch_j", "ngrdext_i", "ngrdext_j")

    def run(name, nctype=3, nobtype=SO.NOBTYPE, nlon=8, nlat=12, null=None, typ=None):
        i = dict(ins, typ_ctype=ins["typ_ctype"] if typ is None else np.array(typ, np.int32))
        o = {key: S.canary_buffer(3, np.float64 if key.startswith("grdspc") else np.int32) for key in outs}
        a = {key: (None if key == null else hp(v)) for key, v in {**i, **o}.items()}
        rc = pkg.lib().letkf_obs_mesh_dims(nctype, a["typ_ctype"], a["hori_loc_ctype"], nobtype, a["obs_sort_grid_spacing"],
                                           a["max_nobs_per_grid"], a["obs_min_spacing"], 1000.0, 1000.0, nlon, nlat,
                                           *[a[key] for key in outs])
        refused(env, rc, name)
        assert all(canaries(v) for v in o.values())
    for key in list(ins) + list(outs):
        run(key, null=key)
    run("nctype", nctype=-1)
    run("nobtype", nobtype=0)
    run("nlon", nlon=0)
    run("nlat", nlat=0)
    run("typ_ctype", typ=[1, 0, 22])
    run("typ_ctype", typ=[1, 8, SO.NOBTYPE + 1])


class Local:
    """the arguments of letkf_set_obs_local_dev for a small one-rank world, each open to one change"""

    def __init__(self, env, h08=False):
        pkg, ctx, dev = env
        self.env, self.w = env, small_world(h08)
        self.nml = SO.namelist()
        self.rk = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in self.w["ranks"][0].items()}
        self.f = {k: v.copy() for k, v in self.w["files"].items()}
        self.off = np.ascontiguousarray(self.w["off"], np.int64)
        self.p, self.keep = SO.setobs_params(pkg.SetObsParams, self.w, self.nml)
        self.q = SO.qc_of(self.w)
        self.null, self.nobs, self.kld, self.nfile = set(), len(self.rk["qc"]), self.w["kld"], 2
        self.no = set()

    def run(self, entry="letkf_set_obs_local_dev"):
        pkg, ctx, dev = self.env
        d = {k: dev(v) for k, v in self.f.items()}
        files = pkg.ObsFileRows(nfile=self.nfile, off=None if "off" in self.null else self.off.ctypes.data,
                                **{k: (None if k in self.null else t.data_ptr()) for k, t in d.items()})
        o = {k: dev(self.rk[k]) for k in ("set", "idx", "qc", "ensval", "lev", "val2")}
        if self.w["h08"] and "h08_lev" not in self.null:
            self.q.h08_lev, self.q.h08_val2 = o["lev"].data_ptr(), o["val2"].data_ptr()
        a = {k: (None if k in self.null else ptr(o[k])) for k in ("set", "idx", "qc", "ensval")}
        h = VP(0xDEAD)
        by = lambda name, s: None if name in self.no else C.byref(s)  # noqa: E731
        rc = call(self.env, entry, by("p", self.p), by("qcp", self.q), by("files", files), self.nobs, a["set"], a["idx"],
                  a["qc"], a["ensval"], self.kld, by("tab", h))
        self.files_after = {k: down(t) for k, t in d.items()}
        self.alive = (d, o, files)                           # a table that came into being reads them until it is destroyed
        return rc, h, down(o["qc"]), down(o["ensval"])

    def refused(self, name, entry="letkf_set_obs_local_dev"):
        rc, h, qc, ens = self.run(entry)
        refused(self.env, rc, name)
        assert ("tab" in self.no and h.value == 0xDEAD) or h.value is None
        assert np.array_equal(qc, self.rk["qc"]) and S.same_bits(ens, self.rk["ensval"])


def test_refusals_set_obs_local_host_side(env):
    """every check that needs no device, one by one; the files are then untouched as well"""
    def case(name, change, h08=False):
        a = Local(env, h08)
        change(a)
        a.refused(name)
        assert all(S.same_bits(v, a.f[k]) for k, v in a.files_after.items()), name

    def setp(**kw):
        return lambda a: [setattr(a.p, k, v) for k, v in kw.items()]

    def setq(**kw):
        return lambda a: [setattr(a.q, k, v) for k, v in kw.items()]
    for arg in ("p", "qcp", "files", "tab"):
        case(arg, lambda a, arg=arg: a.no.add(arg))
    case("nobtype", setp(nobtype=0))
    case("nobtype", setp(nobtype=33))
    for arr in ("hori_local", "vert_local", "obs_sort_grid_spacing", "obs_min_spacing", "max_nobs_per_grid"):
        case(arr, setp(**{arr: None}))
    for key, bad in (("nlon", 0), ("nlat", 0), ("nprocs", 0), ("prc_num_x", 0), ("prc_num_x", 2), ("myrank", -1), ("myrank", 1),
                     ("dx", 0.0), ("dx", float("nan")), ("dy", -1.0), ("dy", float("nan"))):
        case(key, setp(**{key: bad}))
    case("nfile", lambda a: setattr(a, "nfile", -1))
    case("off", lambda a: a.null.add("off"))
    case("nobs", lambda a: setattr(a, "nobs", -1))
    case("member", setq(member=0))
    case("kld", lambda a: setattr(a, "kld", 3))              # MEMBER = 3 with DET_RUN needs 4
    case("kld", lambda a: setattr(a, "kld", 1 << 20))
    for arr in ("set", "idx", "qc", "ensval"):
        case(arr, lambda a, arr=arr: a.null.add(arr))
    case("nfile", lambda a: setattr(a, "nfile", 0))          # rows without files
    case("h08_lev", lambda a: a.null.add("h08_lev"), h08=True)
    case("off", lambda a: a.off.__setitem__(0, 1))
    case("off", lambda a: a.off.__setitem__(1, a.off[2] + 1))
    for arr in ("elm", "typ", "lev", "dat", "err", "ri", "rj"):
        case(arr, lambda a, arr=arr: a.null.add(arr))
    a = Local(env)
    a.p.nprocs, a.p.prc_num_x = 2, 2
    a.refused("nprocs", entry="letkf_set_obs_dev")


def test_refusals_set_obs_local_device_side(env):
    """a file row or an obsda row that the device finds wrong: refused, no table, qc and ensval as they came (`files` may already
    be converted, as the header says)"""
    def case(name, change):
        a = Local(env)
        change(a)
        a.refused(name)
    row = 5
    case("elm", lambda a: a.f["elm"].__setitem__(row, 1234))
    case("typ", lambda a: a.f["typ"].__setitem__(row, 0))
    case("typ", lambda a: a.f["typ"].__setitem__(row, SO.NOBTYPE + 1))
    case("set", lambda a: a.rk["set"].__setitem__(row, 0))
    case("set", lambda a: a.rk["set"].__setitem__(row, 3))
    case("idx", lambda a: a.rk["idx"].__setitem__(row, 0))

    def past(a):
        a.rk["idx"][row] = a.off[a.rk["set"][row]] - a.off[a.rk["set"][row] - 1] + 1
    case("idx", past)
    inf = np.full(SO.NOBTYPE, np.inf)                        # every mesh of zero cells: found after the pre-processing
    case("obs_sort_grid_spacing", lambda a: (a.keep.append(inf), setattr(a.p, "obs_sort_grid_spacing", inf.ctypes.data)))


def test_refusals_finish_and_table(env):
    pkg, ctx, dev = env
    L = pkg.lib()
    a = Local(env)
    rc, h, qc, ens = a.run()
    assert rc == 0 and h.value, message(env)
    info = pkg.ObsTableInfo()
    assert L.letkf_obs_table_info_get(h, C.byref(info)) == 0 and info.finished == 0
    n_all = dev(copy_dev(info.n_cell, I32, info.ncell))
    recv = dev(copy_dev(info.sendbuf, F64, info.nsorted * info.ld_send))
    ns = info.nsorted
    tables, ones = pkg.SearchTables(), np.ones(info.nctype)
    refused(env, L.letkf_obs_table_search(h, C.byref(tables)), "tab")                      # before the finish half
    refused(env, L.letkf_obs_table_set_varloc(ctx._c, h, hp(ones)), "tab")
    refused(env, L.letkf_obs_table_download(ctx._c, h, *[None] * 9), "tab")
    fin = lambda tab, na, nrecv, rv: call(env, "letkf_set_obs_finish_dev", tab, ptr(na), None, nrecv, ptr(rv))  # noqa: E731
    refused(env, fin(None, n_all, ns, recv), "tab")
    refused(env, fin(h, None, ns, recv), "n_all")
    refused(env, fin(h, n_all, -1, recv), "nrecv")
    refused(env, fin(h, n_all, ns, None), "recv")
    neg = n_all.clone()
    neg[0] = -1
    refused(env, fin(h, neg, ns, recv), "n_all")
    refused(env, fin(h, n_all, ns - 1, recv), "nrecv")
    refused(env, fin(h, n_all, ns + 1, recv), "nrecv")
    assert L.letkf_obs_table_info_get(h, C.byref(info)) == 0 and info.finished == 0 and info.nobstotal == 0
    assert fin(h, n_all, ns, recv) == 0, message(env)                                     # the refusals left the table usable
    refused(env, fin(h, n_all, ns, recv), "tab")                                           # a second run on one table
    assert L.letkf_obs_table_info_get(h, C.byref(info)) == 0 and info.finished == 1 and info.nobstotal == ns
    refused(env, L.letkf_obs_table_info_get(None, C.byref(info)), "tab")
    refused(env, L.letkf_obs_table_info_get(h, None), "info")
    refused(env, L.letkf_obs_table_search(None, C.byref(tables)), "tab")
    refused(env, L.letkf_obs_table_search(h, None), "tables")
    refused(env, L.letkf_obs_table_set_varloc(ctx._c, None, hp(ones)), "tab")
    refused(env, L.letkf_obs_table_set_varloc(ctx._c, h, None), "varloc")
    refused(env, L.letkf_obs_table_download(ctx._c, None, *[None] * 9), "tab")
    assert L.letkf_obs_table_download(ctx._c, h, *[None] * 9) == 0                          # every array may be NULL
    assert L.letkf_obs_table_destroy(h) == 0
