"""letkf_state_to_history_dev and letkf_monit_obs_dev (include/letkf_amd_monit.h) on the device against the numpy statement
of tests/_monit.py: the history fields bit for bit with canaries around them, the departures within the operator's per-row
bound plus one ulp, the records' merge over the two steps, the statistics within the triangle-inequality bounds, key /
nn = 0 / the switches, and every refusal with its outputs untouched."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import _monit as M
import _obsope as O

pytestmark = pytest.mark.gpu
CANARY, ICANARY = -7.25e77, -777


@pytest.fixture(scope="module")
def env():
    from _gpu import ctx, pkg
    return pkg, ctx(), torch.device("cuda:0")


def bits(a):
    return np.ascontiguousarray(a).view(np.int64)


# ------------------------------------------------------------------------------------------------------ state_to_history
def run_s2h(env, g, st, layout_in, out_perm, edge_fill, nv3dd=14, nv2dd=8):
    """one call into canaried buffers of nv3dd / nv2dd slots; returns (v3 [nv3dd, j, i, k], v2 [nv2dd, j, i])"""
    pkg, ctx, dev = env
    c3 = np.full((1, nv3dd, g["nlath"], g["nlonh"], g["nlevh"]), CANARY)
    c2 = np.full((1, nv2dd, g["nlath"], g["nlonh"]), CANARY)
    if out_perm:
        a3, a2, strides = O.permuted(dict(v3=c3, v2=c2), "mkvji", "mjvi")
    else:
        a3, a2 = c3, c2
        nk, ni, nj = g["nlevh"], g["nlonh"], g["nlath"]
        strides = dict(s3k=1, s3i=nk, s3j=nk * ni, s3v=nk * ni * nj, s3m=nk * ni * nj * nv3dd, s2i=1, s2j=ni, s2v=ni * nj,
                       s2m=ni * nj * nv2dd)
    d3, d2 = torch.from_numpy(a3).to(dev), torch.from_numpy(a2).to(dev)
    ds = M.DeviceState(pkg, st, dev, layout_in, edge_fill)
    fl = M.hist_layout(pkg, g, strides)
    fl.nv3dd, fl.nv2dd = nv3dd, nv2dd
    ctx.state_to_history(ds.hs, fl, d3, d2)
    torch.cuda.synchronize()
    first = (d3.cpu().numpy().copy(), d2.cpu().numpy().copy())
    ctx.state_to_history(ds.hs, fl, d3, d2)                        # a second call gives identical bits
    torch.cuda.synchronize()
    assert np.array_equal(bits(first[0]), bits(d3.cpu().numpy())) and np.array_equal(bits(first[1]), bits(d2.cpu().numpy()))
    if out_perm:
        g3 = np.transpose(first[0], ["mkvji".index(c) for c in "mvjik"])
        g2 = np.transpose(first[1], ["mjvi".index(c) for c in "mvji"])
    else:
        g3, g2 = first
    return g3[0], g2[0]


@pytest.mark.parametrize("edge_fill", [0, 15, 1, 2, 4, 8, 5])
@pytest.mark.parametrize("dims", [(5, 3, 8), (33, 17, 9), (70, 3, 70), (4, 3, 128)], ids=lambda d: "x".join(map(str, d)))
def test_state_to_history_has_the_statements_bits(env, dims, edge_fill):
    """(70, 3, 70): a point tile that spans rows of the grid, and a second chunk of the kernel's 64 levels with a remainder;
    (4, 3, 128): two full chunks"""
    nlon, nlat, nlev = dims
    g = O.make_grid(nlev, nlon=nlon, nlat=nlat)
    for nv3d in (11, 12):
        st = M.make_state(g, 40 + nv3d, nv3d=nv3d)
        w3, w2, m3, m2 = M.state_to_history(st["state"], st["topo"], st["cz"], st["ztop"], g, edge_fill)
        e3, e2 = np.full((14,) + w3.shape[1:], CANARY), np.full((8,) + w2.shape[1:], CANARY)
        e3[:13][m3], e2[:7][m2] = w3[m3], w2[m2]
        for layout_in in ("point", "level"):
            for out_perm in (False, True):
                g3, g2 = run_s2h(env, g, st, layout_in, out_perm, edge_fill)
                bad3, bad2 = np.argwhere(bits(g3) != bits(e3)), np.argwhere(bits(g2) != bits(e2))
                assert bad3.size == 0 and bad2.size == 0, (nv3d, layout_in, out_perm, bad3[:5].tolist(), bad2[:5].tolist())


def hist_args(env, g=None):
    pkg, ctx, dev = env
    g = g or O.make_grid(8)
    st = M.make_state(g, 3)
    ds = M.DeviceState(pkg, st, dev)
    fl = M.hist_layout(pkg, g)
    d3 = torch.full((13 * g["nlath"] * g["nlonh"] * g["nlevh"],), CANARY, dtype=torch.float64, device=dev)
    d2 = torch.full((7 * g["nlath"] * g["nlonh"],), CANARY, dtype=torch.float64, device=dev)
    return ds, fl, d3, d2


S2H_REFUSALS = ([("hs", n, None) for n in ("x", "topo", "cz")] + [("hs", n, 0) for n in ("si", "sj", "sl", "sv")] +
                [("fl", n, 0) for n in ("s3k", "s3i", "s3j", "s3v", "s2i", "s2j", "s2v", "khalo", "nlev", "nlon", "nlat")] +
                [("hs", "nv3d", 10), ("hs", "edge_fill", -1), ("hs", "edge_fill", 16), ("hs", "ztop", 0.0), ("hs", "ztop", -5.0),
                 ("hs", "ztop", math.inf), ("hs", "ztop", math.nan), ("fl", "nv3dd", 12), ("fl", "nv2dd", 6), ("fl", "ihalo", -1),
                 ("arg", "s", None), ("arg", "layout", None), ("arg", "v3d", None), ("arg", "v2d", None)])


@pytest.mark.parametrize("what,name,value", S2H_REFUSALS, ids=lambda v: str(v))
def test_state_to_history_refuses(env, what, name, value):
    pkg, ctx, dev = env
    ds, fl, d3, d2 = hist_args(env)
    args = dict(s=C.byref(ds.hs), layout=C.byref(fl), v3d=C.c_void_p(d3.data_ptr()), v2d=C.c_void_p(d2.data_ptr()))
    if what == "arg":
        args[name] = None
    else:
        setattr(ds.hs if what == "hs" else fl, name, value)
    rc = pkg.lib().letkf_state_to_history_dev(ctx._c, args["s"], args["layout"], args["v3d"], args["v2d"])
    torch.cuda.synchronize()
    assert rc == -1 and pkg.lib().letkf_amd_last_error().decode()             # LETKF_E_INVALID
    assert bool((d3 == CANARY).all()) and bool((d2 == CANARY).all())


# ------------------------------------------------------------------------------------------------------------- monit_obs
def dcase(env, case, cfg, which=0, fields=None):
    pkg, ctx, dev = env
    h = case["hist"][which]
    return O.DeviceCase(pkg, dict(case, v3=h[0], v2=h[1]), cfg, dev, fields=fields)


@pytest.mark.parametrize("nlev,method", [(8, 2), (8, 3), (70, 2), (70, 3)])
def test_step_1_on_the_uploaded_history_matches_the_statement(env, nlev, method):
    pkg, ctx, dev = env
    case = M.case(nlev)
    cfg, mcfg = dict(case["cfg"], method_ref_calc=method), M.default_mcfg()
    st = M.monit(cfg, mcfg, case, case["hist"][0], 1, None)
    got = M.run_monit(pkg, ctx, dcase(env, case, cfg), mcfg, 1, dev, canary=(ICANARY, CANARY))
    good = st["qc"] == 0
    print(f"nlev {nlev} method {method}: worst error / tolerance "
          f"{float(np.max(np.abs(got['rec']['omb'] - st['dep'])[good] / st['tol'][good])):.3g}, bias {got['bias'].tolist()}")
    assert M.compare(got, st, 1) == []
    assert bool((got["rec"]["oma"] == CANARY).all())                        # step 1 does not write oma


def test_the_chain_on_the_device_and_the_second_step(env):
    """state_to_history's output fed straight to monit_obs gives the bits of the uploaded-history call; step 2 on the second
    state leaves omb alone, writes oma and merges qc"""
    pkg, ctx, dev = env
    case = M.case(8)
    cfg, mcfg, g = case["cfg"], M.default_mcfg(), case["g"]
    up1 = M.run_monit(pkg, ctx, dcase(env, case, cfg, 0), mcfg, 1, dev)
    dc = dcase(env, case, cfg, 0, fields=(np.full_like(case["hist"][0][0], CANARY), np.full_like(case["hist"][0][1], CANARY)))
    ds_g, ds_a = M.DeviceState(pkg, case["gues"], dev), M.DeviceState(pkg, case["anal"], dev, layout="level")
    ctx.state_to_history(ds_g.hs, dc.fields, dc.d3, dc.d2)
    ch1 = M.run_monit(pkg, ctx, dc, mcfg, 1, dev)
    for n in ("set", "idx", "qc"):
        assert np.array_equal(ch1["rec"][n], up1["rec"][n])
    assert np.array_equal(bits(ch1["rec"]["omb"]), bits(up1["rec"]["omb"]))
    assert np.array_equal(bits(ch1["bias"]), bits(up1["bias"])) and np.array_equal(bits(ch1["rmse"]), bits(up1["rmse"]))
    assert np.array_equal(ch1["nobs"], up1["nobs"])
    # step 2
    s1 = M.monit(cfg, mcfg, case, case["hist"][0], 1, None)
    s2 = M.monit(cfg, mcfg, case, case["hist"][1], 2, s1["rec"])
    assert ((s1["qc"] == 0) & (s2["qc"] != 0)).any() and ((s1["qc"] != 0) & (s2["qc"] == 0)).any()
    ctx.state_to_history(ds_a.hs, dc.fields, dc.d3, dc.d2)
    ch2 = M.run_monit(pkg, ctx, dc, mcfg, 2, dev, rec=ch1["rec_t"])
    assert np.array_equal(bits(ch2["rec"]["omb"]), bits(up1["rec"]["omb"]))
    s2_for_cmp = dict(s2, rec=dict(s2["rec"], omb=ch2["rec"]["omb"]))      # (omb: compared to the statement above, bitwise here)
    assert M.compare(ch2, s2_for_cmp, 2) == []
    flipped = (s1["qc"] != 0) & (s2["qc"] == 0)
    assert np.array_equal(ch2["rec"]["qc"][flipped], s1["qc"][flipped])     # the QC of y_b stays where it was not good


def test_key_nn0_the_switches_and_reproducibility(env):
    pkg, ctx, dev = env
    case = M.case(8)
    cfg, n = case["cfg"], case["nrow"]
    dc = dcase(env, case, cfg)
    full = M.run_monit(pkg, ctx, dc, M.default_mcfg(), 1, dev)
    again = M.run_monit(pkg, ctx, dc, M.default_mcfg(), 1, dev)
    for name in ("set", "idx", "qc", "omb"):
        assert np.array_equal(bits(full["rec"][name].astype(np.float64) if name != "omb" else full["rec"][name]),
                              bits(again["rec"][name].astype(np.float64) if name != "omb" else again["rec"][name]))
    assert np.array_equal(bits(full["bias"]), bits(again["bias"])) and np.array_equal(bits(full["rmse"]), bits(again["rmse"]))
    # a permuted subset with one duplicate: every row as the NULL-key call gave it
    key = np.random.default_rng(2).permutation(n)[: n // 2].astype(np.int32)
    key[7] = key[3]
    mk = M.default_mcfg(key=key)
    sub = M.run_monit(pkg, ctx, dc, mk, 1, dev)
    for name in ("set", "idx", "qc"):
        assert np.array_equal(sub["rec"][name], full["rec"][name][key])
    assert np.array_equal(bits(sub["rec"]["omb"]), bits(full["rec"]["omb"][key]))
    assert M.compare(sub, M.monit(cfg, mk, case, case["hist"][0], 1, None), 1) == []
    # nn = 0: counts 0, statistics undef, nothing else written
    e = M.run_monit(pkg, ctx, dc, M.default_mcfg(key=np.zeros(0, dtype=np.int32)), 1, dev, canary=(ICANARY, CANARY))
    assert not e["nobs"].any() and (e["bias"] == O.UNDEF).all() and (e["rmse"] == O.UNDEF).all()
    assert all(bool((t == (ICANARY if t.dtype == torch.int32 else CANARY)).all()) for t in e["rec_t"].values())
    # DEPARTURE_STAT_RADAR off: radar rows qc 90, undef, not counted
    m0 = M.default_mcfg(departure_stat_radar=0)
    r0, s0 = M.run_monit(pkg, ctx, dc, m0, 1, dev), M.monit(cfg, m0, case, case["hist"][0], 1, None)
    radar = np.array([r["radar"] is not None for r in case["rows"]])
    assert (r0["rec"]["qc"][radar] == O.QC_OTYPE).all() and (r0["rec"]["omb"][radar] == O.UNDEF).all()
    assert not r0["nobs"][[8, 9, 10]].any() and M.compare(r0, s0, 1) == []
    # DEPARTURE_STAT_T_RANGE: a fifth of the rows outside
    mt = M.default_mcfg(t_range=M.T_RANGE)
    rt, stt = M.run_monit(pkg, ctx, dc, mt, 1, dev), M.monit(cfg, mt, case, case["hist"][0], 1, None)
    assert 0.1 < (stt["qc"] == -1).mean() < 0.3 and M.compare(rt, stt, 1) == []


def _raw(pkg, ctx, dc, mp, od, outs, nn, key=None, over=None):
    a = dict(mp=C.byref(mp), op=C.byref(dc.params), files=C.byref(dc.files), f=C.byref(dc.fields), nn=nn,
             key=None if key is None else C.c_void_p(key.data_ptr()), set=C.c_void_p(dc.set.data_ptr()),
             idx=C.c_void_p(dc.idx.data_ptr()), rec=C.byref(od), nobs=C.c_void_p(outs[0].data_ptr()),
             bias=C.c_void_p(outs[1].data_ptr()), rmse=C.c_void_p(outs[2].data_ptr()))
    a.update(over or {})
    return pkg.lib().letkf_monit_obs_dev(ctx._c, a["mp"], a["op"], a["files"], a["f"], a["nn"], a["key"], a["set"], a["idx"], a["rec"],
                                         a["nobs"], a["bias"], a["rmse"])


MONIT_REFUSALS = ([("mp", "step", 0), ("mp", "step", 3), ("mp", "nid", 0), ("mp", "nid", 33), ("mp", "elem_uid", None),
                   ("mp", "t_range+dif", None), ("fl", "nmem", 2), ("fl", "nmem", 0), ("fl", "s3k", 0), ("op", "method_ref_calc", 4),
                   ("op", "nobtype", 0), ("files", "dat", None), ("files", "elm", None), ("arg", "nn", -1), ("key", "negative", None),
                   ("set", "outside", None)] +
                  [("rec", n, None) for n in ("set", "idx", "qc", "omb", "oma")] +
                  [("arg", n, None) for n in ("mp", "op", "files", "f", "set", "idx", "rec", "nobs", "bias", "rmse")])


@pytest.mark.parametrize("what,name,value", MONIT_REFUSALS, ids=lambda v: str(v))
def test_monit_obs_refuses(env, what, name, value):
    pkg, ctx, dev = env
    case = M.case(8)
    dc = dcase(env, case, case["cfg"])
    nn = case["nrow"]
    mp, od, rec_t, ids = M.monit_structs(pkg, dc, M.default_mcfg(), 1, nn, dev, canary=(ICANARY, CANARY))
    outs = (torch.full((16,), ICANARY, dtype=torch.int32, device=dev), torch.full((16,), CANARY, dtype=torch.float64, device=dev),
            torch.full((16,), CANARY, dtype=torch.float64, device=dev))
    key, over = None, {}
    if what == "mp" and name == "t_range+dif":
        mp.t_range, mp.dif = 100.0, None
    elif what in ("mp", "fl", "op", "files", "rec"):
        setattr(dict(mp=mp, fl=dc.fields, op=dc.params, files=dc.files, rec=od)[what], name, value)
    elif what == "arg":
        over[name] = value
    elif what == "key":
        k = np.arange(nn, dtype=np.int32)
        k[nn // 2] = -1
        key = torch.from_numpy(k).to(dev)
    elif what == "set":
        bad = case["set"].copy()
        bad[5] = 9
        dc.set = torch.from_numpy(bad).to(dev)
    rc = _raw(pkg, ctx, dc, mp, od, outs, nn, key, over)
    torch.cuda.synchronize()
    assert rc == -1 and pkg.lib().letkf_amd_last_error().decode()             # LETKF_E_INVALID
    for t in list(rec_t.values()) + list(outs):
        assert bool((t == (ICANARY if t.dtype == torch.int32 else CANARY)).all())
