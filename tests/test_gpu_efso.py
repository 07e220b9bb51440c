"""EFSO on the device (letkf_efso_points_dev / _columns_dev / _obsense_dev, das_efso = scale/letkf/letkf_tools.f90:1158-1302)
against the numpy restatement tests/_efso.py, on the oracle's obs_local lists and on the device search's: every (j, t)
within 1e-12 of the sum of |terms|, untouched rows bit-identical, two calls bit-identical, the column route bit-identical
to the points route on the same lists whatever the slab size."""
import numpy as np
import pytest
import torch

import _efso
from _search import build_case, device_struct, host_struct, oracle_csr

pytestmark = pytest.mark.gpu


def _ctx():
    from _gpu import ctx
    return ctx()


def _d(a, dt=None):
    from _gpu import dev
    return dev(a, dt)


_CASE = {}


def oracle_case(seed=51, npts=120, nobs=(500, 150, 200, 90)):
    if seed not in _CASE:
        case = build_case(seed, nobs_per_ctype=nobs, npts=npts)
        h, keep = host_struct(case)
        p = case["pts"]
        off, idx, rd, rl, _ = oracle_csr(h, p["ri"], p["rj"], p["rlev"], p["rz"])
        _CASE[seed] = (case, off, idx, rd, rl)
    return _CASE[seed]


def run_points(k, nterm, term, off, idx, rd, rl, ya, fcst, fcer, djdy0, kld=None, var_mask=0, pair_bytes=0, view=0,
               nan_pad=True):
    """djdy after letkf_efso_points_dev (djdy0 [nobs, nterm] prefilled); view > 0 places fcst / fcer inside a field of
    view extra points on either side (a slab of a larger field)."""
    npts, _, nv = fcst.shape
    nobs = ya.shape[0]
    kld = kld or k
    tab = np.full((nobs, kld), np.nan if nan_pad else 0.0)
    tab[:, :k] = ya
    if view:
        big_f = np.zeros((npts + 2 * view, k, nv))
        big_f[view:view + npts] = fcst
        big_e = np.zeros((npts + 2 * view, nv))
        big_e[view:view + npts] = fcer
        f, fs, e, es = _efso.ref_layout(big_f, big_e)
        f_t, e_t = _d(f)[view:], _d(e)[view:]
    else:
        f, fs, e, es = _efso.ref_layout(fcst, fcer)
        f_t, e_t = _d(f), _d(e)
    dj = _d(djdy0.ravel())
    _ctx().efso_points(k, nv, term, nterm, _d(off), _d(idx), _d(rd), _d(rl), _d(tab.ravel()), kld, nobs, f_t, *fs, e_t, *es, dj,
                       var_mask=var_mask, pair_bytes=pair_bytes)
    torch.cuda.synchronize()
    return dj.cpu().numpy().reshape(nobs, nterm)


@pytest.mark.parametrize("k", [3, 10, 20, 50, 100, 320])
def test_points_against_numpy(k):
    case, off, idx, rd, rl = oracle_case()
    nterm, term = 3, [0, 0, 1, 2, -1, 1, -1]
    fcst, fcer, ya, _ = _efso.inputs(np.random.default_rng(k), len(off) - 1, k, len(term), case["nobs"])
    exp, scale = _efso.efso_loop(off, idx, rd, rl, ya, fcst, fcer, term, nterm)
    got = run_points(k, nterm, term, off, idx, rd, rl, ya, fcst, fcer, np.zeros_like(exp))
    assert _efso.within(got, exp, scale) < 1e-12
    assert "efso_pairs_kernel<3>" in _ctx().last_path()


@pytest.mark.parametrize("nterm,term", [(1, [0, -1, 0, -1]), (2, [1, 0, -1, 1, 0]), (3, [2, -1, 1, 0, 0, 1]),
                                        (4, [3, 2, 1, 0, -1, 3, 2, 1, 0, -1, 1])])
def test_every_term_count(nterm, term):
    case, off, idx, rd, rl = oracle_case()
    fcst, fcer, ya, _ = _efso.inputs(np.random.default_rng(nterm), len(off) - 1, 20, len(term), case["nobs"])
    exp, scale = _efso.efso_loop(off, idx, rd, rl, ya, fcst, fcer, term, nterm)
    got = run_points(20, nterm, term, off, idx, rd, rl, ya, fcst, fcer, np.zeros_like(exp))
    assert _efso.within(got, exp, scale) < 1e-12


def test_two_classes_empty_points_unreached_rows_kld_and_view():
    """two variable classes accumulate through var_mask; points with no list; rows no point reaches keep their prefilled
    bits; kld = k + 7 with NaN in the unread columns; fcst / fcer a slab view of a larger field"""
    case, off, idx, rd, rl = oracle_case()
    npts = len(off) - 1
    # every fifth point loses its list
    keep = np.ones(len(idx), bool)
    for p in range(0, npts, 5):
        keep[off[p]:off[p + 1]] = False
    cnt = np.diff(off) * np.array([p % 5 != 0 for p in range(npts)])
    off2 = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
    idx2, rd2, rl2 = idx[keep], rd[keep], rl[keep]
    k, nterm, term = 12, 3, [0, 0, 1, 2, 1, 2, -1]
    fcst, fcer, ya, _ = _efso.inputs(np.random.default_rng(7), npts, k, len(term), case["nobs"])
    prefill = np.random.default_rng(8).standard_normal((case["nobs"], nterm))
    m1, m2 = 0b0001011, 0b1110100
    # class 2: the same rows with another localisation factor
    rl_b, rd_b = rl2 * 0.6, rd2 / 0.6
    exp, _ = _efso.efso_loop(off2, idx2, rd2, rl2, ya, fcst, fcer, term, nterm, var_mask=m1, djdy=prefill)
    exp, _ = _efso.efso_loop(off2, idx2, rd_b, rl_b, ya, fcst, fcer, term, nterm, var_mask=m2, djdy=exp)
    s1 = _efso.efso_loop(off2, idx2, rd2, rl2, ya, fcst, fcer, term, nterm, var_mask=m1)[1]
    s2 = _efso.efso_loop(off2, idx2, rd_b, rl_b, ya, fcst, fcer, term, nterm, var_mask=m2)[1]
    got = run_points(k, nterm, term, off2, idx2, rd2, rl2, ya, fcst, fcer, prefill, kld=k + 7, var_mask=m1, view=9)
    got = run_points(k, nterm, term, off2, idx2, rd_b, rl_b, ya, fcst, fcer, got, kld=k + 7, var_mask=m2, view=9)
    unreached = np.setdiff1d(np.arange(case["nobs"]), idx2)
    assert len(unreached) > 20
    assert np.array_equal(got[unreached].view(np.int64), prefill[unreached].view(np.int64))
    reached = np.unique(idx2)
    scale = np.abs(prefill) + s1 + s2
    assert _efso.within(got[reached], exp[reached], scale[reached]) < 1e-12
    assert np.isfinite(got).all()


def test_kld_equals_k_and_chunks_and_repeat_are_bitwise():
    """kld = k (rows end at the last member); a pair_bytes budget that forces many chunks of points gives the same bits as one
    chunk; two identical calls give identical bits"""
    case, off, idx, rd, rl = oracle_case()
    k, nterm, term = 50, 3, [0, 1, 2, 0, 1, 2, -1, 0]
    fcst, fcer, ya, _ = _efso.inputs(np.random.default_rng(9), len(off) - 1, k, len(term), case["nobs"])
    z = np.zeros((case["nobs"], nterm))
    a = run_points(k, nterm, term, off, idx, rd, rl, ya, fcst, fcer, z)
    b = run_points(k, nterm, term, off, idx, rd, rl, ya, fcst, fcer, z)
    c = run_points(k, nterm, term, off, idx, rd, rl, ya, fcst, fcer, z, pair_bytes=300 * (8 * nterm + 16))
    assert np.array_equal(a.view(np.int64), b.view(np.int64))
    assert np.array_equal(a.view(np.int64), c.view(np.int64))
    exp, scale = _efso.efso_loop(off, idx, rd, rl, ya, fcst, fcer, term, nterm)
    assert _efso.within(a, exp, scale) < 1e-12


@pytest.mark.parametrize("nlev", [1, 7])
def test_columns_equal_points_on_the_device_lists(nlev):
    """letkf_efso_columns_dev (column search + EFSO by slabs of levels) against letkf_efso_points_dev on the lists of
    letkf_obs_search_columns_dev: identical bits, with one slab and with list_bytes small enough for one level per slab; and
    against numpy on those lists"""
    case = build_case(61, npts=90)
    t, keep = device_struct(case, "cuda")
    p = case["pts"]
    nij1 = 90
    rng = np.random.default_rng(nlev)
    rlev = rng.uniform(2.5e4, 1.0e5, nij1 * nlev)
    rz = rng.uniform(0.0, 12000.0, nij1 * nlev)
    c = _ctx()
    o, i, d, l = c.obs_search_columns(t, nij1, nlev, _d(p["ri"]), _d(p["rj"]), _d(rlev), _d(rz))
    off, idx, rd, rl = (x.cpu().numpy() for x in (o, i, d, l))
    k, nterm, term = 20, 3, [0, 0, 1, 2, -1, 1]
    npts = nij1 * nlev
    fcst, fcer, ya, _ = _efso.inputs(np.random.default_rng(10 + nlev), npts, k, len(term), case["nobs"])
    z = np.zeros((case["nobs"], nterm))
    ref = run_points(k, nterm, term, off, idx, rd, rl, ya, fcst, fcer, z)
    exp, scale = _efso.efso_loop(off, idx, rd, rl, ya, fcst, fcer, term, nterm)
    assert _efso.within(ref, exp, scale) < 1e-12
    f, fs, e, es = _efso.ref_layout(fcst, fcer)
    tab = _d(ya.ravel())
    for lb in (0, 1):
        dj = torch.zeros(case["nobs"] * nterm, dtype=torch.float64, device="cuda")
        c.efso_columns(k, len(term), term, nterm, t, nij1, nlev, _d(p["ri"]), _d(p["rj"]), _d(rlev), _d(rz), tab, k,
                       case["nobs"], _d(f), *fs, _d(e), *es, dj, list_bytes=lb)
        torch.cuda.synchronize()
        got = dj.cpu().numpy().reshape(-1, nterm)
        assert np.array_equal(got.view(np.int64), ref.view(np.int64)), lb
    assert "search_columns" in c.last_path()


def test_obsense():
    rng = np.random.default_rng(12)
    for nterm in (1, 3, 4):
        dj = rng.standard_normal((1000, nterm))
        dep = rng.standard_normal(1000)
        out = torch.full((1000 * nterm,), np.nan, dtype=torch.float64, device="cuda")
        _ctx().efso_obsense(nterm, _d(dj.ravel()), _d(dep), out)
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy().reshape(1000, nterm), dj * dep[:, None])


def test_invalid_arguments():
    from _gpu import pkg
    case, off, idx, rd, rl = oracle_case()
    k, term = 10, [0, 1, 2]
    fcst, fcer, ya, _ = _efso.inputs(np.random.default_rng(1), len(off) - 1, k, 3, case["nobs"])
    f, fs, e, es = _efso.ref_layout(fcst, fcer)
    g = dict(off=_d(off), idx=_d(idx), rd=_d(rd), rl=_d(rl), tab=_d(ya.ravel()), f=_d(f), e=_d(e))
    dj = torch.zeros(case["nobs"] * 4, dtype=torch.float64, device="cuda")

    def call(k_=k, nterm=3, term_=term, kld=k, fcst_=g["f"], idx_=g["idx"]):
        _ctx().efso_points(k_, len(term_), term_, nterm, g["off"], idx_, g["rd"], g["rl"], g["tab"], kld, case["nobs"], fcst_,
                           *fs, g["e"], *es, dj)

    for bad in (dict(nterm=0), dict(nterm=5), dict(k_=1, kld=1), dict(kld=k - 1), dict(fcst_=None), dict(idx_=None),
                dict(term_=[0, 3, 1]), dict(term_=[0, -2, 1])):
        with pytest.raises(pkg.LetkfError, match="error -1"):
            call(**bad)
    with pytest.raises(pkg.LetkfError, match="error -1"):
        _ctx().efso_obsense(5, dj, _d(np.zeros(case["nobs"])), dj)
    torch.cuda.synchronize()
    assert float(dj.abs().max()) == 0.0


def test_rows_outside_the_table_are_skipped():
    """list entries with a row outside [0, nobs) -- nobs itself with nobs a power of two (its low bits are row 0), beyond
    it, negative -- contribute nothing and leave every other row's sum as numpy has it without them"""
    nobs_ct = (500, 150, 200, 174)
    case, off, idx, rd, rl = oracle_case(seed=71, nobs=nobs_ct)
    nobs = case["nobs"]
    assert nobs == 1024
    npts = len(off) - 1
    bad_rows = [nobs, -1, nobs + 3, 2 * nobs, -nobs]
    li, ld, ll = [], [], []
    for p in range(npts):
        i0, i1 = off[p], off[p + 1]
        li.append(idx[i0:i1]); ld.append(rd[i0:i1]); ll.append(rl[i0:i1])
        if p % 3 == 0:                                  # a bad entry at the front, the middle and the end of the list
            for pos in (0, (i1 - i0) // 2, i1 - i0):
                b = bad_rows[(p + pos) % len(bad_rows)]
                li[-1] = np.insert(li[-1], pos, b); ld[-1] = np.insert(ld[-1], pos, 2.0); ll[-1] = np.insert(ll[-1], pos, 0.5)
    off2 = np.concatenate([[0], np.cumsum([len(a) for a in li])]).astype(np.int64)
    idx2, rd2, rl2 = np.concatenate(li).astype(np.int32), np.concatenate(ld), np.concatenate(ll)
    k, nterm, term = 16, 3, [0, 1, 2, 0, -1]
    fcst, fcer, ya, _ = _efso.inputs(np.random.default_rng(13), npts, k, len(term), nobs)
    prefill = np.random.default_rng(14).standard_normal((nobs, nterm))
    exp, scale = _efso.efso_loop(off, idx, rd, rl, ya, fcst, fcer, term, nterm, djdy=prefill)
    got = run_points(k, nterm, term, off2, idx2, rd2, rl2, ya, fcst, fcer, prefill)
    assert _efso.within(got, exp, scale) < 1e-12
    unreached = np.setdiff1d(np.arange(nobs), idx)
    assert len(unreached) > 0
    assert np.array_equal(got[unreached].view(np.int64), prefill[unreached].view(np.int64))
