"""The no-limit column search (letkf_search_columns_kernel<FILL>) at the boundaries of its two vertical passes: the
counting pass with lane = level (level groups of 64), the fill pass with its ring of accepted candidates (64 per full
step), the survivor buffers' flush thresholds (buffer - 64: 448 in the counting pass, 320 in the fill pass), the
per-type fallback of the counting pass where varloc <= 1e-290, and nobs_ctype on either call or on none.

Every case: counts == diff(obs_off) of the per-point kernel; obs_idx, rdiag_l, rloc_l and nobs_ctype array_equal to the
per-point kernel's; rdiag / rloc within rtol 1e-13 of the oracle (as tests/test_gpu_search.py); two calls byte-identical.

About "a weight that underflows": a type is searched only if varloc >= tiny = 2.2e-308, and inside the cut-off
nd <= 13.33, so rloc = varloc exp(-nd / 2) >= 2.2e-308 x 1.27e-3 = 2.8e-311, a nonzero (subnormal) double: no admissible
table makes the weight vanish.  The varloc = 1e-300 type below therefore takes the not-wsafe path with nd up to the
cut-off (rloc down to 1.3e-303, rdiag up to 2e304) and must keep every entry, like the per-point kernel and the oracle."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import _search
from _search_types import I_ORG, J_ORG, NLAT, NLON, make_case, types_case

pytestmark = pytest.mark.gpu


def count_call(c, t, nij1, nlev, rig, rjg, rlev, rz, nct):
    """The counting call of letkf_obs_search_columns_dev alone, with nobs_ctype (Context.obs_search_columns asks for it on
    the fill call only)."""
    counts = torch.full((nij1 * nlev,), -7, dtype=torch.int32, device="cuda")
    p = lambda x: None if x is None else C.c_void_p(x.data_ptr())
    c._check(c._l.letkf_obs_search_columns_dev(c._c, C.byref(t), C.c_int64(nij1), C.c_int32(nlev), p(rig), p(rjg), p(rlev),
                                               p(rz), C.c_int32(0), p(counts), None, None, None, None, p(nct), None))
    return counts


def check_case(case, rig, rjg, rlev, rz, nlev):
    """All the module's assertions for one table and one set of columns; returns the per-point counts [nlev, nij1]."""
    from _gpu import ctx, dev
    c = ctx()
    nij1, nct_n = len(rig), case["scal"]["nctype"]
    npts = nij1 * nlev
    t, keep = _search.device_struct(case, "cuda")
    d = [dev(x) for x in (rig, rjg, rlev, rz)]
    ri_p, rj_p = np.tile(rig, nlev), np.tile(rjg, nlev)
    o1, i1, d1, l1 = c.obs_search(t, dev(ri_p), dev(rj_p), d[2], d[3])
    want_n = (o1[1:] - o1[:-1]).to(torch.int32)
    edges = torch.tensor(case["ctype_rows"], device="cuda")
    want_ct = torch.zeros(npts, nct_n, dtype=torch.int32, device="cuda")
    if i1.numel():
        which = torch.bucketize(i1.long(), edges, right=True) - 1
        pt_of = torch.repeat_interleave(torch.arange(npts, device="cuda"), o1[1:] - o1[:-1])
        want_ct.index_put_((pt_of, which), torch.ones_like(which, dtype=torch.int32), accumulate=True)
    # nobs_ctype on the count call / not at all
    nct_c = torch.full((npts, nct_n), -1, dtype=torch.int32, device="cuda")
    n_with = count_call(c, t, nij1, nlev, *d, nct_c)
    n_without = count_call(c, t, nij1, nlev, *d, None)
    assert torch.equal(n_with, want_n) and torch.equal(n_without, want_n)
    # the types the search skips (varloc < tiny) or that find nothing keep what the caller put there, as before
    seen = want_ct.sum(0) > 0
    assert torch.equal(nct_c[:, seen], want_ct[:, seen])
    # nobs_ctype on the fill call / not at all, twice each
    runs = []
    for with_ct in (True, False, True, False):
        nct_f = torch.full((npts, nct_n), -1, dtype=torch.int32, device="cuda") if with_ct else None
        o2, i2, d2, l2 = c.obs_search_columns(t, nij1, nlev, *d, nobs_ctype=nct_f)
        torch.cuda.synchronize()
        assert torch.equal(o1, o2) and torch.equal(i1, i2) and torch.equal(d1, d2) and torch.equal(l1, l2)
        if with_ct:
            assert torch.equal(nct_f[:, seen], want_ct[:, seen])
            assert torch.equal(nct_f, nct_c)
        runs.append(tuple(x.cpu().numpy().tobytes() for x in (o2, i2, d2, l2)))
    assert runs[0] == runs[1] == runs[2] == runs[3]
    # the oracle
    h, alive = _search.host_struct(case)
    off, idx, rd, rl, tied = _search.oracle_csr(h, ri_p, rj_p, rlev, rz)
    assert np.array_equal(off, o1.cpu().numpy()) and np.array_equal(idx, i1.cpu().numpy())
    np.testing.assert_allclose(d1.cpu().numpy(), rd, rtol=1e-13, atol=0)
    np.testing.assert_allclose(l1.cpu().numpy(), rl, rtol=1e-13, atol=0)
    return want_n.cpu().numpy().reshape(nlev, nij1)


# ---- survivors per column and accepted entries per level, to the entry ------------------------------------------
BAND = 1.0e5          # height of band b: far more than the vertical cut-off apart
CLUSTERS = {          # survivors of a column -> observations per band (what a level at that band accepts)
    "a": {0: (), 64: (0, 1, 63), 448: (0, 1, 63, 64, 65, 255), 449: (0, 1, 63, 64, 65, 256)},
    "b": {320: (0, 1, 63, 64, 65, 127), 321: (0, 1, 63, 64, 65, 128), 600: (1, 63, 64, 65, 130, 277)},
}


def cluster_case(which, rng):
    """One type (height localisation): every column stands alone, more than two horizontal cut-offs from the next, with
    its survivors on a fine lattice around it and a ring of observations just outside the cut-off around that."""
    hloc, vloc = 1000.0, 500.0
    ob = {k: [] for k in ("ri", "rj", "lev", "dat", "err")}
    rig, rjg, bands = [], [], []
    for n, (nsurv, per_band) in enumerate(CLUSTERS[which].items()):
        assert sum(per_band) == nsurv
        ci, cj = 6.3 + 9.0 * (n % 4), 7.6 + 12.0 * (n // 4)
        rig.append(I_ORG + ci)
        rjg.append(J_ORG + cj)
        bands.append(per_band)
        side = max(math.ceil(math.sqrt(max(nsurv, 1))), 2)
        lat = (np.arange(side) / (side - 1) - 0.5) * 1.3          # +-0.65 cells: several mesh cells, nd_h <= 0.92
        gi, gj = (x.reshape(-1) for x in np.meshgrid(lat, lat))
        slot = rng.permutation(side * side)[:nsurv]
        band_of = np.repeat(np.arange(len(per_band)), np.asarray(per_band, dtype=np.int64))
        ob["ri"].append(ci + gi[slot])
        ob["rj"].append(cj + gj[slot])
        ob["lev"].append(BAND * (band_of + 1) + rng.uniform(-vloc, vloc, nsurv))      # nd_v <= 1: nd <= 1.9
        ang = rng.uniform(0.0, 2.0 * np.pi, 12)                                        # the ring: nd_h in (3.66, 4.1)
        rad = rng.uniform(3.66, 4.1, 12)
        ob["ri"].append(ci + rad * np.cos(ang))
        ob["rj"].append(cj + rad * np.sin(ang))
        ob["lev"].append(BAND * rng.integers(1, 7, 12).astype(np.float64))
    o = {k: np.concatenate(v) for k, v in ob.items() if v}
    o["dat"] = np.full(o["ri"].size, 9.5e4)
    o["err"] = rng.choice([1.0, 3.0, 5.0], o["ri"].size)
    types = dict(vmode=[1], hori_loc=[hloc], vert_loc=[vloc], varloc=[0.9])
    return make_case(types, [[0]], [o]), np.array(rig), np.array(rjg), bands


@pytest.mark.parametrize("nlev", [1, 2, 63, 64, 65, 130])
@pytest.mark.parametrize("which", ["a", "b"])
def test_flush_and_queue_boundaries(which, nlev):
    rng = np.random.default_rng(100 + nlev)
    case, rig, rjg, bands = cluster_case(which, rng)
    nij1 = len(rig)
    # level l of column c looks at band (l + c) % 7 of that column; band 6 and the bands a column lacks are empty
    band = (np.arange(nlev)[:, None] + np.arange(nij1)[None, :]) % 7
    rz = (BAND * (band + 1)).astype(np.float64)
    rlev = np.full(nij1 * nlev, 5.0e4)
    got = check_case(case, rig, rjg, rlev, rz.reshape(-1), nlev)
    want = np.array([[bands[c][band[l, c]] if band[l, c] < len(bands[c]) else 0 for c in range(nij1)] for l in range(nlev)])
    assert np.array_equal(got, want)
    if nlev >= 63:                                               # every queue boundary really occurs
        assert {0, 1, 63, 64, 65}.issubset(set(got.reshape(-1).tolist())) and got.max() >= 129


# ---- combined types, random geometry (types_case: tests/_search_types.py) ---------------------------------------
@pytest.mark.parametrize("nij1,nlev", [(1, 65), (5, 2), (37, 1), (37, 63), (5, 130), (1, 64)])
def test_combined_types(nij1, nlev):
    rng = np.random.default_rng(7 * nij1 + nlev)
    case = types_case(rng, (500, 400, 300, 200, 400, 200))
    rig = I_ORG + rng.uniform(0.5, NLON - 0.5, nij1)
    rjg = J_ORG + rng.uniform(0.5, NLAT - 0.5, nij1)
    rlev = rng.uniform(2.5e4, 1.0e5, nij1 * nlev)                # the rain-base type accepts the levels below ~490 hPa
    rz = rng.uniform(0.0, 12000.0, nij1 * nlev)
    got = check_case(case, rig, rjg, rlev, rz, nlev)
    assert got.sum() > 10 * nij1 * nlev
    # the weights of the 1e-300 type reach down to its cut-off
    from _gpu import ctx, dev
    t, keep = _search.device_struct(case, "cuda")
    o, i, d, l = ctx().obs_search_columns(t, nij1, nlev, dev(rig), dev(rjg), dev(rlev), dev(rz))
    r = case["ctype_rows"]
    mine = l[(i >= int(r[4])) & (i < int(r[5]))]
    assert mine.numel() > 0 and float(mine.max()) <= 1e-300 and float(mine.min()) >= 1.27e-303
    assert not bool(((i >= int(r[5])) & (i < int(r[6]))).any())
