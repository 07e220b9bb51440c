"""letkf_nobs_fields_dev (include/letkf_amd_nobsout.h): work3dn and the reference's eleven fields from the counts and cut-offs per
combined type, held to the numpy statement tests/_nobsout.py exactly -- the integers arrive in the doubles, the cut-offs are
copied -- for one point, both sides of the kernel's tile of 128 points and of a wave, many tiles; 1, 5 and 64 combined types; 24 and
32 report types; the (nij1, nlev, 11) layout and the transposed one; each optional pointer NULL; canaries; the refusals.  And the
chain: letkf_das_columns_nobs_dev -> letkf_nobs_fields_dev -> the statement on the domain of tests/test_gpu_nobsout.py."""
import numpy as np
import pytest
import torch

import _nobsout as N

pytestmark = pytest.mark.gpu

PAD = 64


def tables(nctype, nobtype, rng):
    """elm_u / typ of nctype distinct (uid, report type) pairs: the three radar types first where there is room, two pairs in report
    type 1 and one in the last report type"""
    pairs = [(9, 22), (10, 22), (11, 22), (1, 1), (2, 1), (3, nobtype), (4, 8), (3, 3), (3, 4)][:nctype] if nctype > 1 else [(10, 22)]
    while len(pairs) < nctype:
        p = (int(rng.integers(1, 17)), int(rng.integers(1, nobtype + 1)))
        if p not in pairs:
            pairs.append(p)
    order = rng.permutation(nctype)
    return [pairs[i][0] for i in order], [pairs[i][1] for i in order]


def canary(n, fill=-4.0):
    full = torch.full((n + 2 * PAD,), fill, dtype=torch.float64, device="cuda")
    return full, full[PAD:PAD + n]


def held(full, fill=-4.0):
    return bool((full[:PAD] == fill).all()) and bool((full[-PAD:] == fill).all())


def same(t, want):
    return np.array_equal(t.cpu().numpy().view(np.int64), np.ascontiguousarray(want).view(np.int64))


@pytest.mark.parametrize("nobtype", [24, 32])
@pytest.mark.parametrize("nctype", [1, 5, 64])
@pytest.mark.parametrize("npts", [1, 63, 64, 65, 127, 129, 1000])
def test_work3dn_and_fields_are_the_statement(npts, nctype, nobtype):
    from _gpu import ctx, dev
    rng = np.random.default_rng(npts * 100 + nctype + nobtype)
    elm_u, typ = tables(nctype, nobtype, rng)
    nobs = rng.integers(0, 120, (npts, nctype)).astype(np.int32)
    cutd = rng.uniform(0.0, 3.0e4, (npts, nctype))
    w_want = N.work3dn(nobs, cutd, elm_u, typ, nobtype=nobtype)
    f_want = N.fields(w_want, nobtype=nobtype)
    c = ctx()
    d_n, d_c = dev(nobs), dev(cutd)
    nrow = nobtype + 6
    wf, w = canary(npts * nrow)
    ff, f = canary(npts * 11)                                     # (nij1, nlev, 11): element (p, f) at p + f * npts
    c.nobs_fields(npts, elm_u, typ, d_n, d_c, work3dn=w, fields=f, nobtype=nobtype)
    gf, g = canary(npts * 11)                                     # transposed: (p, f) at 11 p + f
    c.nobs_fields(npts, elm_u, typ, d_n, d_c, fields=g, sp=11, sv=1, nobtype=nobtype)
    torch.cuda.synchronize()
    assert same(w, w_want.reshape(-1)) and held(wf)
    assert same(f, f_want.T.reshape(-1)) and held(ff)
    assert same(g, f_want.reshape(-1)) and held(gf)
    # each optional pointer NULL: no cut-offs (zeros in the three rows), work3dn alone
    w0f, w0 = canary(npts * nrow)
    c.nobs_fields(npts, elm_u, typ, d_n, None, work3dn=w0, nobtype=nobtype)
    torch.cuda.synchronize()
    assert same(w0, N.work3dn(nobs, None, elm_u, typ, nobtype=nobtype).reshape(-1)) and held(w0f)
    # strides with room between the elements, other picks and uids
    sp, sv = 3, 3 * npts + 5
    hf, h = canary((npts - 1) * sp + 10 * sv + 1)
    pick = (nobtype, 1, 1, 8, 22)
    c.nobs_fields(npts, elm_u, typ, d_n, d_c, fields=h, sp=sp, sv=sv, nobtype=nobtype, pick=pick, uid_ref=1, uid_re0=2, uid_vr=3, typ_radar=1)
    torch.cuda.synchronize()
    f2 = N.fields(N.work3dn(nobs, cutd, elm_u, typ, nobtype=nobtype, uid=(1, 2, 3), typ_radar=1), nobtype=nobtype, pick=pick)
    hh = h.cpu().numpy()
    idx = (np.arange(npts)[:, None] * sp + np.arange(11)[None, :] * sv)
    assert np.array_equal(hh[idx].view(np.int64), f2.view(np.int64)) and held(hf)
    rest = np.ones(hh.size, dtype=bool)
    rest[idx.reshape(-1)] = False
    assert (hh[rest] == -4.0).all()


def test_two_calls_give_the_same_bits_and_no_points_is_no_error():
    from _gpu import ctx, dev
    rng = np.random.default_rng(3)
    elm_u, typ = tables(20, 24, rng)
    npts = 5000
    d_n, d_c = dev(rng.integers(0, 100, (npts, 20)).astype(np.int32)), dev(rng.uniform(0, 1e4, (npts, 20)))
    c = ctx()
    out = []
    for _ in range(2):
        w = torch.full((npts * 30,), -1.0, dtype=torch.float64, device="cuda")
        f = torch.full((npts * 11,), -1.0, dtype=torch.float64, device="cuda")
        c.nobs_fields(npts, elm_u, typ, d_n, d_c, work3dn=w, fields=f)
        torch.cuda.synchronize()
        out.append((w, f))
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1]) and float(out[0][0].min()) >= 0.0
    w = torch.full((30,), -1.0, dtype=torch.float64, device="cuda")
    c.nobs_fields(0, elm_u, typ, d_n, d_c, work3dn=w, fields=w, sv=1)
    torch.cuda.synchronize()
    assert bool((w == -1.0).all())


def test_refusals_write_nothing():
    from _gpu import ctx, dev, pkg
    rng = np.random.default_rng(4)
    elm_u, typ = tables(5, 24, rng)
    npts = 70
    d_n, d_c = dev(rng.integers(0, 100, (npts, 5)).astype(np.int32)), dev(rng.uniform(0, 1e4, (npts, 5)))
    c = ctx()
    wf, w = canary(npts * 30)
    ff, f = canary(npts * 11)

    def refused(match, *a, **kw):
        base = dict(work3dn=w, fields=f)
        base.update(kw)
        with pytest.raises(pkg.LetkfError, match=match):
            c.nobs_fields(*(a or (npts, elm_u, typ, d_n, d_c)), **base)
        torch.cuda.synchronize()
        assert bool((wf == -4.0).all()) and bool((ff == -4.0).all()), match

    refused("nobs_ctype is NULL", npts, elm_u, typ, None, d_c)
    refused("both NULL", work3dn=None, fields=None)
    refused("npts < 0", -1, elm_u, typ, d_n, d_c)
    refused("nctype must be", npts, [], [], d_n, d_c)
    refused("nctype must be", npts, [1] * 65, list(range(1, 66)), d_n, d_c)
    refused("nobtype must be", nobtype=0)
    refused("nobtype must be", nobtype=33)
    refused("uid_ref", uid_vr=17)
    refused("uid_ref", uid_ref=0)
    refused("typ_radar", typ_radar=25)
    refused("pick must be", pick=(1, 3, 4, 8, 25))
    refused("pick must be", pick=(0, 3, 4, 8, 22))
    refused("elm_u_ctype must be", npts, [17] + elm_u[1:], typ, d_n, d_c)
    refused("typ_ctype must be", npts, elm_u, [25] + typ[1:], d_n, d_c)
    refused("same \\(elm_u, typ\\)", npts, elm_u[:4] + elm_u[:1], typ[:4] + typ[:1], d_n, d_c)
    # strides that make two elements coincide
    refused("strides", sp=1, sv=npts - 1)
    refused("strides", sp=10, sv=1)
    refused("strides", sp=0, sv=npts)
    refused("strides", sp=-1, sv=npts)
    refused("strides", sp=2, sv=npts)
    # outputs on the inputs, or on each other
    refused("output overlaps an input", work3dn=d_c[0])
    refused("output overlaps an input", fields=d_c[-1], sv=1, sp=11)
    refused("output overlaps an input", fields=d_n.view(-1).view(torch.float64))
    refused("work3dn overlaps fields", work3dn=w, fields=w[npts * 30 - 8:], sv=1, sp=11)
    assert held(wf) and held(ff)


def test_chain_main_loop_then_fields_then_statement():
    from test_gpu_nobsout import ELM_U, NIJ1, NLEV, NPTS, TYP, Setup, three_slabs
    s = Setup(10, 1, True)
    off, n_ref, c_ref = s.search()
    r, _ = s.new(three_slabs(off))
    w = torch.full((NPTS * 30,), -1.0, dtype=torch.float64, device="cuda")
    f = torch.full((11, NLEV, NIJ1), -1.0, dtype=torch.float64, device="cuda")          # Fortran's (nij1, nlev, 11)
    s.c.nobs_fields(NPTS, ELM_U, TYP, r.nobs_ctype, r.cutd_ctype, work3dn=w, fields=f)
    torch.cuda.synchronize()
    live = s.beta_np != 0.0
    n = np.where(live[:, None], n_ref.cpu().numpy(), 0)
    cu = np.where(live[:, None], c_ref.cpu().numpy(), 0.0)
    w_want = N.work3dn(n, cu, ELM_U, TYP)
    assert same(w, w_want.reshape(-1))
    assert same(f.reshape(-1), N.fields(w_want).T.reshape(-1))
    # what the fields say about this domain: type 22 is the merged pair on its master, type 1 the unlimited T, type 3 the limited ps
    ff = f.cpu().numpy().reshape(11, NPTS)
    assert np.array_equal(ff[4], ff[5]) and not ff[6].any() and not ff[7].any() and ff[4].max() == 12.0
    assert ff[0].max() > 12.0 and ff[1].max() == 3.0 and not ff[2].any() and not ff[3].any()
    assert np.array_equal(ff[0] + ff[1] + ff[4], r.nobs_out.cpu().numpy().astype(np.float64))
    assert (ff[8][live] > 0.0).all() and not ff[8][~live].any() and not ff[9].any() and not ff[10].any()
