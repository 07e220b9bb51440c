"""letkf_obsda_assemble_dev and letkf_obsda_encode_dev (include/letkf_amd_obsfile.h) against the statement of tests/_obsfile.py:
every output is equal to it, floats as their bit patterns; the columns of ensval that no image names keep their canary, and so
does everything beyond the arrays' extent.  The tile's sizes are read from the package (OBSFILE_TILE_ROWS / _MEMBERS), which the
binding test ties to the header the kernel is built from."""
import functools
import re

import numpy as np
import pytest
import torch

import _obsfile as O
from __graft_entry__ import load_package

pytestmark = pytest.mark.gpu
I32_CANARY, F64_CANARY, EXTRA = 0x5A5A5A5A, -7.25e77, 16
NMEM = (1, 2, 3, 20, 50, 51, 64, 65, 130)
KLD_EXTRA = (0, 1, 13)
COLS = ("identity", "reversed", "last_to_end")


@pytest.fixture(scope="module")
def env():
    from _gpu import ctx, pkg
    return pkg, ctx()


TILE = load_package().OBSFILE_TILE_ROWS                  # (the module alone: no library, no device)
NOBS = sorted({0, 1, 63, 64, 65, TILE - 1, TILE + 1, 3 * TILE + 7})


def col_map(kind, nmem, kld):
    col = np.arange(nmem, dtype=np.int32)
    if kind == "reversed":
        col = col[::-1].copy()
    if kind == "last_to_end":
        col[-1] = kld - 1                                # the mean's file lands in the last column (mmdetobs)
    return col


def dev_image(rec, be=False):
    return torch.from_numpy(np.frombuffer(O.frame(rec, be), dtype=np.uint8).copy()).cuda()


def guarded_out(nobs, kld, nrec, qc0=None, lev0=None, val20=None):
    full = {k: torch.full((nobs + EXTRA,), I32_CANARY, dtype=torch.int32, device="cuda") for k in ("set", "idx", "qc")}
    full["ensval"] = torch.full((nobs * kld + EXTRA,), F64_CANARY, dtype=torch.float64, device="cuda")
    full["qc"][:nobs] = torch.from_numpy(np.zeros(nobs, dtype=np.int32) if qc0 is None else qc0).cuda()
    for k, v in (("lev", lev0), ("val2", val20)):
        full[k] = None
        if nrec == 6:
            full[k] = torch.full((nobs + EXTRA,), F64_CANARY, dtype=torch.float64, device="cuda")
            full[k][:nobs] = torch.from_numpy(np.zeros(nobs) if v is None else v).cuda()
    views = {k: (None if t is None else t[:nobs]) for k, t in full.items()}
    views["ensval"] = full["ensval"][:nobs * kld].view(nobs, kld)
    return full, views


def run_and_check(ctx, recs, col, kld, nrec=4, be=False, qc0=None, is_member=None, member=0, finish=False, lev0=None, val20=None,
                  ninconsistent=0):
    nobs, nmem = recs[0].shape[0], len(recs)
    images = [dev_image(r, be) for r in recs]
    full, views = guarded_out(nobs, kld, nrec, qc0, lev0, val20)
    res = ctx.obsda_assemble(images, nobs, kld, col=col, nrec=nrec, big_endian=be, is_member=is_member, member=member, finish=finish,
                             check=True, out=views)
    torch.cuda.synchronize()
    ens0 = np.full((nobs, kld), F64_CANARY)
    st = O.assemble(recs, col, ens0, np.zeros(nobs, dtype=np.int32) if qc0 is None else qc0, is_member,
                    (np.zeros(nobs) if lev0 is None else lev0) if nrec == 6 else None,
                    (np.zeros(nobs) if val20 is None else val20) if nrec == 6 else None, member, finish)
    assert (res["nbad"], res["ninconsistent"]) == (0, ninconsistent) and st["ninconsistent"] == ninconsistent
    for k in ("set", "idx", "qc"):
        got = full[k].cpu().numpy()
        assert np.array_equal(got[:nobs], st[k]), k
        assert (got[nobs:] == I32_CANARY).all(), k
    got = full["ensval"].cpu().numpy()
    assert O.same_bits(got[:nobs * kld].reshape(nobs, kld), st["ensval"])          # the untouched columns hold the canary in both
    assert (got[nobs * kld:] == F64_CANARY).all()
    if nobs and kld > nmem:
        assert (st["ensval"] == F64_CANARY).any()
    for k in ("lev", "val2"):
        if nrec == 6:
            got = full[k].cpu().numpy()
            assert O.same_bits(got[:nobs], st[k]), k
            assert (got[nobs:] == F64_CANARY).all(), k
    return full, st, images


@functools.lru_cache(None)
def records(nobs, nmem, nrec=4):
    return O.obsda_records(nobs, nmem, nrec, seed=nobs * 131 + nmem)


def test_the_tile_is_the_headers(env):
    pkg, _ = env
    assert (pkg.OBSFILE_TILE_ROWS, pkg.OBSFILE_TILE_MEMBERS) == (64, 16)
    assert min(NMEM) < pkg.OBSFILE_TILE_MEMBERS < max(NMEM) and 64 in NMEM and 65 in NMEM


@pytest.mark.parametrize("nmem", NMEM)
@pytest.mark.parametrize("nobs", NOBS)
def test_assemble_rows_by_members(env, nobs, nmem):
    """every nobs with every nmem; the three kld and the three column maps take turns, and test_every_kld_and_column_map makes
    all nine of them at one size"""
    pkg, ctx = env
    turn = NOBS.index(nobs) + NMEM.index(nmem)
    kld = nmem + KLD_EXTRA[turn % 3]
    run_and_check(ctx, records(nobs, nmem), col_map(COLS[(turn // 3) % 3], nmem, kld), kld)


@pytest.mark.parametrize("kind", COLS)
@pytest.mark.parametrize("extra", KLD_EXTRA)
@pytest.mark.parametrize("nmem", (3, 51))
def test_every_kld_and_column_map(env, nmem, extra, kind):
    pkg, ctx = env
    nobs, kld = 3 * pkg.OBSFILE_TILE_ROWS + 7, nmem + extra
    full, st, images = run_and_check(ctx, records(nobs, nmem), col_map(kind, nmem, kld), kld)
    again, views = guarded_out(nobs, kld, 4)
    ctx.obsda_assemble(images, nobs, kld, col=col_map(kind, nmem, kld), out=views)
    torch.cuda.synchronize()
    for k in ("set", "idx", "qc", "ensval"):
        assert torch.equal(again[k].view(torch.uint8), full[k].view(torch.uint8)), k      # bitwise equal between two calls


@pytest.mark.parametrize("be", [False, True], ids=["le", "be"])
@pytest.mark.parametrize("where", ["incoming", "first", "middle", "last"])
def test_qc_is_the_maximum_of_the_callers_and_every_image(env, where, be):
    pkg, ctx = env
    nobs, nmem = 130, 50
    recs = [r.copy() for r in records(nobs, nmem)]
    for r in recs:
        r[:, 3] = np.minimum(r[:, 3], 50)
    qc0 = np.zeros(nobs, dtype=np.int32)
    rows = np.arange(0, nobs, 3)
    if where == "incoming":
        qc0[rows] = 97
    else:
        recs[{"first": 0, "middle": 23, "last": nmem - 1}[where]][rows, 3] = 98
    full, st, _ = run_and_check(ctx, recs, col_map("identity", nmem, nmem), nmem, be=be, qc0=qc0)
    assert (st["qc"][rows] == (97 if where == "incoming" else 98)).all()


def sequential_differs_from_pairwise(vals):
    seq = np.float64(0.0)
    for v in vals:
        seq = seq + np.float64(v)
    tree = [np.float64(v) for v in vals]
    while len(tree) > 1:
        tree = [tree[i] + tree[i + 1] if i + 1 < len(tree) else tree[i] for i in range(0, len(tree), 2)]
    return seq != tree[0]


@pytest.mark.parametrize("finish", [False, True])
@pytest.mark.parametrize("nmem", (20, 51))
def test_h08_sums_in_image_order_over_the_members_only(env, nmem, finish):
    pkg, ctx = env
    nobs = pkg.OBSFILE_TILE_ROWS + 1
    recs = records(nobs, nmem, 6)
    is_member = np.ones(nmem, dtype=np.int32)
    is_member[[1, nmem - 1]] = 0                         # a deterministic run in the middle, the mean at the end
    member = int(is_member.sum())
    # the values span 17 decades: a tree's sum differs from the sequential one in the last bits on most rows
    assert sum(sequential_differs_from_pairwise([r[n, 4] for m, r in enumerate(recs) if is_member[m]]) for n in range(nobs)) > nobs // 4
    rng = np.random.default_rng(1)
    lev0, val20 = rng.uniform(0.0, 1.0, nobs), np.zeros(nobs)
    kld = nmem + 1
    full, st, _ = run_and_check(ctx, recs, col_map("last_to_end", nmem, kld), kld, nrec=6, is_member=is_member, member=member,
                                finish=finish, lev0=lev0, val20=val20)
    all_images = O.assemble(recs, col_map("last_to_end", nmem, kld), np.zeros((nobs, kld)), np.zeros(nobs, dtype=np.int32), None, lev0, val20,
                            member, finish)
    assert not O.same_bits(all_images["lev"], st["lev"])                     # the non-members would have shown


@pytest.mark.parametrize("planted", [0, 1, 3])
def test_inconsistent_rows_are_counted(env, planted):
    pkg, ctx = env
    nobs, nmem = 200, 20
    recs = [r.copy() for r in records(nobs, nmem)]
    for (row, m, what) in [(199, 19, 0), (0, 1, 1), (64, 17, 1)][:planted]:
        recs[m][row, what] += 1
    if planted == 3:
        recs[5][64, 0] += 2                              # a second image on an already planted row: still one row
    run_and_check(ctx, recs, col_map("identity", nmem, nmem), nmem, ninconsistent=planted)


def test_bad_markers_are_counted_over_all_images(env):
    pkg, ctx = env
    nobs, nmem = 70, 3
    recs = records(nobs, nmem)
    images = [dev_image(r) for r in recs]
    w = images[2].view(torch.int32)
    w[6 * 69 + 5] = 0
    w[0] = 24
    res = ctx.obsda_assemble(images, nobs, nmem, check=True)
    torch.cuda.synchronize()
    assert (res["nbad"], res["ninconsistent"]) == (2, 0)
    assert O.same_bits(res["ensval"].cpu().numpy(), O.assemble(recs, np.arange(3), np.zeros((nobs, 3)), np.zeros(nobs, dtype=np.int32))["ensval"])


def test_an_unaligned_image_and_a_repeated_column_are_refused(env):
    pkg, ctx = env
    nobs, nmem = 65, 3
    recs = records(nobs, nmem)
    images = [dev_image(r) for r in recs]
    shifted = torch.zeros(images[1].numel() + 4, dtype=torch.uint8, device="cuda")
    shifted[1:1 + images[1].numel()] = images[1]
    for bad_images, col, word in (([images[0], shifted[1:1 + images[1].numel()], images[2]], [0, 1, 2], r"images\[1\]"),
                                  (images, [0, 2, 2], r"col\[2\]")):
        full, views = guarded_out(nobs, nmem, 4)
        with pytest.raises(pkg.LetkfError, match=word):
            ctx.obsda_assemble(bad_images, nobs, nmem, col=np.array(col, dtype=np.int32), out=views)
        torch.cuda.synchronize()
        assert (full["ensval"] == F64_CANARY).all() and (full["set"] == I32_CANARY).all() and (full["idx"] == I32_CANARY).all()


@pytest.mark.parametrize("be", [False, True], ids=["le", "be"])
@pytest.mark.parametrize("nrec", [4, 6])
@pytest.mark.parametrize("nobs", [0, 1, 255, 256, 257, 1000])
def test_obsda_encode(env, nobs, nrec, be):
    pkg, ctx = env
    rng = np.random.default_rng(nobs)
    kld = 7
    set_ = rng.integers(1, 4, nobs).astype(np.int32)
    idx = rng.integers(1, 2 ** 24, nobs).astype(np.int32)
    if nobs > 1:
        idx[1] = 2 ** 24 + 1                             # rounds to 2^24, as the reference's comment says
    qc = rng.integers(0, 99, nobs).astype(np.int32)
    ensval, val = rng.normal(0, 10, (nobs, kld)), rng.normal(0, 10, nobs)
    lev, val2 = (rng.uniform(0, 1e5, nobs), rng.uniform(200, 300, nobs)) if nrec == 6 else (None, None)
    d = lambda a: None if a is None else torch.from_numpy(a).cuda()
    for col in (-1, 0, kld - 1):
        want = O.frame(O.encode_obsda(set_, idx, val if col < 0 else ensval[:, col], qc, lev, val2), be)
        buf = torch.full((len(want) + EXTRA,), 0xA5, dtype=torch.uint8, device="cuda")
        ctx.obsda_encode(d(set_), d(idx), d(qc), ensval=d(ensval), col=col, val=d(val), lev=d(lev), val2=d(val2), nrec=nrec, big_endian=be,
                         out=buf[:len(want)])
        torch.cuda.synchronize()
        got = buf.cpu().numpy()
        assert got[:len(want)].tobytes() == want and (got[len(want):] == 0xA5).all(), col
    if nobs > 1:
        assert O.unframe(want, nrec, be)[0][1, 1] == 2.0 ** 24
