"""letkf_tcvital_rows_dev, letkf_tcvital_search_dev and letkf_tcvital_fill_dev (include/letkf_amd_tcvital.h) against the numpy
restatement of tests/_tcvital.py, on the fixtures tests/test_tcvital_statement.py pins.

The location (tcx, tcy) is compared bit for bit: every fixture keeps the second lowest s at least 1e-9 (relative) above the lowest,
far beyond the bound on s.  mslp is compared within 64 eps * mslp, which is derived, not tuned: prsadj raises the rounding of its
base to the power 6.835 (about 16 eps with the device's pow), 25 positive terms in any order cost at most 24 eps, the weights and
the division about 4.  On the exact fixtures (topo = 0, integer ps) s is exact in any order and is compared bit for bit."""
import ctypes as C

import numpy as np
import pytest
import torch

import _tcvital as T

pytestmark = pytest.mark.gpu
TOL = 64 * T.EPS
CANARY = -7.25e77


@pytest.fixture(scope="module")
def env():
    from _gpu import ctx, pkg
    return pkg, ctx()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def params_of(pkg, p):
    s = pkg.TcvitalParams()
    for k, v in p.items():
        setattr(s, k, v)
    return s


def fields_of(pkg, t, nlon, nlat, ih, jh, nmem, member_fastest=False, nv2dd=T.NV2DD):
    """ObsopeFields over the device tensor t: [nmem][NV2DD][nlath][nlonh], or [NV2DD][nlath][nlonh][nmem] (member fastest)"""
    nlonh, nlath = nlon + 2 * ih, nlat + 2 * jh
    f = pkg.ObsopeFields()
    f.nlev, f.khalo, f.nlon, f.nlat, f.ihalo, f.jhalo = 1, 0, nlon, nlat, ih, jh
    f.nv3dd, f.nv2dd, f.nmem, f.m0 = 13, nv2dd, nmem, 0
    f.v3d, f.v2d = None, C.c_void_p(t.data_ptr())
    f.s3k = f.s3i = f.s3j = f.s3v = f.s3m = 1
    if member_fastest:
        f.s2m, f.s2i, f.s2j, f.s2v = 1, nmem, nmem * nlonh, nmem * nlonh * nlath
    else:
        f.s2i, f.s2j, f.s2v, f.s2m = 1, nlonh, nlonh * nlath, T.NV2DD * nlonh * nlath
    return f


def run(env, v, nlon, nlat, ih, jh, p, ritc, rjtc, member_fastest=False):
    """one search of the host fields v [nmem][NV2DD][nlath][nlonh]: cand [nmem][3] as numpy, its canary checked"""
    pkg, ctx = env
    nmem = v.shape[0]
    t = dev(np.moveaxis(v, 0, -1) if member_fastest else v)
    full = torch.full((nmem * 3 + 8,), CANARY, dtype=torch.float64, device="cuda")
    centre = dev(np.array([ritc, rjtc]))
    ctx.tcvital_search(params_of(pkg, p), fields_of(pkg, t, nlon, nlat, ih, jh, nmem, member_fastest), centre[0:1], centre[1:2],
                       cand=full[:nmem * 3])
    torch.cuda.synchronize()
    out = full.cpu().numpy()
    assert (out[nmem * 3:] == CANARY).all()
    return out[:nmem * 3].reshape(nmem, 3)


def check(got, want, what=""):
    """the location bit for bit, mslp within 64 eps * mslp (printed before it is asserted)"""
    worst = np.max(np.abs(got[:, 2] - want[:, 2]) / (T.EPS * np.abs(want[:, 2])))
    print(f"{what}: mslp differs by at most {worst:.2f} eps (bound 64)")
    assert np.array_equal(bits(got[:, :2]), bits(want[:, :2])), (what, got, want)
    assert (np.abs(got[:, 2] - want[:, 2]) <= TOL * np.abs(want[:, 2])).all(), (what, worst)
    assert (want[:, 2] < T.CAP).all()


def low(name):
    nlon, nlat, ih, jh, nmem, seed = T.FIXTURES[name]
    return (nlon, nlat, ih, jh, nmem) + T.low_fixture(nlon, nlat, ih, jh, nmem, seed)


# ---- the search
def test_main_case_and_its_fill(env):
    """37 x 29 (no multiple of the 32 x 8 tile), halos 2, nmem = 3, m0 = 1, kld = 6"""
    pkg, ctx = env
    nlon, nlat, ih, jh, nmem, v, ci, cj = low("main")
    p = T.params()
    for centre in range(nmem):
        got = run(env, v, nlon, nlat, ih, jh, p, ci[centre], cj[centre])
        check(got, T.search(v, nlon, nlat, ih, jh, p, ci[centre], cj[centre]), f"main, centre {centre}")
    # ... and into the obsda rows: m0 = 1, kld = 6, the neighbouring columns and rows keep their bits
    kld, m0, rows = 6, 1, [4, 2, 7]
    ens = np.random.default_rng(1).standard_normal((9, kld))
    qc = np.array([0, 10, 90, 0, 90, 21, 0, 90, 0], dtype=np.int32)
    ens_d, qc_d = dev(ens), dev(qc)
    ctx.tcvital_fill(dev(got[None]), rows, qc_d, ens_d, kld, m0=m0, qc_replace=True)
    torch.cuda.synchronize()
    want_e, want_q = ens.copy(), qc.copy()
    T.fill(got[None], rows, True, want_q, want_e, m0)
    assert np.array_equal(bits(ens_d.cpu().numpy()), bits(want_e)) and np.array_equal(qc_d.cpu().numpy(), want_q)
    assert want_q.tolist() == [0, 10, 0, 0, 0, 21, 0, 0, 0] and np.array_equal(want_e[4, 1:4], got[:, 0])
    assert np.array_equal(bits(want_e[:, [0, 4, 5]]), bits(ens[:, [0, 4, 5]]))


@pytest.mark.parametrize("name, member_fastest", [("main", True), ("unsmoothed", False), ("wide_halo", False), ("wide_halo", True)])
def test_strides_and_halos(env, name, member_fastest):
    nlon, nlat, ih, jh, nmem, v, ci, cj = low(name)
    p = T.params(**T.CUT_DISC)                                                    # (a disc that cuts the grid, unequal spacings)
    got = run(env, v, nlon, nlat, ih, jh, p, ci[1], cj[1], member_fastest)
    check(got, T.search(v, nlon, nlat, ih, jh, p, ci[1], cj[1]), f"{name}, member fastest {member_fastest}")


def test_ties_go_to_the_lowest_j_then_the_lowest_i(env):
    nlon, nlat, ih, jh = 37, 29, 2, 2
    dips = [(8, 10), (34, 10), (14, 16), (14, 22)]                                # two on one row, two on one column
    v = T.exact_fixture(nlon, nlat, ih, jh, 2, dips)
    p = T.params()
    got = run(env, v, nlon, nlat, ih, jh, p, 18.0, 15.0)
    want = T.search(v, nlon, nlat, ih, jh, p, 18.0, 15.0)
    assert np.array_equal(bits(got), bits(want))
    assert got[0, 0] == 7 * p["dx"] + p["cxg1"] and got[0, 1] == 9 * p["dy"] + p["cyg1"] and got[0, 2] == 100500.0
    # without the first of them the other cell of that row wins, then the lower of the column
    for k, cell in ((1, (34, 10)), (2, (14, 16)), (3, (14, 22))):
        v = T.exact_fixture(nlon, nlat, ih, jh, 2, dips[k:])
        got = run(env, v, nlon, nlat, ih, jh, p, 18.0, 15.0)
        assert np.array_equal(bits(got), bits(T.search(v, nlon, nlat, ih, jh, p, 18.0, 15.0)))
        assert got[1, 0] == (cell[0] - 1) * p["dx"] + p["cxg1"] and got[1, 1] == (cell[1] - 1) * p["dy"] + p["cyg1"]


def test_the_rim_of_the_disc(env):
    nlon, nlat, ih, jh = 37, 29, 2, 2
    v = T.exact_fixture(nlon, nlat, ih, jh, 1, [(23, 16)])                        # offset (3, 4) from the centre (20, 12)
    p = T.params(tc_search_dis=10000.0)
    got = run(env, v, nlon, nlat, ih, jh, p, 20.0, 12.0)
    assert np.array_equal(bits(got), bits(T.search(v, nlon, nlat, ih, jh, p, 20.0, 12.0)))
    assert got[0].tolist() == [22 * 2000.0 + p["cxg1"], 15 * 2000.0 + p["cyg1"], 100500.0]        # rdis == 10000.0: not beyond
    p["tc_search_dis"] = float(np.nextafter(10000.0, 0.0))
    got = run(env, v, nlon, nlat, ih, jh, p, 20.0, 12.0)
    assert np.array_equal(bits(got), bits(T.search(v, nlon, nlat, ih, jh, p, 20.0, 12.0)))
    assert got[0, 2] > 100500.0 and got[0, :2].tolist() != [22 * 2000.0 + p["cxg1"], 15 * 2000.0 + p["cyg1"]]


@pytest.mark.parametrize("case", ["disc outside", "dis 0 off a cell", "nan ritc", "nan rjtc", "nan cells", "dis 0 on a cell",
                                  "nan minimum", "above the cap"])
def test_nothing_to_find(env, case):
    pkg, ctx = env
    nlon, nlat, ih, jh, nmem = T.FIXTURES["main"][:5]
    v, p, ritc, rjtc = T.nothing_cases()[case]
    got = run(env, v, nlon, nlat, ih, jh, p, ritc, rjtc)
    want = T.search(v, nlon, nlat, ih, jh, p, ritc, rjtc)
    if case == "dis 0 on a cell":                                                 # that one cell is found
        check(got, want, case)
        assert got[0, 0] == 19 * p["dx"] + p["cxg1"] and got[0, 1] == 11 * p["dy"] + p["cyg1"]
        return
    if case == "nan minimum":                                                     # a NaN s never wins: the 25 cells around it are out
        check(got, want, case)
        assert (np.hypot((got[:, 0] - p["cxg1"]) / p["dx"] + 1 - ritc, (got[:, 1] - p["cyg1"]) / p["dy"] + 1 - rjtc) > 2).all()
        return
    if case == "above the cap":                                                   # found by the search, refused by the fill
        assert np.array_equal(bits(got), bits(want)) and (got[:, 2] >= T.CAP).all() and (got[:, 2] < T.NONE).all()
    else:
        assert got.tolist() == [[T.NONE] * 3] * nmem == want.tolist()
    ens, qc = np.ones((4, nmem)), np.array([90, 90, 90, 7], dtype=np.int32)
    ens_d, qc_d = dev(ens), dev(qc)
    ctx.tcvital_fill(dev(got[None]), [0, 1, 2], qc_d, ens_d, nmem, qc_replace=True)
    torch.cuda.synchronize()
    assert ens_d.cpu().numpy().tolist() == [[T.UNDEF] * nmem] * 3 + [[1.0] * nmem] and qc_d.cpu().numpy().tolist() == [50, 50, 50, 7]


def test_a_two_by_two_decomposition_gives_the_bits_of_the_one_subdomain_run(env):
    pkg, ctx = env
    nlon, nlat, ih, jh, nmem, v, ci, cj = low("seams")
    sub_i, sub_j = nlon // 2, nlat // 2
    p = T.params()
    one = run(env, v, nlon, nlat, ih, jh, p, ci[0], cj[0])
    check(one, T.search(v, nlon, nlat, ih, jh, p, ci[0], cj[0]), "seams, undivided")
    cands = np.array([run(env, T.cut(v, r % 2, r // 2, sub_i, sub_j, ih, jh), sub_i, sub_j, ih, jh,
                          dict(p, i_off=(r % 2) * sub_i, j_off=(r // 2) * sub_j), ci[0], cj[0]) for r in range(4)])
    assert (cands[:, :, 2] < T.NONE).sum() >= nmem + 1
    ens_d, qc_d = torch.zeros((3, nmem), dtype=torch.float64, device="cuda"), torch.full((3,), 90, dtype=torch.int32, device="cuda")
    ctx.tcvital_fill(dev(cands), [0, 1, 2], qc_d, ens_d, nmem)
    torch.cuda.synchronize()
    assert np.array_equal(bits(ens_d.cpu().numpy().T), bits(one)) and qc_d.cpu().numpy().tolist() == [0, 0, 0]


def test_a_minimum_duplicated_across_a_seam_goes_to_the_lower_rank(env):
    pkg, ctx = env
    nlon, nlat, ih, jh, sub_i, sub_j = 24, 20, 2, 2, 12, 10
    v = T.exact_fixture(nlon, nlat, ih, jh, 2, [(10, 5), (15, 5), (3, 14)])      # ranks 0, 1 and 2 hold the same minimum
    p = T.params()
    cands = np.array([run(env, T.cut(v, r % 2, r // 2, sub_i, sub_j, ih, jh), sub_i, sub_j, ih, jh,
                          dict(p, i_off=(r % 2) * sub_i, j_off=(r // 2) * sub_j), 12.0, 9.0) for r in range(4)])
    assert (cands[:3, :, 2] == cands[0, :, 2]).all() and (cands[3, :, 2] > cands[0, :, 2]).all()
    ens_d, qc_d = torch.zeros((3, 2), dtype=torch.float64, device="cuda"), torch.full((3,), 90, dtype=torch.int32, device="cuda")
    ctx.tcvital_fill(dev(cands), [0, 1, 2], qc_d, ens_d, 2)
    torch.cuda.synchronize()
    assert np.array_equal(bits(ens_d.cpu().numpy().T), bits(cands[0]))
    assert ens_d.cpu().numpy()[0].tolist() == [9 * p["dx"] + p["cxg1"]] * 2


def test_two_calls_give_the_same_bits(env):
    nlon, nlat, ih, jh, nmem, v, ci, cj = low("main")
    a = run(env, v, nlon, nlat, ih, jh, T.params(), ci[2], cj[2])
    b = run(env, v, nlon, nlat, ih, jh, T.params(), ci[2], cj[2])
    assert np.array_equal(bits(a), bits(b))


# ---- the fill
def test_fill_replaces_or_merges_and_skips_a_negative_row(env):
    pkg, ctx = env
    cand = np.array([[[1.0, 2.0, 990.0e2], [T.NONE] * 3], [[3.0, 4.0, 990.0e2], [5.0, 6.0, 1100.0e2]]])
    for replace, rows, qc0 in ((True, [1, -1, 3], [0, 90, 90, 90]), (False, [1, 2, 3], [0, 90, 10, 0]), (True, [-1, -1, -5], [1, 2, 3, 4])):
        for members in (slice(0, 2), slice(0, 1)):                                # with and without a member that has no rank
            ens, qc = np.full((4, 4), 0.5), np.array(qc0, dtype=np.int32)
            ens_d, qc_d = dev(ens), dev(qc)
            sub = np.ascontiguousarray(cand[:, members])
            ctx.tcvital_fill(dev(sub), rows, qc_d, ens_d, 4, m0=1, qc_replace=replace)
            torch.cuda.synchronize()
            T.fill(sub, rows, replace, qc, ens, 1)
            assert np.array_equal(bits(ens_d.cpu().numpy()), bits(ens)) and np.array_equal(qc_d.cpu().numpy(), qc), (replace, rows)
    assert qc.tolist() == [1, 2, 3, 4] and (ens == 0.5).all()


# ---- the rows
def rows_case(n, seed, at):
    rng = np.random.default_rng(seed)
    elm = rng.choice(np.array([2819, 3073, 14593, 4001], dtype=np.int32), n)
    dif = rng.uniform(-3.0, 3.0, n).round(2)
    for row, e, d in at:
        elm[row], dif[row] = e, d
    return elm, dif


@pytest.mark.parametrize("n", [7, 300, 70001])
def test_rows_the_last_occurrence_wins(env, n):
    pkg, ctx = env
    at = [(0, T.ID_TCX, 9.0), (1, T.ID_TCY, 9.0), (2, T.ID_TCP, 9.0), (n - 3, T.ID_TCP, 0.5), (n - 2, T.ID_TCX, 0.5), (n - 4, T.ID_TCY, 0.5)]
    elm, dif = rows_case(n, n, at)
    for lb, ub in ((0.0, 1.0), (0.5, 1.0), (0.0, 0.5), (0.6, 1.0), (-1.0, 0.0)):   # dif on both bounds: (lb, ub]
        got = ctx.tcvital_rows(dev(elm), dev(dif), lb, ub)
        want = T.rows(elm, dif, lb, ub)
        assert got[0].tolist() == want[0].tolist() == [n - 1, n - 3, n - 2] and got[1] == want[1] == (lb < 0.5 <= ub)


def test_rows_missing_unequal_and_empty(env):
    pkg, ctx = env
    elm, dif = rows_case(500, 3, [(100, T.ID_TCX, 0.5), (300, T.ID_TCP, 0.5)])
    assert [x.tolist() if hasattr(x, "tolist") else x for x in ctx.tcvital_rows(dev(elm), dev(dif), 0.0, 1.0)] == [[101, 0, 301], False]
    elm, dif = rows_case(500, 4, [(100, T.ID_TCX, 0.5), (200, T.ID_TCY, 0.5), (300, T.ID_TCP, 0.25)])
    got = ctx.tcvital_rows(dev(elm), dev(dif), 0.0, 1.0)
    assert got[0].tolist() == [101, 201, 301] and got[1] is False and T.rows(elm, dif, 0.0, 1.0)[1] is False
    dif[300] = 0.5
    assert ctx.tcvital_rows(dev(elm), dev(dif), 0.0, 1.0)[1] is True
    dif[[100, 200, 300]] = np.nan                                                 # NaN is equal to nothing
    assert ctx.tcvital_rows(dev(elm), dev(dif), 0.0, 1.0)[1] is False
    empty = ctx.tcvital_rows(torch.zeros(0, dtype=torch.int32, device="cuda"), torch.zeros(0, dtype=torch.float64, device="cuda"), 0.0, 1.0)
    assert empty[0].tolist() == [0, 0, 0] and empty[1] is False


# ---- refusals: LETKF_E_INVALID with a message, nothing written
def test_refusals(env):
    pkg, ctx = env
    lib = pkg.tcvital_lib()
    nlon, nlat, ih, jh, nmem = 12, 10, 2, 2, 2
    v = dev(T.low_fixture(nlon, nlat, ih, jh, nmem, 3)[0])
    centre = dev(np.array([5.0, 5.0]))
    cand = torch.full((nmem, 3), CANARY, dtype=torch.float64, device="cuda")

    def search(p=None, f=None, args=None):
        ps = params_of(pkg, dict(T.params(), **(p or {})))
        fs = fields_of(pkg, v, nlon, nlat, ih, jh, nmem)
        for k, val in (f or {}).items():
            setattr(fs, k, val)
        a = [ctx._c, C.addressof(ps), C.addressof(fs), centre[0:1].data_ptr(), centre[1:2].data_ptr(), cand.data_ptr()]
        for k, val in (args or {}).items():
            a[k] = val
        return lib.letkf_tcvital_search_dev(*a)

    def refused(rc):
        assert rc == -1 and pkg.lib().letkf_amd_last_error().decode()
        torch.cuda.synchronize()
        assert bool((cand == CANARY).all())

    assert search() == 0
    torch.cuda.synchronize()
    assert bool((cand != CANARY).all())
    cand.fill_(CANARY)
    for k in range(1, 6):
        refused(search(args={k: None}))
    for f in (dict(v2d=None), dict(nmem=0), dict(nlon=0), dict(nlat=0), dict(ihalo=-1), dict(jhalo=-1), dict(nv2dd=6), dict(s2i=0),
              dict(s2j=0), dict(s2v=0), dict(s2m=0)):
        refused(search(f=f))
    for p in (dict(dx=0.0), dict(dy=-1.0), dict(dx=np.inf), dict(dy=np.nan), dict(tc_search_dis=-1.0), dict(tc_search_dis=np.inf),
              dict(tc_search_dis=np.nan)):
        refused(search(p=p))

    ens, qc = torch.full((4, 4), CANARY, dtype=torch.float64, device="cuda"), torch.full((4,), 77, dtype=torch.int32, device="cuda")
    cands = dev(np.tile(np.array([1.0, 2.0, 990.0e2]), (2, 2, 1)))
    rows = np.array([0, 1, 2], dtype=np.int64)

    def fill(nproc=2, nm=2, m0=0, kld=4, args=None):
        a = [ctx._c, nproc, nm, m0, cands.data_ptr(), rows.ctypes.data, 1, qc.data_ptr(), ens.data_ptr(), kld]
        for k, val in (args or {}).items():
            a[k] = val
        rc = lib.letkf_tcvital_fill_dev(*a)
        torch.cuda.synchronize()
        return rc

    for kw in (dict(nproc=0), dict(nm=0), dict(m0=-1), dict(m0=3), dict(kld=1), dict(args={4: None}), dict(args={5: None}),
               dict(args={7: None}), dict(args={8: None}), dict(args={0: None})):
        rc = fill(**kw)
        assert rc != 0 and pkg.lib().letkf_amd_last_error().decode(), kw
        assert bool((ens == CANARY).all()) and bool((qc == 77).all()), kw
    assert fill(m0=2) == 0 and bool((ens[:3, 2:] != CANARY).all()) and bool((ens[:, :2] == CANARY).all())

    elm, dif = dev(np.array([T.ID_TCX], dtype=np.int32)), dev(np.array([0.0]))
    out, valid = np.full(3, -7, dtype=np.int64), C.c_int32(-7)

    def rows_call(n=1, lb=0.0, ub=1.0, args=None):
        a = [ctx._c, n, elm.data_ptr(), dif.data_ptr(), lb, ub, out.ctypes.data, C.addressof(valid)]
        for k, val in (args or {}).items():
            a[k] = val
        return lib.letkf_tcvital_rows_dev(*a)

    for kw in (dict(n=-1), dict(lb=1.0, ub=0.5), dict(args={2: None}), dict(args={3: None}), dict(args={6: None}), dict(args={7: None}),
               dict(args={0: None})):
        assert rows_call(**kw) != 0 and pkg.lib().letkf_amd_last_error().decode(), kw
        assert out.tolist() == [-7, -7, -7] and valid.value == -7, kw
    assert rows_call(lb=0.5, ub=0.5) == 0 and out.tolist() == [1, 0, 0] and valid.value == 0
