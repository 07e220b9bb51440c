"""CPU checks of tests/_interpspace.py: the layouts' index maps are injective and stay inside their buffer, the slab view of a larger
field addresses what the dense case holds and leaves the rest canary, every new grid has a statement (_interp.expected runs, its
coarse lists go from none to beyond the limit, and no coarse point's selection fell between equal keys -- coarse_lists asserts
it), the default tile_case is the one the interp tests have always built, and the k table names every instantiation."""
import zlib

import numpy as np
import pytest

import _interp as I
import _interpspace as S
from _argspace import CANARY

LAYOUTS = ["ref", "member", "var", "padded"]


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("nlev_total,l0", [(None, 0), (5, 1), (5, 2), (3, 0)])
def test_slab_view_places_every_element_once(layout, nlev_total, l0):
    c = I.tile_case(3)
    a = S.whole_arrays(c)
    fv = S.field_view(c, a, layout, nlev_total, l0)
    idx = fv["idx"]
    assert fv["p0"] == l0 * c["nij1"] and fv["nf"] == fv["infl_sv"] == c["nij1"] * (nlev_total or c["nlev"])
    assert idx.shape == (c["nv"], c["nens"], c["npts"])
    assert len(np.unique(idx)) == idx.size and idx.min() >= 0 and idx.max() < fv["size"]
    buf = S.place_state(a, fv)
    assert np.array_equal(buf[idx], c["gues"])
    rest = np.ones(fv["size"], bool)
    rest[idx.ravel()] = False
    assert (buf.view(np.int64)[rest] == CANARY).all()
    v, m, p = 3, 2, c["npts"] - 1
    assert idx[v, m, p] == fv["off"] + (fv["p0"] + p) * fv["sp"] + m * fv["sm"] + v * fv["sv"]
    if (nlev_total or c["nlev"]) == c["nlev"] and layout != "padded":
        assert not rest.any()
    else:
        assert rest.any()
    # the fields per point and per (variable, point): the call's values at p0 .., the fill elsewhere
    infl = S.place_field(fv, a["infl"], 1.0 + 0.001 * np.arange(c["nv"] * fv["nf"]))
    assert infl.shape == (c["nv"], fv["nf"])
    assert np.array_equal(infl[:, fv["p0"]:fv["p0"] + c["npts"]], a["infl"])
    beta = S.place_field(fv, S.beta_field(c), np.nan)
    assert np.isnan(beta).sum() == fv["nf"] - c["npts"]


def test_the_window_cut_goes_through_the_same_view():
    """a rectangle of the case (the form of the window tests' cut) in the padded layout as levels 1..3 of 5"""
    c = I.tile_case(3)
    nx, ny, nlev = 3, 3, c["nlev"]
    col = (np.arange(4, 7)[None, :] + c["nx"] * np.arange(2, 5)[:, None]).ravel()
    gp = (col[None, :] + c["nij1"] * np.arange(nlev)[:, None]).ravel()
    a = dict(nx=nx, ny=ny, npts=nx * ny * nlev, gues=c["gues"][:, :, gp], infl=c["infl"].reshape(c["nv"], -1)[:, gp])
    fv = S.field_view(c, a, "padded", 5, 1)
    assert fv["p0"] == 9 and fv["nf"] == 45
    assert len(np.unique(fv["idx"])) == fv["idx"].size and fv["idx"].max() < fv["size"]
    assert np.array_equal(S.place_state(a, fv)[fv["idx"]], c["gues"][:, :, gp])


# CRC32 over rig, rjg, rlev, rz, ensval, dep, gues, infl (case_crc) of tile_case(3) and tile_case(20, nv=5), taken from
# tests/_interp.py as it was before tile_case took dxs and dys (git show 375036c:tests/_interp.py, imported beside this module)
RECORDED = (1192735023, 868545029)


def case_crc(c):
    h = 0
    for n in ("rig", "rjg", "rlev", "rz", "ensval", "dep", "gues", "infl"):
        h = zlib.crc32(np.ascontiguousarray(c[n]).tobytes(), h)
    return h


def test_default_tile_case_is_unchanged():
    """the spacings' defaults and the nv > 4 guard leave the cases of the interp tests as they were: CRC32 of the arrays of
    tile_case(3) and tile_case(20, nv=5), recorded before tile_case took dxs and dys"""
    want = {(3, 11): RECORDED[0], (20, 5): RECORDED[1]}
    for (k, nv), crc in want.items():
        c = I.tile_case(k, nv=nv)
        assert case_crc(c) == crc, (k, nv, case_crc(c))
    assert I.tile_case(3) is I.tile_case(3)                     # (memoised: one case object per argument list)


def q_update_cuts(c):
    """Q_UPDATE_TOP lies between the levels' mean pressures: some points skip their moisture variables, some do not"""
    top = c["gues"][4, c["k"]] < S.Q_UPDATE_TOP
    return top.any() and not top.all()


@pytest.mark.parametrize("name,k", [(n, 50) for n in S.GRIDS] + [("full_cells", 100)])
def test_every_grid_has_a_statement(name, k):
    c, sx, sy = S.grid_case(name, k=k)
    cfg = S.cfg_of(c)
    assert cfg["q_update_top"] == S.Q_UPDATE_TOP and cfg["relax_to_inflated_prior"] == 1 and cfg["det_run"] == 1
    assert q_update_cuts(c) == (c["nlev"] > 1)
    nx, ny, nlev = S.GRIDS[name][:3]
    assert (c["nx"], c["ny"], c["nlev"]) == (nx, ny, nlev)
    i_org, j_org = c["tc"]["scal"]["i_org"], c["tc"]["scal"]["j_org"]
    assert c["rig"].max() < i_org + 40 and c["rjg"].max() < j_org + 32          # inside build_case's domain
    exp = S.expected(c, cfg, sx, sy, beta=S.beta_field(c))                      # (coarse_lists asserts that no point is tied)
    n = exp["ncoarse"]
    assert len(n) == len(exp["ix"]) * len(exp["iy"]) * nlev
    if S.GRIDS[name][8]:
        assert (n == 0).any() and (n > S.LIMITS[0]).any(), n
    else:
        assert (n > S.LIMITS[0]).all(), n
    k = c["k"]
    assert np.isfinite(exp["anal"][:, S.members(k, True)]).all() and np.isfinite(exp["rtps"]).all()
    assert np.isnan(exp["anal"][:, k]).all()


def test_grid_shapes_are_the_edges_they_stand_for():
    ax = lambda name: (list(I.coarse_axis(S.GRIDS[name][0], S.GRIDS[name][3])), list(I.coarse_axis(S.GRIDS[name][1], S.GRIDS[name][4])))
    assert ax("one_column") == ([0], [0])
    assert ax("two_columns_stride_8") == ([0, 1], [0])
    assert ax("extent_is_stride_plus_1") == ([0, 8], [0, 1])
    assert ax("last_cell_one_wide") == ([0, 8, 9], [0, 4, 8])
    assert ax("full_cells") == ([0, 8, 16], [0, 8])
    # a full cell: 8 x 8 points of 11 variables, 704 rows -- 6 chunks of 128, 11 of 64
    assert 8 * 8 * 11 == 704 and -(-704 // 128) == 6 and -(-704 // 64) == 11


@pytest.mark.parametrize("k", sorted(S.K_BOUNDS))
def test_k_bounds_cases_are_untied(k):
    c = I.tile_case(k)
    n = S.level_counts(c, 2, 2)                                  # (coarse_lists asserts that no point is tied)
    assert (n == 0).any() and (n > S.LIMITS[0]).any() and q_update_cuts(c)
    nct = -(-k // 16)
    assert S.K_BOUNDS[k][0] == (1 if nct <= 1 else 2 if nct <= 2 else 4 if nct <= 4 else 8)
    assert S.apply_kernel_name(k) == "letkf_interp_apply_kernel<NCT=%d,NW=%d>" % S.K_BOUNDS[k]
    kp = (k + 3) & ~3
    assert (kp != k) == (k % 4 != 0) and kp <= 16 * S.K_BOUNDS[k][0]


@pytest.mark.parametrize("nv,k", [(1, 20), (2, 20), (15, 20), (32, 20), (1, 100)])
def test_nv_cases(nv, k):
    c = I.tile_case(k, nv=nv)
    assert c["gues"].shape == (nv, k + 2, c["npts"])
    cfg = S.cfg_of(c)
    if nv > 4:
        assert np.array_equal(c["gues"][4, k], c["rlev"]) and q_update_cuts(c) and cfg["q_update_top"] > 0.0
    else:
        assert "q_update_top" not in cfg and "relax_to_inflated_prior" not in cfg      # no pressure slot: neither rule
    exp = S.expected(c, cfg, 2, 2, beta=S.beta_field(c))
    assert np.isfinite(exp["anal"][:, S.members(k, True)]).all()


def test_the_rules_that_read_the_point_itself_are_active():
    """on the layout cases (k = 20, 50, 100) Q_UPDATE_TOP changes the answer of the moisture variables where a point skips them,
    RELAX_TO_INFLATED_PRIOR changes every updated variable, and the moisture class's solves take two different rho"""
    for k in S.K_LAYOUTS:
        c = I.tile_case(k)
        assert q_update_cuts(c)
        cfg = S.cfg_of(c)
        skip = c["gues"][4, k] < S.Q_UPDATE_TOP
        full = S.expected(c, cfg, 2, 2)
        no_top = S.expected(c, dict(cfg, q_update_top=0.0), 2, 2)
        no_rip = S.expected(c, dict(cfg, relax_to_inflated_prior=0), 2, 2)
        assert not np.array_equal(full["anal"][5:, :k][:, :, skip], no_top["anal"][5:, :k][:, :, skip])
        assert np.array_equal(full["anal"][5:, :k][:, :, skip], (c["gues"][5:, :k] + c["gues"][5:, k:k + 1])[:, :, skip])
        assert not np.array_equal(full["rtps"], no_rip["rtps"])
        ix, iy, pts = S.coarse_points(c, 2, 2)
        moist = sum(1 << v for v in (5, 7, 10))
        rho = np.array([I.solve_rho(c, cfg, int(p), moist) for p in pts])
        assert (rho[skip[pts]] == 1.0).all() and np.array_equal(rho[~skip[pts]], c["infl"][pts[~skip[pts]] + c["npts"] * 5])
        assert skip[pts].any() and not skip[pts].all()


def test_slab_budget_and_beta_field():
    c = I.tile_case(50, nlev=5)
    full = S.ws_bytes_all(c, 2, 2)
    ix, iy, pts = S.coarse_points(c, 2, 2)
    n = np.array([len(v[0]) for v in S.coarse_lists(c, pts).values()]).reshape(5, -1)
    one_level = max(20 * n[l].sum() + n.shape[1] * 8 * (50 * 50 + 100 + max(1, n[l].max()) * 54) for l in range(5))
    assert one_level < 0.3 * full                               # 0.3 of it already holds more than any single level
    # the cuts the fractions give, replayed from the header's formula: apart from one level per slab (ws_bytes = 1; 0.3 gives
    # the same) they are three different uneven cuts, none of them the single slab
    cuts = [S.slab_cuts(c, 2, 2, int(f * full)) for f in S.SLAB_FRACTIONS]
    assert S.slab_cuts(c, 2, 2, 1) == (1, 1, 1, 1, 1) and S.slab_cuts(c, 2, 2, full) == (5,)
    assert all(sum(x) == 5 for x in cuts)
    uneven = {x for x in cuts if x not in ((5,), (1, 1, 1, 1, 1))}
    assert len(uneven) >= 3 and all(len(set(x)) > 1 for x in uneven), cuts
    for name in list(S.GRIDS) + ["base"]:
        cc = I.tile_case(50) if name == "base" else S.grid_case(name)[0]
        b = S.beta_field(cc)
        assert (b == 0.0).any() and (b == 0.37).any() and ((b == 1.0).any() or cc["npts"] < 3)
