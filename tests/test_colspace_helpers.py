"""CPU checks of tests/_colspace.py: the slab view of a larger field places every element of the slab once and leaves the rest of
the field canary, the per-class composition of the oracle is the single call's answer where the classes cannot differ, and the
route table reaches every route of letkf_das_columns_dev."""
import numpy as np
import pytest

from _argspace import CANARY, CFG
from _colspace import (AXIS_ROUTES, COL_ROUTES, DEFAULTS, FREE, VARLOC, col_case, field_view, oracle, place_field,
                       route_family)


@pytest.mark.parametrize("layout", ["ref", "member", "var", "padded"])
@pytest.mark.parametrize("nlev_total,l0", [(None, 0), (7, 2), (7, 3), (5, 0)])
def test_slab_view_places_every_element_once(layout, nlev_total, l0):
    c = col_case("free_k9", seed=1, nij1=5, nlev=4)
    sp, sm, sv, off, size, p0, idx = field_view(c, layout, nlev_total, l0)
    assert p0 == l0 * c["nij1"]
    assert idx.shape == (c["nv"], c["nens"], c["npts"])
    assert len(np.unique(idx)) == idx.size and idx.min() >= 0 and idx.max() < size
    buf = place_field(c, idx, size)
    assert np.array_equal(buf[idx].ravel(), c["gues"])
    rest = np.ones(size, bool)
    rest[idx.ravel()] = False
    assert (buf.view(np.int64)[rest] == CANARY).all()
    # the slab is exactly the field's points p0 .. p0 + npts: element (v, m, p) at off + (p0 + p) sp + m sm + v sv
    v, m, p = 3, 2, c["npts"] - 1
    assert idx[v, m, p] == off + (p0 + p) * sp + m * sm + v * sv
    if nlev_total is None and layout != "padded":
        assert not rest.any()


@pytest.mark.parametrize("det", [False, True])
def test_two_complementary_classes_compose_to_the_single_call(det):
    """identical var_local factors and one inflation value per point: the class of a variable cannot change its answer, so the
    composition of the per-class oracle runs is the all-variables run, bit for bit (the class's first updated variable drives
    its solve, hence the flat inflation)"""
    c = col_case("free_k20", seed=3, det=det, nij1=12, nlev=3, infl_flat=True)
    vl = VARLOC["free"]
    one = oracle(c, [(0, vl)])
    two = oracle(c, [(0b11111, vl), (0b11111100000, vl)])
    assert not np.isnan(one["anal"]).all()
    assert np.array_equal(one["anal"], two["anal"], equal_nan=True)
    assert np.array_equal(one["infl"], two["infl"])
    assert np.array_equal(one["rtps"], two["rtps"])
    assert np.array_equal(one["counts"], two["counts"])
    # (and other factors for the second class do change its variables: the composition is not trivially the same)
    other = oracle(c, [(0b11111, vl), (0b11111100000, (1.0, 1.0, 0.4, 1.0))], cfg=CFG)
    k = c["k"]
    assert np.array_equal(other["anal"][:5], one["anal"][:5], equal_nan=True)
    assert not np.array_equal(other["anal"][5:, :k], one["anal"][5:, :k])


def test_route_table_reaches_every_route():
    fam = {name: route_family(name) for name in COL_ROUTES}
    want = {"free", "free_batches", "trio16", "trio20", "wave1", "wave2", "staged_poly", "staged_poly_nv7", "staged_wg",
            "staged_block", "point", "list_levels", "lim_lds", "lim_rings", "lim_rings_gen", "lim_rings_release"}
    assert set(fam.values()) == want, sorted(want ^ set(fam.values()))
    # the list-free route at every one-wave size the issue names, the list families at the sizes that split them
    assert {COL_ROUTES[n][0] for n in fam if fam[n] == "free"} == {9, 20, 33, 50, 62}
    assert {COL_ROUTES[n][0] for n in fam if fam[n] == "staged_poly"} == {100, 144}
    assert {COL_ROUTES[n][0] for n in fam if fam[n] == "wave2"} >= {63, 100}
    # every per-axis selection reaches every family the list route and the list-free route have
    assert {fam[n] for n in AXIS_ROUTES} >= want - {"lim_rings_gen", "lim_rings_release"}
    for name, (k, nv, tables, opt, lb, has, hasnot) in COL_ROUTES.items():
        assert set(opt) <= set(DEFAULTS) and lb in ("all", "columns", "level", "slabs") and has, name
        assert (FREE in has) == fam[name].startswith("free"), name
        if not fam[name].startswith("free"):
            assert "FUSED" in hasnot or "staged:" in has or "letkf_point_kernel" in has, name
