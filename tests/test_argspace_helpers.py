"""CPU checks of tests/_argspace.py: the re-laid-out state holds das_case's elements where the strides say and the canary
everywhere else, the observation table keeps the members and poisons what the call must not read, and every route of the
table is a configuration the header allows."""
import numpy as np
import pytest

from _argspace import CANARY, ROUTES, TAIL, obs_table, place_state, route_case, state_index, state_layout


@pytest.mark.parametrize("layout", ["ref", "member", "var", "padded"])
@pytest.mark.parametrize("det", [False, True])
def test_state_layouts_place_every_element_once(layout, det):
    c = route_case("wave1", seed=1, det=det, npts=7)
    sp, sm, sv, off, size = state_layout(c, layout)
    buf = place_state(c, sp, sm, sv, off, size)
    idx = state_index(c, sp, sm, sv, off)
    assert len(np.unique(idx)) == idx.size and idx.max() < size
    assert np.array_equal(buf[idx].ravel(), c["gues"])
    rest = np.ones(size, bool)
    rest[idx.ravel()] = False
    assert (buf.view(np.int64)[rest] == CANARY).all()
    assert (layout in ("ref", "member", "var")) == (not rest.any())
    if layout == "ref":
        assert (sp, sm, sv) == (c["sp"], c["sm"], c["sv"])


@pytest.mark.parametrize("dk,det", [(0, False), (1, False), (2, True), (7, False)])
def test_obs_table_poisons_what_is_not_read(dk, det):
    c = route_case("staged_poly", seed=2, det=det, npts=5)
    k = c["k"]
    tab = obs_table(c, k + dk, det)
    ens = c["ensval"].reshape(-1, c["kld"])
    t = tab[:-TAIL].reshape(-1, k + dk)
    assert np.array_equal(t[:, :k], ens[:, :k])
    if det:
        assert np.array_equal(t[:, k], ens[:, k])
    assert np.isnan(t[:, k + int(det):]).all() and np.isnan(tab[-TAIL:]).all()


def test_route_table_is_inside_the_abi():
    for name, (k, nv, kk, has, hasnot) in ROUTES.items():
        assert k >= 2 and 1 <= nv <= 32 and kk in (None, "trans", "pa", "nopoly") and has, name
