"""The argument space of letkf_das_interp_dev and letkf_das_interp_window_dev (include/letkf_amd_interp.h,
include/letkf_amd_interp_window.h): the cases of tests/_interp.py (tile_case) at the k of the apply kernel's instantiation bounds,
at other nv and on the edge grids, and the arrays of one call -- the whole case, or the rectangle of a window -- re-laid out: other
state strides, a slab of levels of a larger field, other observation-table leading dimensions, inside buffers whose every element
the call must not write holds a fixed canary.  The statement of the answer (_interp.expected: the oracle's obs_local and
letkf_core, the blend and the rules in numpy) always gets the dense arrays of the case; only the library sees the re-laid-out
copies.  The layouts, the canary and the observation table come from tests/_argspace.py, the slab view from tests/_colspace.py.
Pure numpy and the oracle: the CPU checks in tests/test_interpspace_helpers.py import it."""
import numpy as np

import _colspace
from _argspace import canary_buffer, members  # noqa: F401  (members: the CPU checks take it from here)
from _interp import LIMITS, coarse_lists, coarse_points, expected, tile_case

NOT_WRITTEN = -(1 << 30)
CFG = dict(relax_alpha_spread=0.95, det_run=1)              # RTPS and the deterministic member: every output is written
# ... and, where the case has a pressure slot (nv >= 5), the two rules that read the state's mean and the inflation field at the
# point itself: Q_UPDATE_TOP (the mean of iv_p through sp / sm / sv, in the gather and in the apply kernel; the top level of the
# base grid lies below it, the others above) and RELAX_TO_INFLATED_PRIOR (every variable's slot, through infl_sv)
Q_UPDATE_TOP = 5.0e4


def cfg_of(c, det=True):
    cfg = dict(relax_alpha_spread=CFG["relax_alpha_spread"])
    if det:
        cfg["det_run"] = 1
    if c["nv"] >= 5:
        cfg.update(q_update_top=Q_UPDATE_TOP, relax_to_inflated_prior=1)
    return cfg


# k -> (NCT, NW) of letkf_interp_apply_kernel (letkf_interp.hip interp_apply_nct: column tiles of 16 in 1, 2, 4, 8; the largest
# runs four waves, the others eight), on either side of every switch, the smallest k the entry admits and the last below 128
K_BOUNDS = {2: (1, 8), 16: (1, 8), 17: (2, 8), 32: (2, 8), 33: (4, 8), 64: (4, 8), 65: (8, 4), 127: (8, 4)}
K_LAYOUTS = (20, 50, 100)                                   # NCT 2, NCT 4, and NCT 8 with NW 4

# name -> (nx, ny, nlev, stride_x, stride_y, dxs, dys, seed, coarse counts hold a 0 and a value above the limit)
GRIDS = {
    "one_column": (1, 1, 3, 2, 2, 5.5, 6.0, 5, False),       # ib == ia and jd == jc; among the observations (tile_case, nx == 1)
    "two_columns_stride_8": (2, 1, 3, 8, 8, 30.0, 6.0, 5, True),
    "extent_is_stride_plus_1": (9, 2, 2, 8, 8, 4.0, 6.0, 5, True),     # n - 1 an exact multiple of the stride
    "last_cell_one_wide": (10, 9, 2, 8, 4, 3.5, 3.0, 5, True),         # coarse x = {0, 8, 9}: the last cell owns its far line alone
    "full_cells": (17, 9, 2, 8, 8, 2.0, 3.0, 5, True),                 # two cells of 8 x 8 (+ far lines) points
    "one_level": (7, 5, 1, 2, 2, 5.5, 6.0, 5, True),
}


def grid_case(name, k=50, nv=11):
    nx, ny, nlev, sx, sy, dxs, dys, seed, _ = GRIDS[name]
    return tile_case(k, nv=nv, nx=nx, ny=ny, nlev=nlev, seed=seed, dxs=dxs, dys=dys), sx, sy


def apply_kernel_name(k):
    """the instantiation that serves k: that of the smallest bound of K_BOUNDS at or above it"""
    nct, nw = K_BOUNDS[min(b for b in K_BOUNDS if b >= k)] if k <= max(K_BOUNDS) else (8, 4)
    return f"letkf_interp_apply_kernel<NCT={nct},NW={nw}>"


def beta_field(c):
    """zeros and tapers on any grid: a ninth of the points (one at least) at 0, as many at 0.37, the rest 1"""
    rng = np.random.default_rng(3)
    npts = c["npts"]
    n = max(1, npts // 9)
    pick = rng.permutation(npts)
    b = np.ones(npts)
    b[pick[:n]] = 0.0
    b[pick[n:2 * n]] = 0.37
    return b


def whole_arrays(c, beta=None):
    """the arrays of a call on the whole case, in the form of the window tests' cut: every point owned, no window"""
    nv, npts = c["nv"], c["npts"]
    return dict(nx=c["nx"], ny=c["ny"], npts=npts, rig=c["rig"], rjg=c["rjg"], rlev=c["rlev"], rz=c["rz"], gues=c["gues"],
                infl=c["infl"].reshape(nv, npts), beta=beta, owned=np.ones(npts, bool), gp=np.arange(npts), window=None)


def field_view(c, a, layout, nlev_total=None, l0=0):
    """The arrays `a` of a call on case c (nx x ny columns, c's nlev levels) as levels l0 .. l0 + nlev - 1 of a field of
    nlev_total levels in one of the layouts of _argspace.state_layout.  beta, infl, status and rtps_infl_out belong to the field:
    nf points, infl_sv = nf, the call's pointers at the field's point p0.  idx: the flat index of every element (v, m, p) of the
    arrays' state, shaped (nv, nens, npts)."""
    nlev = c["nlev"]
    nij1 = a["nx"] * a["ny"]
    assert a["npts"] == nij1 * nlev
    nlev_total = nlev_total or nlev
    assert 0 <= l0 and l0 + nlev <= nlev_total
    t = dict(nv=c["nv"], nens=c["nens"], nij1=nij1, nlev=nlev, npts=a["npts"])
    sp, sm, sv, off, size, p0, idx = _colspace.field_view(t, layout, nlev_total, l0)
    return dict(sp=sp, sm=sm, sv=sv, off=off, size=size, p0=p0, idx=idx, nf=nij1 * nlev_total, infl_sv=nij1 * nlev_total)


def place_state(a, fv):
    buf = canary_buffer(fv["size"])
    buf[fv["idx"]] = a["gues"]
    return buf


def place_field(fv, values, fill):
    """a per-point (npts) or per-variable-and-point (nv, npts) array of the call inside the field's, `fill` elsewhere; `fill`
    may be an array of the field's shape"""
    values = np.asarray(values)
    p0, nf = fv["p0"], fv["nf"]
    shape = values.shape[:-1] + (nf,)
    out = np.broadcast_to(np.asarray(fill, dtype=values.dtype), shape).copy() if np.ndim(fill) == 0 else np.array(fill).reshape(shape)
    out[..., p0:p0 + values.shape[-1]] = values
    return out


def level_counts(c, sx, sy):
    """the coarse points' list lengths, (nlev, coarse columns)"""
    ix, iy, pts = coarse_points(c, sx, sy)
    lists = coarse_lists(c, pts)
    return np.array([len(lists[int(p)][0]) for p in pts]).reshape(c["nlev"], -1)


def slab_bytes(c, n):
    """the header's formula for a slab whose coarse points have the list lengths n (levels, coarse columns): 20 B per list
    entry, and per coarse point (k*k + 2k) doubles and the gathered rows (k + 4 doubles each) of the slab's longest list"""
    k = c["k"]
    return int(20 * n.sum() + n.size * 8 * (k * k + 2 * k + max(1, n.max()) * (k + 4)))


def ws_bytes_all(c, sx, sy):
    return slab_bytes(c, level_counts(c, sx, sy))


SLAB_FRACTIONS = (0.3, 0.5, 0.7, 0.85)


def slab_cuts(c, sx, sy, ws_bytes):
    """levels per slab when slabs are filled greedily to ws_bytes by the header's formula, a slab holding one level at least"""
    n = level_counts(c, sx, sy)
    cuts, l0 = [], 0
    while l0 < c["nlev"]:
        l1 = l0 + 1
        while l1 < c["nlev"] and slab_bytes(c, n[l0:l1 + 1]) <= ws_bytes:
            l1 += 1
        cuts.append(l1 - l0)
        l0 = l1
    return tuple(cuts)
