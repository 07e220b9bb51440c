"""letkf_das_interp_dev and letkf_das_interp_window_dev across the argument space their headers allow (include/letkf_amd_interp.h,
include/letkf_amd_interp_window.h), through the C ABI.  The axes:
  1. state layouts (ref, member, var, padded of _argspace.state_layout) at k = 20, 50, 100 -- NCT 2, NCT 4 and NCT 8 / NW 4 of
     letkf_interp_apply_kernel -- and anal == gues in the padded layout;                                              (=)
  2. levels 1..3 of a 5-level field (ref, padded): beta, infl, status, rtps_infl_out at the slab's first point, infl_sv the field's; (=)
  3. the observation table's leading dimension: kld = k without det_run, k + 1, k + 5, NaN padding and a NaN tail;    (=)
  4. k in {2, 16, 17, 32, 33, 64, 65, 127}: either side of every instantiation switch, named by last_path;
  5. nv in {1, 2, 15, 32} (nv = 15 as two scattered classes in two calls), nv = 33 refused;
  6. the edge grids of _interpspace.GRIDS: one column, two columns at stride 8, n - 1 = stride, a last cell one column wide, full
     8 x 8 cells (also at k = 100: 11 chunks of 64 rows), one level;
  7. uneven slab cuts of five levels: ws_bytes at 0.3, 0.5, 0.7, 0.85 of the header's formula (the cuts are replayed on the CPU
     in tests/test_interpspace_helpers.py: three of them differ from each other, from one slab and from one level per slab),
     against one slab and ws_bytes = 1;                                                                              (=)
  8. status, rtps_infl_out, nobs_coarse, beta NULL, each alone and all together (beta NULL is beta = 1 everywhere: compared
     with the call that passes an array of ones);                                                                     (=)
  9. axes 1, 2, 3, 8 through the window entry: the owned rectangle [1, 6) x [1, 4) of the base grid, a halo line on all four sides,
     NaN in every halo input off the coarse columns (the cut of tests/test_gpu_interp_window.py);
 10. refusals (NULL gues / anal / infl / coordinates / tables, kld too small, nv = 33): LETKF_E_INVALID, nothing written.
Unless an axis says otherwise: RTPS 0.95, det_run, beta with zeros and tapers, stride (2, 2) on the 7 x 5 x 3 grid, k = 50, and
-- wherever nv >= 5, so that the mean of iv_p is read through sp / sm / sv and every variable's inflation slot through infl_sv, in
the gather and in the apply kernel -- q_update_top = 5e4 Pa (it cuts through the levels) and relax_to_inflated_prior; axis 2 also
runs a class of three moisture variables, whose solves take the slot of variable 5, or 1 below q_update_top.
Every element the call must not write is pre-filled -- anal: the CANARY bit pattern (gues' own bits where anal == gues);
rtps_infl_out: NaN; status and nobs_coarse: NOT_WRITTEN; gues, infl and beta: their own values -- and compared bit for bit
afterwards: padding and lead-in, the mean slot, the deterministic slot without det_run, variables outside var_mask, the field's
levels outside the slab, every halo point of a window.  The written elements are checked twice: against the numpy statement
(_interp.expected on the dense case; members and the deterministic member within 1e-10 max(|mean|, |x'|) per variable,
rtps_infl_out within 1e-10 relative, status and nobs_coarse exact -- the tolerances of tests/test_gpu_interp.py), and, on the
axes marked (=), bit for bit against the same case called in the dense reference layout with every output: nothing the route
computes depends on a stride, a leading dimension, a pointer offset, a NULL output or a slab cut."""
import ctypes as C

import numpy as np
import pytest
import torch

import _interp as I
import _interpspace as S
from _argspace import canary_buffer, mask_vars, members, obs_table

pytestmark = pytest.mark.gpu

NAN = float("nan")
NOT_WRITTEN = S.NOT_WRITTEN
OUTS = ("status", "rtps", "nobs")
NOBS_TAIL = 8                                # NOT_WRITTEN elements behind nobs_coarse
E_INVALID = -1
OWN = (1, 6, 1, 4)                           # the window axis' owned rectangle [p0, p1) x [q0, q1) of the 7 x 5 grid
bits = lambda z: np.ascontiguousarray(z).view(np.int64)


def beta_of(c, kind):
    return S.beta_field(c) if kind == "field" else np.ones(c["npts"]) if kind == "ones" else None


def window_arrays(c, sx, sy, beta):
    import test_gpu_interp_window as W
    a = W.cut(c, sx, sy, OWN, beta=beta)
    assert a["window"] == (7, 5, 0, 0, 1, 1, 5, 3) and a["lx"] == [0, 2, 4, 6] and a["ly"] == [0, 2, 4]
    assert a["dead"].any() and not a["owned"][~a["dead"]].all()          # NaN columns, and coarse columns, in the halo
    return a


class Run:
    """the device buffers of one call: the arrays of the call (the whole case, or the window's cut) as levels l0 .. of a field of
    nlev_total levels in a layout, the per-point and per-(variable, point) fields of that field, the observation table with its
    leading dimension -- everything pre-filled"""

    def __init__(self, c, sx=2, sy=2, layout="ref", slab=None, outs=OUTS, alias=False, kld=None, det=True, beta="field",
                 window=False):
        from _gpu import dev
        from _search import device_struct
        self.c, self.sx, self.sy, self.det, self.outs_asked = c, sx, sy, det, outs
        self.beta_kind = beta
        bg = beta_of(c, beta)
        self.a = a = window_arrays(c, sx, sy, bg) if window else S.whole_arrays(c, bg)
        nv, nlev = c["nv"], c["nlev"]
        nlev_total, l0 = slab or (nlev, 0)
        self.fv = fv = S.field_view(c, a, layout, nlev_total, l0)
        nf = fv["nf"]
        self.gues_before = S.place_state(a, fv)
        self.gues = dev(self.gues_before)
        self.anal = self.gues if alias else dev(canary_buffer(fv["size"]))
        self.anal_before = self.gues_before if alias else canary_buffer(fv["size"])
        self.infl_before = S.place_field(fv, a["infl"], 1.0 + 0.001 * np.arange(nv * nf)).reshape(-1)
        self.infl = dev(self.infl_before)
        self.beta_before = None if a["beta"] is None else S.place_field(fv, a["beta"], NAN)
        self.beta = None if a["beta"] is None else dev(self.beta_before)
        if window:
            self.ncoarse = len(a["lx"]) * len(a["ly"]) * nlev
        else:
            self.ncoarse = len(I.coarse_axis(c["nx"], sx)) * len(I.coarse_axis(c["ny"], sy)) * nlev
        i32 = lambda n: torch.full((n,), NOT_WRITTEN, dtype=torch.int32, device="cuda")
        make = {"status": lambda: i32(nf), "nobs": lambda: i32(self.ncoarse + NOBS_TAIL),
                "rtps": lambda: torch.full((nf * nv,), NAN, dtype=torch.float64, device="cuda")}
        self.outs = {o: make[o]() for o in outs}
        self.kld = kld or c["k"] + 1
        self.table = dev(obs_table(c, self.kld, det and self.kld > c["k"]))     # (kld = k has no column for det_run: refused)
        self.dep = dev(c["dep"])
        self.rig, self.rjg, self.rlev, self.rz = dev(a["rig"]), dev(a["rjg"]), dev(a["rlev"]), dev(a["rz"])
        self.t, self.keep = device_struct(c["tc"], "cuda")
        self.path = None

    def view(self, t, scale=1):
        return None if t is None else t[self.fv["p0"] * scale:]

    def result(self):
        """the call's arrays back in the dense shapes: anal (nv, nens, npts), rtps (nv, npts), status (npts), nobs (ncoarse)"""
        fv, nv, npts = self.fv, self.c["nv"], self.a["npts"]
        p0, nf = fv["p0"], fv["nf"]
        out = dict(anal=self.anal.cpu().numpy()[fv["idx"]])
        if "rtps" in self.outs:
            out["rtps"] = self.outs["rtps"].cpu().numpy().reshape(nv, nf)[:, p0:p0 + npts]
        if "status" in self.outs:
            out["status"] = self.outs["status"].cpu().numpy()[p0:p0 + npts]
        if "nobs" in self.outs:
            out["nobs"] = self.outs["nobs"].cpu().numpy()[:self.ncoarse]
        return out


def ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def call(r, mask=0, ws_bytes=0, **raw):
    """the entry through the C ABI on the buffers of r: pointers at the slab's first point, the field's strides and infl_sv; the
    window entry where r has a window.  raw: DasArgs fields, coordinate pointers or tables=None to override.  (rc, last error)"""
    from _gpu import ctx, pkg
    c, a, fv = r.c, r.a, r.fv
    k, nv = c["k"], c["nv"]
    cx = ctx()
    g = pkg.DasArgs()
    g.k, g.nv, g.det_run = k, nv, int(r.det)
    g.iv_p, g.iv_q_first, g.iv_q_last = 4, 5, min(10, nv - 1)
    cfg = S.cfg_of(c, r.det)
    g.relax_alpha_spread, g.q_update_top = cfg["relax_alpha_spread"], cfg.get("q_update_top", 0.0)
    g.relax_to_inflated_prior = cfg.get("relax_to_inflated_prior", 0)
    g.npts = a["npts"]
    g.ensval, g.kld, g.dep = ptr(r.table), r.kld, ptr(r.dep)
    g.beta, g.infl = ptr(r.view(r.beta)), ptr(r.view(r.infl))
    o = fv["off"] + fv["p0"] * fv["sp"]
    g.gues, g.anal, g.sp, g.sm, g.sv = ptr(r.gues[o:]), ptr(r.anal[o:]), fv["sp"], fv["sm"], fv["sv"]
    g.status, g.rtps_infl_out = ptr(r.view(r.outs.get("status"))), ptr(r.view(r.outs.get("rtps")))
    g.var_mask, g.infl_sv = mask, fv["infl_sv"]
    ia = pkg.InterpArgs()
    ia.nx, ia.ny, ia.nlev, ia.stride_x, ia.stride_y, ia.ws_bytes = a["nx"], a["ny"], c["nlev"], r.sx, r.sy, int(ws_bytes)
    coords = dict(rig=r.rig, rjg=r.rjg, rlev=r.rlev, rz=r.rz)
    tables = C.byref(r.t)
    for f, v in raw.items():
        if f in coords:
            coords[f] = v
        elif f == "tables":
            tables = v
        else:
            setattr(g, f, v)
    ia.rig, ia.rjg, ia.rlev, ia.rz = (ptr(coords[n]) for n in ("rig", "rjg", "rlev", "rz"))
    ia.nobs_coarse = ptr(r.outs.get("nobs"))
    if a["window"] is None:
        rc = cx._l.letkf_das_interp_dev(cx._c, C.byref(g), tables, C.byref(ia))
    else:
        w = pkg.InterpWindow(*[int(v) for v in a["window"]])
        rc = cx._l.letkf_das_interp_window_dev(cx._c, C.byref(g), tables, C.byref(ia), C.byref(w))
    torch.cuda.synchronize()
    r.path = cx.last_path()
    return rc, cx._l.letkf_amd_last_error().decode()


_statements = {}


def statement(c, sx, sy, det, beta, masks):
    """_interp.expected on the dense case, one run per class, each class keeping its own variables"""
    key = (id(c), sx, sy, det, beta, tuple(masks))
    if key not in _statements:
        cfg = S.cfg_of(c, det)
        exp = None
        for mask in masks:
            e = S.expected(c, cfg, sx, sy, beta=beta_of(c, beta), mask=mask)
            if exp is None:
                exp = e
            else:
                assert np.array_equal(e["ncoarse"], exp["ncoarse"])
                for v in mask_vars(c["nv"], mask):
                    exp["anal"][v], exp["rtps"][v] = e["anal"][v], e["rtps"][v]
        _statements[key] = exp
    return _statements[key]


def coarse_block(r, n):
    """the call's part of the counts of the whole case's coarse lattice (all of it without a window)"""
    c, a = r.c, r.a
    if a["window"] is None:
        return n
    Lx, Ly = list(I.coarse_axis(c["nx"], r.sx)), list(I.coarse_axis(c["ny"], r.sy))
    full = n.reshape(c["nlev"], len(Ly), len(Lx))
    return full[:, [Ly.index(l) for l in a["ly"]]][:, :, [Lx.index(l) for l in a["lx"]]].ravel()


def check(r, masks=(0,)):
    """the classes' variables at the call's owned points against the statement; every other element of every buffer, and every
    input, bit for bit its pre-fill"""
    c, a, fv = r.c, r.a, r.fv
    k, nv, nf, p0, npts = c["k"], c["nv"], fv["nf"], fv["p0"], a["npts"]
    exp = statement(c, r.sx, r.sy, r.det, r.beta_kind, masks)
    assert S.apply_kernel_name(k) in r.path and r.path.startswith("interp:"), r.path
    o, g = a["owned"], a["gp"][a["owned"]]
    vs = sorted(set(v for m in masks for v in mask_vars(nv, m)))
    mem = members(k, r.det)
    x = c["gues"]
    got = r.anal.cpu().numpy()
    written = np.zeros(got.size, bool)
    for v in vs:
        scale = max(np.abs(x[v, k]).max(), np.abs(x[v, :k]).max())
        sel = fv["idx"][v][mem][:, o]
        e = exp["anal"][v][mem][:, g]
        assert np.isfinite(e).all() and np.isfinite(got[sel]).all(), v
        err = np.abs(got[sel] - e).max()
        print(f"v={v} err/scale={err / scale:.3e}")
        assert err <= 1e-10 * scale, (v, err / scale)
        written[sel.ravel()] = True
    bad = np.flatnonzero((bits(got) != bits(r.anal_before)) & ~written)
    assert bad.size == 0, ("anal elements the call must not write were written", bad[:8], bad.size)
    if r.anal is not r.gues:
        assert np.array_equal(bits(r.gues.cpu().numpy()), bits(r.gues_before))
    assert np.array_equal(bits(r.infl.cpu().numpy()), bits(r.infl_before))
    if r.beta is not None:
        assert np.array_equal(bits(r.beta.cpu().numpy()), bits(r.beta_before))
    pts = np.zeros(nf, bool)
    pts[p0:p0 + npts] = o
    if "rtps" in r.outs:
        gr = r.outs["rtps"].cpu().numpy().reshape(nv, nf)
        inside = np.zeros((nv, nf), bool)
        inside[np.ix_(vs, np.flatnonzero(pts))] = True
        assert np.isnan(gr[~inside]).all()
        rerr = np.abs(gr[vs][:, pts] / exp["rtps"][vs][:, g] - 1.0).max()
        print(f"rtps {rerr:.3e}")
        assert rerr <= 1e-10, rerr
    if "status" in r.outs:
        st = r.outs["status"].cpu().numpy()
        assert (st[~pts] == NOT_WRITTEN).all() and (st[pts] == 0).all(), st
    if "nobs" in r.outs:
        nb = r.outs["nobs"].cpu().numpy()
        assert (nb[r.ncoarse:] == NOT_WRITTEN).all()
        assert np.array_equal(nb[:r.ncoarse], coarse_block(r, exp["ncoarse"])), (nb, exp["ncoarse"])


def run(c, masks=(0,), ws_bytes=0, **kw):
    """one call (one per class) on c, checked; returns the Run"""
    r = Run(c, **kw)
    for mask in masks:
        rc, err = call(r, mask=mask, ws_bytes=ws_bytes)
        assert rc == 0, err
    check(r, masks)
    return r


_dense = {}


def dense(c, sx=2, sy=2, det=True, beta="field", masks=(0,)):
    """the case in the dense reference layout (sp = 1, sm = npts, sv = npts * nens, kld = k + 1, every output, one slab) through
    letkf_das_interp_dev, checked, once per setting: what the other calls must reproduce bit for bit"""
    key = (id(c), sx, sy, det, beta, tuple(masks))
    if key not in _dense:
        r = run(c, masks=masks, sx=sx, sy=sy, det=det, beta=beta)
        r.frozen = r.result()
        _dense[key] = r
    return _dense[key]


def same_bits(r, ref, fields=("anal", "rtps", "status", "nobs")):
    """the written elements of r (its owned points) hold the bits of the whole-case call ref at the same points"""
    c, a = r.c, r.a
    x, y = r.result(), ref.frozen
    o, g = a["owned"], a["gp"][a["owned"]]
    mem = members(c["k"], r.det)
    assert r.det == ref.det and np.array_equal(ref.a["gp"], np.arange(c["npts"]))
    assert np.array_equal(bits(x["anal"][:, mem][:, :, o]), bits(y["anal"][:, mem][:, :, g]))
    if "rtps" in x and "rtps" in fields:
        assert np.array_equal(bits(x["rtps"][:, o]), bits(y["rtps"][:, g]))
    if "status" in x and "status" in fields:
        assert np.array_equal(x["status"][o], y["status"][g])
    if "nobs" in x and "nobs" in fields:
        assert np.array_equal(x["nobs"], coarse_block(r, y["nobs"]))


def refused(r, why, **raw):
    """rc -1 for the reason under test (a fragment of letkf_amd_last_error) and every buffer of r still its pre-fill"""
    rc, err = call(r, **raw)
    assert rc == E_INVALID and why in err, (rc, err)
    assert np.array_equal(bits(r.anal.cpu().numpy()), bits(r.anal_before))
    assert np.array_equal(bits(r.gues.cpu().numpy()), bits(r.gues_before))
    assert np.array_equal(bits(r.infl.cpu().numpy()), bits(r.infl_before))
    assert np.isnan(r.outs["rtps"].cpu().numpy()).all()
    for o in ("status", "nobs"):
        assert (r.outs[o].cpu().numpy() == NOT_WRITTEN).all(), o


ENTRY = pytest.mark.parametrize("window", [False, True], ids=["whole", "window"])


# ---- 1 (and 9): state layouts
@pytest.mark.parametrize("layout,window", [("member", False), ("var", False), ("padded", False), ("ref", True), ("member", True),
                                           ("var", True), ("padded", True)],
                         ids=["member", "var", "padded", "window-ref", "window-member", "window-var", "window-padded"])
@pytest.mark.parametrize("k", S.K_LAYOUTS)
def test_state_layouts(k, layout, window):
    c = I.tile_case(k)
    same_bits(run(c, layout=layout, window=window), dense(c))


@ENTRY
def test_in_place_in_the_padded_layout(window):
    """anal == gues: the mean slot, the padding and the lead-in (and the window's halo) keep gues' bits"""
    c = I.tile_case(50)
    r = run(c, layout="padded", alias=True, window=window)
    k = c["k"]
    assert np.array_equal(r.result()["anal"][:, k], r.a["gues"][:, k], equal_nan=True)
    same_bits(r, dense(c))


# ---- 2 (and 9): a slab of levels of a larger field
MOIST = sum(1 << v for v in (5, 7, 10))


@ENTRY
@pytest.mark.parametrize("mask", [0, MOIST], ids=["all", "moist"])
@pytest.mark.parametrize("layout", ["ref", "padded"])
def test_levels_of_a_larger_field(layout, mask, window):
    """levels 1..3 of five: the other levels of gues, anal, infl, beta, status and rtps_infl_out keep every bit.  With the class of
    three moisture variables the rho of a coarse solve is the field's slot of variable 5 -- infl[pt + infl_sv * 5] -- where the
    point's mean pressure (read through the field's strides) is above Q_UPDATE_TOP, and 1 where it is below."""
    c = I.tile_case(50)
    r = run(c, masks=(mask,), layout=layout, slab=(5, 1), window=window)
    assert r.fv["p0"] == r.a["nx"] * r.a["ny"] and r.fv["infl_sv"] == 5 * r.a["nx"] * r.a["ny"]
    same_bits(r, dense(c, masks=(mask,)))


# ---- 3 (and 9): the observation table's leading dimension
@ENTRY
@pytest.mark.parametrize("dk,det", [(0, False), (1, False), (1, True), (5, False), (5, True)],
                         ids=["kld_eq_k", "kld_k_plus_1", "kld_k_plus_1_det", "kld_k_plus_5", "kld_k_plus_5_det"])
def test_obs_table_leading_dimension(dk, det, window):
    c = I.tile_case(50)
    ref = dense(c, det=det)                      # kld = k + 1; column k is NaN without det_run
    same_bits(run(c, kld=c["k"] + dk, det=det, window=window), ref)


@ENTRY
def test_kld_eq_k_with_det_run_is_refused(window):
    c = I.tile_case(50)
    refused(Run(c, kld=c["k"], det=True, window=window), "kld too small for k")


# ---- 4: k at the instantiation bounds
@pytest.mark.parametrize("k", sorted(S.K_BOUNDS))
def test_k_at_the_instantiation_bounds(k):
    r = dense(I.tile_case(k))
    assert "letkf_interp_apply_kernel<NCT=%d,NW=%d>" % S.K_BOUNDS[k] in r.path, r.path


# ---- 5: nv
@pytest.mark.parametrize("nv,k", [(1, 20), (2, 20), (32, 20), (1, 100)])
def test_number_of_variables(nv, k):
    dense(I.tile_case(k, nv=nv))


CLASS_A = sum(1 << v for v in (0, 3, 7, 12))
CLASS_B = sum(1 << v for v in (1, 4, 8, 13, 14))


def test_two_scattered_classes_of_fifteen_variables():
    """das_letkf_amd's pattern: one call per class on the same buffers; each class keeps its own variables, the six variables of
    neither class stay canary"""
    c = I.tile_case(20, nv=15)
    assert CLASS_A & CLASS_B == 0 and bin(CLASS_A | CLASS_B).count("1") == 9
    r = run(c, masks=(CLASS_A, CLASS_B))
    # class A holds variable 0, so its solves take the rho of the all-variables call: its variables are that call's bit for bit
    vs = mask_vars(15, CLASS_A)
    mem = members(20, True)
    assert vs[0] == 0
    assert np.array_equal(bits(r.result()["anal"][vs][:, mem]), bits(dense(c).frozen["anal"][vs][:, mem]))


def test_thirty_three_variables_are_refused():
    c = I.tile_case(20, nv=32)
    refused(Run(c), "nv must be <= 32", nv=33)


# ---- 6: grid edges
@pytest.mark.parametrize("name,k", [(n, 50) for n in S.GRIDS] + [("full_cells", 100)])
def test_grid_edges(name, k):
    c, sx, sy = S.grid_case(name, k=k)
    r = dense(c, sx, sy)
    n = r.frozen["nobs"]
    if S.GRIDS[name][8]:
        assert (n == 0).any() and (n > S.LIMITS[0]).any()


# ---- 7: slab cuts
def test_uneven_slab_cuts_change_no_bit():
    c = I.tile_case(50, nlev=5)
    one = dense(c)
    full = S.ws_bytes_all(c, 2, 2)
    for ws in [1] + [int(f * full) for f in S.SLAB_FRACTIONS]:
        same_bits(run(c, ws_bytes=ws), one)


# ---- 8 (and 9): optional pointers
@ENTRY
@pytest.mark.parametrize("null", ["status", "rtps", "nobs", "beta", "all"])
def test_null_outputs_and_null_beta(null, window):
    c = I.tile_case(50)
    beta = "null" if null in ("beta", "all") else "field"
    outs = tuple(o for o in OUTS if null not in (o, "all"))
    ref = dense(c, beta="ones" if beta == "null" else "field")
    r = run(c, outs=outs, beta=beta, window=window)
    assert (r.beta is None) == (beta == "null") and len(r.outs) == (0 if null == "all" else 3 if null == "beta" else 2)
    same_bits(r, ref)


# ---- 10: refusals
@ENTRY
@pytest.mark.parametrize("what", ["gues", "anal", "infl", "rig", "rjg", "rlev", "rz", "tables"])
def test_null_arguments_are_refused_and_nothing_is_written(what, window):
    c = I.tile_case(50)
    why = "a required device pointer is NULL" if what in ("gues", "anal", "infl") else \
        "args / tables / interp is NULL" if what == "tables" else "a point coordinate array is NULL"
    refused(Run(c, layout="padded", window=window), why, **{what: None})

