"""letkf_obsmake_slot_dev and letkf_obsmake_noise_dev (include/letkf_amd_obsmake.h) against the numpy statement of
tests/_obsmake.py on the fixtures of tests/_obsope.py (about 300 file rows; nlev = 8, and one nlev = 70 configuration).

Slot entry: a processed row whose qc is 0 is within the tolerance tests/test_gpu_obsope.py derives for its kind (tests/_obsope.py
operator() computes it per row); undef and every untouched row are compared bit for bit.  The fixtures hold reflectivity and
Doppler-velocity rows with qc 11, which the plain operator passes with qc 0; a report type with use_obs = 0 and radar rows above
radar_zmax, all computed here; dif exactly on slot_lb (out) and on slot_ub (in); own of all three kinds.

Noise entry: err bit for bit; dat within |err| * 16 ulp(|e|) plus one rounding, ulp(|dat'|), of the sum -- e the statement's
deviate, 16 ulp tests/test_gpu_randn.py's bound on the device's.  (The product's own rounding, half an ulp of |err e| <=
|err| ulp(|e|) on each side, is inside the first term as long as the deviate is within 14 ulp.)"""
import ctypes as C

import numpy as np
import pytest
import torch

import _obsmake as M
import _obsope as O

pytestmark = pytest.mark.gpu

CONFIGS = [(8, dict(method_ref_calc=m, stggrd=s)) for m in (1, 2, 3) for s in (0, 1)] + [(70, dict(method_ref_calc=2, stggrd=1))]
_CASES = {}


def case_of(nlev):
    if nlev not in _CASES:
        _CASES[nlev] = O.make_case(nlev)
    return _CASES[nlev]


@pytest.fixture(scope="module")
def env():
    from _gpu import ctx, pkg
    return pkg, ctx(), torch.device("cuda:0")


def bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def check_slot(got, want, tol):
    exact = tol == 0.0
    assert np.array_equal(bits(got[exact]), bits(want[exact])), np.nonzero(bits(got) != bits(want))[0][:10]
    err = np.abs(got[~exact] - want[~exact])
    assert (err <= tol[~exact]).all(), (err / tol[~exact]).max()
    return float((err / tol[~exact]).max()) if err.size else 0.0


@pytest.mark.parametrize("nlev,kw", CONFIGS, ids=lambda v: "-".join(f"{k[0]}{x}" for k, x in v.items()) if isinstance(v, dict) else str(v))
@pytest.mark.parametrize("outside_undef", [0, 1])
def test_slot_matches_the_statement(env, nlev, kw, outside_undef):
    pkg, ctx, dev = env
    case, cfg = case_of(nlev), M.cfg_of(**kw)
    st = M.operator_rows(case, cfg, 0)
    dif, own = M.slot_inputs(case, 3)
    dat0 = np.random.default_rng(5).uniform(1.0, 2.0, size=case["nrow"])
    want, tol, counts = M.slot_statement(case, cfg, 0, dif, own, M.LB, M.UB, outside_undef, dat0)
    # the fixtures hold what the docstring lists, inside the slot and processed
    proc = (dif > M.LB) & (dif <= M.UB) & (own == 1)
    typ, lev = case["files"]["typ"], case["files"]["lev"]
    for elms in ((O.ID_REF, O.ID_REF_ZERO), (O.ID_VR,)):
        assert (proc & (st["qc"] == O.QC_REF_LOW) & np.isin(st["elm"], elms)).any()
    assert (proc & (typ == 3) & (st["qc"] == 0)).any() and cfg["use_obs"][2] == 0
    assert (proc & st["radar"] & (lev > cfg["radar_zmax"]) & (st["qc"] == 0)).any()
    assert ((dif == M.LB) & (own == 1)).any() and ((dif == M.UB) & (own == 1)).any()
    assert all(((own == v) & (dif > M.LB) & (dif <= M.UB)).any() for v in (1, 0, -1))
    assert set(np.unique(st["qc"][proc])) >= {0, 10, 11, 20, 21, 90, 98}
    dc = M.device_case(pkg, case, cfg, dev, 0, dat0)
    got, gcounts = M.run_slot(pkg, ctx, dc, dif, own, M.LB, M.UB, outside_undef)
    worst = check_slot(got, want, tol)
    print(f"nlev {nlev} {kw} outside_undef {outside_undef}: worst error / tolerance {worst:.3g}, counts {gcounts}")
    assert np.array_equal(gcounts, counts) and counts[1] > 100
    assert ((want == M.UNDEF) & (dif > M.LB) & (dif <= M.UB) & (own == -1)).any() == bool(outside_undef)
    # the plain operator gives these rows qc 0: the mode, not the fixture, makes them undef
    dc_plain = O.DeviceCase(pkg, case, cfg, dev, members=(0, 1))
    _, qc_plain = dc_plain.run(ctx)
    low = np.zeros(case["nrow"], dtype=bool)
    low[M.file_row_of(case)] = qc_plain == 0
    assert (low & proc & (st["qc"] == O.QC_REF_LOW) & (got == M.UNDEF)).any()


def test_two_slots_with_different_fields_and_the_operator_around_them(env):
    """slot 1 on member 0, slot 2 on member 1: the second call leaves the first slot's rows alone.  letkf_obsope_dev before and
    after the obsmake calls: bitwise equal, so the mode does not leak."""
    pkg, ctx, dev = env
    case, cfg = case_of(8), M.cfg_of()
    dif, own = M.slot_inputs(case, 3)
    dif = np.where(np.random.default_rng(8).uniform(size=len(dif)) < 0.5, dif, dif + 600.0)      # half of the rows move to slot 2
    plain = O.DeviceCase(pkg, case, cfg, dev)
    val_a, qc_a = plain.run(ctx, canary=-3.0)
    dat = np.zeros(case["nrow"])
    for m, (lb, ub) in enumerate(((M.LB, M.UB), (M.UB, M.UB + 600.0))):
        want, tol, counts = M.slot_statement(case, cfg, m, dif, own, lb, ub, 1, dat)
        got, gcounts = M.run_slot(pkg, ctx, M.device_case(pkg, case, cfg, dev, m, dat), dif, own, lb, ub, 1)
        check_slot(got, want, tol)
        assert np.array_equal(gcounts, counts) and counts[1] > 40
        if m == 1:
            first = (dif > M.LB) & (dif <= M.UB)
            assert np.array_equal(bits(got[first]), bits(dat[first]))
        dat = got
    val_b, qc_b = plain.run(ctx, canary=-3.0)
    assert np.array_equal(bits(val_a), bits(val_b)) and np.array_equal(qc_a, qc_b)
    st = O.statement(case, cfg)                                       # (the plain operator still folds 11 and tests use_obs, radar_zmax)
    assert np.array_equal(qc_a, st["qc"]) and (st["qc"] == O.QC_RADAR_VHI).any() and not (st["qc"] == O.QC_REF_LOW).any()


def noise_files(case):
    """three files: conventional, radar, and an empty one; 2 * k + 1 rows; undef in dat, undef in err, elements outside the list"""
    f = case["files"]
    off = case["off"]
    keep = np.concatenate([np.arange(off[0], off[1]), np.arange(off[1], off[2])])
    if len(keep) % 2 == 0:
        keep = keep[:-1]
    elm = f["elm"][keep].copy()
    rng = np.random.default_rng(12)
    dat = rng.uniform(-30.0, 30.0, size=len(keep))
    err = rng.uniform(0.5, 2.0, size=len(keep))
    dat[rng.permutation(len(keep))[:25]] = M.UNDEF
    other = ~np.isin(elm, list(M.ERR_OF))
    assert other.sum() >= 2
    elm[rng.permutation(len(keep))[:6]] = O.ID_RAIN                  # more elements outside the list ...
    other = ~np.isin(elm, list(M.ERR_OF))
    err[np.nonzero(other)[0][::2]] = M.UNDEF                         # ... half of them with err = undef: never perturbed
    n0 = int((keep < off[1]).sum())
    return elm, dat, err, np.array([0, n0, len(keep), len(keep)], dtype=np.int64)


def run_noise(pkg, ctx, dev, elm, dat, err, off, seed):
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    d = dict(elm=t(elm), dat=t(dat), err=t(err))
    f = pkg.ObsFileRows()
    f.nfile, f.off = len(off) - 1, off.ctypes.data_as(C.c_void_p)
    for n, v in d.items():
        setattr(f, n, C.c_void_p(v.data_ptr()))
    r = pkg.Rand(seed)
    r.set_chunk(64)
    ctx.obsmake_noise(M.err_struct(pkg), f, r)
    torch.cuda.synchronize()
    return d["dat"].cpu().numpy(), d["err"].cpu().numpy(), r


def test_noise_matches_the_statement(env):
    pkg, ctx, dev = env
    elm, dat, err, off = noise_files(case_of(8))
    n = len(elm)
    assert n % 2 == 1 and off[3] == off[2] and off[1] > 0 and off[2] > off[1]
    want, werr, e, hit = M.noise_statement(elm, dat, err, 77)
    other = ~np.isin(elm, list(M.ERR_OF))
    assert (dat == M.UNDEF).any() and (other & (err == M.UNDEF)).any() and (other & (err != M.UNDEF) & hit).any()
    got, gerr, r = run_noise(pkg, ctx, dev, elm, dat, err, off, 77)
    assert np.array_equal(bits(gerr), bits(werr))
    assert np.array_equal(bits(got[~hit]), bits(dat[~hit]))
    tol = np.abs(werr) * 16.0 * np.spacing(np.abs(e)) + np.spacing(np.abs(want))
    d = np.abs(got - want)[hit]
    print(f"noise: {int(hit.sum())} of {n} rows perturbed, worst error / tolerance {(d / tol[hit]).max():.3g}")
    assert (d <= tol[hit]).all() and hit.sum() > 150
    # a row that is skipped still owns its deviate: the stream went on by n + 1 uniforms
    import _sfmt as S
    g = S.Sfmt(77, 0)
    g.res53(n + 1)
    assert np.array_equal(bits(r.res53(3)), bits(g.res53(3)))
    again, _, _ = run_noise(pkg, ctx, dev, elm, dat, err, off, 77)
    assert np.array_equal(bits(again), bits(got))
    other_seed, _, _ = run_noise(pkg, ctx, dev, elm, dat, err, off, 78)
    assert not np.array_equal(other_seed[hit], got[hit]) and np.array_equal(bits(other_seed[~hit]), bits(got[~hit]))
