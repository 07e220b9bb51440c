"""letkf_obsmake_slot_dev and letkf_obsmake_noise_dev (include/letkf_amd_obsmake.h) across their argument space: every
refusal the header lists leaves dat, err, counts and the random stream as they were; fields in another storage order; own = NULL;
counts = NULL; a slot without rows; files without rows."""
import ctypes as C

import numpy as np
import pytest
import torch

import _obsmake as M
import _obsope as O
import _sfmt as S

pytestmark = pytest.mark.gpu
_CASE = []


def the_case():
    if not _CASE:
        _CASE.append(O.make_case(8))
    return _CASE[0]


@pytest.fixture(scope="module")
def env():
    from _gpu import ctx, pkg
    return pkg, ctx(), torch.device("cuda:0")


def bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def slot_struct(pkg, dev, dif, own, lb=M.LB, ub=M.UB, outside_undef=1):
    s = pkg.ObsmakeSlot()
    keep = [torch.from_numpy(np.ascontiguousarray(dif)).to(dev), torch.from_numpy(np.ascontiguousarray(own)).to(dev)]
    s.slot_lb, s.slot_ub, s.dif, s.own, s.outside_undef = lb, ub, keep[0].data_ptr(), keep[1].data_ptr(), outside_undef
    return s, keep


SLOT_REFUSALS = ["slot-null", "dif-null", "dat-null", "nmem-2", "lb-nan", "ub-inf", "lb-eq-ub", "lb-gt-ub", "params-null",
                 "files-null", "fields-null", "method-4", "khalo-0", "stride-0", "nfile-17", "typ-0-device", "typ-25-device"]


@pytest.mark.parametrize("what", SLOT_REFUSALS)
def test_every_slot_refusal_writes_nothing(env, what):
    pkg, ctx, dev = env
    case, cfg = the_case(), M.cfg_of()
    dif, own = M.slot_inputs(case, 3)
    dat0 = np.random.default_rng(5).uniform(1.0, 2.0, size=case["nrow"])
    c = case
    if what.startswith("typ-"):                        # a processed row with a report type outside 1..nobtype: the device's check
        proc = np.nonzero((dif > M.LB) & (dif <= M.UB) & (own == 1))[0]
        typ = case["files"]["typ"].copy()
        typ[proc[len(proc) // 2]] = 0 if what == "typ-0-device" else O.NOBTYPE + 1
        c = dict(case, files=dict(case["files"], typ=typ))
    dc = M.device_case(pkg, c, cfg, dev, 0, dat0)
    s, keep = slot_struct(pkg, dev, dif, own)
    counts = torch.full((2,), -7, dtype=torch.int64, device=dev)
    args = [C.byref(s), C.byref(dc.params), C.byref(dc.files), C.byref(dc.fields)]
    if what == "slot-null":
        args[0] = None
    elif what == "dif-null":
        s.dif = None
    elif what == "dat-null":
        dc.files.dat = None
    elif what == "nmem-2":
        dc.fields.nmem = 2
    elif what == "lb-nan":
        s.slot_lb = float("nan")
    elif what == "ub-inf":
        s.slot_ub = float("inf")
    elif what == "lb-eq-ub":
        s.slot_lb = s.slot_ub
    elif what == "lb-gt-ub":
        s.slot_lb, s.slot_ub = M.UB, M.LB
    elif what == "params-null":
        args[1] = None
    elif what == "files-null":
        args[2] = None
    elif what == "fields-null":
        args[3] = None
    elif what == "method-4":
        dc.params.method_ref_calc = 4
    elif what == "khalo-0":
        dc.fields.khalo = 0
    elif what == "stride-0":
        dc.fields.s3i = 0
    elif what == "nfile-17":
        dc.files.nfile = 17
    rc = pkg.osse_lib().letkf_obsmake_slot_dev(ctx._c, *args, counts.data_ptr())
    torch.cuda.synchronize()
    assert rc == -1 and len(pkg.lib().letkf_amd_last_error()) > 0, (what, rc)      # LETKF_E_INVALID
    assert np.array_equal(bits(dc.d["dat"].cpu().numpy()), bits(dat0)) and (counts.cpu().numpy() == -7).all()


def test_a_bad_report_type_outside_the_processed_rows_is_not_read(env):
    pkg, ctx, dev = env
    case, cfg = the_case(), M.cfg_of()
    dif, own = M.slot_inputs(case, 3)
    idle = np.nonzero(~((dif > M.LB) & (dif <= M.UB) & (own == 1)))[0]
    typ = case["files"]["typ"].copy()
    typ[idle] = 0
    dat0 = np.zeros(case["nrow"])
    want, tol, counts = M.slot_statement(case, cfg, 0, dif, own, M.LB, M.UB, 1, dat0)
    got, gc = M.run_slot(pkg, ctx, M.device_case(pkg, dict(case, files=dict(case["files"], typ=typ)), cfg, dev, 0, dat0), dif, own,
                         M.LB, M.UB, 1)
    assert (np.abs(got - want) <= tol).all() and np.array_equal(gc, counts)


@pytest.mark.parametrize("order3,order2", [("mkijv", "mijv"), ("mjivk", "mvij")])
def test_fields_in_another_storage_order(env, order3, order2):
    pkg, ctx, dev = env
    case, cfg = the_case(), M.cfg_of(stggrd=1)
    a3, a2, strides = O.permuted(case, order3, order2)
    dif, own = M.slot_inputs(case, 3)
    dat0 = np.zeros(case["nrow"])
    want, tol, counts = M.slot_statement(case, cfg, 1, dif, own, M.LB, M.UB, 0, dat0)
    got, gc = M.run_slot(pkg, ctx, M.device_case(pkg, case, cfg, dev, 1, dat0, fields=(a3, a2), strides=strides), dif, own, M.LB,
                         M.UB, 0)
    exact = tol == 0.0
    assert np.array_equal(bits(got[exact]), bits(want[exact])) and (np.abs(got - want) <= tol).all() and np.array_equal(gc, counts)
    ref, _ = M.run_slot(pkg, ctx, M.device_case(pkg, case, cfg, dev, 1, dat0), dif, own, M.LB, M.UB, 0)
    assert np.array_equal(bits(got), bits(ref))                       # the layout changes no bit


def test_own_null_counts_null_and_no_rotation(env):
    pkg, ctx, dev = env
    case, cfg = the_case(), M.cfg_of()
    dif, _ = M.slot_inputs(case, 3)
    dat0 = np.full(case["nrow"], 0.25)
    want, tol, counts = M.slot_statement(case, cfg, 0, dif, None, M.LB, M.UB, 1, dat0)
    got, gc = M.run_slot(pkg, ctx, M.device_case(pkg, case, cfg, dev, 0, dat0), dif, None, M.LB, M.UB, 1)
    assert (np.abs(got - want) <= tol).all() and np.array_equal(gc, counts) and counts[0] == counts[1]
    got2, none = M.run_slot(pkg, ctx, M.device_case(pkg, case, cfg, dev, 0, dat0), dif, None, M.LB, M.UB, 1, want_counts=False)
    assert none is None and np.array_equal(bits(got2), bits(got))
    # rotc = NULL: U and V unrotated -- the statement with rotc (1, 0)
    unrot = dict(case, rotc=np.tile([1.0, 0.0], (case["nrow"], 1)))
    want3, tol3, _ = M.slot_statement(unrot, cfg, 0, dif, None, M.LB, M.UB, 1, dat0)
    got3, _ = M.run_slot(pkg, ctx, M.device_case(pkg, case, cfg, dev, 0, dat0, rotc=None), dif, None, M.LB, M.UB, 1)
    assert (np.abs(got3 - want3) <= tol3).all() and not np.array_equal(got3, got)


def test_a_slot_without_rows_and_files_without_rows(env):
    pkg, ctx, dev = env
    case, cfg = the_case(), M.cfg_of()
    dif, own = M.slot_inputs(case, 3)
    dat0 = np.full(case["nrow"], 0.25)
    got, gc = M.run_slot(pkg, ctx, M.device_case(pkg, case, cfg, dev, 0, dat0), dif, own, 5000.0, 5600.0, 1)
    assert np.array_equal(bits(got), bits(dat0)) and gc.tolist() == [0, 0]
    got, gc = M.run_slot(pkg, ctx, M.device_case(pkg, case, cfg, dev, 0, dat0), dif, np.zeros_like(own), M.LB, M.UB, 1)
    assert np.array_equal(bits(got), bits(dat0)) and gc[0] > 200 and gc[1] == 0
    # no file rows at all: counts 0, 0
    dc = M.device_case(pkg, case, cfg, dev, 0, dat0)
    off0 = np.zeros(4, dtype=np.int64)
    dc.files.off = off0.ctypes.data_as(C.c_void_p)
    s, keep = slot_struct(pkg, dev, dif, own)
    counts = torch.full((2,), -7, dtype=torch.int64, device=dev)
    ctx.obsmake_slot(s, dc.params, dc.files, dc.fields, counts)
    torch.cuda.synchronize()
    assert counts.cpu().numpy().tolist() == [0, 0] and np.array_equal(bits(dc.d["dat"].cpu().numpy()), bits(dat0))


NOISE_REFUSALS = ["err-struct-null", "files-null", "rand-null", "err-null", "dat-null", "elm-null", "nfile-0", "off-null", "off-descends"]


@pytest.mark.parametrize("what", NOISE_REFUSALS)
def test_every_noise_refusal_writes_nothing_and_consumes_nothing(env, what):
    pkg, ctx, dev = env
    n = 33
    rng = np.random.default_rng(3)
    elm = np.full(n, O.ID_T, dtype=np.int32)
    dat0, err0 = rng.uniform(1, 2, size=n), rng.uniform(1, 2, size=n)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    d = dict(elm=t(elm), dat=t(dat0), err=t(err0))
    off = np.array([0, 20, n], dtype=np.int64)
    f = pkg.ObsFileRows()
    f.nfile, f.off = 2, off.ctypes.data_as(C.c_void_p)
    for k, v in d.items():
        setattr(f, k, v.data_ptr())
    e, r = M.err_struct(pkg), pkg.Rand(9)
    args = [C.byref(e), C.byref(f), r._r]
    if what == "err-struct-null":
        args[0] = None
    elif what == "files-null":
        args[1] = None
    elif what == "rand-null":
        args[2] = None
    elif what in ("err-null", "dat-null", "elm-null"):
        setattr(f, what.split("-")[0], None)
    elif what == "nfile-0":
        f.nfile = 0
    elif what == "off-null":
        f.off = None
    elif what == "off-descends":
        off[1] = n + 1
    rc = pkg.osse_lib().letkf_obsmake_noise_dev(ctx._c, *args)
    torch.cuda.synchronize()
    assert rc == -1 and len(pkg.lib().letkf_amd_last_error()) > 0, (what, rc)
    assert np.array_equal(bits(d["dat"].cpu().numpy()), bits(dat0)) and np.array_equal(bits(d["err"].cpu().numpy()), bits(err0))
    assert np.array_equal(bits(r.res53(4)), bits(S.Sfmt(9, 0).res53(4)))
