"""letkf_obssim_dev across its argument space: permuted field layouts, lists of length 1 and 16, repeated ids, ids the operator
does not know, every refusal (outputs untouched, the argument named), and the plain operator unchanged by a simulator call."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import _obsope as O
import _obssim as S

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env():
    from _gpu import ctx, pkg
    return pkg, ctx(), torch.device("cuda:0")


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64 if a.dtype == np.float64 else np.int32)


@pytest.mark.parametrize("order3,order2", [("mvjik", "mvji"), ("vmkji", "jimv"), ("jikvm", "vjim"), ("kijmv", "ijvm")])
def test_permuted_field_layouts_give_the_same_bits(env, order3, order2):
    pkg, ctx, dev = env
    case, cfg = S.make_case("8x5x3"), S.default_cfg(method_ref_calc=3, stggrd=1, ps_adjust_thres=1.0e4)
    want = S.DeviceCase(pkg, case, cfg, S.VARS3, S.VARS2, dev).run(ctx)
    a3, a2, strides = O.permuted(case, order3, order2)
    got = S.DeviceCase(pkg, case, cfg, S.VARS3, S.VARS2, dev, fields=(a3, a2), strides=strides).run(ctx)
    for n in ("v3", "v2", "rec"):
        assert np.array_equal(bits(got[n]), bits(want[n])), n
    assert (want["v2"][:, 0] != O.UNDEF).all()                       # (PS is a value at this threshold)


def test_lists_of_length_1_and_16_repeated_and_unknown_ids(env):
    pkg, ctx, dev = env
    case, cfg = S.make_case("8x5x3"), S.default_cfg()
    full = S.DeviceCase(pkg, case, cfg, S.VARS3, S.VARS2, dev).run(ctx)
    pos = {e: n for n, e in enumerate(S.VARS3)}
    for e in (O.ID_T, O.ID_VR, O.ID_PRH):
        one = S.DeviceCase(pkg, case, cfg, (e,), (), dev).run(ctx, want=("v3", "rec"))
        assert np.array_equal(bits(one["v3"][:, 0]), bits(full["v3"][:, pos[e]])), e
    one2 = S.DeviceCase(pkg, case, cfg, (), (O.ID_T,), dev).run(ctx, want=("v2",))
    assert np.array_equal(bits(one2["v2"][:, 0]), bits(full["v2"][:, S.VARS2.index(O.ID_T)]))
    # 16 entries: repeated ids and ids the operator does not know (H08 8800, TC vitals 99991, rain 19999, 0, -1)
    l16 = (O.ID_REF, O.ID_T, O.ID_REF, 8800, O.ID_VR, O.ID_VR, 99991, O.ID_RAIN, O.ID_U, 0, -1, O.ID_TV, O.ID_T, O.ID_Q, O.ID_PS, O.ID_REF_ZERO)
    got = S.DeviceCase(pkg, case, cfg, l16, l16, dev).run(ctx)
    for n, e in enumerate(l16):
        if e in pos:
            assert np.array_equal(bits(got["v3"][:, n]), bits(full["v3"][:, pos[e]])), (n, e)
        else:
            assert (got["v3"][:, n] == O.UNDEF).all(), (n, e)
        if e in S.RADAR_IDS or e not in pos:
            assert (got["v2"][:, n] == O.UNDEF).all(), (n, e)          # the 2-D list knows no radar id
        else:
            assert np.array_equal(bits(got["v2"][:, n]), bits(full["v3"][:, pos[e], :, :, 0])), (n, e)
    assert np.array_equal(bits(got["rec"]), bits(S.records(got["v3"], got["v2"])))


def test_every_refusal_names_its_argument_and_writes_nothing(env):
    pkg, ctx, dev = env
    case, cfg = S.make_case("8x5x3"), S.default_cfg()
    lib = pkg.obssim_lib()
    err = lambda: pkg.lib().letkf_amd_last_error().decode()

    def attempt(word, mutate=None, want=("v3", "v2", "rec"), null=None, vars3=S.VARS3, vars2=S.VARS2):
        dc = S.DeviceCase(pkg, case, cfg, vars3, vars2, dev)
        out = dc.outputs(("v3", "v2", "rec"))
        o = pkg.ObssimOut()
        for n in ("v3", "v2", "rec"):
            setattr(o, n, C.c_void_p(out[n].data_ptr()) if n in want else None)
        o.sm3, o.sm2 = out["v3"][0].numel(), out["v2"][0].numel()
        if mutate:
            mutate(dc.params, dc.fields, o)
        args = [ctx._c, C.byref(dc.params), C.byref(dc.fields), C.byref(o)]
        if null is not None:
            args[null] = None
        rc = lib.letkf_obssim_dev(*args)
        torch.cuda.synchronize()
        assert rc != 0, word
        assert word in err(), (word, err())
        for n in ("v3", "v2", "rec"):
            assert bool((out[n] == -777.0).all()), (word, n)

    attempt("context", null=0)
    attempt("params", null=1)
    attempt("fields", null=2)
    attempt("out", null=3)
    attempt("lon", lambda p, f, o: setattr(p, "lon", None))
    attempt("lat", lambda p, f, o: setattr(p, "lat", None))
    attempt("v3d", lambda p, f, o: setattr(f, "v3d", None))
    attempt("v2d", lambda p, f, o: setattr(f, "v2d", None))
    attempt("all NULL", want=())
    for name, v in (("nvar3", -1), ("nvar3", 17), ("nvar2", -1), ("nvar2", 17)):
        attempt(name, lambda p, f, o, name=name, v=v: setattr(p, name, v))
    attempt("both 0", lambda p, f, o: (setattr(p, "nvar3", 0), setattr(p, "nvar2", 0)), want=("rec",))
    attempt("v3 is given", lambda p, f, o: setattr(p, "nvar3", 0))
    attempt("v2 is given", lambda p, f, o: setattr(p, "nvar2", 0))
    for name in ("nlev", "nlon", "nlat"):
        attempt("grid extents", lambda p, f, o, name=name: setattr(f, name, 0))
    attempt("grid extents", lambda p, f, o: setattr(f, "ihalo", -1))
    attempt("grid extents", lambda p, f, o: setattr(f, "jhalo", -1))
    attempt("khalo", lambda p, f, o: setattr(f, "khalo", 0))
    for name in ("s3k", "s3i", "s3j", "s3v", "s3m", "s2i", "s2j", "s2v", "s2m"):
        attempt("stride", lambda p, f, o, name=name: setattr(f, name, 0))
    attempt("nv3dd", lambda p, f, o: setattr(f, "nv3dd", 12))
    attempt("nv2dd", lambda p, f, o: setattr(f, "nv2dd", 6))
    attempt("m0", lambda p, f, o: setattr(f, "m0", 1))
    attempt("nmem", lambda p, f, o: setattr(f, "nmem", 0))
    for v in (0, 4):
        attempt("method_ref_calc", lambda p, f, o, v=v: setattr(p, "method_ref_calc", v))
    for v in (-1, 2):
        attempt("stggrd", lambda p, f, o, v=v: setattr(p, "stggrd", v))
        attempt("round_single", lambda p, f, o, v=v: setattr(p, "round_single", v))
    for name in ("radar_lon", "radar_lat", "radar_z"):
        for v in (math.nan, math.inf):
            attempt("radar", lambda p, f, o, name=name, v=v: setattr(p, name, v))


def test_the_plain_operator_is_unchanged_by_a_simulator_call(env):
    pkg, ctx, dev = env
    ocase, ocfg = O.make_case(8), O.default_cfg(method_ref_calc=2)
    odc = O.DeviceCase(pkg, ocase, ocfg, dev)
    v1, q1 = odc.run(ctx)
    S.DeviceCase(pkg, S.make_case("70x5x3"), S.default_cfg(), S.VARS3, S.VARS2, dev).run(ctx)
    v2, q2 = odc.run(ctx)
    assert np.array_equal(bits(v1), bits(v2)) and np.array_equal(q1, q2)
