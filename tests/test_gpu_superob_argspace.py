"""letkf_superob_dev across its argument space: every refusal the header lists (the argument named, nothing written), each
optional output as NULL, and a context on a stream of the caller's."""
import ctypes as C

import numpy as np
import pytest
import torch

import _superob as S

pytestmark = pytest.mark.gpu
METHODS = S.uniform_methods(4, 4, v=2, t=1, h=3)


@pytest.fixture(scope="module")
def env():
    from _gpu import ctx, pkg
    return pkg, ctx(), torch.device("cuda:0")


@pytest.fixture(scope="module")
def case():
    return S.base_case(seed=7, n=400, special=False)


def test_every_refusal_names_its_argument_and_writes_nothing(env, case):
    pkg, ctx, dev = env
    lib = pkg.superob_lib()
    rows = S.device_rows(case, dev)
    err = lambda: pkg.lib().letkf_amd_last_error().decode()

    def attempt(word, mutate=None, null=None, methods=METHODS):
        p, o, out, keep = S.raw_call(pkg, case, methods, rows)
        if mutate:
            keep.append(mutate(p, o, keep))
        args = [ctx._c, C.byref(p), C.byref(o)]
        if null is not None:
            args[null] = None
        rc = lib.letkf_superob_dev(*args)
        torch.cuda.synchronize()
        assert rc != 0, word
        assert word in err(), (word, err())
        for name, t in out.items():
            assert bool((t == -777).all()), (word, name)

    def table(x, v):
        def mutate(p, o, keep):
            t = keep[2 + x].copy()
            t[1, 2] = v
            setattr(p, ("method_g", "method_v", "method_t", "method_h")[x], t.ctypes.data)
            return t
        return mutate

    def slots(values):
        def mutate(p, o, keep):
            so = np.array(values, dtype=np.int64)
            p.slot_off = so.ctypes.data
            return so
        return mutate

    n = rows["elm"].numel()
    attempt("context", null=0)
    attempt("params", null=1)
    attempt("out", null=2)
    for name in ("elm", "typ") + S.FIELDS:
        attempt("input array", lambda p, o, k, name=name: setattr(p, name, None))
    for name in S.ROW_FIELDS:
        attempt("output array", lambda p, o, k, name=name: setattr(o, name, None))
    attempt("nout", lambda p, o, k: setattr(o, "nout", None))
    for name in ("slot_off", "elem_uid", "method_g", "method_v", "method_t", "method_h"):
        attempt("is NULL", lambda p, o, k, name=name: setattr(p, name, None))
    for v in (-1, 2 ** 31):
        attempt("nobs", lambda p, o, k, v=v: setattr(p, "nobs", v))
    for name in ("nlon", "nlat", "nlevx"):
        attempt("nlevx", lambda p, o, k, name=name: setattr(p, name, 0))
    for v in (0, 65):
        attempt("nslots", lambda p, o, k, v=v: setattr(p, "nslots", v))
    for v in (0, 4):
        attempt("nbslot", lambda p, o, k, v=v: setattr(p, "nbslot", v))
    for name in ("nobtype", "nid"):
        for v in (0, 33):
            attempt("nobtype and nid", lambda p, o, k, name=name, v=v: setattr(p, name, v))
    for x, v in ((0, -1), (0, 2), (1, -1), (1, 4), (2, -1), (2, 3), (3, -1), (3, 4)):
        attempt("method", table(x, v))
    attempt("slot_off", slots([1, 1, 200, n]))
    attempt("slot_off", slots([0, 0, 200, n - 1]))
    attempt("slot_off", slots([0, 0, 200, n + 1]))
    attempt("decreases", slots([0, 300, 200, n]))
    attempt("cells", lambda p, o, k: (setattr(p, "nlon", 2 ** 31 - 1), setattr(p, "nlat", 2 ** 31 - 1)) and None)
    for name in ("lon", "dat", "elm"):                            # an output on top of an input, and one that only overlaps it
        attempt("overlaps", lambda p, o, k, name=name: setattr(o, name, getattr(p, name)))
    attempt("overlaps", lambda p, o, k: setattr(o, "rk", p.ri + 8 * (n - 1)))
    attempt("overlaps", lambda p, o, k: setattr(o, "counts", p.err + 16))
    attempt("overlaps", lambda p, o, k: setattr(o, "qc1", p.typ))


def test_each_optional_output_as_null(env, case):
    pkg, ctx, dev = env
    rows = S.device_rows(case, dev)
    want = S.superob(case, METHODS)
    nout = int(want["nout"][0])
    optional = ("slot_off_out", "qc1", "counts", "obsnum")
    for absent in [()] + [(name,) for name in optional] + [optional]:
        p, o, out, keep = S.raw_call(pkg, case, METHODS, rows)
        for name in absent:
            setattr(o, name, None)
        assert pkg.superob_lib().letkf_superob_dev(ctx._c, C.byref(p), C.byref(o)) == 0, pkg.lib().letkf_amd_last_error()
        torch.cuda.synchronize()
        got = {name: t.cpu().numpy() for name, t in out.items()}
        for name in absent:
            assert (got[name] == -777).all(), name
        for name in S.ROW_FIELDS:
            assert (got[name][nout:] == -777).all(), name         # nothing past nout
            got[name] = got[name][:nout]
        S.assert_same_bits(got, want, [name for name in want if name not in absent])


def test_a_context_on_a_stream_of_the_callers(env, case):
    pkg, _, dev = env
    want = S.superob(case, METHODS)
    stream = torch.cuda.Stream()
    own = pkg.Context(0, stream.cuda_stream)
    with torch.cuda.stream(stream):
        rows = S.device_rows(case, dev)
        out = own.superob(rows, case["slot_off"], case["grid"], case["nbslot"], case["elem_uid"], METHODS,
                          surface_typ_mask=case["surface_typ_mask"])
        got = {name: t.cpu().numpy() for name, t in out.items()}    # (the copies are on the same stream and wait for the call)
    stream.synchronize()
    for name in S.ROW_FIELDS:
        got[name] = got[name][:int(got["nout"][0])]
    S.assert_same_bits(got, want)
