"""letkf_obsscan_dev and letkf_obsope_slot_dev across their argument space: every refusal the header lists (the argument named,
nothing written: all outputs canary-filled), each optional output present and NULL, own for every myrank_d, and a context on a
stream of the caller's."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

import _obsscan as S

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env():
    from _gpu import ctx, pkg
    return pkg, ctx(), torch.device("cuda:0")


@pytest.fixture(scope="module")
def case():
    return S.edge_case(file_rows=(0, 7, 300), run=[1, 0, 1])


def test_every_refusal_names_its_argument_and_writes_nothing(env, case):
    pkg, ctx, dev = env
    lib = pkg.obsscan_lib()
    err = lambda: pkg.lib().letkf_amd_last_error().decode()
    n = int(case["off"][-1])

    def attempt(word, mutate=None, null=None):
        p, f, o, out, keep = S.raw_call(pkg, case, dev)
        if mutate:
            keep.append(mutate(p, f, o, keep))
        args = [ctx._c, C.byref(p), C.byref(f), C.byref(o)]
        if null is not None:
            args[null] = None
        rc = lib.letkf_obsscan_dev(*args)
        torch.cuda.synchronize()
        assert rc != 0, word
        assert word in err(), (word, err())
        for name, t in out.items():
            assert bool((t == S.CANARY).all()), (word, name)

    def offsets(values):
        def mutate(p, f, o, keep):
            so = np.array(values, dtype=np.int64)
            f.off = so.ctypes.data_as(C.c_void_p)
            return so
        return mutate

    def put(struct, name, value):
        return lambda p, f, o, keep: setattr({"p": p, "f": f, "o": o}[struct], name, value)

    attempt("context", null=0)
    attempt("params", null=1)
    attempt("files", null=2)
    attempt("out", null=3)
    attempt("off", put("f", "off", None))
    for name in ("bsn", "bsna"):
        attempt("bsn", put("o", name, None))
    for name in ("ri", "rj"):
        attempt("ri / rj / dif", put("f", name, None))
    attempt("ri / rj / dif", put("p", "dif", None))
    for name in ("set", "idx", "qc"):
        attempt("set / idx / qc", put("o", name, None))
    for v in (0, 17):
        attempt("nfile", put("f", "nfile", v))
    for name in ("nlon", "nlat"):
        attempt("nlon and nlat", put("p", name, 0))
    for name in ("prc_num_x", "prc_num_y"):
        attempt("prc_num_x and prc_num_y", put("p", name, 0))
    for name in ("ihalo", "jhalo"):
        attempt("ihalo and jhalo", put("p", name, -1))
    attempt("2^31", put("p", "nlon", 2 ** 30))
    attempt("2^31", put("p", "jhalo", 2 ** 31 - 5))
    attempt("slot_start", put("p", "slot_start", 0))
    attempt("slot_end", put("p", "slot_end", 0))
    for v in (0.0, -600.0, float("nan"), float("inf")):
        attempt("slot_tinterval", put("p", "slot_tinterval", v))
    attempt("start at 0", offsets([1, 1, 8, n]))
    attempt("decreases", offsets([0, 9, 7, n]))
    attempt("2^31 file rows", offsets([0, 0, 7, 2 ** 31]))
    attempt("buckets", put("p", "slot_end", 3 + 2 ** 20))                     # 6 subdomains x (2^20 + 5) buckets
    attempt("buckets", lambda p, f, o, k: (setattr(p, "prc_num_x", 2 ** 11), setattr(p, "prc_num_y", 2 ** 10)) and None)
    for v in (-1, 6):
        attempt("myrank_d", put("p", "myrank_d", v))
    for dst, src in itertools.product(("set", "qc", "rank", "own"), ("ri", "dif")):   # an output on top of an input
        attempt("overlaps", lambda p, f, o, k, dst=dst, src=src: setattr(o, dst, f.ri if src == "ri" else p.dif))
    attempt("overlaps", lambda p, f, o, k: setattr(o, "slot", f.rj + 8 * (n - 1)))      # ... and one that only touches its end
    attempt("overlaps", lambda p, f, o, k: setattr(o, "idx", p.dif + 4))


def test_myrank_d_is_not_read_without_own(env, case):
    pkg, ctx, dev = env
    p, f, o, out, keep = S.raw_call(pkg, case, dev, myrank_d=99)
    o.own = None
    assert pkg.obsscan_lib().letkf_obsscan_dev(ctx._c, C.byref(p), C.byref(f), C.byref(o)) == 0, pkg.lib().letkf_amd_last_error()
    torch.cuda.synchronize()
    got = S.host(out, case)
    assert (got.pop("own") == S.CANARY).all()
    S.assert_same_bits(got, S.scan(case))


def test_each_optional_output_present_and_null(env, case):
    pkg, ctx, dev = env
    want = S.scan(case, myrank_d=3)
    optional = ("rank", "slot", "own")
    for absent in [()] + [(name,) for name in optional] + [optional]:
        p, f, o, out, keep = S.raw_call(pkg, case, dev, myrank_d=3)
        for name in absent:
            setattr(o, name, None)
        assert pkg.obsscan_lib().letkf_obsscan_dev(ctx._c, C.byref(p), C.byref(f), C.byref(o)) == 0, pkg.lib().letkf_amd_last_error()
        torch.cuda.synchronize()
        got = S.host(out, case)
        for name in absent:
            assert (got[name] == S.CANARY).all(), name
        S.assert_same_bits(got, want, [name for name in want if name not in absent])


def test_own_for_every_myrank_d(env, case):
    pkg, ctx, dev = env
    for myrank_d in range(6):
        p, f, o, out, keep = S.raw_call(pkg, case, dev, myrank_d=myrank_d)
        assert pkg.obsscan_lib().letkf_obsscan_dev(ctx._c, C.byref(p), C.byref(f), C.byref(o)) == 0, pkg.lib().letkf_amd_last_error()
        torch.cuda.synchronize()
        want = S.scan(case, myrank_d=myrank_d)
        assert (want["own"] == 1).any() and (want["own"] == -1).any() and (want["own"] == 0).any()
        S.assert_same_bits(S.host(out, case), want)


def test_a_context_on_a_stream_of_the_callers(env, case):
    pkg, _, dev = env
    want = S.scan(case, myrank_d=0)
    stream = torch.cuda.Stream()
    own = pkg.Context(0, stream.cuda_stream)
    with torch.cuda.stream(stream):
        p, f, o, out, keep = S.raw_call(pkg, case, dev)
        got = own.obsscan(f, keep[1]["dif"], case["layout"], case["slots"], obsda_run=case["run"], myrank_d=0)
        got = {k: (v if isinstance(v, np.ndarray) else v.cpu().numpy()) for k, v in got.items()}
    stream.synchronize()
    S.assert_same_bits(got, want)


def test_the_slot_operator_refuses_what_it_cannot_resolve(env):
    pkg, ctx, dev = env
    lib = pkg.obsscan_lib()
    err = lambda: pkg.lib().letkf_amd_last_error().decode()
    bsna = np.array([[0, 2, 3, 3, 4, 4], [4, 4, 4, 5, 5, 5]], dtype=np.int32)
    l = pkg.ObsscanLists()
    l.nprocs_d, l.slot_start, l.slot_end, l.bsna = 2, 1, 3, bsna.ctypes.data
    ens = torch.full((5, 2), float(S.CANARY), dtype=torch.float64, device=dev)
    for word, args in (("lists", (None, 0, 1)), ("ip", (C.byref(l), 2, 1)), ("ip", (C.byref(l), -1, 1)),
                       ("islot", (C.byref(l), 0, 0)), ("islot", (C.byref(l), 0, 4))):
        assert lib.letkf_obsope_slot_dev(ctx._c, args[0], args[1], args[2], None, None, None, ens.data_ptr(), 2) != 0, word
        assert word in err(), (word, err())
    assert lib.letkf_obsope_slot_dev(None, C.byref(l), 0, 1, None, None, None, ens.data_ptr(), 2) != 0
    assert "context" in err()
    l.bsna = None
    assert lib.letkf_obsope_slot_dev(ctx._c, C.byref(l), 0, 1, None, None, None, ens.data_ptr(), 2) != 0
    assert "bsna" in err()
    l.bsna = bsna.ctypes.data
    assert lib.letkf_obsope_slot_dev(ctx._c, C.byref(l), 0, 1, None, None, None, ens.data_ptr(), 2) != 0     # the operator's own check
    torch.cuda.synchronize()
    assert bool((ens == float(S.CANARY)).all())
