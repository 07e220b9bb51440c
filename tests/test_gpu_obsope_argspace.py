"""letkf_obsope_dev across its argument space: the bits of the dense call (reference layout, kld = k, m0 = 0, every row) under
other field layouts, row lengths, slots and row ranges, rotc NULL against all-(1, 0), and every refusal of the header."""
import ctypes as C

import numpy as np
import pytest
import torch

import _obsope as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env():
    from _gpu import ctx, pkg
    case, cfg = O.make_case(8), O.default_cfg(method_ref_calc=3)
    dev = torch.device("cuda:0")
    dense = O.DeviceCase(pkg, case, cfg, dev).run(ctx())
    return pkg, ctx(), dev, case, cfg, dense


def bits(a):
    return np.ascontiguousarray(a).view(np.int64)


@pytest.mark.parametrize("order3,order2", [("mvjik", "mvji"), ("kjimv", "ijvm"), ("vmikj", "jmiv")])
def test_field_layouts(env, order3, order2):
    pkg, ctx, dev, case, cfg, (v0, q0) = env
    a3, a2, strides = O.permuted(case, order3, order2)
    if order3 == "mvjik":
        assert strides == O.reference_strides(case["g"])
    v, q = O.DeviceCase(pkg, case, cfg, dev, fields=(a3, a2), strides=strides).run(ctx)
    assert np.array_equal(bits(v), bits(v0)) and np.array_equal(q, q0)


@pytest.mark.parametrize("pad", [0, 1, 2, 3])
def test_row_lengths_and_slots(env, pad):
    pkg, ctx, dev, case, cfg, (v0, q0) = env
    k = case["nmem"]
    for m0 in range(pad + 1):
        v, q = O.DeviceCase(pkg, case, cfg, dev).run(ctx, kld=k + pad, m0=m0, canary=3.25)
        want = np.full((case["nrow"], k + pad), 3.25)
        want[:, m0:m0 + k] = v0
        assert np.array_equal(bits(v), bits(want)) and np.array_equal(q, q0)


def test_a_short_row_range(env):
    pkg, ctx, dev, case, cfg, (v0, q0) = env
    for row0, nrows in ((5, 3), (case["nrow"] - 1, 1), (40, 0)):
        v, q = O.DeviceCase(pkg, case, cfg, dev).run(ctx, row0=row0, nrows=nrows, canary=-7.5)
        want, want_q = np.full_like(v0, -7.5), np.zeros_like(q0)
        want[row0:row0 + nrows], want_q[row0:row0 + nrows] = v0[row0:row0 + nrows], q0[row0:row0 + nrows]
        assert np.array_equal(bits(v), bits(want)) and np.array_equal(q, want_q)


def test_rotc_null_is_one_zero(env):
    pkg, ctx, dev, case, cfg, _ = env
    ones = np.tile(np.array([1.0, 0.0]), (case["nrow"], 1))
    v1, q1 = O.DeviceCase(pkg, case, cfg, dev, rotc=None).run(ctx)
    v2, q2 = O.DeviceCase(pkg, case, cfg, dev, rotc=ones).run(ctx)
    assert np.array_equal(bits(v1), bits(v2)) and np.array_equal(q1, q2)
    assert O.compare(v1, q1, O.statement(case, cfg, rotc="identity")) == []


def refused(pkg, ctx, dc, words, **run):
    canary = 9.75
    with pytest.raises(pkg.LetkfError) as e:
        dc.run(ctx, canary=canary, **run)
    assert any(w in str(e.value) for w in words), str(e.value)


def test_refusals_carry_a_message_and_write_nothing(env):
    pkg, ctx, dev, case, cfg, (v0, q0) = env
    k = case["nmem"]
    mk = lambda: O.DeviceCase(pkg, case, cfg, dev)
    dc = mk()
    dc.fields.nmem = 0
    refused(pkg, ctx, dc, ["nmem"], kld=k)
    refused(pkg, ctx, mk(), ["kld"], kld=k + 1, m0=2)
    for name in ("s3k", "s3i", "s3j", "s3v", "s3m", "s2i", "s2j", "s2v", "s2m"):
        dc = mk()
        setattr(dc.fields, name, 0)
        refused(pkg, ctx, dc, ["stride"])
    for method in (0, 4):
        dc = mk()
        dc.params.method_ref_calc = method
        refused(pkg, ctx, dc, ["method_ref_calc"])
    dc = mk()
    dc.fields.khalo = 0
    refused(pkg, ctx, dc, ["khalo"])
    # set / idx outside the files: checked on the device, nothing is written
    for arr, row, value in (("set", 11, 0), ("set", 12, 4), ("idx", 13, 0), ("idx", 14, 10 ** 6)):
        bad = dict(case, **{arr: case[arr].copy()})
        bad[arr][row] = value
        dc = O.DeviceCase(pkg, bad, cfg, dev)
        ens = torch.full((case["nrow"], k), 9.75, dtype=torch.float64, device=dev)
        qc = torch.zeros(case["nrow"], dtype=torch.int32, device=dev)
        with pytest.raises(pkg.LetkfError) as e:
            dc.run(ctx, qc=qc, ensval=ens)
        assert "outside the files" in str(e.value)
        assert bool((ens == 9.75).all()) and int(qc.abs().max()) == 0
    # the context still serves the next call
    v, q = mk().run(ctx)
    assert np.array_equal(bits(v), bits(v0)) and np.array_equal(q, q0)
