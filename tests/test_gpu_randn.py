"""letkf_randn_dev (include/letkf_amd_obsmake.h) against com_randn as tests/_sfmt.py states it: the uniforms come from the
host generator bit for bit (tests/test_rand_host.py), Box-Muller runs on the device.

Tolerance (derived, not tuned): the angle (2.0 * pi) * u2 and log's argument u1 are bit-identical on both sides; what differs
is the device's log, sin and cos against libm's.  With OpenCL's documented bounds for double (log 3 ulp, sin and cos 4 ulp, sqrt
correctly rounded) and libm's own error of about 1 ulp: the radius sqrt(-2 log u1) carries half of log's relative error,
(3 + 1) / 2 = 2 ulp, plus sqrt's rounding on each side, 1 ulp; the sine or cosine (4 + 1) = 5 ulp of its own value (the angle
is exact, so there is no amplification near its zeros); the product one rounding on each side, 1 ulp: 9 ulp, and at most twice
that when the errors are counted in units of the smaller neighbour across a binade.  The bound is 16 ulp of the deviate.  u1 = 0
gives +inf on both sides and is compared as equal.  If a deviate exceeds the bound the kernel or the statement is wrong: the
tolerance stays."""
import numpy as np
import pytest
import torch

import _sfmt as S

pytestmark = pytest.mark.gpu

COUNTS = (1, 2, 3, 623, 624, 625, 4097)
SEED = 20141
_WANT = {}


@pytest.fixture(scope="module")
def env():
    from _gpu import ctx, pkg
    return pkg, ctx(), torch.device("cuda:0")


def want(n):
    if n not in _WANT:
        _WANT[n] = S.randn(S.Sfmt(SEED, 0), n)
        _WANT[n].setflags(write=False)
    return _WANT[n]


def draw(pkg, ctx, dev, n, chunk=None, seed=SEED):
    r = pkg.Rand(seed)
    if chunk is not None:
        r.set_chunk(chunk)
    out = torch.full((n + 2,), -5.0, dtype=torch.float64, device=dev)
    ctx.randn(r, n, out)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert (got[n:] == -5.0).all()                     # nothing beyond n, the cosine of an odd count's last pair included
    return got[:n], r


def worst_ulp(got, exp):
    same = (got == exp)
    return float(np.max(np.where(same, 0.0, np.abs(got - exp) / np.spacing(np.abs(exp)))))


@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("chunk", [None, 100], ids=["chunk-default", "chunk-100"])
def test_randn_is_com_randn_within_16_ulp(env, n, chunk):
    """chunk 100: 4097 deviates are 2049 pairs in 21 chunks, so each pinned buffer is refilled ten times"""
    pkg, ctx, dev = env
    got, r = draw(pkg, ctx, dev, n, chunk)
    w = worst_ulp(got, want(n))
    print(f"n {n} chunk {chunk}: worst {w:.2f} ulp")
    assert w <= 16.0
    # the stream went on by 2 * ceil(n / 2) uniforms
    g = S.Sfmt(SEED, 0)
    g.res53(2 * ((n + 1) // 2))
    assert np.array_equal(r.res53(5).view(np.int64), g.res53(5).view(np.int64))


def test_randn_is_bitwise_equal_from_call_to_call_and_whatever_the_chunk(env):
    pkg, ctx, dev = env
    a, _ = draw(pkg, ctx, dev, 4097)
    b, _ = draw(pkg, ctx, dev, 4097)
    c, _ = draw(pkg, ctx, dev, 4097, chunk=100)
    d, _ = draw(pkg, ctx, dev, 4097, chunk=1)
    assert np.array_equal(a.view(np.int64), b.view(np.int64))
    assert np.array_equal(a.view(np.int64), c.view(np.int64)) and np.array_equal(a.view(np.int64), d.view(np.int64))
    e, _ = draw(pkg, ctx, dev, 4097, seed=SEED + 1)
    assert not np.array_equal(a, e)


def test_two_calls_on_one_stream_continue_it(env):
    """623 then 3474 deviates: an odd count ends on a fresh pair's sine and the next call starts a new pair"""
    pkg, ctx, dev = env
    r = pkg.Rand(SEED)
    r.set_chunk(64)
    out = torch.zeros(623 + 3474, dtype=torch.float64, device=dev)
    ctx.randn(r, 623, out)
    ctx.randn(r, 3474, out[623:])
    torch.cuda.synchronize()
    g = S.Sfmt(SEED, 0)
    exp = np.concatenate([S.randn(g, 623), S.randn(g, 3474)])
    assert worst_ulp(out.cpu().numpy(), exp) <= 16.0


def test_refusals_write_nothing_and_consume_nothing(env):
    pkg, ctx, dev = env
    r = pkg.Rand(SEED)
    out = torch.full((8,), -5.0, dtype=torch.float64, device=dev)
    l = pkg.osse_lib()
    assert l.letkf_randn_dev(ctx._c, None, 4, out.data_ptr()) != 0
    assert l.letkf_randn_dev(ctx._c, r._r, -1, out.data_ptr()) != 0
    assert l.letkf_randn_dev(ctx._c, r._r, 4, None) != 0
    assert l.letkf_randn_dev(None, r._r, 4, out.data_ptr()) != 0
    ctx.randn(r, 0, None)
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == -5.0).all()
    assert np.array_equal(r.res53(4).view(np.int64), S.Sfmt(SEED, 0).res53(4).view(np.int64))
