"""letkf_rand_res53 (include/letkf_amd_obsmake.h) without a device: bitwise the statement of tests/_sfmt.py with inner0 = 0,
the stream of a process's first init_gen_rand(seed) -- at the counts around the 312-value regeneration of the state, split
over several calls, for the seeds at the ends of the 32-bit range -- and the refusals."""
import ctypes as C

import numpy as np
import pytest

import _sfmt as S
from __graft_entry__ import load_package

SEEDS = (0, 1, 59999, 2 ** 31 - 1)
COUNTS = (1, 2, 311, 312, 313, 624, 625, 1000)
_WANT = {}


@pytest.fixture(scope="module")
def pkg():
    p = load_package()
    p.build()
    return p


def want(seed):
    if seed not in _WANT:
        _WANT[seed] = S.Sfmt(seed, 0).res53(1000)
        _WANT[seed].setflags(write=False)
    return _WANT[seed]


def bits(a):
    return np.ascontiguousarray(a).view(np.int64)


@pytest.mark.parametrize("seed", SEEDS)
def test_res53_is_the_first_call_stream_bit_for_bit(pkg, seed):
    for n in COUNTS:
        got = pkg.Rand(seed).res53(n)
        assert np.array_equal(bits(got), bits(want(seed)[:n])), (seed, n)
    r = pkg.Rand(seed)
    parts = np.concatenate([r.res53(n) for n in (7, 305, 1, 687)])
    assert np.array_equal(bits(parts), bits(want(seed)))
    assert r.res53(0).size == 0
    assert ((want(seed) >= 0.0) & (want(seed) <= 1.0)).all()


def test_a_negative_seed_is_its_32_bit_pattern(pkg):
    assert np.array_equal(bits(pkg.Rand(-1).res53(20)), bits(S.Sfmt(0xffffffff, 0).res53(20)))


def test_refusals(pkg):
    l = pkg.osse_lib()
    r = pkg.Rand(5)
    out = np.full(4, 7.0)
    assert l.letkf_rand_create(1, None) != 0 and b"NULL" in pkg.lib().letkf_amd_last_error()
    assert l.letkf_rand_res53(None, 4, out.ctypes.data_as(C.c_void_p)) != 0
    assert l.letkf_rand_res53(r._r, -1, out.ctypes.data_as(C.c_void_p)) != 0
    assert l.letkf_rand_res53(r._r, 4, None) != 0
    assert l.letkf_rand_set_chunk(r._r, 0) != 0 and l.letkf_rand_set_chunk(None, 8) != 0
    assert (out == 7.0).all()
    assert np.array_equal(bits(r.res53(4)), bits(S.Sfmt(5, 0).res53(4)))        # nothing was consumed by the refused calls
    assert l.letkf_rand_destroy(None) == 0
