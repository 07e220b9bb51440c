"""tests/_sfmt.py against the compiled reference (oracle/_ref/libletkf_ref.so exports init_gen_rand_, genrand_res53_ and
com_randn), in a fresh child process so that the saved parity flag of period_certification starts from 0:
  six seedings in a row, 700 values each (two regenerations of the 312-value state): bitwise the statement with the flag
    carried from seeding to seeding;
  a throw-away com_randn(2) forces its clock-seeded init_gen_rand, after which the flag is unknown: the next seeded draw
    must match exactly one of the two candidate streams over 700 values;
  com_randn(100 001) within 4 ulp of the numpy Box-Muller with pi = 3.1415926535 (two libm calls and two roundings apart;
    the issue's own probe measured 2 ulp)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import _sfmt as S
from __graft_entry__ import ROOT

REF = os.path.join(ROOT, "oracle", "_ref", "libletkf_ref.so")
SEEDS = (1234, 59999, 0, 77, 31337, 5)
NDRAW, NRANDN, SEED2 = 700, 100001, 4321

CHILD = r"""
import ctypes as C, sys, numpy as np
L = C.CDLL(sys.argv[1]); L.genrand_res53_.restype = C.c_double
out = []
def init(s):
    ss = C.c_int(s); L.init_gen_rand_(C.byref(ss))
def randn(n):
    a = np.zeros(n); nn = C.c_int(n); L._QMcommonPcom_randn(C.byref(nn), a.ctypes.data_as(C.c_void_p)); return a
for seed in (%s):
    init(seed); out.append(np.array([L.genrand_res53_() for _ in range(%d)]))
randn(2)
init(%d); out.append(np.array([L.genrand_res53_() for _ in range(%d)]))
init(%d); out.append(randn(%d))
np.concatenate(out).tofile(sys.argv[2])
""" % (", ".join(str(s) for s in SEEDS), NDRAW, SEED2, NDRAW, SEED2, NRANDN)


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    if not os.path.exists(REF):
        pytest.skip("oracle/_ref not built (reference tree absent)")
    path = str(tmp_path_factory.mktemp("sfmt") / "ref.bin")
    subprocess.run([sys.executable, "-c", CHILD, REF, path], check=True, timeout=120)
    a = np.fromfile(path, dtype=np.float64)
    assert a.size == (len(SEEDS) + 1) * NDRAW + NRANDN
    return dict(seq=a[:len(SEEDS) * NDRAW].reshape(len(SEEDS), NDRAW), after=a[len(SEEDS) * NDRAW:(len(SEEDS) + 1) * NDRAW],
                randn=a[(len(SEEDS) + 1) * NDRAW:])


def bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def test_six_seedings_in_a_row_are_the_statement_with_the_carried_flag(ref):
    inner, flags = 0, []
    for n, seed in enumerate(SEEDS):
        g = S.Sfmt(seed, inner)
        assert np.array_equal(bits(g.res53(NDRAW)), bits(ref["seq"][n])), (seed, inner)
        flags.append(inner)
        inner = g.inner
    assert 1 in flags                                  # a seeding that started from inner = 1 is among them
    # the textbook conversion (v >> 11) * 2^-53 is NOT the reference's
    g = S.Sfmt(SEEDS[0])
    text = np.array([(g.next64() >> 11) * 2.0 ** -53 for _ in range(NDRAW)])
    assert not np.array_equal(bits(text), bits(ref["seq"][0])) and np.allclose(text, ref["seq"][0], rtol=0, atol=2.0 ** -52)


def test_after_a_clock_seeding_exactly_one_candidate_stream_matches_and_com_randn_follows_it(ref):
    cand = [S.Sfmt(SEED2, i0) for i0 in (0, 1)]
    draws = [g.res53(NDRAW) for g in cand]
    match = [np.array_equal(bits(d), bits(ref["after"])) for d in draws]
    assert sum(match) == 1, match
    mine = S.randn(S.Sfmt(SEED2, cand[match.index(True)].inner), NRANDN)       # (one more seeding: the flag carries once more)
    e = ref["randn"]
    assert np.isfinite(e).all()
    ulp = np.abs(mine - e) / np.spacing(np.abs(e))
    print(f"com_randn vs numpy Box-Muller: worst {ulp.max():.2f} ulp, {100.0 * (ulp > 0).mean():.2f} % differ")
    assert ulp.max() <= 4.0
