"""The integer magnitude rule of the Jacobi rotation (scale-letkf_amd/csrc/letkf_rot_rule.h: g2 > 2^-e ab decided on the upper
dwords) as a host program: a host compiler builds the header alone, the program reads pairs of doubles and writes the rule's
three decisions (rotate 2^-100, stop 2^-80, early 2^-54) for each.  Against g2 > 2^-e ab in float64 (the scaling by a power of
two is exact) on 10^6 random positive pairs, a third of them round each threshold with the ratio g2 / (2^-e ab) spread from
2^-12 away down into the band, the rest spread over many decades: the rule agrees everywhere outside |ratio - 1| < 2^-19 (both
operands truncated to 20 mantissa bits: 2^-20 each).  Then the special values, each with the decision the header documents:
g2 = 0, NaN and inf never exceed anything, whatever ab is; ab = 0 and a subnormal ab pass a normal g2; a subnormal g2 fails
against a normal ab; ab = inf or NaN fails."""
import os
import subprocess
import textwrap

import numpy as np
import pytest

from __graft_entry__ import ROOT

CSRC = os.path.join(ROOT, "scale-letkf_amd", "csrc")
EXPS = (100, 80, 54)

MAIN = textwrap.dedent(r"""
    #include <cstdio>
    #include <cstring>
    #include <vector>
    #include "letkf_rot_rule.h"

    static int32_t hi(const double x) {
      uint64_t u;
      std::memcpy(&u, &x, 8);
      return static_cast<int32_t>(u >> 32);
    }

    int main(int argc, char** argv) {
      using namespace letkf::rot_rule;
      static_assert(kRotExp == 100 && kStopExp == 80 && kEarlyExp == 54, "the exponents this test sweeps");
      if (argc != 3) return 2;
      FILE* f = std::fopen(argv[1], "rb");
      if (!f) return 3;
      std::vector<double> v;
      double buf[4096];
      size_t n;
      while ((n = std::fread(buf, 8, 4096, f)) > 0) v.insert(v.end(), buf, buf + n);
      std::fclose(f);
      std::vector<unsigned char> out(v.size() / 2);
      for (size_t i = 0; i < out.size(); ++i) {
        const int32_t m = margin(hi(v[2 * i]), hi(v[2 * i + 1]));
        out[i] = (exceeds(m, limit(kRotExp)) ? 1 : 0) | (exceeds(m, limit(kStopExp)) ? 2 : 0) | (exceeds(m, limit(kEarlyExp)) ? 4 : 0);
        if (out[i] != ((gt_pow2(hi(v[2 * i]), hi(v[2 * i + 1]), kRotExp) ? 1 : 0) | (gt_pow2(hi(v[2 * i]), hi(v[2 * i + 1]), kStopExp) ? 2 : 0) |
                       (gt_pow2(hi(v[2 * i]), hi(v[2 * i + 1]), kEarlyExp) ? 4 : 0)))
          return 4;
      }
      f = std::fopen(argv[2], "wb");
      if (!f) return 5;
      std::fwrite(out.data(), 1, out.size(), f);
      std::fclose(f);
      return 0;
    }
""")


@pytest.fixture(scope="module")
def rule(tmp_path_factory):
    d = tmp_path_factory.mktemp("rot_rule")
    main = d / "main.cpp"
    main.write_text(MAIN)
    exe = d / "rot_rule"
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-I", CSRC, str(main), "-o", str(exe)])

    def decide(g2, ab):
        """the rule's decisions for the pairs, [3, n] booleans in the order of EXPS"""
        pairs = np.empty((len(g2), 2))
        pairs[:, 0], pairs[:, 1] = g2, ab
        pairs.tofile(d / "in.bin")
        r = subprocess.run([str(exe), str(d / "in.bin"), str(d / "out.bin")], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, (r.returncode, r.stderr)
        bits = np.fromfile(d / "out.bin", dtype=np.uint8)
        assert bits.size == len(g2)
        return np.stack([(bits >> j) & 1 for j in range(3)]).astype(bool)
    return decide


def test_random_positive_pairs_agree_outside_the_band(rule):
    rng = np.random.default_rng(1100)
    n = 1_000_000
    ab = np.exp2(rng.uniform(-300.0, 300.0, size=n))
    e = np.array(EXPS)[rng.integers(0, 3, size=n)]
    # a third round the threshold of one of the three rules: |ratio - 1| log-uniform from 2^-22 (inside the band) to 2^-12, either sign
    near = rng.random(n) < 1.0 / 3.0
    ratio = np.where(near, 1.0 + rng.choice([-1.0, 1.0], size=n) * np.exp2(rng.uniform(-22.0, -12.0, size=n)),
                     np.exp2(rng.uniform(-60.0, 60.0, size=n)))
    g2 = np.ldexp(ab, -e) * ratio
    got = rule(g2, ab)
    checked = 0
    for j, ej in enumerate(EXPS):
        thr = np.ldexp(ab, -ej)
        want = g2 > thr
        outside = np.abs(g2 / thr - 1.0) >= 2.0 ** -19
        bad = outside & (got[j] != want)
        assert not bad.any(), (ej, int(bad.sum()), g2[bad][:3], ab[bad][:3])
        checked += int((outside & near & (e == ej)).sum())
        assert want[outside].any() and (~want[outside]).any()
    assert checked > 200_000        # the pairs round a threshold are mostly outside its band, and decided there
    # inside the band the rule is the comparison of the truncated values: never more than a rotate / stop / early nesting apart
    assert (got[0] >= got[1]).all() and (got[1] >= got[2]).all()


def test_zero_nan_inf_and_subnormal_operands(rule):
    nan, inf, tiny = float("nan"), float("inf"), 5e-324
    never, always = [], []
    # g2 = 0 (either sign), NaN (either sign), inf: nothing, whatever ab is -- ab = 0 included
    for g2 in (0.0, -0.0, nan, -nan, inf, -inf):
        for ab in (0.0, tiny, 1e-310, 1e-300, 1.0, 1e300, inf, nan):
            never.append((g2, ab))
    # a subnormal g2 against a normal ab; any g2 of ordinary size against ab = inf or NaN
    never += [(tiny, 1.0), (1e-310, 1e-200), (1e-310, 1.0), (1e-10, inf), (1.0, inf), (1e100, nan), (1.0, nan), (1e-300, 1e300)]
    # ab = 0 or subnormal: every normal g2 of a size a squared inner product can have exceeds all three
    always += [(g2, ab) for g2 in (1e-250, 1e-30, 1.0, 1e300) for ab in (0.0, tiny, 1e-310)]
    always += [(1e300, 1e-300), (1.0, 1.0), (1e-16 * 1.0001, 1.0)]
    pairs = np.array(never + always)
    got = rule(pairs[:, 0], pairs[:, 1])
    for i, (g2, ab) in enumerate(never):
        assert not got[:, i].any(), (g2, ab, got[:, i])
    for i, (g2, ab) in enumerate(always, start=len(never)):
        assert got[:, i].all(), (g2, ab, got[:, i])
    # and these are the floating-point comparison's decisions wherever that one is defined by a finite g2
    with np.errstate(invalid="ignore"):
        for j, ej in enumerate(EXPS):
            fin = np.isfinite(pairs[:, 0])
            want = pairs[:, 0] > np.ldexp(pairs[:, 1], -ej)
            assert (got[j][fin] == want[fin]).all(), (ej, pairs[fin][got[j][fin] != want[fin]])
    # between the rules: 2^-90 of ab rotates and does not stop the iteration; 2^-70 counts as not converged, early stop allowed
    got = rule(np.array([2.0 ** -90, 2.0 ** -70, 2.0 ** -40, 2.0 ** -110]), np.ones(4))
    assert got.T.tolist() == [[True, False, False], [True, True, False], [True, True, True], [False, False, False]]
