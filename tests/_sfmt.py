"""SFMT19937 as com_rand / com_randn draw from it, in plain Python and numpy: the CPU statement that letkf_rand_res53 and
letkf_randn_dev (include/letkf_amd_obsmake.h) are compared with.  Written from the published algorithm (Saito and Matsumoto,
parameter set 19937) and the behaviour of the reference's port (common/SFMT.f90, common/common.f90:260-298);
tests/test_sfmt_statement.py anchors it to the compiled reference.

Three things differ from a textbook generator:
  inner0       period_certification keeps its parity flag from call to call (SFMT.f90:436): Sfmt(seed, inner0) starts from the
               flag the previous seeding left (0 in a fresh process) and .inner is the flag it leaves
  conversion   genrand_res53 = dble(ishft(v, -1)) * 2^-63: the 63-bit integer is rounded to double (SFMT.f90:730-736)
  pi           3.1415926535 (common.f90:28) in Box-Muller's angle (2.0 * pi) * u2
"""
import numpy as np

N, N32, POS1, SL1, SR1 = 156, 624, 122, 18, 11
MSK = (0xdfffffef, 0xddfecb7f, 0xbffaffff, 0xbffffff6)
PARITY = (0x00000001, 0x00000000, 0x00000000, 0x13c9e684)
M32, M64, M128 = (1 << 32) - 1, (1 << 64) - 1, (1 << 128) - 1
PI = 3.1415926535


def _lanes(f, x):
    return sum((f((x >> (32 * k)) & M32, k) & M32) << (32 * k) for k in range(4))


class Sfmt:
    def __init__(self, seed, inner0=0):
        p = [seed & M32]
        for i in range(1, N32):
            p.append((1812433253 * (p[-1] ^ (p[-1] >> 30)) + i) & M32)
        inner = inner0
        for i in range(4):
            inner ^= bin(p[i] & PARITY[i]).count("1") & 1
        self.inner = inner                         # what the next init_gen_rand of the process starts from
        if inner != 1:
            p[0] ^= 1                              # the lowest set bit of the parity vector
        self.w = [p[4 * i] | (p[4 * i + 1] << 32) | (p[4 * i + 2] << 64) | (p[4 * i + 3] << 96) for i in range(N)]
        self.idx = N32

    def _regenerate(self):
        w = self.w
        r1, r2 = w[N - 2], w[N - 1]
        for i in range(N):
            a, b = w[i], w[i + POS1 if i + POS1 < N else i + POS1 - N]
            w[i] = a ^ ((a << 8) & M128) ^ _lanes(lambda v, k: (v >> SR1) & MSK[k], b) ^ (r1 >> 8) ^ _lanes(lambda v, k: v << SL1, r2)
            r1, r2 = r2, w[i]

    def next64(self):
        if self.idx >= N32:
            self._regenerate()
            self.idx = 0
        v = (self.w[self.idx // 4] >> (32 * (self.idx % 4))) & M64
        self.idx += 2
        return v

    def res53(self, n):
        """the next n values of genrand_res53 (Python's int -> float rounds to nearest even, as DBLE does)"""
        return np.array([float(self.next64() >> 1) * (1.0 / 9223372036854775808.0) for _ in range(n)], dtype=np.float64)


def randn_from(u, n):
    """com_randn's Box-Muller over the uniforms u [2 * ceil(n / 2)]: n deviates"""
    u = np.asarray(u, dtype=np.float64).reshape(-1, 2)
    with np.errstate(divide="ignore"):
        r = np.sqrt(-2.0 * np.log(u[:, 0]))
    th = (2.0 * PI) * u[:, 1]
    out = np.empty(2 * len(u))
    out[0::2] = r * np.sin(th)
    out[1::2] = r * np.cos(th)
    return out[:n]


def randn(gen, n):
    """com_randn(n) from the generator gen: 2 * ceil(n / 2) uniforms consumed"""
    return randn_from(gen.res53(2 * ((n + 1) // 2)), n)
