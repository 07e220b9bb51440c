// letkf_sfmt.cpp -- SFMT19937 on the host, written from the published algorithm (M. Saito, M. Matsumoto, "SIMD-oriented Fast
// Mersenne Twister", MCQMC 2006; parameter set 19937) and from how the reference's port behaves (common/SFMT.f90), as
// include/letkf_amd_obsmake.h states it.  The recurrence is serial -- word i needs words i - 1 and i - 2 -- so it stays on the
// host; the device does Box-Muller (letkf_obsmake.hip).
#include "letkf_sfmt.h"

namespace letkf {
namespace {

constexpr int kPos1 = 122, kSl1 = 18, kSr1 = 11;                                   // SL2 = SR2 = 1 byte, as 64-bit shifts below
constexpr uint32_t kMsk[4] = {0xdfffffefu, 0xddfecb7fu, 0xbffaffffu, 0xbffffff6u};
constexpr uint32_t kParity[4] = {0x00000001u, 0x00000000u, 0x00000000u, 0x13c9e684u};

// r = a ^ (a << 8 as 128 bits) ^ ((b >> 11 per 32-bit lane) & mask) ^ (c >> 8 as 128 bits) ^ (d << 18 per lane); r may be a
inline void recursion(uint32_t* r, const uint32_t* a, const uint32_t* b, const uint32_t* c, const uint32_t* d) {
  const uint64_t alo = a[0] | ((uint64_t)a[1] << 32), ahi = a[2] | ((uint64_t)a[3] << 32);
  const uint64_t clo = c[0] | ((uint64_t)c[1] << 32), chi = c[2] | ((uint64_t)c[3] << 32);
  const uint64_t xlo = alo << 8, xhi = (ahi << 8) | (alo >> 56);
  const uint64_t ylo = (clo >> 8) | (chi << 56), yhi = chi >> 8;
  const uint32_t x[4] = {(uint32_t)xlo, (uint32_t)(xlo >> 32), (uint32_t)xhi, (uint32_t)(xhi >> 32)};
  const uint32_t y[4] = {(uint32_t)ylo, (uint32_t)(ylo >> 32), (uint32_t)yhi, (uint32_t)(yhi >> 32)};
  for (int k = 0; k < 4; ++k) r[k] = a[k] ^ x[k] ^ ((b[k] >> kSr1) & kMsk[k]) ^ y[k] ^ (d[k] << kSl1);
}

}  // namespace

void Sfmt::seed(uint32_t s) {
  w[0] = s;
  for (int i = 1; i < kN32; ++i) w[i] = 1812433253u * (w[i - 1] ^ (w[i - 1] >> 30)) + (uint32_t)i;
  idx = kN32;
  // period certification, with the flag of a process's first call (0): an even parity flips the lowest set bit of the vector
  uint32_t inner = 0;
  for (int i = 0; i < 4; ++i) inner ^= w[i] & kParity[i];
  for (int sh = 16; sh > 0; sh >>= 1) inner ^= inner >> sh;
  if (!(inner & 1u)) w[0] ^= 1u;
}

void Sfmt::regenerate() {
  const uint32_t *r1 = &w[4 * (kN - 2)], *r2 = &w[4 * (kN - 1)];
  for (int i = 0; i < kN; ++i) {
    const int j = i + kPos1 < kN ? i + kPos1 : i + kPos1 - kN;
    recursion(&w[4 * i], &w[4 * i], &w[4 * j], r1, r2);
    r1 = r2;
    r2 = &w[4 * i];
  }
}

void Sfmt::res53(int64_t n, double* out) {
  for (int64_t k = 0; k < n; ++k) {
    if (idx >= kN32) {
      regenerate();
      idx = 0;
    }
    const uint64_t v = w[idx] | ((uint64_t)w[idx + 1] << 32);
    idx += 2;
    out[k] = (double)(v >> 1) * (1.0 / 9223372036854775808.0);      // uint64 -> double rounds to nearest even, as DBLE does
  }
}

}  // namespace letkf
