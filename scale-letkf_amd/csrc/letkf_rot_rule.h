// letkf_rot_rule.h -- the magnitude tests of a Jacobi rotation, cos^2 = g2 / ab against a power of two, decided on the
// upper dwords of the two doubles with 32-bit integer instructions (letkf_jacobi_dev.h, jacobi_split on one wave).
// g2 = gamma^2 is the squared inner product of the two columns, ab the product of their squared norms.  The three rules
//   rotate   g2 > 2^-100 ab   (was 1e-30)        stop   g2 > 2^-80 ab   (was 1e-24)        early   g2 > 2^-54 ab   (was 1e-16)
// are heuristic magnitudes: they need neither a multiply nor 53 bits.  For a non-negative double the upper dword (sign,
// exponent, 20 mantissa bits) read as an integer grows with the value, and a factor 2^-e is e << 20 taken off it, so
//   hi(g2) - hi(ab) > -(e << 20)
// is the exact comparison of the two values truncated to 20 mantissa bits: it can differ from g2 > 2^-e ab only where
// g2 / (2^-e ab) is within 2^-20 of 1.  One subtraction serves all three rules (`margin`), one compare each (`exceeds`).
//
// What the floating-point comparison gave for free, and how the integers keep it without a select or a second compare:
//   g2 = 0 exceeds nothing, whatever ab is, ab = 0 too -- the lanes without a partner, the inert column of an odd k and two
//     zero columns have g2 = 0 exactly.  hi(ab) is raised to kRotExp << 20 first, so hi(g2) = 0 lies kRotExp << 20 below it
//     at the least.  (So does every g2 < 2^-1042, whose upper dword is 0.)
//   g2 = NaN or inf, of either sign, exceeds nothing: nothing can be rotated by it.  kBias carries their exponent field of all
//     ones into the sign bit, and the SATURATING subtraction leaves them at the bottom.
//   ab with the sign bit set -- a squared norm that the rotation identities rounded below zero -- passes every g2 from 2^-1022
//     on, as the comparison against a negative product did: the signed maximum reads it as the floor.
// ab = +inf or NaN fails every g2 < 2^(1023 - kRotExp) (in the iteration ab is not finite only where g2 is not either).
// The floor under hi(ab) is the price: a product 2^-e ab below 2^(kRotExp - e - 1023) is read as that, so that with
// ab < 2^(kRotExp - 1023) a g2 below 2^(kRotExp - e - 1022) may be decided either way -- squared cosines of columns whose
// norms are below 1e-139.  Everywhere else in the non-negative doubles the rule is the truncated comparison.
// Plain C++: a host compiler builds it alone (tests/test_rot_rule.py sweeps it there).
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define LETKF_ROT_HD __host__ __device__ __forceinline__
#else
#define LETKF_ROT_HD inline
#endif

#ifndef LETKF_ROT_EXP
#define LETKF_ROT_EXP 100
#endif
#ifndef LETKF_STOP_EXP
#define LETKF_STOP_EXP 80
#endif
#ifndef LETKF_EARLY_EXP
#define LETKF_EARLY_EXP 54
#endif

namespace letkf {
namespace rot_rule {

constexpr int kRotExp = LETKF_ROT_EXP;       // rotate when cos^2 > 2^-100 (7.9e-31 <= 1e-30)
constexpr int kStopExp = LETKF_STOP_EXP;     // not converged when cos^2 > 2^-80 (8.3e-25 <= 1e-24)
constexpr int kEarlyExp = LETKF_EARLY_EXP;   // no early stop when cos^2 > 2^-54 (5.6e-17 <= 1e-16)
static_assert(0 < kEarlyExp && kEarlyExp < kStopExp && kStopExp < kRotExp && kRotExp < 1023, "early within stop within rotate");
constexpr int32_t kBias = 1 << 20;           // one exponent step: a finite hi(g2) + kBias stays positive, inf and NaN do not
constexpr int32_t kFloor = kRotExp << 20;    // hi(ab) from below: no e <= kRotExp takes it past 0

// the limit a margin is compared with, for e <= kRotExp: exceeds(m, limit(e)) is hi(g2) - hi(ab) > -(e << 20)
LETKF_ROT_HD constexpr int32_t limit(const int e) { return kBias - (e << 20) + 1; }

LETKF_ROT_HD int32_t sub_sat(const int32_t x, const int32_t y) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_elementwise_sub_sat(x, y);      // v_sub_i32 ... clamp
#else
  const int64_t d = static_cast<int64_t>(x) - static_cast<int64_t>(y);
  return d > INT32_MAX ? INT32_MAX : d < INT32_MIN ? INT32_MIN : static_cast<int32_t>(d);
#endif
}

// hi(g2) + kBias - max(hi(ab), kFloor), saturating: three integer instructions
LETKF_ROT_HD int32_t margin(const int32_t hi_g2, const int32_t hi_ab) {
  const int32_t u = static_cast<int32_t>(static_cast<uint32_t>(hi_g2) + static_cast<uint32_t>(kBias));   // (wraps by design)
  const int32_t h = hi_ab > kFloor ? hi_ab : kFloor;
  return sub_sat(u, h);
}

LETKF_ROT_HD bool exceeds(const int32_t m, const int32_t lim) { return m >= lim; }

// the whole rule from the two doubles' upper dwords: g2 > 2^-e ab, e <= kRotExp
LETKF_ROT_HD bool gt_pow2(const int32_t hi_g2, const int32_t hi_ab, const int e) { return exceeds(margin(hi_g2, hi_ab), limit(e)); }

}  // namespace rot_rule
}  // namespace letkf
