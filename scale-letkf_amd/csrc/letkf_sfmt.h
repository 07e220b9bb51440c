// letkf_sfmt.h -- SFMT19937 (Saito and Matsumoto 2008) as com_rand / com_randn draw from it: the generator of one
// init_gen_rand(seed) of a fresh process, 64-bit outputs, and the reference's conversion to double (letkf_sfmt.cpp).  Host only.
#pragma once
#include <stdint.h>

namespace letkf {

struct Sfmt {
  static constexpr int kN = 156, kN32 = 4 * kN;   // 128-bit words of the state, 32-bit words
  uint32_t w[kN32];
  int idx;                                        // next 32-bit word; kN32: the state is used up

  void seed(uint32_t s);
  // the next n values of genrand_res53: the 64-bit output shifted right by one, ROUNDED to double, times 2^-63
  void res53(int64_t n, double* out);

 private:
  void regenerate();
};

}  // namespace letkf
