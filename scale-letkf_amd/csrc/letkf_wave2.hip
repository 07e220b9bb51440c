// letkf_wave2.hip -- the two-wave instantiations (63 <= k <= 100) of the solve kernel of letkf_wave_dev.h.  A unit of their own:
// they take hipcc's max-memory-clause scheduling strategy (Makefile FLAGS_letkf_wave2: k = 100 +5 %, measured A/B; the one-wave
// kernels lose 1 % with it), and the two units compile side by side.
#include <hip/hip_runtime.h>

#include "letkf_wave_dev.h"

namespace letkf {

hipError_t launch_wave_kernel_two(const PointArgs& a, int num_cu, hipStream_t st) {
  const int k = a.k;
  const bool kkout = a.trans_out || a.pa_out;
  LETKF_WAVE_CASE(64, 2)
  LETKF_WAVE_CASE(80, 2)
  LETKF_WAVE_CASE(100, 2)
  return hipErrorInvalidValue;
}
#undef LETKF_WAVE_CASE

}  // namespace letkf
