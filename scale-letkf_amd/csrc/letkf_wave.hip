// letkf_wave.hip -- the one-wave instantiations (k <= 62) of the solve kernel of letkf_wave_dev.h, and the host helpers of the
// wave route: which calls it serves, the PROF twin's grid knob.
// (The two-wave instantiations are letkf_wave2.hip; the device helpers shared with other units are letkf_lane_dev.h and
// letkf_sched_dev.h.)
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstdlib>

#include "letkf_wave_dev.h"

namespace letkf {

bool wave_kernel_supports(int k, int nv, int mode) {
  // one wave per point up to k = 62 (k + 2 augmented Gram columns in 64 lanes); two waves for 63..100 (at k >= 65 the
  // half-columns no longer fit the 256 VALU-addressable VGPRs three times over and part of them lives in AGPRs)
  if (k > 100) return false;
  if (mode == 2 || mode == 3) return nv == 11 && k <= 62;   // the fused search / the column-survivor mode are written for one wave per point
  if (mode == 0) return nv == 11;
  return nv == 0;
}

int wave_grid_per_cu() {   // letkf_launch_shape.h, grid_ws
#ifdef LETKF_WAVE_PROF
  if (const char* e = std::getenv("LETKF_AMD_WAVE_GRID")) return std::atoi(e);   // PROF twin only
#endif
  return 16;
}

hipError_t launch_wave_kernel_two(const PointArgs& a, int num_cu, hipStream_t st);   // letkf_wave2.hip

hipError_t launch_wave_kernel(const PointArgs& a, int num_cu, hipStream_t st) {
  const int k = a.k;
  const bool kkout = a.trans_out || a.pa_out;
  LETKF_WAVE_CASE(16, 1)
  LETKF_WAVE_CASE(20, 1)   // MEMBER = 20: the reference's test configuration (BASELINE configs[0]); in the 32-row instantiation a third of the rows were padding
  LETKF_WAVE_CASE(32, 1)
  LETKF_WAVE_CASE(48, 1)
  LETKF_WAVE_CASE(50, 1)
  LETKF_WAVE_CASE(64, 1)
  return launch_wave_kernel_two(a, num_cu, st);
}
#undef LETKF_WAVE_CASE

}  // namespace letkf
