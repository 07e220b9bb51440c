// letkf_wave.hip -- the one-wave instantiations (k <= 62) of the solve kernel of letkf_wave_dev.h, and the host helpers of the
// wave route: which calls it serves, instantiation and launch shape for a k, the host-side check of a scheduling plan.
// (The two-wave instantiations are letkf_wave2.hip; the device helpers shared with other units are letkf_lane_dev.h and
// letkf_sched_dev.h.)
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstdlib>
#include <vector>

#include "letkf_wave_dev.h"

namespace letkf {

// include/letkf_amd.h, letkf_sched_plan_check: every run exactly once (whole or as four quarters)?
int sched_plan_check(long npts, long stride, int run_len, int grid, int ppw, int resident_per_xcd, int ub_of) {
  if (npts < 0 || grid < 1 || ppw < 1 || run_len < 1 || ub_of < 1) return -1;
  SchedPlan P;
  sched_make_plan(P, npts, stride, run_len, grid, ppw, resident_per_xcd, ub_of);
  if (P.nruns > (1L << 27)) return -2;
  if (P.ub % ub_of != 0) return -9;                            // (letkf_trio.hip: units are whole multiples of three runs)
  std::vector<unsigned char> seen((size_t)P.nruns, 0);   // bit 7: whole, bits 0-3: quarters
  for (int x = 0; x < 8; ++x) {
    if (P.nstat[x] < 0 || P.nstat[x] > P.whole[x] + 4 * P.f[x]) return -3;
    for (int i = 0; i < P.whole[x] + 4 * P.f[x]; ++i) {
      const int code = sched_unit(P, x, i);
      const long u = code >> 3;
      for (long rid = u * P.ub; rid < (u + 1) * P.ub && rid < P.nruns; ++rid) {
        if (rid < 0) return -4;
        const unsigned char bit = (code & 4) ? (unsigned char)(1u << (code & 3)) : (unsigned char)0x80;
        if ((code & 4) && P.ub != 1) return -5;
        if (seen[(size_t)rid] & (bit | ((code & 4) ? 0x80 : 0x0f))) return -6;    // handed out twice
        seen[(size_t)rid] |= bit;
      }
      if (u * P.ub >= P.nruns) return -7;                                          // a unit beyond the last run
    }
  }
  for (long rid = 0; rid < P.nruns; ++rid)
    if (seen[(size_t)rid] != 0x80 && seen[(size_t)rid] != 0x0f) return -8;         // missed, or quartered in part
  return 0;
}

bool wave_kernel_supports(int k, int nv, int mode) {
  // one wave per point up to k = 62 (k + 2 augmented Gram columns in 64 lanes); two waves for 63..100 (at k >= 65 the
  // half-columns no longer fit the 256 VALU-addressable VGPRs three times over and part of them lives in AGPRs)
  if (k > 100) return false;
  if (mode == 2 || mode == 3) return nv == 11 && k <= 62;   // the fused search / the column-survivor mode are written for one wave per point
  if (mode == 0) return nv == 11;
  return nv == 0;
}

int wave_kernel_kr(int k);
static int wave_kr(int k) { return wave_kernel_kr(k); }
int wave_kernel_kr(int k) {
  return k <= 16 ? 16 : k <= 20 ? 20 : k <= 32 ? 32 : k <= 48 ? 48 : k <= 50 ? 50 : k <= 62 ? 64 : k <= 64 ? 64 : k <= 80 ? 80 : 100;
}
int wave_kernel_nw(int k) { return k <= 62 ? 1 : 2; }

// Launch shape of the wave kernel: run length of the warm-started runs, grid, and the bytes of warm-start workspace
// (one [KR][64] slot per resident-or-not wave of the grid).  run_req: 0 = library default, 1 = every point cold,
// n > 1 = runs of n points.
void wave_launch_shape(int k, int mode, long npts, int num_cu, int run_req, long stride, int* run_len, int* grid,
                       size_t* ws_bytes) {
  const bool one_wave = wave_kernel_nw(k) == 1;
  const long ppw = one_wave ? 4 : 1;           // points in flight per workgroup
  int R = 1;
  if (mode != 1) {
    if (run_req > 0) R = run_req;
    else {
      // runs of 16 (first point of a run is a cold start), shortened until there are >= 4 workgroups per CU
      long r = npts / (ppw * num_cu * 4);
      R = (int)(r < 1 ? 1 : r > 16 ? 16 : r);
    }
    if (R > 4096) R = 4096;
  }
  if (stride < 1) stride = 1;
  const long nA = npts / stride;
  // strided runs (up a column): the whole column in one run by default -- one cold start per column, and the wave stays
  // with one set of observation rows (C2, 60 levels: 401 ms against 426 ms for runs of 30 and 457 ms for runs of 16
  // along ij)
  if (mode != 1 && run_req <= 0 && stride > 1) R = (int)(nA < 128 ? nA : 128);
  if (R > nA) R = (int)(nA > 0 ? nA : 1);      // (a run does not leave its column)
  const long nwg = (stride * ((nA + R - 1) / R) + ppw - 1) / ppw;
  long g = (long)num_cu * 16;   // 8x oversubscribed: the static block stride balances better (measured 573 ms at 2x, 541 at 16x)
#ifdef LETKF_WAVE_PROF
  if (const char* e = std::getenv("LETKF_AMD_WAVE_GRID")) g = (long)num_cu * std::atoi(e);   // PROF twin only
#endif
  *grid = (int)(nwg < g ? (nwg > 0 ? nwg : 1) : g);
  *run_len = R;
  // one [KR][lanes of a point] slot per wave-group of the grid
  *ws_bytes = (R > 1) ? (size_t)*grid * ppw * (size_t)wave_kr(k) * (one_wave ? 64 : 128) * sizeof(double) : 0;
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
