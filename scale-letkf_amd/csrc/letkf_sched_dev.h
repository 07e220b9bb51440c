// letkf_sched_dev.h -- the dynamic run scheduling of the solve kernels (letkf_wave_dev.h: one run per unit; letkf_trio.hip:
// units of three runs): how a wave draws its next unit on the device, and how the host readies the counters for a launch
// and walks a plan for the tests.  The plan itself is made with the launch shape, in letkf_launch_shape.h.
#pragma once
#include <hip/hip_runtime.h>

#include <vector>

#include "letkf_launch_shape.h"

namespace letkf {

// Dynamic run scheduling (PointArgs::sched, PointArgs::plan).  The runs are handed out in UNITS of `ub` consecutive run
// ids (1 for runs of 16 points or more; short runs are bundled so that a draw covers ~16 points), and the units [0, n) are
// cut into 8 contiguous ranges, one per XCD -- the same ranges as the static dealing of round 1, so that neighbouring
// columns still meet in one L2.  Every wave (two-wave points: every workgroup) starts with a unit that is its own by its
// position in the grid -- no 2048 waves queueing at 8 counters when the kernel starts -- and then draws the next one from
// its XCD's counter (a device-scope load, so that a finished range costs no read-modify-write, then one atomicAdd by one
// lane); when that range is used up it takes units from the range that has most left.  A domain whose observations sit
// in one place (a radar disc: the columns outside have no observation and cost a hundredth of a column inside) left
// whole XCDs idle under the static dealing (C2-disc: 259 -> 147 ms).
// f units of every range (ub = 1 only) are handed out last and in quarters, so that the waves do not end a whole run (C2:
// a column of 60 points, 14 ms) apart: every t-th one, a sample spread over the range, so that the quarters carry the
// range's average work wherever its observations sit.  Which points start a quarter -- i.e. start cold -- is a fixed
// function of the launch shape, so results stay bitwise reproducible from run to run.
// A drawn unit is coded as 8 * unit id + (0: whole, 4 + s: quarter s of its run), -1: nothing left.
// Everything here is wave-uniform and written so that it stays in scalar registers (the plan comes from the kernel
// arguments; the one division is a multiplication by a host-made reciprocal): the first version did this arithmetic in
// lane 0's vector registers, and the vector registers it needed around every draw cost the kernel 250 B/lane of scratch
// and 50 GB of spill traffic per C2 launch.
__host__ __device__ __forceinline__ int sched_unit(const SchedPlan& P, const int x, const int i) {
  const int whole = P.whole[x], f = P.f[x], t = P.t[x], base = P.base[x];
  if (i < whole) {
    const int head = f * (t - 1);
    if (i < head) {
      const int g = (int)(((unsigned long long)(unsigned)i * P.magic[x]) >> 40);   // i / (t - 1)
      return 8 * (base + g * t + (i - g * (t - 1)));
    }
    return 8 * (base + f * t + (i - head));
  }
  return 8 * (base + ((i - whole) >> 2) * t + (t - 1)) + 4 + ((i - whole) & 3);
}
// the same word in every lane, as a scalar
__device__ __forceinline__ int sched_peek(const unsigned* c) {
  return __builtin_amdgcn_readfirstlane((int)__hip_atomic_load(c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
}
__device__ __forceinline__ int sched_take(unsigned* c) {
  int i = 0;
  if ((threadIdx.x & 63) == 0) i = (int)atomicAdd(c, 1u);
  return __builtin_amdgcn_readfirstlane(i);
}
// called by a whole wave; slot = the wave's (workgroup's) position among those of its XCD, or -1 after its first unit
__device__ __forceinline__ int sched_next(const SchedPlan& P, unsigned* cnt, const int xcd, const int slot) {
  if (slot >= 0 && slot < P.nstat[xcd]) return sched_unit(P, xcd, slot);
  {
    const int dyn = P.whole[xcd] + 4 * P.f[xcd] - P.nstat[xcd];
    if (dyn > 0 && sched_peek(&cnt[16 * xcd]) < dyn) {
      const int i = sched_take(&cnt[16 * xcd]);
      if (i < dyn) return sched_unit(P, xcd, P.nstat[xcd] + i);
    }
  }
  // own range used up: help where most is left (so that all ranges end together, each with its quartered runs last)
#pragma unroll 1
  for (int tries = 0; tries < 64; ++tries) {
    int best = -1, most = 0;
#pragma unroll 1
    for (int x = 0; x < 8; ++x) {
      const int left = P.whole[x] + 4 * P.f[x] - P.nstat[x] - sched_peek(&cnt[16 * x]);
      if (left > most) {
        most = left;
        best = x;
      }
    }
    if (best < 0) return -1;
    const int i = sched_take(&cnt[16 * best]);
    if (i < P.whole[best] + 4 * P.f[best] - P.nstat[best]) return sched_unit(P, best, P.nstat[best] + i);
  }
  return -1;
}

// host (include/letkf_amd.h, letkf_sched_plan_check): every run exactly once, whole or as four quarters?  0, or what failed
inline int sched_plan_check(long npts, long stride, int run_len, int grid, int ppw, int resident_per_xcd, int ub_of) {
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

// host, before the launch: the counters start at zero where the shape's plan draws from them
inline hipError_t sched_reset_counters(const LaunchShape& s, unsigned* sched, hipStream_t st) {
  return s.reset_counters ? hipMemsetAsync(sched, 0, 512, st) : hipSuccess;
}

}  // namespace letkf
