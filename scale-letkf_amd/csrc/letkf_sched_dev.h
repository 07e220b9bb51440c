// letkf_sched_dev.h -- the dynamic run scheduling of the solve kernels (letkf_wave_dev.h: one run per unit; letkf_trio.hip:
// units of three runs): how a wave draws its next unit on the device, and how the host makes the plan and readies the
// counters for a launch.  sched_plan_check (letkf_wave.hip) walks a plan on the host for the tests.
#pragma once
#include <hip/hip_runtime.h>

#include "letkf_device.h"

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

// host: the plan for a grid of `grid` workgroups with ppw wave-slots each, `resident` wave-slots in flight per XCD
inline void sched_make_plan(SchedPlan& P, const long npts, const long stride, const int run_len, const int grid, const int ppw,
                            const int resident_per_xcd, const int ub_of = 1) {
  const long S = stride > 1 ? stride : 1, rl = run_len > 1 ? run_len : 1;
  const long nruns = S * ((npts / S + rl - 1) / rl);
  // short runs are bundled (a draw should cover ~16 points), as long as that leaves every wave-slot of the grid four units
  int ub = rl >= 16 ? 1 : (int)((16 + rl - 1) / rl);
  const long most = nruns / (4L * grid * ppw);
  if (ub > most) ub = most < 1 ? 1 : (int)most;
  // ub_of > 1 (letkf_trio.hip: three runs are walked in step): whole multiples of it
  if (ub_of > 1) ub = (ub + ub_of - 1) / ub_of * ub_of;
  const long n = (nruns + ub - 1) / ub;
  // whole runs of 8 points or more may be quartered at the end of a range: as many as the XCD has wave-slots in flight
  const int fs = (ub == 1 && rl >= 8) ? ((long)grid * ppw / 8 < resident_per_xcd ? (int)((long)grid * ppw / 8) : resident_per_xcd) : 0;
  const int q = (int)(n >> 3), r = (int)(n & 7);
  for (int x = 0; x < 8; ++x) {
    const int len = q + (x < r ? 1 : 0);
    P.base[x] = x * q + (x < r ? x : r);
    P.f[x] = fs < len ? fs : len;
    P.whole[x] = len - P.f[x];
    P.t[x] = P.f[x] > 0 ? len / P.f[x] : 1;
    const long mine = (long)((grid - x + 7) >> 3) * ppw;              // wave-slots of the grid that sit on XCD x
    const long units = (long)P.whole[x] + 4L * P.f[x];
    P.nstat[x] = (int)(mine < units ? mine : units);
    P.magic[x] = P.t[x] > 1 ? ((1ull << 40) / (unsigned long long)(P.t[x] - 1)) + 1ull : 0ull;
  }
  P.ub = ub;
  P.nruns = nruns;
}

// host, after sched_make_plan and before the launch: the counters start at zero -- unless every unit is given out by position
// (a small batch): then nothing is drawn, and whatever non-negative counts an earlier launch left behind read as "nothing left"
inline hipError_t sched_reset_counters(const SchedPlan& P, unsigned* sched, hipStream_t st) {
  bool draws = false;
  for (int x = 0; x < 8; ++x) draws = draws || P.whole[x] + 4 * P.f[x] > P.nstat[x];
  return draws ? hipMemsetAsync(sched, 0, 512, st) : hipSuccess;
}

}  // namespace letkf
