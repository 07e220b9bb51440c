// letkf_launch_shape.h -- the launch shape of the two register kernels (letkf_wave_kernel, k <= 100; letkf_trio_kernel,
// k <= 20), decided in one host function: run length of the warm-started runs, grid, scheduling plan, workspace bytes.
// Which points start cold is a function of this shape alone (letkf_sched_dev.h), so a rule changed here changes results:
// tests/test_launch_shape.py holds every field against recorded shapes and walks every plan, on a CPU.  Plain host C++.
#pragma once
#include "letkf_device.h"

namespace letkf {

inline int wave_kernel_kr(int k) {   // rows of the wave kernel's instantiation that serves k
  return k <= 16 ? 16 : k <= 20 ? 20 : k <= 32 ? 32 : k <= 48 ? 48 : k <= 50 ? 50 : k <= 64 ? 64 : k <= 80 ? 80 : 100;
}
inline int wave_kernel_nw(int k) { return k <= 62 ? 1 : 2; }   // ... and its wavefronts per point
constexpr int kTrioRuns = 3;   // runs (points) one wave of the trio kernel walks in step
#ifndef LETKF_SMALL_OCC
#define LETKF_SMALL_OCC 2      // workgroups per CU in the launch bounds of the KR <= 20 instantiations (letkf_wave_dev.h wave_occupancy)
#endif

// runs of run_len points in npts points of stride S: the points as an array [npts / S][S], a run walks the first index
inline long sched_nruns(const long npts, const long stride, const int run_len) {
  const long S = stride > 1 ? stride : 1, rl = run_len > 1 ? run_len : 1;
  return S * ((npts / S + rl - 1) / rl);
}

// the plan for a grid of `grid` workgroups with ppw wave-slots each, `resident` wave-slots in flight per XCD
inline void sched_make_plan(SchedPlan& P, const long npts, const long stride, const int run_len, const int grid, const int ppw,
                            const int resident_per_xcd, const int ub_of = 1) {
  const long rl = run_len > 1 ? run_len : 1;
  const long nruns = sched_nruns(npts, stride, run_len);
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

struct LaunchShape {
  int run_len;            // points per run, as the kernel walks them (PointArgs::run_len)
  int grid;               // workgroups launched
  int grid_ws;            // ... before the clamp to the resident ones (PointArgs::wave_grid): sizes the per-wave workspaces, bounds blockIdx.x in the CHECKED build
  size_t warm_bytes;      // warm-start workspace: one [KR][lanes of a point] slot per wave-group of grid_ws (trio: none, it parks in LDS)
  int ppw;                // wave-slots per workgroup (points in flight)
  int resident_per_xcd;   // wave-slots in flight per XCD (32 CUs) by the launch bounds: so many runs per range are quartered
  int ub_of;              // runs a wave walks in step: units are whole multiples of it
  SchedPlan plan;         // dynamic dealing with a known occupancy only, else zero
  bool reset_counters;    // the plan draws: zero the counters before the launch.  (Not when every unit is given out by position, a small
                          // batch: nothing is drawn then, and whatever non-negative counts an earlier launch left read as "nothing left".)
};

// The shape of one launch of the trio kernel (mode 0, k <= 20) or else the wave kernel, from the call's numbers:
//   run_req      0 = library default, 1 = every point cold, n > 1 = runs of n points.  A launcher passes the run length
//                prepare_wave got: the rules below leave a length they made as it is
//   resident     workgroups per CU (resident_blocks); 0 = not queried yet (prepare_wave sizes the workspaces before the launcher
//                asks): grid = grid_ws, no plan, the trio's runs at their full length -- as with dynamic = false, the PROF twin's
//                static dealing.  grid_per_cu: workgroups per CU of grid_ws (wave_grid_per_cu)
inline LaunchShape launch_shape(const bool trio, const int k, const int mode, const long npts, long stride, const int run_req,
                                const int num_cu, const int resident, const bool dynamic, const int grid_per_cu) {
  LaunchShape s{};
  const bool one_wave = wave_kernel_nw(k) == 1;
  const long ppw = s.ppw = one_wave ? 4 : 1;
  s.ub_of = trio ? kTrioRuns : 1;
  s.resident_per_xcd = trio ? 256 : one_wave ? 128 * (k <= 20 ? LETKF_SMALL_OCC : 2) : 64;
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
  const long nruns = sched_nruns(npts, stride, R), nwg = (nruns + ppw - 1) / ppw;
  // 8x oversubscribed, from the static dealing: its block stride balances better (measured 573 ms at 2x, 541 at 16x)
  const long g = (long)num_cu * grid_per_cu;
  s.run_len = R;
  s.grid = s.grid_ws = (int)(nwg < g ? (nwg > 0 ? nwg : 1) : g);
  if (!trio && R > 1) s.warm_bytes = (size_t)s.grid_ws * ppw * (size_t)wave_kernel_kr(k) * (one_wave ? 64 : 128) * sizeof(double);
  if (!dynamic || resident < 1) return s;

  // Dynamic scheduling: a grid of at most the workgroups that are resident together (every wave owns its first unit by
  // its position, the rest is drawn; a workgroup that had to wait for a slot would sit on its first unit until the others
  // have drawn everything else).
  const long res = (long)resident * num_cu;
  if (trio) {
    // a small domain (BASELINE configs[0]: 1600 columns of 30 levels) has fewer units of three whole runs than the GPU has
    // waves: shorter runs then (the first point of a run starts cold), down to 4 points, until there are two units per wave
    constexpr long kMinRun = 4, kUnitsPerWave = 2;
    long want = npts / (kTrioRuns * kUnitsPerWave * res * 4);
    if (want < kMinRun) want = kMinRun;
    if (s.run_len > want) s.run_len = (int)want;
    const long wgs = ((sched_nruns(npts, stride, s.run_len) + kTrioRuns - 1) / kTrioRuns + 3) / 4;   // a wave-slot per unit of three runs
    s.grid = (int)(wgs > res ? res : wgs < 1 ? 1 : wgs);
  } else {
    if (one_wave && nruns < 8 * res * ppw) {
      // A small batch (fewer than 8 runs per resident wave) on one-wave points: every wave gets exactly one run, by its
      // position, and the hardware starts the next workgroup when one is done.  Measured with the PROF twin on C2-mini
      // (2.25 runs per wave): of two waves on a SIMD the older one is served first and draws most of the runs, the
      // younger one is left with its last run when everything is drawn, alone on its SIMD -- 4.9 ms against 4.4 ms.
      const long need = 8 * (((nruns + 7) / 8 + ppw - 1) / ppw);
      if (s.grid > need) s.grid = (int)need;
    } else if (s.grid > res) s.grid = (int)res;
  }
  sched_make_plan(s.plan, npts, stride, s.run_len, s.grid, s.ppw, s.resident_per_xcd, s.ub_of);
  for (int x = 0; x < 8; ++x) s.reset_counters = s.reset_counters || s.plan.whole[x] + 4 * s.plan.f[x] > s.plan.nstat[x];
  return s;
}

}  // namespace letkf
