// The launch shape of the register kernels for a list of cases, and the walk of every plan among them: the stand-alone
// program of tests/test_launch_shape.py (host code only; includes the library's headers, links nothing of it).
//   launch_shape_cases CASES   reads "trio k mode npts stride run_req num_cu resident dynamic grid_per_cu" per line and
//   prints per case every field of the shape, the plan, and for a case with a plan: whether the plan that sched_plan_check
//   makes from the shape's own numbers is the shape's (1), and what sched_plan_check answers for them (0 = every run handed
//   out exactly once, whole or as four quarters).
#include <cstdio>

#include "letkf_sched_dev.h"

int main(int argc, char** argv) {
  using namespace letkf;
  FILE* f = argc == 2 ? std::fopen(argv[1], "r") : nullptr;
  if (!f) return 2;
  int trio, k, mode, run_req, num_cu, resident, dynamic, grid_per_cu;
  long npts, stride;
  while (std::fscanf(f, "%d %d %d %ld %ld %d %d %d %d %d", &trio, &k, &mode, &npts, &stride, &run_req, &num_cu, &resident, &dynamic,
                     &grid_per_cu) == 10) {
    const LaunchShape s = launch_shape(trio != 0, k, mode, npts, stride, run_req, num_cu, resident, dynamic != 0, grid_per_cu);
    const SchedPlan& P = s.plan;
    std::printf("%d %d %d %zu %d %d %d %d", s.run_len, s.grid, s.grid_ws, s.warm_bytes, s.ppw, s.resident_per_xcd, s.ub_of,
                (int)s.reset_counters);
    for (const int* a : {P.base, P.whole, P.f, P.t, P.nstat})
      for (int x = 0; x < 8; ++x) std::printf(" %d", a[x]);
    for (int x = 0; x < 8; ++x) std::printf(" %llu", P.magic[x]);
    std::printf(" %d %ld", P.ub, P.nruns);
    int same = 0, walk = 0;
    if (dynamic && resident > 0) {
      walk = sched_plan_check(npts, stride, s.run_len, s.grid, s.ppw, s.resident_per_xcd, s.ub_of);
      if (walk != -1) {   // (-1: it refused the numbers and made no plan)
        SchedPlan Q;
        sched_make_plan(Q, npts, stride, s.run_len, s.grid, s.ppw, s.resident_per_xcd, s.ub_of);
        same = Q.ub == P.ub && Q.nruns == P.nruns;
        for (int x = 0; x < 8; ++x)
          same = same && Q.base[x] == P.base[x] && Q.whole[x] == P.whole[x] && Q.f[x] == P.f[x] && Q.t[x] == P.t[x] &&
                 Q.nstat[x] == P.nstat[x] && Q.magic[x] == P.magic[x];
      }
    }
    std::printf(" %d %d\n", same, walk);
  }
  std::fclose(f);
  return 0;
}
