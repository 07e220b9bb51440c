// letkf_obsanal.hip -- the analysis ensemble in observation space: das_letkf_obs, scale/letkf/letkf_tools.f90:933-1156
//   (commented out in the reference), which runs the LETKF at every observation's own location and keeps
//   obsanal(nn, m) = obsdat - obsdep + sum_k obshdxf(nn, k) * trans(k, m),  i.e.  H xbar^b + Y^b (wbar + T).
//
// The library reaches it through the existing loop body (letkf_das_points_dev semantics, :313-527) on a PSEUDO-STATE of
// one point per target row j of obsda_sort and two variables:
//   variable 0  the target itself:  members ensval[j*kld + m] (perturbations), mean ob_dat[j] - dep[j] (H xbar^b),
//               deterministic member ob_dat[j] - ensval[j*kld + k]
//   variable 1  the target's pressure rlev in the mean and det slots (perturbations 0): what Q_UPDATE_TOP compares
// and coordinates (ob_ri, ob_rj, and the vertical one by the target ctype's vmode).  The entry (letkf_api_das.hip) runs the
// search on those coordinates, the loop body with var_mask = 1 (variable 1 is never written), then the finish kernel.
//   obsanal_targets_kernel  one thread per target: ctype (the ctype block of ac_ext that holds the row), coordinates,
//                           pseudo-state, inflation; argument faults (a row outside [0, nobs) or outside every ctype
//                           block, a missing vertical coordinate) are ORed into a flag word the entry reads back
//   obsanal_finish_kernel   one thread per target: members, mean, perturbation table row, O - A
// Plain loads and stores, no atomics on floating-point data: a duplicate target writes the same bits to the same row.
#include <hip/hip_runtime.h>

#include "letkf_device.h"

namespace letkf {

namespace {

__global__ void __launch_bounds__(256) obsanal_targets_kernel(const ObsAnalArgs a) {
  const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= a.ntgt) return;
  const letkf_search_tables& s = a.tab;
  unsigned flag = 0;
  long row = a.tgt_row ? (long)a.tgt_row[t] : t;
  if (row < 0 || row >= a.nobs) {
    flag |= kObsAnalBadRow;
    row = 0;   // (a safe row: the call fails before anything reads what this target computes)
  }
  // the target's ctype, and which vertical coordinates the tables use at all
  int ic = -1;
  bool use_lev = a.q_top != 0, use_z = false;
  for (int c = 0; c < s.nctype; ++c) {
    const int vm = s.vmode[c];
    if (vm == 1) use_z = true;
    else use_lev = true;
    const long ni = s.ngrdext_i[c], nj = s.ngrdext_j[c];
    if (ni < 1 || nj < 1) continue;
    const int* ac = s.ac_ext + s.ac_off[c];
    if (row >= ac[0] && row < ac[(ni + 1) * nj - 1]) ic = c;
  }
  int vm = 0;
  if (ic < 0) flag |= kObsAnalNoCtype;
  else vm = s.vmode[ic];
  const double lev = s.ob_lev[row], dat = s.ob_dat[row];
  double rlev = a.rlev_tgt ? a.rlev_tgt[t] : 0.0, rz = a.rz_tgt ? a.rz_tgt[t] : 0.0;
  switch (vm) {
    case 1: rz = lev; break;               // radar (type 22): height
    case 2: rlev = dat; break;             // ps: the observed pressure (das_letkf_obs: rlev = obsdat)
    case 3: rlev = s.rain_base; break;     // rain: VERT_LOCAL_RAIN_BASE
    default: rlev = lev; break;            // pressure of the observation (H08 rows: their sensitive height, already in ob_lev)
  }
  if (vm == 1 && use_lev && !a.rlev_tgt) flag |= kObsAnalNoCoord;
  if (vm != 1 && use_z && !a.rz_tgt) flag |= kObsAnalNoCoord;
  a.ri[t] = s.ob_ri[row];
  a.rj[t] = s.ob_rj[row];
  a.rlev[t] = rlev;
  a.rz[t] = rz;
  // pseudo-state: element (t, m, v) at t + m * ntgt + v * ntgt * (k + 2)
  const int k = a.k;
  const long n = a.ntgt, sv = n * (long)(k + 2);
  const double* ev = a.ensval + row * a.kld;
  double* g = a.gues + t;
  for (int m = 0; m < k; ++m) {
    g[m * n] = ev[m];
    g[m * n + sv] = 0.0;
  }
  g[k * n] = dat - a.dep[row];
  g[(k + 1) * n] = a.det_run ? dat - ev[k] : 0.0;
  g[k * n + sv] = rlev;
  g[(k + 1) * n + sv] = rlev;
  const double rho = a.infl ? a.infl[t] : a.infl_mul;
  a.infl_ws[t] = rho;
  a.infl_ws[t + n] = rho;
  if (flag) atomicOr(a.flags, flag);
}

__global__ void __launch_bounds__(256) obsanal_finish_kernel(const ObsAnalArgs a) {
  const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= a.ntgt) return;
  const long row = a.tgt_row ? (long)a.tgt_row[t] : t;   // (in range: checked before the search ran)
  const int k = a.k;
  const long n = a.ntgt;
  const double* an = a.anal + t;
  double sum = 0.0;
  for (int m = 0; m < k; ++m) sum += an[m * n];
  const double mean = sum / (double)k;
  const double dat = a.tab.ob_dat[row];
  double* ya = a.ya + t * a.lda;
  double* yt = a.ya_table ? a.ya_table + row * a.kld : nullptr;
  for (int m = 0; m < k; ++m) {
    const double v = an[m * n];
    ya[m] = v;
    if (yt) yt[m] = v - mean;
  }
  if (a.det_run) {
    const double d = an[(k + 1) * n];
    ya[k] = d;
    if (yt) yt[k] = dat - d;   // (the table's convention for the det slot: a departure, like ensval(mmdetobs, :))
  }
  if (a.ya_mean) a.ya_mean[t] = mean;
  if (a.dep_a) a.dep_a[t] = dat - mean;
}

}  // namespace

hipError_t launch_obsanal_targets(const ObsAnalArgs& a, hipStream_t st) {
  if (a.ntgt <= 0) return hipSuccess;
  hipLaunchKernelGGL(obsanal_targets_kernel, dim3((unsigned)((a.ntgt + 255) / 256)), dim3(256), 0, st, a);
  return hipGetLastError();
}

hipError_t launch_obsanal_finish(const ObsAnalArgs& a, hipStream_t st) {
  if (a.ntgt <= 0) return hipSuccess;
  hipLaunchKernelGGL(obsanal_finish_kernel, dim3((unsigned)((a.ntgt + 255) / 256)), dim3(256), 0, st, a);
  return hipGetLastError();
}

}  // namespace letkf
