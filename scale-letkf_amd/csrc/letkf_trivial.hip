// letkf_trivial.hip -- the grid points of the das_letkf loop body (scale/letkf/letkf_tools.f90:313-527) that have nothing
// to solve, as ONE streaming pass with a thread per (point, variable):
//   * beta == 0 (letkf_tools.f90:333-359: above the radar top / outside the buffer zone): analysis = first guess;
//   * no local observation (common/common_letkf.f90:89-107): T = sqrt(rho) I, w-bar = 0 in closed form; what is left is
//     the relaxation, the beta blend, the q clamp and the class copy of the inflation slot (letkf_rules_dev.h).
// The register kernels (letkf_wave_dev.h) give such a point a whole wavefront, lane = member: with the reference's
// point-fastest state (gues3d(nij1, nlev, nens, nv3d)) every one of its 11 x (k + 1) state values is an 8-byte access
// npts * 8 bytes from the next -- 70 KB of cache lines fetched and as many written per point for 4.5 KB of data, ~30 us
// of a wave's time, nothing to hide it behind.  On a domain whose observations sit in a radar disc most points are of
// this kind (bench workload C2-disc: 71 % of the points, a quarter of the kernel time).  Here consecutive lanes are
// consecutive POINTS (of one variable): they read consecutive addresses of every member plane, so the pass runs at HBM speed.
// PointArgs::skip_trivial tells the solve kernel that these points are done.
//
// The arithmetic follows the solve kernel's closed-form branch (letkf_wave_dev.h, `!solved`) statement by statement.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "letkf_device.h"
#include "letkf_rules_dev.h"

// Two passes of the same kind for the host API: a thread per element, zero where the point has nothing to solve.
// (extern "C": a profile lists them under these plain names)
extern "C" {
namespace {
// transmd of letkf_core without depd (common/common_letkf.f90:97-99: zeroed at nobsl == 0 whatever depd is)
__global__ void zero_transmd_where_nobsl_is_zero(int64_t nbatch, int ne, const int32_t* __restrict__ nobsl,
                                                 double* __restrict__ transmd) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < nbatch * ne && nobsl[i / ne] == 0) transmd[i] = 0.0;
}

// reported observation counts: the reference does not run obs_local at beta = 0 (letkf_tools.f90:333-359)
__global__ void zero_where_beta_is_zero(int64_t n, const double* __restrict__ beta, int32_t* __restrict__ cnt) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n && beta[i] == 0.0) cnt[i] = 0;
}
}  // namespace
}  // extern "C"

namespace letkf {

using namespace rules_dev;

// One thread per (point, variable), points fastest: 11 x the threads of a thread-per-point pass and chains of 3 k instead
// of 33 k dependent accesses -- with few trivial points (C2-mini-disc: 3520 of them = 55 waves) the pass is bound by the
// latency of one thread's chain, not by bandwidth.  The member loops are unrolled by hand with their loads first: gues
// and anal are different buffers (trivial_pass_supports), which the compiler cannot know.
__global__ void __launch_bounds__(256) letkf_trivial_points_kernel(const PointArgs A) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const int nv = A.nv;
  if (idx >= A.npts * nv) return;
  const int v = (int)(idx / A.npts);
  const long pt = idx - (long)v * A.npts;
  const int n = (int)(A.obs_off[pt + 1] - A.obs_off[pt]);
  const double beta = A.beta ? A.beta[pt] : 1.0;
  if (n != 0 && beta != 0.0) return;
  const int k = A.k;
  const double km1 = (double)(k - 1);
  const bool inclass = in_class(A, v);
  const double* __restrict__ gv = A.gues + pt * A.sp + v * A.sv;
  double* __restrict__ av = A.anal + pt * A.sp + v * A.sv;
  const long sm = A.sm;
  constexpr int U = 10;                                // members in flight per thread

  if (beta == 0.0) {                                   // letkf_tools.f90:333-359
    if (inclass) {
      const double xm = gv[k * sm];
      for (int m0 = 0; m0 < k; m0 += U) {
        double x[U];
#pragma unroll
        for (int u = 0; u < U; ++u) x[u] = gv[(m0 + u < k ? m0 + u : k - 1) * sm];
#pragma unroll
        for (int u = 0; u < U; ++u)
          if (m0 + u < k) av[(m0 + u) * sm] = xm + x[u];
      }
      if (A.det_run) av[(k + 1) * sm] = gv[(k + 1) * sm];
      if (A.rtps_out) A.rtps_out[pt + A.infl_sv * (long)v] = 1.0;
    }
    if (v == 0) {
      if (A.status) A.status[pt] = 0;
      if (A.nsweep) A.nsweep[pt] = 0;
      if (A.nobs_out) A.nobs_out[pt] = 0;
    }
    return;
  }

  const bool qskip = q_update_skipped(A, A.gues + pt * A.sp + k * sm, A.sv);
  const double infl_old = solve_inflation(A, pt, nv, qskip);
  const double lam = km1 / infl_old;                   // every eigenvalue of A = (k-1)/rho I
  const Spectra sc = spectra(lam, km1, true);          // T = sqrt(rho) I, Pa = rho/(k-1) I
  if (v == 0) {
    if (A.status) A.status[pt] = spectrum_status(true, lam, lam);
    if (A.nsweep) A.nsweep[pt] = 0;
    if (A.nobs_out) A.nobs_out[pt] = 0;
  }
  if (!inclass) return;

  const bool skip = var_skipped(A, qskip, v);
  const double xm = gv[k * sm];
  const double parm = relax_parm(A, pt, v);
  double var_g = 0.0;
  if (wants_variances(A)) {                            // Pa = sc2 I
    for (int m0 = 0; m0 < k; m0 += U) {
      double x[U];
#pragma unroll
      for (int u = 0; u < U; ++u) x[u] = gv[(m0 + u < k ? m0 + u : k - 1) * sm];
#pragma unroll
      for (int u = 0; u < U; ++u)
        if (m0 + u < k) var_g = fma(x[u], x[u], var_g);
    }
  }
  const double cfv = relax_factor(A, parm, var_g, var_g * sc.sc2, km1);
  if (A.rtps_out) A.rtps_out[pt + A.infl_sv * (long)v] = rtps_reported(A, skip, cfv);
  const double cdv = rtpp_diag(A, parm);
  // one member's analysis value, w-bar = 0
  auto value = [&](const double x) { return skip ? xm + x : analysis_value(xm, x, beta, cfv * (sc.sc1 * x) + cdv * x, 0.0); };
  double q_mean = 0.0, q_sprd = 0.0;
  bool do_clamp = false;
  if (!skip && A.q_sprd_max > 0.0 && v == A.iv_q_first) {
    double s_ = 0.0;
    for (int m0 = 0; m0 < k; m0 += U) {
      double x[U];
#pragma unroll
      for (int u = 0; u < U; ++u) x[u] = gv[(m0 + u < k ? m0 + u : k - 1) * sm];
#pragma unroll
      for (int u = 0; u < U; ++u)
        if (m0 + u < k) s_ += value(x[u]);
    }
    q_mean = s_ / (double)k;
    double ss = 0.0;
    for (int m0 = 0; m0 < k; m0 += U) {
      double x[U];
#pragma unroll
      for (int u = 0; u < U; ++u) x[u] = gv[(m0 + u < k ? m0 + u : k - 1) * sm];
#pragma unroll
      for (int u = 0; u < U; ++u)
        if (m0 + u < k) {
          const double dq = value(x[u]) - q_mean;
          ss = fma(dq, dq, ss);
        }
    }
    q_sprd = sqrt(ss / km1) / q_mean;
    do_clamp = q_sprd > A.q_sprd_max;
  }
  for (int m0 = 0; m0 < k; m0 += U) {
    double x[U];
#pragma unroll
    for (int u = 0; u < U; ++u) x[u] = gv[(m0 + u < k ? m0 + u : k - 1) * sm];
#pragma unroll
    for (int u = 0; u < U; ++u)
      if (m0 + u < k) {
        double val = value(x[u]);
        if (do_clamp) val = q_clamped(val, q_mean, val - q_mean, q_sprd, A.q_sprd_max);
        av[(m0 + u) * sm] = val;
      }
  }
  if (A.det_run) av[(k + 1) * sm] = gv[(k + 1) * sm];   // :489-497 with w-bar_det = 0
  // :396-398: the class copies its first slot (no observation: the value is unchanged); every parm of this point was
  // read by the thread that writes it
  if (A.infl_adaptive && !skip) A.infl[pt + A.infl_sv * (long)v] = infl_old;
}

// which launches may hand their trivial points to this pass: the list-driven loop body without per-point matrix outputs
// (and with an analysis buffer of its own: the pass re-reads a variable's first guess after writing its analysis)
bool trivial_pass_supports(const PointArgs& a) {
  return a.mode == 0 && a.nv > 0 && a.gues && a.anal && a.gues != a.anal && !a.trans_out && !a.pa_out && !a.transm_out && !a.transmd_out;
}

hipError_t launch_trivial_points(const PointArgs& a, hipStream_t st) {
  const unsigned grid = (unsigned)((a.npts * a.nv + 255) / 256);
  if (grid == 0) return hipSuccess;
  hipLaunchKernelGGL(letkf_trivial_points_kernel, dim3(grid), dim3(256), 0, st, a);
  return hipGetLastError();
}

hipError_t launch_zero_transmd_unobserved(int64_t nbatch, int ne, const int32_t* nobsl, double* transmd, hipStream_t st) {
  const int64_t n = nbatch * (int64_t)ne;
  hipLaunchKernelGGL(zero_transmd_where_nobsl_is_zero, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, nbatch, ne, nobsl, transmd);
  return hipGetLastError();
}

hipError_t launch_zero_counts_where_beta_is_zero(int64_t n, const double* beta, int32_t* cnt, hipStream_t st) {
  hipLaunchKernelGGL(zero_where_beta_is_zero, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, n, beta, cnt);
  return hipGetLastError();
}

}  // namespace letkf
