// letkf_rules_dev.h -- the per-point scalar rules of the das_letkf loop body (scale/letkf/letkf_tools.f90:313-527) that every
// solver route applies around its eigen-decomposition, each defined once for every unit: the q-update skip, the class mask,
// the inflation slot, the RTPP / RTPS relaxation, the analysis value, the q-spread clamp, the adaptive inflation, the status
// of the eigen-solve.  Plain scalars and PointArgs only: no LDS, no reduction, no lane logic -- the kernels compute var_g,
// var_a, q_mean and the other sums in their own way.  Device code only; everything is inlined.
#pragma once
#include <hip/hip_runtime.h>

#include "letkf_device.h"

namespace letkf {
namespace rules_dev {

// letkf_tools.f90:333-359: below q_update_top (pressure of the first-guess mean) the moisture variables keep their first
// guess.  xmean: the point's means, sv doubles from one variable to the next; read only when the rule is switched on.
__device__ __forceinline__ bool q_update_skipped(const PointArgs& A, const double* xmean, const long sv) {
  return A.q_update_top > 0.0 && xmean[A.iv_p * sv] < A.q_update_top;
}
__device__ __forceinline__ bool var_skipped(const PointArgs& A, const bool qskip, const int v) { return qskip && v >= A.iv_q_first && v <= A.iv_q_last; }
// variables of this variable-localisation class (letkf_tools.f90:387-418) ...
__device__ __forceinline__ bool in_class(const PointArgs& A, const int v) { return (A.var_mask >> v) & 1u; }
// ... and those of them the point updates
__device__ __forceinline__ bool var_updated(const PointArgs& A, const bool qskip, const int v) { return in_class(A, v) && !var_skipped(A, qskip, v); }
// the first of them: its inflation slot is the rho of the point's solve (nv: none, rho = 1), and after an adaptive update
// every updated variable of the class gets that slot's new value (:396-398)
__device__ __forceinline__ int first_updated_var(const PointArgs& A, const int nv, const bool qskip) {
  int v0 = 0;
  while (v0 < nv && !var_updated(A, qskip, v0)) ++v0;
  return v0;
}
__device__ __forceinline__ double solve_inflation(const PointArgs& A, const long pt, const int nv, const bool qskip) {
  const int v0 = first_updated_var(A, nv, qskip);
  return v0 < nv ? A.infl[pt + A.infl_sv * (long)v0] : 1.0;
}

// letkf_tools.f90:387-391: the relaxation refers to the inflated prior where RELAX_TO_INFLATED_PRIOR is set.  A variable's
// slot is read before the adaptive update writes it.
__device__ __forceinline__ double relax_parm(const PointArgs& A, const long pt, const int v) {
  return A.relax_to_inflated_prior ? A.infl[pt + A.infl_sv * (long)v] : 1.0;
}
// only RTPS needs var_g = |x'|^2 and var_a = x'^T Pa x' (letkf_tools.f90:1982-1989)
__device__ __forceinline__ bool wants_variances(const PointArgs& A) { return A.relax_alpha == 0.0 && A.relax_alpha_spread != 0.0; }
// factor on T x' (letkf_tools.f90:457-469): RTPP (:1953-1966), else RTPS (:1971-2002; a variable without spread keeps 1), else 1.
// relax_factor is the whole rule; a kernel that sums var_g and var_a only under RTPS branches itself and takes the two parts.
__device__ __forceinline__ double rtpp_factor(const PointArgs& A) { return A.relax_alpha != 0.0 ? 1.0 - A.relax_alpha : 1.0; }
__device__ __forceinline__ double rtps_factor(const PointArgs& A, const double parm, const double var_g, const double var_a, const double km1) {
  double cf = 1.0;
  if (var_g > 0.0 && var_a > 0.0) cf = A.relax_alpha_spread * sqrt(var_g * parm / (var_a * km1)) - A.relax_alpha_spread + 1.0;
  return cf;
}
__device__ __forceinline__ double relax_factor(const PointArgs& A, const double parm, const double var_g, const double var_a, const double km1) {
  if (A.relax_alpha != 0.0) return 1.0 - A.relax_alpha;
  if (A.relax_alpha_spread != 0.0) return rtps_factor(A, parm, var_g, var_a, km1);
  return 1.0;
}
// work3da (letkf_tools.f90:460-462): the RTPS factor of an updated variable, 1 otherwise
__device__ __forceinline__ double rtps_reported(const PointArgs& A, const bool skipv, const double cfv) { return (wants_variances(A) && !skipv) ? cfv : 1.0; }
// RTPP's term on x' itself, alpha sqrt(parm) (letkf_tools.f90:1960-1963); the second form reads the slot only under RTPP
__device__ __forceinline__ double rtpp_diag(const PointArgs& A, const double parm) { return A.relax_alpha != 0.0 ? A.relax_alpha * sqrt(parm) : 0.0; }
__device__ __forceinline__ double rtpp_diag(const PointArgs& A, const long pt, const int v) {
  return A.relax_alpha != 0.0 ? A.relax_alpha * sqrt(relax_parm(A, pt, v)) : 0.0;
}

// letkf_tools.f90:472-487: pert = the relaxed (T x')_m, sdot = x' . w-bar; beta blends with the first guess (:333-359)
__device__ __forceinline__ double analysis_value(const double xm, const double x, const double beta, const double pert, const double sdot) {
  return xm + beta * (pert + sdot) + (1.0 - beta) * x;
}
// letkf_tools.f90:500-513: the analysis spread of q relative to its mean is held at q_sprd_max; dq = val - q_mean
__device__ __forceinline__ double q_clamped(const double val, const double q_mean, const double dq, const double q_sprd, const double q_sprd_max) {
  return q_sprd > q_sprd_max ? q_mean + dq * q_sprd_max / q_sprd : val;
}

// common_letkf.f90:233-254: parm1 = sum dep^2 / rdiag, parm2 = trace(Ys^T Ys) / (k-1), parm3 = sum rloc; prior error
// variance of the estimate 0.04^2.  Every other use of rho at the point takes the old value.
__device__ __forceinline__ double adaptive_inflation(const double infl_old, const double parm1, const double parm2, const double parm3) {
  const double parm4 = (parm1 - parm3) / parm2 - infl_old;
  const double tq = (infl_old * parm2 + parm3) / parm2;
  const double sigma_o = 2.0 / parm3 * (tq * tq);
  const double gain = 0.04 * 0.04 / (sigma_o + 0.04 * 0.04);
  return infl_old + gain * parm4;
}

// common_mtx.f90:66-78 on the largest and smallest eigenvalue: 1 not converged, 2 no positive eigenvalue, 3 ratio below
// sqrt(DBL_EPSILON), else 0
__device__ __forceinline__ int spectrum_status(const bool converged, const double lmx, const double lmn) {
  int st = 0;
  if (!converged) st = 1;
  else if (!(lmx > 0.0)) st = 2;
  else if (lmn < lmx * 1.4901161193847656e-08) st = 3;
  return st;
}
// ... for the Jacobi solves: converging in the last permitted sweep is converged, and a cap below kMaxSweep
// (PointArgs::max_sweep) is the profiling knob's, which reports nothing
constexpr int kMaxSweep = 60;
__device__ __forceinline__ int eig_status(const int jconv, const int max_sweep, const double lmx, const double lmn) {
  return spectrum_status(!(!jconv && max_sweep >= kMaxSweep), lmx, lmn);
}

// spectra of T = V diag(sc1) V^T and Pa = V diag(sc2) V^T (common_letkf.f90:190-216); a padding column has none
struct Spectra { double sc1, sc2; };
__device__ __forceinline__ Spectra spectra(const double lam, const double km1, const bool colvalid) {
  return Spectra{colvalid ? sqrt(km1 / lam) : 0.0, colvalid ? 1.0 / lam : 0.0};
}

}  // namespace rules_dev
}  // namespace letkf
