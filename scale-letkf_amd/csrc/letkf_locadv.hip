// letkf_locadv.hip -- localisation advection for EFSO: loc_advection (scale/letkf/efso_tools.f90:158-195, called from
//   efso.f90:136-156) in SCALE's grid frame.  Every point p = ij + nij1*lev gets its own search position, the column's
//   moved upstream by half the sum of the winds at the initial and the evaluation time over locadv_rate * eft hours:
//     ri[p] = rig[ij] - (0.5 * (u0[p] + u1[p])) * ci,   ci = locadv_rate * eft * 3600 / dx   (host)
//     rj[p] = rjg[ij] - (0.5 * (v0[p] + v1[p])) * cj,   cj = locadv_rate * eft * 3600 / dy
//   SCALE's positions are fractional grid indices on a Cartesian grid: the reference's 1/cos(lat), pole reflection and
//   longitude wrap (lon/lat of the GFS / SPEEDY grid) have no counterpart here.
//   No multiply-add fusion (the pragma below): the bits are those of the formula evaluated one IEEE operation at a time,
//   as numpy evaluates it.  A point whose position is not finite or moved by more than kLocAdvMaxCells is counted in *bad.
#include <hip/hip_runtime.h>

#include "letkf_device.h"

#pragma clang fp contract(off)

namespace letkf {

namespace {

__global__ void __launch_bounds__(256) efso_locadv_kernel(long nij1, long npts, const double* __restrict__ rig,
                                                          const double* __restrict__ rjg, const double* __restrict__ u0,
                                                          const double* __restrict__ v0, const double* __restrict__ u1,
                                                          const double* __restrict__ v1, double ci, double cj,
                                                          double* __restrict__ ri, double* __restrict__ rj,
                                                          unsigned* __restrict__ bad) {
  unsigned nbad = 0;
  for (long p = (long)blockIdx.x * blockDim.x + threadIdx.x; p < npts; p += (long)gridDim.x * blockDim.x) {
    const long ij = p % nij1;
    const double x0 = rig[ij], y0 = rjg[ij];
    const double x = x0 - (0.5 * (u0[p] + u1[p])) * ci;
    const double y = y0 - (0.5 * (v0[p] + v1[p])) * cj;
    ri[p] = x;
    rj[p] = y;
    // (false for NaN: a non-finite position or column counts as bad)
    const bool ok = fabs(x - x0) <= kLocAdvMaxCells && fabs(y - y0) <= kLocAdvMaxCells;
    nbad += ok ? 0u : 1u;
  }
  if (nbad) atomicAdd(bad, nbad);
}

}  // namespace

hipError_t launch_efso_locadv(long nij1, long npts, const double* rig, const double* rjg, const double* u0, const double* v0,
                              const double* u1, const double* v1, double ci, double cj, double* ri, double* rj,
                              unsigned* bad, int num_cu, hipStream_t st) {
  if (npts <= 0) return hipSuccess;
  const long nb = (npts + 255) / 256, cap = (long)num_cu * 32;
  hipLaunchKernelGGL(efso_locadv_kernel, dim3((unsigned)(nb < cap ? nb : cap)), dim3(256), 0, st, nij1, npts, rig, rjg, u0, v0,
                     u1, v1, ci, cj, ri, rj, bad);
  return hipGetLastError();
}

}  // namespace letkf
