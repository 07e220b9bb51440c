// letkf_setup.hip -- what das_letkf derives before its loop (C ABI section 7) on the
// device: relax_beta and the inflation-field initialisation as streaming passes.  (The host half -- the variable-localisation
// classes, the merge groups of the obs-number limit and radar_only -- is in letkf_api_grid.hip.)
// scale/letkf/letkf_tools.f90:237-267, :1911-1948.

#include <hip/hip_runtime.h>

#include <cmath>

#include "letkf_device.h"

namespace letkf {

// relax_beta, letkf_tools.f90:1911-1948; dist_zero_fac is the single-precision literal of letkf_obs.f90:27
__global__ void relax_beta_kernel(const letkf_beta_params P, long nij1, long npts, const double* __restrict__ rig,
                                  const double* __restrict__ rjg, const double* __restrict__ hgt,
                                  double* __restrict__ beta) {
  const double zcut = P.radar_zmax + P.vert_local_radar * (double)3.651483717f;
  for (long p = blockIdx.x * (long)blockDim.x + threadIdx.x; p < npts; p += (long)gridDim.x * blockDim.x) {
    const long ij = p % nij1;
    double b = 1.0;
    if (P.radar_only && hgt[p] > zcut) {
      b = 0.0;
    } else if (P.boundary_buffer_width > 0.0) {
      const double ri = rig[ij], rj = rjg[ij];
      const double di = fmin(ri - (double)P.ihalo, (double)(P.nlong + P.ihalo + 1) - ri) * P.dx;
      const double dj = fmin(rj - (double)P.jhalo, (double)(P.nlatg + P.jhalo + 1) - rj) * P.dy;
      const double dist_bdy = fmin(di, dj) / P.boundary_buffer_width;
      if (dist_bdy < 1.0) b = fmax(dist_bdy, 0.0);
    }
    beta[p] = b;
  }
}

// letkf_tools.f90:237-267
__global__ void infl_init_kernel(long n, double* __restrict__ w, double infl_mul, double infl_mul_min) {
  for (long e = blockIdx.x * (long)blockDim.x + threadIdx.x; e < n; e += (long)gridDim.x * blockDim.x) {
    double v = infl_mul > 0.0 ? infl_mul : w[e];
    if (infl_mul_min > 0.0) v = fmax(v, infl_mul_min);
    w[e] = v;
  }
}

static unsigned stream_grid(long n, int num_cu) {
  long g = (n + 255) / 256;
  const long cap = (long)num_cu * 32;
  return (unsigned)(g < 1 ? 1 : g > cap ? cap : g);
}

hipError_t launch_relax_beta(const letkf_beta_params& p, long nij1, int nlev, const double* rig, const double* rjg,
                             const double* hgt, double* beta, int num_cu, hipStream_t st) {
  const long npts = nij1 * nlev;
  hipLaunchKernelGGL(relax_beta_kernel, dim3(stream_grid(npts, num_cu)), dim3(256), 0, st, p, nij1, npts, rig, rjg, hgt,
                     beta);
  return hipGetLastError();
}

hipError_t launch_infl_init(long n, double* w, double infl_mul, double infl_mul_min, int num_cu, hipStream_t st) {
  hipLaunchKernelGGL(infl_init_kernel, dim3(stream_grid(n, num_cu)), dim3(256), 0, st, n, w, infl_mul, infl_mul_min);
  return hipGetLastError();
}

}  // namespace letkf
