// letkf_mapproj.hip -- the map projection on the device (include/letkf_amd_mapproj.h): three kernels, a lane per row (or grid
// point) with a grid-stride loop, around the inline functions of letkf_mapproj_point.h.
//   phys2ij_kernel        lon / lat in degrees to ri / rj and, where asked for, rotc: 16 B read, 16 or 32 B written per row
//   ij2phys_kernel        ri / rj to lon / lat in degrees, rotc from the longitude it returns
//   mapproj_grid_kernel   the loop of common_mpi_scale.f90:193-203 over a subdomain's points
// The projection's constants are a kernel argument (a uniform struct: scalar registers).  Loads and stores are 8 B per lane and
// coalesced, rotc is one 16 B store per lane.  No LDS, no atomics, no shared counter: every value has one writer.  Built with
// -ffp-contract=off and without fast-math: each step rounds as the header writes it, through the double-precision device
// functions tan, pow, sincos, atan2, hypot and atan.
#include <hip/hip_runtime.h>

#include "letkf_mapproj_dev.h"
#include "letkf_mapproj_point.h"

namespace letkf {
namespace {

constexpr int kBlock = 256;
constexpr int64_t kMaxBlocks = 2048;   // 8 per CU of 256: a pass of the loop is 524 288 lanes
typedef double v2d __attribute__((ext_vector_type(2)));   // rotc's pair: 16-byte aligned (the entry tests it), one store

__global__ void __launch_bounds__(kBlock) phys2ij_kernel(letkf_mapproj p, int64_t n, const double* __restrict__ lon,
                                                         const double* __restrict__ lat, double* __restrict__ ri, double* __restrict__ rj,
                                                         v2d* __restrict__ rotc) {
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  for (int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x; r < n; r += stride) {
    double i, j, r0, r1;
    mapproj::phys2ij_point(p, lon[r], lat[r], &i, &j, &r0, &r1);
    ri[r] = i;
    rj[r] = j;
    if (rotc) rotc[r] = v2d{r0, r1};
  }
}

__global__ void __launch_bounds__(kBlock) ij2phys_kernel(letkf_mapproj p, int64_t n, const double* __restrict__ ri,
                                                         const double* __restrict__ rj, double* __restrict__ lon, double* __restrict__ lat,
                                                         v2d* __restrict__ rotc) {
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  for (int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x; r < n; r += stride) {
    double lo, la;
    mapproj::ij2phys_point(p, ri[r], rj[r], &lo, &la);
    lon[r] = lo;
    lat[r] = la;
    if (rotc) {
      double r0, r1;
      mapproj::rotc_at(p, lo, la, &r0, &r1);
      rotc[r] = v2d{r0, r1};
    }
  }
}

__global__ void __launch_bounds__(kBlock) mapproj_grid_kernel(letkf_mapproj p, int32_t nlon, int32_t npoint, int32_t ihalo, int32_t jhalo,
                                                              double cx1, double cy1, double* __restrict__ lon2d, double* __restrict__ lat2d,
                                                              v2d* __restrict__ rotc2d) {
  const int32_t stride = (int32_t)gridDim.x * kBlock;
  for (int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x; t < npoint; t += stride) {
    const int32_t j = (int32_t)t / nlon, i = (int32_t)t - j * nlon;
    const double ri = (double)(i + 1 + ihalo), rj = (double)(j + 1 + jhalo);           // :196-197
    double lo, la;
    mapproj::xy2phys_point(p, (ri - 1.0) * p.dx + cx1, (rj - 1.0) * p.dy + cy1, &lo, &la);
    if (lon2d) lon2d[t] = lo;
    if (lat2d) lat2d[t] = la;
    if (rotc2d) {
      double r0, r1;
      mapproj::rotc_at(p, lo, la, &r0, &r1);
      rotc2d[t] = v2d{r0, r1};
    }
  }
}

dim3 blocks_for(int64_t n) {
  const int64_t b = (n + kBlock - 1) / kBlock;
  return dim3((unsigned)(b < kMaxBlocks ? b : kMaxBlocks));
}

}  // namespace

hipError_t phys2ij_run(hipStream_t st, const letkf_mapproj& p, int64_t n, const double* lon, const double* lat, double* ri, double* rj,
                       double* rotc) {
  hipLaunchKernelGGL(phys2ij_kernel, blocks_for(n), dim3(kBlock), 0, st, p, n, lon, lat, ri, rj, reinterpret_cast<v2d*>(rotc));
  return hipGetLastError();
}

hipError_t ij2phys_run(hipStream_t st, const letkf_mapproj& p, int64_t n, const double* ri, const double* rj, double* lon, double* lat,
                       double* rotc) {
  hipLaunchKernelGGL(ij2phys_kernel, blocks_for(n), dim3(kBlock), 0, st, p, n, ri, rj, lon, lat, reinterpret_cast<v2d*>(rotc));
  return hipGetLastError();
}

hipError_t mapproj_grid_run(hipStream_t st, const letkf_mapproj& p, int32_t nlon, int32_t nlat, int32_t ihalo, int32_t jhalo, double cx1,
                            double cy1, double* lon2d, double* lat2d, double* rotc2d) {
  const int32_t npoint = nlon * nlat;                  // (the entry refused 2^31 or more)
  hipLaunchKernelGGL(mapproj_grid_kernel, blocks_for(npoint), dim3(kBlock), 0, st, p, nlon, npoint, ihalo, jhalo, cx1, cy1, lon2d, lat2d,
                     reinterpret_cast<v2d*>(rotc2d));
  return hipGetLastError();
}

}  // namespace letkf
