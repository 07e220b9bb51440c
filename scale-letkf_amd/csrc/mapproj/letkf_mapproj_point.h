// letkf_mapproj_point.h -- the map projection at one point, as the kernels (letkf_mapproj.hip) and the host helpers
// (letkf_mapproj_entry.hip) both compile it: Lambert conformal conic on a sphere in SCALE-RM's parameterisation, and around it
// the reference's phys2ij / ij2phys with their 10-digit pi.  include/letkf_amd_mapproj.h states the mathematics; every line here
// is one step of it, in its order, and both units are built with -ffp-contract=off.  Internal.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#include "../../../include/letkf_amd_mapproj.h"

namespace letkf {
namespace mapproj {

constexpr double kPi = 3.14159265358979323846;           // the projection's
constexpr double kPiRef = LETKF_MAPPROJ_PI_REF;          // common/common.f90:28, the conversions'
constexpr double kRad2DegRef = 180.0 / kPiRef;           // common/common.f90:40

// dlam into [-pi, pi] by one turn; what is still outside (|dlam| > 3 pi, an infinity) is undefined: NaN
__host__ __device__ inline double wrap_once(double dl) {
  if (dl > kPi) dl -= 2.0 * kPi;
  else if (dl < -kPi) dl += 2.0 * kPi;
  return fabs(dl) <= kPi ? dl : NAN;
}

// (lam, phi) in radians to x, y and (cs, sn) = (cos, sin)(c dlam), which the rotation shares
__host__ __device__ inline void lc_forward(const letkf_mapproj& p, double lam, double phi, double* x, double* y, double* cs, double* sn) {
  double dl = wrap_once(lam - p.lon0);
  if (!(fabs(phi) <= kPi)) dl = NAN;                     // a latitude that is not finite leaves no rotation either
  const double h = p.hemisphere;
  const double rho = p.fact * p.radius * pow(tan((0.5 * kPi - h * phi) * 0.5), p.c);
  sincos(p.c * dl, sn, cs);
  *x = p.pole_x + rho * *sn;
  *y = p.pole_y - h * rho * *cs;
}

// alpha = -h c dlam: cos is even, sin odd
__host__ __device__ inline void lc_rotc(const letkf_mapproj& p, double cs, double sn, double* r0, double* r1) {
  *r0 = cs;
  *r1 = -p.hemisphere * sn;
}

__host__ __device__ inline void lc_inverse(const letkf_mapproj& p, double x, double y, double* lam, double* phi) {
  const double h = p.hemisphere, rf = p.radius * p.fact;
  const double xx = (x - p.pole_x) / rf, yy = -h * (y - p.pole_y) / rf;
  *lam = p.lon0 + atan2(xx, yy) / p.c;
  *phi = h * (0.5 * kPi - 2.0 * atan(pow(hypot(xx, yy), 1.0 / p.c)));
}

// phys2ij (common_obs_scale.f90:1257-1259): rlon * pi / 180.0 in that order
__host__ __device__ inline void phys2ij_point(const letkf_mapproj& p, double lon, double lat, double* ri, double* rj, double* r0, double* r1) {
  double x, y, cs, sn;
  lc_forward(p, lon * kPiRef / 180.0, lat * kPiRef / 180.0, &x, &y, &cs, &sn);
  *ri = (x - p.cxg1) / p.dx + 1.0;
  *rj = (y - p.cyg1) / p.dy + 1.0;
  lc_rotc(p, cs, sn, r0, r1);
}

// the rotation at a longitude in degrees (Trans_XtoY:396 from lon2d); lat only says whether there is a point
__host__ __device__ inline void rotc_at(const letkf_mapproj& p, double lon, double lat, double* r0, double* r1) {
  double dl = wrap_once(lon * kPiRef / 180.0 - p.lon0);
  if (!(fabs(lat) <= 180.0)) dl = NAN;
  double cs, sn;
  sincos(p.c * dl, &sn, &cs);
  lc_rotc(p, cs, sn, r0, r1);
}

// MPRJ_xy2lonlat and the two products by rad2deg (:1284-1287, common_mpi_scale.f90:198-200)
__host__ __device__ inline void xy2phys_point(const letkf_mapproj& p, double x, double y, double* lon, double* lat) {
  double lam, phi;
  lc_inverse(p, x, y, &lam, &phi);
  *lon = lam * kRad2DegRef;
  *lat = phi * kRad2DegRef;
}

// ij2phys (:1281-1287)
__host__ __device__ inline void ij2phys_point(const letkf_mapproj& p, double ri, double rj, double* lon, double* lat) {
  xy2phys_point(p, (ri - 1.0) * p.dx + p.cxg1, (rj - 1.0) * p.dy + p.cyg1, lon, lat);
}

}  // namespace mapproj
}  // namespace letkf
