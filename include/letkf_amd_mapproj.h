/* letkf_amd_mapproj.h -- the map projection on the device: lon / lat to the grid coordinates ri / rj and back, and the rotation
 * rotc of the horizontal wind -- phys2ij and ij2phys (scale/common/common_obs_scale.f90:1241-1290), the degree / radian
 * conversions around MPRJ_rotcoef (:294, :396) and the grid loops scale/common/common_mpi_scale.f90:193-203 and
 * scale/obs/obsope_tools.f90:1090-1100.
 *
 * Companion of letkf_amd.h (which it includes for letkf_ctx).  The entries are exported by a library of their own,
 * libletkf_amd_mapproj.so, which links against libletkf_amd.so for the context, its stream and letkf_amd_last_error().  Their
 * outputs are what letkf_obs_file_rows.ri / rj, the rotc of letkf_obsope_dev and letkf_obsmake_slot_dev and the lon / lat / rotc
 * of letkf_obssim_dev take; the row-wise entries feed letkf_superob_dev and letkf_obsscan_dev.  DESIGN.md section 19.
 *
 * WHAT IS THE REFERENCE'S AND WHAT IS NOT.  The lines named above are in the reference's tree and are followed to the letter:
 * phys2ij passes rlon * pi / 180.0 (in that order), ij2phys and the grid loops multiply by rad2deg = 180.0 / pi, and that pi is
 * common/common.f90:28's 3.1415926535d0, a 10-digit value (LETKF_MAPPROJ_PI_REF).  Trans_XtoY passes lon * deg2rad, which is the
 * same real number and can differ from phys2ij's by the last bit; letkf_phys2ij_dev makes x, y and rotc from phys2ij's.
 * MPRJ_lonlat2xy, MPRJ_xy2lonlat, MPRJ_rotcoef and MPRJ_setup are SCALE-RM's and are not in the reference's tree: NO BIT-FOR-BIT
 * CLAIM AGAINST SCALE-RM IS MADE.  The contract for that part is the mathematics below, with the exact pi, checked against a
 * 50-digit evaluation (tests/_mapproj.py).
 *
 * THE PROJECTION: a spherical Earth, Snyder's Lambert conformal conic with two standard parallels in SCALE-RM's
 * parameterisation.  type 1 = LC; every other type (NONE, PS, MER, EC) and MPRJ_rotation are refused.
 * With D = pi / 180, h = the sign of lc_lat1 + lc_lat2, the colatitudes psi_i = pi/2 - h * lat_i * D (psi0 from basepoint_lat):
 *   c      = (ln sin psi1 - ln sin psi2) / (ln tan(psi1/2) - ln tan(psi2/2))
 *   fact   = sin psi1 / (c * tan(psi1/2)^c)
 *   pole   = (basepoint_x, basepoint_y + h * fact * radius * tan(psi0/2)^c)
 *   lon0   = basepoint_lon * D
 * FORWARD for (lam, phi) in radians:
 *   dlam = lam - lon0; above pi it loses 2 pi, below -pi it gains 2 pi, ONCE
 *   rho  = fact * radius * tan((pi/2 - h phi) / 2)^c
 *   x    = pole_x + rho sin(c dlam),  y = pole_y - h rho cos(c dlam)
 * ROTATION: alpha = -h c dlam, rotc = (cos alpha, sin alpha); the operator uses it as u * rotc[0] - v * rotc[1].
 * INVERSE of (x, y), with xx = (x - pole_x) / (radius * fact), yy = -h (y - pole_y) / (radius * fact):
 *   lam = lon0 + atan2(xx, yy) / c,  phi = h (pi/2 - 2 atan(hypot(xx, yy)^(1/c)))
 * GRID: ri = (x - cxg1) / dx + 1, rj = (y - cyg1) / dy + 1; x = (ri - 1) * dx + cxg1 on the way back.
 * Per point, each step is one double-precision operation or library function in the order written; no contraction, no
 * fast-math.  The derived constants are made once on the host with a 64-bit significand and rounded to double, so that each is
 * within an ulp of its real value: the error of c is multiplied by dlam in every sincos(c dlam).
 *
 * WHERE THE MATHEMATICS IS UNDEFINED -- decisions, nothing is clamped silently:
 *   a NaN in lon or lat gives NaN in ri, rj and rotc (both elements); so does a latitude that is not finite
 *   the pole of the other hemisphere (h phi = -pi/2) has rho = infinity: non-finite ri / rj, which letkf_obsscan_dev books outside
 *     the domain.  Through the degree entries lat = -h 90 becomes -h 90 * pi / 180 with the 10-digit pi, 4.5e-11 rad short of that
 *     pole: rho is then finite and huge (1e11 .. 1e15 m for c between 0.45 and 0.75), ri / rj outside every domain as well
 *   the near pole has rho = 0 and finite results; lat = h 90 in degrees lands the same 4.5e-11 rad short of it (rho of some metres)
 *   a latitude beyond a pole gives NaN in ri / rj
 *   |lon| beyond one wrap (|dlam| > 3 pi) gives NaN; an infinite lon does too.  A longitude given one turn away (-225 for 135) is
 *     NOT the same point to rounding: the conversion makes 2 * 3.1415926535 rad of 360 degrees and the wrap takes 2 pi off, which
 *     leaves 1.8e-10 rad, a millimetre.  That is the reference's conversion, kept
 *   at dlam = +-pi the cone is cut: x and y jump there, and which side a row within rounding of the cut takes is decided by the
 *     double-precision dlam
 * ij2phys' rotc is the rotation at the longitude it returns, as the reference makes it from lon2d (Trans_XtoY:396).
 *
 * letkf_mapproj_setup (host only, no device): the derived constants of p in *proj, a plain struct the other entries take.
 * letkf_phys2ij_dev: per row n, lon / lat (dev, degrees, as the files hold them) to ri / rj (dev) and, where rotc (dev [n][2]) is
 *   not NULL, the rotation.  One lane per row, one sincos for x, y and rotc; every value has one writer, results are bitwise equal
 *   from call to call.  Asynchronous on the context's stream.
 * letkf_ij2phys_dev: per row, ri / rj to lon / lat in degrees; rotc optional.
 * letkf_mapproj_grid_dev: the loop of common_mpi_scale.f90:193-203 for a subdomain of nlon x nlat points with halos ihalo, jhalo
 *   whose GRID_CX(1) / GRID_CY(1) are cx1 / cy1: ri = i + IHALO, x = (ri - 1) * dx + cx1, times rad2deg.  lon2d, lat2d: dev
 *   [nlat][nlon]; rotc2d: dev [nlat][nlon][2] -- the layouts letkf_obssim_dev takes.  Each may be NULL, not all three.
 * letkf_phys2ij_host, letkf_ij2phys_host: one point on the host from the same inline functions the kernels use (a radar site, a
 *   namelist position); rotc is [2] or NULL.  Host and device math libraries differ: agreement is to a few ulp, not bitwise.
 *
 * REFUSED with LETKF_E_INVALID and a letkf_amd_last_error() message that names the argument, nothing written: a NULL argument
 * other than the optional outputs; type other than 1; lc_lat1 >= lc_lat2, or the two on opposite sides of the equator with sum 0;
 * a parallel or the base latitude at +-90 or beyond, or any parameter not finite; radius, dx, dy not finite or <= 0; a proj that
 * letkf_mapproj_setup did not make (type, hemisphere, c, fact, radius, dx, dy are tested); n < 0; nlon or nlat < 1, or
 * nlon * nlat, nlon + ihalo or nlat + jhalo of 2^31 or more; a negative halo; cx1 or cy1 not finite; a rotc that is not 16-byte
 * aligned (it is stored as one pair); a device output that overlaps a device input or another output.  With n = 0 the arrays may
 * be NULL.
 */
#ifndef LETKF_AMD_MAPPROJ_H
#define LETKF_AMD_MAPPROJ_H

#include "letkf_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LETKF_AMD_MAPPROJ_VERSION 1
#define LETKF_MAPPROJ_LC 1                      /* MPRJ_type = 'LC' */
#define LETKF_MAPPROJ_RADIUS_SCALE 6.37122e6    /* SCALE-RM's CONST_RADIUS, m */
#define LETKF_MAPPROJ_PI_REF 3.1415926535       /* common/common.f90:28, in the degree / radian conversions only */

typedef struct {          /* PARAM_MAPPROJ and what phys2ij reads of the grid */
  int32_t type, reserved0;                        /* 1 = LC */
  double basepoint_lon, basepoint_lat;            /* MPRJ_basepoint_lon / lat, degrees */
  double basepoint_x, basepoint_y;                /* MPRJ_basepoint_x / y, m */
  double lc_lat1, lc_lat2;                        /* MPRJ_LC_lat1 < MPRJ_LC_lat2, degrees */
  double radius;                                  /* m */
  double cxg1, cyg1;                              /* GRID_CXG(1), GRID_CYG(1), m */
  double dx, dy;                                  /* m */
} letkf_mapproj_params;

typedef struct {          /* what letkf_mapproj_setup derives; plain data, copied into the kernels' arguments */
  int32_t type, reserved0;
  double hemisphere;                              /* h: +1 or -1 */
  double lon0;                                    /* basepoint_lon * D, rad */
  double c, fact, radius;
  double pole_x, pole_y;
  double cxg1, cyg1, dx, dy;
} letkf_mapproj;

int letkf_mapproj_setup(const letkf_mapproj_params *p, letkf_mapproj *proj);

int letkf_phys2ij_dev(letkf_ctx *ctx, const letkf_mapproj *proj, int64_t n, const double *lon, const double *lat, double *ri,
                      double *rj, double *rotc);
int letkf_ij2phys_dev(letkf_ctx *ctx, const letkf_mapproj *proj, int64_t n, const double *ri, const double *rj, double *lon,
                      double *lat, double *rotc);
int letkf_mapproj_grid_dev(letkf_ctx *ctx, const letkf_mapproj *proj, int32_t nlon, int32_t nlat, int32_t ihalo, int32_t jhalo,
                           double cx1, double cy1, double *lon2d, double *lat2d, double *rotc2d);

int letkf_phys2ij_host(const letkf_mapproj *proj, double lon, double lat, double *ri, double *rj, double *rotc);
int letkf_ij2phys_host(const letkf_mapproj *proj, double ri, double rj, double *lon, double *lat, double *rotc);

#ifdef __cplusplus
}
#endif
#endif
