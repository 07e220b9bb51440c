/* letkf_amd_obssim.h -- obssim_cal on the device: the observation operator H(x) at every interior grid point, as doubles in
 * the reference's array order and as the single-precision GrADS records of write_grd_mpi.
 *
 * Companion of letkf_amd_obsope.h (which it includes for letkf_obsope_fields).  The one entry is exported by a library of its
 * own, libletkf_amd_obssim.so, which links against libletkf_amd.so for the context, its stream and scratch buffer and
 * letkf_amd_last_error().  One call is the loop nest of scale/obs/obsope_tools.f90:1090-1146 for f->nmem model states (for
 * example the time steps of scale/obs/obssim.f90:93-100) plus, where `rec` is asked for, this subdomain's part of the records
 * of write_grd_mpi (:1184-1204).  DESIGN.md section 15 has the details.
 *
 * FIELDS.  `f` is the operator's structure, unchanged: strides, halos, nv3dd >= 13, nv2dd >= 7.  nmem is the number of states
 * in the call and m0 must be 0.  The history fields of a restart file come from letkf_state_to_history_dev
 * (letkf_amd_monit.h); that is the `restart` branch of obssim.f90:79-86.
 *
 * PER STATE, INTERIOR POINT (k, i, j) AND LIST ENTRY (0-based here; the reference's ri = i + IHALO, rj = j + JHALO,
 * rk = k + KHALO are the 1-based coordinates of the same point, :1091-1100).
 *   3-D list, REF (4001), RE0 (4004), Vr (4002), pseudo-RH (4003):  Trans_XtoY_radar (common_obs_scale.f90:342-493) with the
 *       radar at radar_lon / radar_lat / radar_z, the point's lon / lat, lev = hgt(k, i, j) and the rotation rotc(i, j).
 *       qc 11 becomes 0 (:1108): a reflectivity below MIN_RADAR_REF stores min_radar_ref_dbz + low_ref_shift, Vr stores its
 *       value.  The pseudo-RH id falls to CASE DEFAULT there: qc 90, undef.  A point on the radar's own lon / lat: qc 98, undef.
 *   3-D list, any other id:  Trans_XtoY (:264-338): U, V (rotated), T, Tv, Q, RH, PS; an id it does not know (H08, TC vitals,
 *       rain, ...) gives undef.
 *   2-D list:  EVERY id goes through Trans_XtoY at k = 1, rk = 1 + KHALO (:1122-1131), literally as the reference does.  A 3-D
 *       element there gives its lowest-level value; a radar id gives undef.  PS calls prsadj with dz = rk - topo, a level index
 *       minus metres: with a realistic ps_adjust_thres that is nearly always qc 10, undef.  This is the reference's behaviour
 *       and is kept, not repaired (PS in the 3-D list does the same with its own rk).
 *   A value whose qc is not 0 is stored as undef (:1114-1118).
 * INTEGER COORDINATES.  The operator's rule holds (letkf_amd_obsope.h, "where the reference is undefined"): a corner of weight
 * exactly 0 never contributes and an index below 1 is clamped.  Un-staggered variables are therefore the point's own value.
 * Under stggrd = 1, U is the two-column sum at ri - 0.5, V the two rows at rj - 0.5 and W (radar operator only) the two levels at
 * rk - 0.5, each in itpl_3d's term order (:1339-1366), left to right, without contraction.
 * STGGRD IS EXPLICIT.  obssim_cal's optional stggrd reaches Trans_XtoY*, whose `INTEGER :: stggrd_ = 0` is an implicitly SAVEd
 * variable that a call without the argument never resets.  Here the caller says what it means: the `restart` branch of
 * obssim.f90 passes 1, the `history` branch means 0.
 * ROUNDING.  round_single = 1 is the reference: every value goes through real(., r_sngl) before it is stored in the double
 * arrays (:1115, :1135) and undef is (double)(float)(-9.99e33).  round_single = 0 keeps the double and undef = -9.99e33.
 * `rec` is single precision either way.
 *
 * OUTPUTS (any of v3, v2, rec may be NULL, not all three).
 *   v3   dev double, v3dgsim(nlev, nlon, nlat, nvar3): v3[s * sm3 + ((n * nlat + j) * nlon + i) * nlev + k]
 *   v2   dev double, v2dgsim(nlon, nlat, nvar2):       v2[s * sm2 + (n * nlat + j) * nlon + i]
 *   rec  dev float,  rec[((s * nrec + r) * nlat + j) * nlon + i], nrec = nvar3 * nlev + nvar2, r = n * nlev + k for 3-D
 *        variable n and level k, r = nvar3 * nlev + n for 2-D variable n: record order, one subdomain
 * What stays the host's: reading the files, the map projection (lon / lat / rotc are its MPRJ_xy2lonlat * rad2deg and
 * MPRJ_rotcoef), the MPI_REDUCE of the subdomains into the global record, and the file.
 *
 * REFUSED with LETKF_E_INVALID and a letkf_amd_last_error() message, nothing written: a NULL ctx / p / f / o; NULL lon / lat /
 * fields; all three outputs NULL; nvar3 or nvar2 outside 0..16, or both 0; v3 with nvar3 = 0 or v2 with nvar2 = 0; the field
 * checks of letkf_obsope_dev (sizes, halos, zero strides, nv3dd, nv2dd); m0 != 0; nmem < 1; method_ref_calc outside 1..3; stggrd
 * or round_single outside 0..1; a non-finite radar position; nlat or nmem above 65535, or nlev * nlon above 2^31 - 256 (launch
 * dimensions).
 * There are no rows to check, so there is no read-back: everything is asynchronous on the context's stream.  Every value has
 * one writer and results are bitwise equal from call to call.
 */
#ifndef LETKF_AMD_OBSSIM_H
#define LETKF_AMD_OBSSIM_H

#include "letkf_amd_obsope.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LETKF_AMD_OBSSIM_VERSION 1
#define LETKF_OBSSIM_MAX_VARS 16

typedef struct {          /* a host struct; pointers are device pointers */
  int32_t nvar3, vars3[16];           /* OBSSIM_NUM_3D_VARS, OBSSIM_3D_VARS_LIST: element ids, common_obs_scale.f90:48-72 */
  int32_t nvar2, vars2[16];           /* OBSSIM_NUM_2D_VARS, OBSSIM_2D_VARS_LIST */
  double radar_lon, radar_lat, radar_z;   /* OBSSIM_RADAR_LON / _LAT / _Z */
  const double *lon, *lat;            /* dev [nlat][nlon], degrees */
  const double *rotc;                 /* dev [nlat][nlon][2], or NULL: 1, 0 */
  int32_t method_ref_calc, use_terminal_velocity, stggrd, round_single;
  double min_radar_ref_dbz, low_ref_shift, ps_adjust_thres;
} letkf_obssim_params;

typedef struct {
  double *v3, *v2;                    /* dev, or NULL */
  float *rec;                         /* dev, or NULL */
  int64_t sm3, sm2;                   /* elements between two states in v3 / v2 */
} letkf_obssim_out;

int letkf_obssim_dev(letkf_ctx *ctx, const letkf_obssim_params *p, const letkf_obsope_fields *f, const letkf_obssim_out *o);

#ifdef __cplusplus
}
#endif
#endif
