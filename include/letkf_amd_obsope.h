/* letkf_amd_obsope.h -- the observation operator H(x) of obsope_cal for every member, feeding letkf_set_obs_dev.
 *
 * Companion of letkf_amd.h (which it includes for letkf_ctx and letkf_obs_file_rows).  One call computes, for the obsda rows
 * row0 .. row0 + nrows - 1 and for nmem model fields, the body of the loop at scale/obs/obsope_tools.f90:454-507 and the
 * reduction of common_mpi_scale.f90:1862-1865:
 *   ensval[row * kld + m0 + m] = H(x_m)(row),   qc[row] = max(qc[row], qc_m(row))   (qc is INOUT)
 * so a host that calls member by member, or slot by slot, gets what one call gives.  DESIGN.md section 12 has the details.
 *
 * ROWS.  set / idx (dev, 1-based file and row of `files`) name the observation of an obsda row, as in letkf_set_obs_dev.
 * `files` is read BEFORE letkf_set_obs_dev pre-processes it (that call converts reflectivities and rewrites elements in
 * place): call the operator first.  Only elm, typ, lev, ri and rj of `files` are read; nfile <= 16.  lon / lat are per
 * file row, rotc per obsda row.
 *
 * PER ROW AND MEMBER (common_obs_scale.f90).  ril = ri - ri_off, rjl = rj - rj_off (rij_g2l: rank_i * nlon, rank_j * nlat).
 *   use_obs[typ - 1] == 0                        qc 90, value 0
 *   conventional file (file_radar[f] < 0)        phys2ijk (:999-1110) on the pressure field, then Trans_XtoY (:264-338):
 *       U, V (rotated by rotc), T, Tv, Q, RH, PS (prsadj; qc 10 beyond ps_adjust_thres, the value is still returned);
 *       any other element qc 90 and the value undef (-9.99e33)
 *   radar file (file_radar[f] = r >= 0)          lev > radar_zmax: qc 19; else phys2ijkz (:1116-1237) on the height
 *       field, then Trans_XtoY_radar (:342-493) with radar r of radar_meta: eleven interpolations, the rotation, azimuth
 *       and elevation, calc_ref_vr (:626-990, METHOD_REF_CALC 1..3, USE_TERMINAL_VELOCITY), the element select; qc 11
 *       becomes 0 (obsope_tools.f90:488).  A target on the radar's own lon / lat: qc 98, value undef.
 *   qc from the coordinate search (98 outside 1 .. nlonh / nlath, 20 too high, 21 too low) leaves the value 0.
 * The real literals the reference writes without a kind (273.16, 1e-3, 1.84, ...) are single precision there and are
 * widened from single precision here.  H08, TC vitals, rain and USE_RADAR_PSEUDO_RH are not covered: qc 90.
 * (H08 rows are served by letkf_amd_h08.h after this entry, TC vitals by letkf_amd_tcvital.h.)
 * stggrd = 1 (what monit_obs passes): U is read at ri - 0.5, V at rj - 0.5 and, in the radar operator only, W at rk - 0.5.
 *
 * WHERE THE REFERENCE IS UNDEFINED.  CEILING of an integer coordinate puts weight exactly 0 on index i - 1; at
 * ri == 1.0 (rj == 1.0) that index is 0, outside the array.  The library never reads it: an index below 1 is clamped to
 * 1, and a corner of weight exactly 0 never contributes (a NaN there does not spread).  The same clamp serves the cases
 * that follow from it: U at ri - 0.5 < 1 or V at rj - 0.5 < 1 under stggrd (the edge column is used); a target exactly on
 * the top level finds no crossing and gets rk = nlev + khalo (the reference divides 0 by a halo difference); a corner
 * column without any valid level gives qc 21; a NaN coordinate gives qc 98.
 *
 * REFUSED with LETKF_E_INVALID and a letkf_amd_last_error() message, nothing written: a NULL argument; nmem < 1;
 * m0 < 0 or m0 + nmem > kld; a zero stride; method_ref_calc outside 1..3; khalo < 1; nlev, nlon, nlat < 1 or a negative
 * halo; nv3dd < 13 or nv2dd < 7; nobtype outside 1..32; nfile outside 1..16; file_radar below -1, or a radar
 * file without radar_meta; row0 or nrows negative; and, checked on the device before the operator is launched (one read-back,
 * as letkf_set_obs_local_dev does), set / idx outside the files or a report type outside 1..nobtype.
 * Apart from that read-back everything is asynchronous on the context's stream.  Results are bitwise equal from call to
 * call: every value has one writer and qc is merged by an integer maximum.
 */
#ifndef LETKF_AMD_OBSOPE_H
#define LETKF_AMD_OBSOPE_H

#include "letkf_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LETKF_AMD_OBSOPE_VERSION 1
#define LETKF_OBSOPE_MAX_FILES 16

typedef struct {          /* model fields of nmem members (history variables, common_scale.f90:60-85) */
  int32_t nlev, nlon, nlat, khalo, ihalo, jhalo;      /* nlevh = nlev + 2 khalo, nlonh = nlon + 2 ihalo, nlath = nlat + 2 jhalo */
  int32_t nv3dd, nv2dd;                               /* 13, 7; the iv3dd_* / iv2dd_* order of the reference */
  int32_t nmem, m0;                                   /* fields in this call; first ensval slot they fill */
  const double *v3d; int64_t s3k, s3i, s3j, s3v, s3m; /* dev; element strides; the reference: 1, nlevh, nlevh*nlonh, ... */
  const double *v2d; int64_t s2i, s2j, s2v, s2m;      /* dev; the reference: 1, nlonh, nlonh*nlath, ... */
} letkf_obsope_fields;

typedef struct {          /* what the operator needs beyond letkf_obs_file_rows */
  const double *lon, *lat;          /* dev, per file row */
  const int32_t *file_radar;        /* HOST [nfile]: -1 = conventional format, r >= 0 = radar file, meta row r */
  const double *radar_meta;         /* HOST [nradar][3]: lon, lat, z */
  const double *rotc;               /* dev [rows][2] or NULL */
  const int32_t *use_obs;           /* HOST [nobtype] */
  int32_t nobtype, method_ref_calc, use_terminal_velocity, stggrd;
  double min_radar_ref_dbz, low_ref_shift, radar_zmax, ps_adjust_thres, ri_off, rj_off;
} letkf_obsope_params;

int letkf_obsope_dev(letkf_ctx *ctx, const letkf_obsope_params *p, const letkf_obs_file_rows *files,
                     const letkf_obsope_fields *f, int64_t row0, int64_t nrows,
                     const int32_t *set, const int32_t *idx, int32_t *qc, double *ensval, int64_t kld);

#ifdef __cplusplus
}
#endif
#endif
