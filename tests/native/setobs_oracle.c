/* setobs_oracle.c -- TEST INFRASTRUCTURE, NOT PRODUCT: plain-C restatements of the parts of set_letkf_obs that
 * include/letkf_amd.h section 9 adds (scale/letkf/letkf_obs.f90; line numbers relative to the reference tree).  The tests
 * compose them with the oracle's orc_obs_departure / orc_obs_mesh_sort / orc_obs_halo_plan (oracle/letkf_oracle.c) into
 * the reference answer for letkf_set_obs_dev.  Sequential loops in the reference's order, libm log10. */
#include <math.h>
#include <stdint.h>

#define NID_OBS 16
static const int elem_uid[NID_OBS] = {2819, 2820, 3073, 3074, 3330, 3331, 14593, 19999, 4001, 4004, 4002, 4003,
                                      8800, 99991, 99992, 99993};   /* common_obs_scale.f90:74-77 */
static const double undef = -9.99e33;

static int uid_obs(int id) {                                         /* common_obs_scale.f90:171-211 */
  for (int u = 0; u < NID_OBS; ++u)
    if (elem_uid[u] == id) return u + 1;
  return -1;
}

/* letkf_obs.f90:268-305 over every row of the flattened files.  ctype_use: column-major (NID_OBS, nobtype), 0 / 1.
 * Returns 0, or -1 when a row's element or type lies outside uid_obs / 1..nobtype. */
int orc_obs_preprocess(int64_t nrows, int32_t *elm, const int32_t *typ, double *dat, double *err, int32_t nobtype,
                       double min_radar_ref_dbz, double low_ref_shift, int32_t use_obserr_radar_ref, double obserr_radar_ref,
                       int32_t use_obserr_radar_vr, double obserr_radar_vr, int32_t *ctype_use) {
  const double min_radar_ref = pow(10.0, min_radar_ref_dbz / 10.0);  /* common_obs_scale.f90:251 */
  for (int i = 0; i < NID_OBS * nobtype; ++i) ctype_use[i] = 0;
  int bad = 0;
  for (int64_t n = 0; n < nrows; ++n) {
    switch (elm[n]) {
      case 4001:                                                     /* id_radar_ref_obs, :273-288 */
        if (dat[n] >= 0.0 && dat[n] < 1.0e10) {
          if (dat[n] < min_radar_ref) {
            elm[n] = 4004;
            dat[n] = min_radar_ref_dbz + low_ref_shift;
          } else {
            dat[n] = 10.0 * log10(dat[n]);
          }
        } else {
          dat[n] = undef;
        }
        if (use_obserr_radar_ref) err[n] = obserr_radar_ref;
        break;
      case 4004:                                                     /* id_radar_ref_zero_obs, :289-293 */
        dat[n] = min_radar_ref_dbz + low_ref_shift;
        if (use_obserr_radar_ref) err[n] = obserr_radar_ref;
        break;
      case 4002:                                                     /* id_radar_vr_obs, :294-297 */
        if (use_obserr_radar_vr) err[n] = obserr_radar_vr;
        break;
    }
    const int u = uid_obs(elm[n]);                                   /* :301 */
    if (u < 1 || typ[n] < 1 || typ[n] > nobtype) {
      bad = 1;
      continue;
    }
    ctype_use[(typ[n] - 1) * NID_OBS + (u - 1)] = 1;
  }
  return bad ? -1 : 0;
}

/* letkf_obs.f90:307-342.  Returns nctype; outputs [nctype] (elm_u_ctype, typ_ctype 1-based) and ctype_elmtyp (column-major
 * (NID_OBS, nobtype), 1-based ctype or 0).  hori_local / vert_local [nobtype]; the three radar values resolved. */
int orc_ctype_tables(int32_t nobtype, const int32_t *ctype_use, const double *hori_local, const double *vert_local,
                     double hori_local_radar_obsnoref, double hori_local_radar_vr, double vert_local_radar_vr,
                     int32_t *elm_ctype, int32_t *elm_u_ctype, int32_t *typ_ctype, double *hori_loc_ctype,
                     double *vert_loc_ctype, int32_t *ctype_elmtyp) {
  int ictype = 0;
  for (int i = 0; i < NID_OBS * nobtype; ++i) ctype_elmtyp[i] = 0;
  for (int ityp = 1; ityp <= nobtype; ++ityp)
    for (int ielm_u = 1; ielm_u <= NID_OBS; ++ielm_u) {
      if (!ctype_use[(ityp - 1) * NID_OBS + ielm_u - 1]) continue;
      ctype_elmtyp[(ityp - 1) * NID_OBS + ielm_u - 1] = ictype + 1;
      elm_ctype[ictype] = elem_uid[ielm_u - 1];
      elm_u_ctype[ictype] = ielm_u;
      typ_ctype[ictype] = ityp;
      if (elm_ctype[ictype] == 4004)                                 /* :326-333 */
        hori_loc_ctype[ictype] = hori_local_radar_obsnoref;
      else if (elm_ctype[ictype] == 4002)
        hori_loc_ctype[ictype] = hori_local_radar_vr;
      else
        hori_loc_ctype[ictype] = hori_local[ityp - 1];
      if (elm_ctype[ictype] == 4002)                                 /* :334-339 */
        vert_loc_ctype[ictype] = vert_local_radar_vr;
      else
        vert_loc_ctype[ictype] = vert_local[ityp - 1];
      ++ictype;
    }
  return ictype;
}

/* letkf_obs.f90:657-677; dist_zero_fac = 3.651483717 is a single-precision literal (:27) */
void orc_obs_mesh_dims(int32_t nctype, const int32_t *typ_ctype, const double *hori_loc_ctype,
                       const double *obs_sort_grid_spacing, const int32_t *max_nobs_per_grid, const double *obs_min_spacing,
                       double dx, double dy, int32_t nlon, int32_t nlat, int32_t *ngrd_i, int32_t *ngrd_j, double *grdspc_i,
                       double *grdspc_j, int32_t *ngrdsch_i, int32_t *ngrdsch_j, int32_t *ngrdext_i, int32_t *ngrdext_j) {
  const double dist_zero_fac = (double)3.651483717f;
  for (int ic = 0; ic < nctype; ++ic) {
    const int ityp = typ_ctype[ic];
    double target_grdspc;
    if (obs_sort_grid_spacing[ityp - 1] > 0)
      target_grdspc = obs_sort_grid_spacing[ityp - 1];
    else if (max_nobs_per_grid[ityp - 1] > 0)
      target_grdspc = 0.1 * sqrt((double)max_nobs_per_grid[ityp - 1]) * obs_min_spacing[ityp - 1];
    else
      target_grdspc = hori_loc_ctype[ic] * dist_zero_fac / 6.0;
    const int ci = (int)ceil(dx * (double)nlon / target_grdspc), cj = (int)ceil(dy * (double)nlat / target_grdspc);
    ngrd_i[ic] = ci < nlon ? ci : nlon;
    ngrd_j[ic] = cj < nlat ? cj : nlat;
    grdspc_i[ic] = dx * (double)nlon / (double)ngrd_i[ic];
    grdspc_j[ic] = dy * (double)nlat / (double)ngrd_j[ic];
    ngrdsch_i[ic] = (int)ceil(hori_loc_ctype[ic] * dist_zero_fac / grdspc_i[ic]);
    ngrdsch_j[ic] = (int)ceil(hori_loc_ctype[ic] * dist_zero_fac / grdspc_j[ic]);
    ngrdext_i[ic] = ngrd_i[ic] + ngrdsch_i[ic] * 2;
    ngrdext_j[ic] = ngrd_j[ic] + ngrdsch_j[ic] * 2;
  }
}

/* obsgrd%tot_sub, letkf_obs.f90:744-760: tot[2 ic] rows of ctype ic (0-based), tot[2 ic + 1] those with qc == iqc_good */
void orc_obs_counts(int64_t nobs, int32_t nctype, const int32_t *ctype, const int32_t *qc, int32_t *tot) {
  for (int i = 0; i < 2 * nctype; ++i) tot[i] = 0;
  for (int64_t n = 0; n < nobs; ++n) {
    if (qc[n] == 0) tot[2 * ctype[n] + 1] += 1;
    tot[2 * ctype[n]] += 1;
  }
}
