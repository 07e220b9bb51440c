/* letkf_amd_nobsout.h -- NOBS_OUT on the device: the counts and cut-offs of obs_local out of das_letkf's main loop, and the
 * fields the reference writes from them -- scale/letkf/letkf_tools.f90:440-447 (work3dn) and :763-778 (the eleven work3d fields);
 * all file:line below are in that file.
 *
 * Companion of letkf_amd.h.  The entries are exported by a library of their own, libletkf_amd_nobsout.so, which links against
 * libletkf_amd.so for the context, its stream and buffers, letkf_amd_last_error() and the main loop itself.  DESIGN.md section 21.
 *
 * letkf_das_columns_nobs_dev: letkf_das_columns_dev (letkf_amd.h, 3c) with two more outputs.
 *   nobs_ctype  dev [nij1*nlev][nctype] int32, or NULL
 *   cutd_ctype  dev [nij1*nlev][nctype] double, or NULL          (point p = ij + nij1*lev; either may be NULL on its own)
 * THE ANALYSIS is the one of letkf_das_columns_dev under the same context options: the same routes, the same kernels, the same
 * bits in anal, status, infl, rtps_infl_out and nobs_out.  With both pointers NULL the call IS letkf_das_columns_dev, and
 * letkf_ctx_last_path gives the same string.
 * THE DIAGNOSTICS at a point with beta /= 0 are what letkf_obs_search_columns_dev (letkf_amd.h, 3a) writes for the same tables,
 * columns and options: nobsl_t and cutd_t of obs_local -- their defaults (:1380-1389, :1427-1431), and for a limited group the
 * selected count and the cut-off on its master (:1633-1640, :1713-1727).  The sum of nobs_ctype over the types of a point is that
 * point's nobs_out.  A point without any local observation still carries the default cut-offs.  At a point with beta = 0 both are
 * 0: the reference does not call obs_local there (:333-359) and work3dn keeps its initial zeros; with args->beta NULL no point is
 * zeroed.
 * NO SECOND SELECTION.  On the list route and the ring route the diagnostics come out of the fill passes the call runs anyway
 * (one per slab of levels).  On the list-free route (no limit, LETKF_OPT_COLUMN_SURVIVORS) no search by point exists: the
 * unlimited column kernel's count pass gives nobs_ctype.  Tables without a limit never go through the limited kernel for
 * cutd_ctype: it is the criterion's default, hori_loc[ic] * dist_zero_fac (the single-precision literal of letkf_obs.f90:27 as a
 * double) on the master of every group under criterion 1, 0 elsewhere and under criteria 2 / 3, written by a kernel of this
 * library.  (Without a limit the counts are per combined type, as the reference's, also for a merged group of more than four
 * types, where 3a reports the group's total on its master.)
 * REFUSED with LETKF_E_INVALID, nothing written: whatever letkf_das_columns_dev refuses; with a diagnostic array also nctype or
 * ngroup < 1 and a criterion outside 1..3; a diagnostic array that overlaps nobs_out, args->status or the other diagnostic array.
 * Synchronisations: those of letkf_das_columns_dev; with a diagnostic array and tables->limit_hint = 0 one more read of max_nobs.
 *
 * letkf_nobs_fields_dev: work3dn and the eleven fields from those two arrays.
 *   p            nctype (1..64), nobtype (1..32; the reference's is 24), HOST elm_u_ctype / typ_ctype [nctype] as
 *                letkf_obs_table_info_get returns them (1-based uid 1..16, 1-based report type 1..nobtype), uid_ref, uid_re0, uid_vr
 *                (the reference's 9, 10, 11), typ_radar (22) and pick[5], the report types of fields 1..5 (1, 3, 4, 8, 22), each
 *                1..nobtype
 *   nobs_ctype   dev [npts][nctype], cutd_ctype dev [npts][nctype] or NULL (zeros in the three cut-off rows)
 *   work3dn      dev [npts][nobtype + 6] doubles or NULL: one variable class's work3dn(:,ij,ilev,n).  Rows 1..nobtype: the sum of
 *                the counts over the combined types of that report type (sum(nobsl_t, dim=1), :441); rows nobtype+1..+3: the
 *                counts of (uid_ref | uid_re0 | uid_vr, typ_radar) (:442-444); rows +4..+6: their cut-offs (:445-447).  A
 *                combination no combined type carries gives 0.
 *   fields       dev or NULL, element (p, f) at p*sp + f*sv, f = 0..10: work3d(:,:,1..11) of :768-778 -- the rows pick[0..4], then
 *                rows nobtype+1..+6.  sp = 1, sv = nij1*nlev is the (nij1, nlev, nv3d) array letkf_member_points_dev and the
 *                host's gather_grd_mpi take.
 * The reference reads the class of iv3d_t (:768).  With several variable-localisation classes the caller passes that class's
 * diagnostics, so the copy of :399-400 needs no code here.
 * Integers arrive exactly in the doubles, cut-offs are copied; every output value has one writer, results are bitwise equal from
 * call to call.  No synchronisation.  npts = 0 is no error and launches nothing.
 * REFUSED with LETKF_E_INVALID, nothing written: a NULL ctx / p / nobs_ctype / elm_u_ctype / typ_ctype; work3dn and fields both
 * NULL; npts < 0; nctype, nobtype, a uid, a report type or a pick outside its range; two combined types with the same (uid, report
 * type); strides other than sp >= 1 with sv > (npts - 1) * sp, or sv >= 1 with sp > 10 * sv (two field elements would coincide);
 * an output that overlaps an input or the other output.
 */
#ifndef LETKF_AMD_NOBSOUT_H
#define LETKF_AMD_NOBSOUT_H

#include "letkf_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LETKF_AMD_NOBSOUT_VERSION 1
#define LETKF_NOBSOUT_MAX_CTYPE 64
#define LETKF_NOBSOUT_MAX_OBTYPE 32
#define LETKF_NOBSOUT_NFIELDS 11

typedef struct {          /* a host struct */
  int32_t nctype, nobtype;
  int32_t uid_ref, uid_re0, uid_vr, typ_radar;
  int32_t pick[5];
  int32_t reserved0;
  const int32_t *elm_u_ctype;                         /* HOST [nctype] */
  const int32_t *typ_ctype;                           /* HOST [nctype] */
} letkf_nobsout_params;

int letkf_das_columns_nobs_dev(letkf_ctx *ctx, const letkf_das_args *args, const letkf_search_tables *tables, int64_t nij1,
                               int32_t nlev, const double *rig, const double *rjg, const double *rlev, const double *rz,
                               int64_t list_bytes, int32_t *nobs_out, int32_t *nobs_ctype, double *cutd_ctype);

int letkf_nobs_fields_dev(letkf_ctx *ctx, const letkf_nobsout_params *p, int64_t npts, const int32_t *nobs_ctype,
                          const double *cutd_ctype, double *work3dn, double *fields, int64_t sp, int64_t sv);

#ifdef __cplusplus
}
#endif
#endif
