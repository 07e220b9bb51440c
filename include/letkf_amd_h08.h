/* letkf_amd_h08.h -- Himawari-8 infrared radiances on the device: the records of the H08 observation file, the profiles the
 * host's radiative transfer (RTTOV) takes, and the obsda rows from what it returns.  The reference's version is its -DH08 build:
 * get_nobs_H08 / read_obs_H08 / write_obs_H08 and Trans_XtoY_H08 (scale/common/common_obs_scale.f90:2777-3110), the profile
 * set-up of SCALE_RTTOV_fwd (scale/common/scale_H08_fwd.F90:518-632, :707-749) and the two H08 blocks of obsope_cal
 * (scale/obs/obsope_tools.f90:512-646).  Like search_tc_subdom that last block is tentative -- nobs is never advanced, rig / rjg
 * of its buffer test are left over from another loop -- so this header states the mathematics it computes and names each place
 * WHERE THE REFERENCE IS NOT FOLLOWED, (1) to (6) below.  DESIGN.md section 23.
 *
 * Companion of letkf_amd_obsope.h (included for letkf_obsope_fields, of which nv2dd >= 9 is required here: lsmask = 8, skint = 9
 * in the reference's order, u10m = 4, v10m = 5) and of letkf_amd_obsfile.h (included for letkf_obsfile_cols).  The entries are
 * exported by a library of their own, libletkf_amd_h08.so, which links against libletkf_amd.so for the context, its stream, its
 * scratch buffer, its scan plumbing and letkf_amd_last_error().  The radiative transfer itself stays the host's, as open / read /
 * write of bytes do.
 *
 * THE ORDER OF CALLS for a Himawari-8 file: letkf_h08_decode_dev, the projection's phys2ij, the first scan, the operator for all
 * members (the H08 rows get qc 90: they are not its own), then
 *   letkf_h08_select_dev     which profiles of the file this call's obsda rows name
 *   letkf_h08_profiles_dev   the profile arrays of every member at those profiles
 *   (the host's RTTOV call: btall, btclr, trans per member, profile and channel)
 *   letkf_h08_rows_dev       the obsda rows: value, qc, lev (the weighting function's peak) and val2 (the clear-sky value)
 * and set_letkf_obs with letkf_qc_params.h08 = 1, h08_lev = lev, h08_val2 = val2.
 *
 * LEVELS.  Every device array is described in MODEL level order, k = 0 .. nlev-1 bottom up, k = 0 being array level 1 + khalo.
 * p->top_down != 0 reverses the level index of every profile output and of the transmittance input, l = nlev-1-k: the order RTTOV
 * is given (elev:slev:-1).  nch = LETKF_H08_NCH = 10 everywhere.
 *
 * letkf_h08_count / letkf_h08_bytes (host only): get_nobs_H08.  One record per profile: a marker, 4 + nch float32, a marker, 64
 *   bytes.  nbytes not a multiple of 64: LETKF_E_INVALID.
 * letkf_h08_decode_dev(ctx, big_endian, image, nprof, obserr, cols, nbad): read_obs_H08.  Row np * nch + c (c = 0..9) gets
 *   elm = NINT(wk1), typ = NINT(wk2), lon / lat = wk3 / wk4 widened, dat = double(wk(5 + c)), dif = 0, lev = c + 7 (the reference's
 *   ch + 6.0), err = obserr[c] (HOST [nch], OBSERR_H08).  NINT, NaN, the marker count nbad (HOST or NULL; markers are 4 * 14) and the
 *   byte order follow the rules of letkf_amd_obsfile.h.  Any column of cols may be NULL.
 * letkf_h08_encode_dev(ctx, big_endian, nprof, cols, image): write_obs_H08.  One record per profile from the profile's first row
 *   (elm, typ, lon, lat narrowed to float32) and the dat of its ten rows narrowed.  The reference ignores `missing`; so does this.
 *   elm, typ, lon, lat and dat are required.
 * letkf_h08_select_dev(ctx, set, idx, row0, nrows, h08_set, nprof_file, prof_list, slot_of_prof, nsel): profile fp = (idx-1) / nch
 *   of file h08_set (1-based, 1 .. LETKF_OBSOPE_MAX_FILES) is selected when at least one obsda row of [row0, row0 + nrows) with
 *   set == h08_set names it (a row whose idx lies outside 1 .. nprof_file * nch names none).  prof_list (dev int32 [nprof_file], the
 *   first *nsel written, ascending fp) and slot_of_prof (dev int32 [nprof_file], -1 where not selected) come from a stable
 *   compaction: a 0 / 1 flag per profile, the main library's scan, one writer per position; no shared counter.  *nsel (HOST) is the
 *   entry's one read-back.
 * letkf_h08_profiles_dev(ctx, p, f, nsel, prof_list, ri, rj, lon, lat, rotc, out): the first loop of Trans_XtoY_H08 (:2842-2875)
 *   for every member of f, and with p->rttov_units lines 518-632 of scale_H08_fwd.F90.
 *   ri, rj, lon, lat  dev, per FILE profile (the values of the profile's first row); ril = ri - p->ri_off, rjl = rj - p->rj_off
 *   rotc              dev [file profile][2], or NULL: no rotation (usfc = u10m, vsfc = v10m as interpolated)
 *   itpl_2d:  i = CEILING(ril), ai = ril - (i-1), likewise j; v(i-1,j-1)(1-ai)(1-aj) + v(i,j-1) ai (1-aj) + v(i-1,j)(1-ai) aj +
 *     v(i,j) ai aj, each product left to right, summed left to right.  Indexes are clamped into the array and a corner of weight
 *     exactly 0 never contributes: the WHERE THE REFERENCE IS UNDEFINED rules of letkf_amd_obsope.h.
 *   out->sfc   [nmem][nsel][8] = tsfc (itpl_2d of skint), qsfc (q2m), psfc (ps), usfc, vsfc (u10m read at ril - 0.5 and v10m at
 *     rjl - 0.5 under p->stggrd, then u rotc1 - v rotc2 and u rotc2 + v rotc1), topo, lsmask, zenith
 *   out->lev3  [nmem][nsel][5][nlev] = the column interpolation (itpl_2d_column over the nlev interior levels) of p, t, q, qc and
 *     of (qi + qs + qg), summed per corner in that order and then weighted
 *   out->pflag [nsel] = 0, or 98 where ril or rjl is a NaN or lies outside 1 .. nlonh / nlath, or where prof_list names a
 *     profile outside 0 .. p->nprof_file-1 (ri .. rotc hold p->nprof_file entries and are not read there); every value of
 *     that profile is then undef (-9.99e33), the zenith included
 *   zenith (:551-572), always:  rlat = lat d2r, rlon = lon d2r (d2r = 3.14159265358979 / 180, SCALE-RM's CONST_D2R);
 *     c = atan(p->ell_tan tan(rlat)); Rl = r_pol / sqrt(1 - ell_ecc cos(c) cos(c)); dl = rlon - sub_lon d2r;
 *     r1 = r_sat - Rl cos(c) cos(dl), r2 = -Rl cos(c) sin(dl), r3 = Rl sin(c); rnps = |r|; e = (r1 - r_sat, r2, r3), rnep = |e|;
 *     zenith = acos(((-r1) e1 + (-r2) e2 + (-r3) e3) / (rnps rnep)) / d2r, every operation rounded on its own, left to right.
 *     The one value not held bit for bit by the tests (two libm implementations): DESIGN.md section 23 has its tolerance.
 *   p->rttov_units != 0: the values RTTOV's profile structure takes, each operation rounded on its own: p * 0.01; q * q_ppmv, a
 *     value below qmin becoming qmin + qmin * 0.01 (qsfc too); psfc * 0.01; topo * 0.001.  lsmask stays the interpolated
 *     value in either units: the reference truncates it only where it is copied into the integer skin%surftype (:542), which
 *     the host's copy does by itself, and H08_REJECT_LAND tests the interpolated one (common_obs_scale.f90:2951) -- the rows
 *     entry reads it here, so the units never change a qc.  And
 *   out->cloud [nmem][nsel][3][nlev-1] (required then, not written otherwise; :604-630), from the values BEFORE the conversion:
 *     tv = t (1 + q repsb) / (1 + q), repsb = 1 / (rd / rv); g = p / (rd tv) * 1000; liqc = fmax(qc, 0) g, icec = fmax(qice, 0) g
 *     (a NaN content counts as 0); layer (k, k+1): liq = (liqc[k] + liqc[k+1]) * 0.5, ice likewise, at index k, or nlev-2-k under
 *     top_down (RTTOV's layer numbering); cfrac = 1 where liq + ice > minq else 0 when cfrac_cnst <= 0, else
 *     fmin((liq + ice) / cfrac_cnst, 1).  [.][.][0] = liq, [1] = ice, [2] = cfrac.
 *   One wave per (profile, member), lanes along the level, looping when nlev > 64: with the reference's strides (s3k = 1) the
 *   four corner columns of the seven fields are contiguous loads, and the outputs are written level-fastest in either direction.
 *   Other strides are correct, not fast.  One writer per value.
 * letkf_h08_rows_dev(ctx, p, row0, nrows, set, idx, h08_set, slot_of_prof, nsel, nmem, m0, lev3, sfc, pflag, btall, btclr, trans,
 *     rig, rjg, qc_replace, qc, ensval, kld, lev, val2): the second half of Trans_XtoY_H08 (:2913-2966) and the fill of
 *   obsope_tools.f90:594-634, per obsda row and member.
 *   btall, btclr dev [nmem][nsel][nch], trans dev [nmem][nsel][nch][nlev]: what the radiative transfer returned; lev3, sfc, pflag
 *   as the profiles entry wrote them (p->nlev, p->top_down and p->rttov_units as they were then; with rttov_units the pressure
 *   is read back as lev3 * 100.0, one rounding away from the reference's Pa).  rig, rjg dev per file profile, GLOBAL.
 *   A row r of [row0, row0 + nrows) with set[r] == h08_set, 1 <= idx[r] <= p->nprof_file * nch and s = slot_of_prof[fp] >= 0 is
 *   served, its channel c = (idx-1) % nch; every other row is untouched.  Per member, prs and tau in model order:
 *     w1 = abs((tau[1]-tau[0]) * (1 / (prs[1]-prs[0]))), plev = (prs[1]+prs[0]) * 0.5; for j = 2 .. nlev-1
 *     w = (tau[j]-tau[j-1]) * (1 / abs(prs[j]-prs[j-1])) -- signed, no abs -- and where w > the running maximum it becomes the
 *     maximum and plev = (prs[j]+prs[j-1]) * 0.5.  Hence the first layer that attains the maximum wins, a NaN weight never wins
 *     and a NaN w1 keeps the first layer.
 *     yobs = btall, negated where abs(btall - btclr) > p->cldsky_thrs (with the reference's default -5 every finite row is cloudy)
 *     qc_m = 0 where p->ch_use[c] == 1 else 50; 50 where p->reject_land and lsmask > 0.5; 50 where it was 0 and rig <= bris or
 *     rig >= brie or rjg <= brjs or rjg >= brje; then max with pflag[s]
 *   ensval[r * kld + m0 + m] = yobs_m;  qc[r] = max over the members, replacing the row's code with qc_replace != 0 (the call that
 *   takes over from the operator's 90) and maxed with it otherwise;  lev[r] / val2[r] INOUT += plev_m / btclr_m, added
 *   sequentially for m = 0 .. nmem-1 from the caller's value by one writer, then divided by double(p->member) where p->finish: the
 *   convention of the obsda assemble entry of letkf_amd_obsfile.h.  p->use_obs23 == 0: the served rows get qc 90 (replaced or
 *   maxed in the same way), nothing else is written, and only set, idx, slot_of_prof and qc are read: every other array may
 *   be NULL (no profiles and no radiative transfer are needed; the selection still says which rows are served).
 *   One block per row takes all its members, a wave per (row, member) with lanes along the layer; the first maximum is a wave
 *   reduction folded in a fixed order that equals the sequential statement.  No atomics; same bits from call to call.
 *
 * WHERE THE REFERENCE IS NOT FOLLOWED.  (1) The argument of acos is clamped to [-1, 1]: the sub-satellite point gives 0, not a
 * NaN.  (2) The buffer test uses the profile's own global coordinates rig / rjg (the reference's are left over from the loop
 * before).  (3) obsope_cal never advances nobs for H08 rows; here the rows are the first scan's, named by set / idx.  (4) A profile
 * outside the array or on a NaN coordinate is flagged (pflag 98, values undef) instead of read out of bounds.  (5) MAX of a NaN
 * cloud content is 0 (fmax); NINT(NaN) = 0.  (6) The reference hands RTTOV every profile of the slot on the rank; here the
 * caller's rows decide (select), so a call per slot or per batch of rows gives what one call gives.
 *
 * REFUSED with LETKF_E_INVALID and a letkf_amd_last_error() message that names the argument, nothing written: NULL required
 * pointers; an image not 4-byte aligned; negative counts; nmem < 1; m0 < 0 or m0 + nmem > kld; a zero stride; nlev < 2 (or
 * p->nlev != f->nlev); nlon or nlat < 1, khalo, ihalo or jhalo negative; nv3dd < 13 or nv2dd < 9; rd, rv, q_ppmv or qmin not
 * finite or not positive; member < 1 with finish; a negative p->nprof_file; an output overlapping another output or an input
 * (every input array of the entry at its stated extent; the fields at the extent their sizes and strides span, where no stride
 * is negative); h08_set outside 1 .. LETKF_OBSOPE_MAX_FILES; more
 * than 2^31 - 1 rows, profiles or (profile, member) pairs in one call.  Zero profiles or zero rows launch nothing and are no error.
 */
#ifndef LETKF_AMD_H08_H
#define LETKF_AMD_H08_H

#include "letkf_amd_obsope.h"
#include "letkf_amd_obsfile.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LETKF_AMD_H08_VERSION 1
#define LETKF_H08_NCH 10
#define LETKF_H08_ID 8800
#define LETKF_H08_QC_BAD 50

typedef struct {          /* a host struct */
  int32_t nlev, nprof_file;                           /* interior levels; profiles of the file: entries of the per-profile arrays */
  int32_t top_down, stggrd, rttov_units, reject_land; /* H08_REJECT_LAND */
  int32_t use_obs23, finish, member, reserved0;       /* USE_OBS(23); divide lev / val2 by MEMBER */
  int32_t ch_use[10];                                 /* H08_CH_USE */
  double ri_off, rj_off;                              /* rank_i * nlon, rank_j * nlat */
  double rd, rv, q_ppmv, qmin, minq, cfrac_cnst;      /* Rdry, Rvap, q_mixratio_to_ppmv, qmin, H08_RTTOV_MINQ, H08_RTTOV_CFRAC_CNST */
  double sub_lon, r_pol, r_sat, ell_tan, ell_ecc;     /* 140.7, 6356.7523e3, 42164.0e3, 0.993305616, 0.00669438444 */
  double cldsky_thrs, bris, brie, brjs, brje;         /* H08_CLDSKY_THRS; the buffer box in global grid coordinates */
} letkf_h08_params;

typedef struct {          /* the outputs of letkf_h08_profiles_dev: dev */
  double *lev3, *sfc, *cloud;
  int32_t *pflag;
} letkf_h08_profiles;

int letkf_h08_count(int64_t nbytes, int64_t *nprof);
int letkf_h08_bytes(int64_t nprof, int64_t *nbytes);

int letkf_h08_decode_dev(letkf_ctx *ctx, int32_t big_endian, const uint32_t *image, int64_t nprof, const double *obserr,
                         const letkf_obsfile_cols *cols, int64_t *nbad);
int letkf_h08_encode_dev(letkf_ctx *ctx, int32_t big_endian, int64_t nprof, const letkf_obsfile_cols *cols, uint32_t *image);

int letkf_h08_select_dev(letkf_ctx *ctx, const int32_t *set, const int32_t *idx, int64_t row0, int64_t nrows, int32_t h08_set,
                         int64_t nprof_file, int32_t *prof_list, int32_t *slot_of_prof, int64_t *nsel);

int letkf_h08_profiles_dev(letkf_ctx *ctx, const letkf_h08_params *p, const letkf_obsope_fields *f, int64_t nsel,
                           const int32_t *prof_list, const double *ri, const double *rj, const double *lon, const double *lat,
                           const double *rotc, const letkf_h08_profiles *out);

int letkf_h08_rows_dev(letkf_ctx *ctx, const letkf_h08_params *p, int64_t row0, int64_t nrows, const int32_t *set,
                       const int32_t *idx, int32_t h08_set, const int32_t *slot_of_prof, int64_t nsel, int32_t nmem, int32_t m0,
                       const double *lev3, const double *sfc, const int32_t *pflag, const double *btall, const double *btclr,
                       const double *trans, const double *rig, const double *rjg, int32_t qc_replace, int32_t *qc,
                       double *ensval, int64_t kld, double *lev, double *val2);

#ifdef __cplusplus
}
#endif
#endif
