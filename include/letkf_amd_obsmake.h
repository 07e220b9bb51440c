/* letkf_amd_obsmake.h -- obsmake_cal on the device: synthetic observations for an OSSE from a nature run, H(x) per time
 * slot plus the reference's own stream of normal deviates.
 *
 * Companion of letkf_amd_obsope.h (which it includes for the operator's structures).  The entries live in a library of
 * their own, libletkf_amd_osse.so, which links against libletkf_amd.so and uses its context, stream, scratch buffer,
 * operator and letkf_amd_last_error().  They stand where the obsmake program calls obsmake_cal
 * (scale/obs/obsope_tools.f90:767-1058):
 *   letkf_obsmake_slot_dev    one time slot of the loop at :812-987
 *   letkf_obsmake_noise_dev   the observation errors and the perturbation, :991-1049
 *   letkf_rand_* / letkf_randn_dev   com_rand / com_randn (common/common.f90:234-298) over SFMT19937 (common/SFMT.f90)
 * DESIGN.md section 14 has the details.  THE HOST'S PART: zeroing files->dat before the first slot (:807-809); the
 * MPI_REDUCE of dat over the subdomains (:1008) between the slots and the noise; write_obs_all (:1055); reading the nature
 * run (read_ens_history_iter, :817); the clock seed idate(8) + idate(7) * 1000 of com_randn, if the clock is wanted.
 * H08-format files are not passed (their records and operator are letkf_amd_h08.h; the reference marks obsmake for H08 unavailable).
 *
 * THE RANDOM STREAM.  letkf_rand is host state: the generator of one init_gen_rand(seed).
 *   letkf_rand_res53(r, n, out)   out (HOST) = the next n values of genrand_res53: com_rand without its clock seeding.
 *   letkf_randn_dev(ctx, r, n, out)   out (dev) = com_randn(n, out): 2 * ceil(n / 2) uniforms are consumed;
 *       out[2i] = sqrt(-2 log u1) * sin((2.0 * pi) * u2), out[2i + 1] = the same radius times the cosine; for odd n the
 *       last value is the sine of a fresh pair (:292-294).  log(0) follows IEEE as in the reference (u1 = 0 gives +inf).
 * Three properties of the reference are kept, bit for bit in the uniforms:
 *   conversion   genrand_res53 is dble(ishft(v, -1)) * (1d0 / 9223372036854775808d0) (SFMT.f90:730-736): the 63-bit integer
 *                is ROUNDED to double, so the low bits differ from the textbook (v >> 11) * 2^-53 and 1.0 is reachable.
 *   pi           3.1415926535d0 (common.f90:28), ten digits, in the angle (2.0d0 * pi) * rnd(2).
 *   parity flag  period_certification keeps its flag `inner` from call to call (SFMT.f90:436, an implicitly SAVEd
 *                variable).  The first init_gen_rand of a process starts from 0 and gives the published SFMT19937 state;
 *                THE LIBRARY'S STREAM IS THAT FIRST-CALL STREAM, for every letkf_rand_create.  (The obsmake program seeds once.)
 * Where each part runs: the SFMT recurrence is serial and runs on the host, filled in chunks into two pinned staging
 * buffers of the letkf_rand object and sent with hipMemcpyAsync on the context's stream, an event per buffer guarding its
 * reuse; Box-Muller is a device kernel, one lane per pair.  No device-wide synchronisation, nothing on the null stream.
 * letkf_rand_set_chunk(r, pairs) sets the staging chunk (pairs of uniforms per buffer, >= 1; default 262144); the results
 * do not depend on it.  One letkf_rand serves one context's device at a time.
 *
 * letkf_obsmake_slot_dev.  `op`, `files`, `f` are letkf_obsope_dev's arguments; f->nmem must be 1 (the nature run of the
 * slot).  For every file row n with s->slot_lb < s->dif[n] <= s->slot_ub (:825):
 *   own[n] == -1 (outside the global domain)   files->dat[n] = undef (-9.99e33) where s->outside_undef != 0, the
 *                                              myrank_d == 0 rule of :835-837; else untouched
 *   own[n] ==  1 (this subdomain's; own NULL: every row)   conventional file: phys2ijk, then Trans_XtoY (:858-862);
 *                radar file: phys2ijkz, then Trans_XtoY_radar (:866-872); dat[n] = H(x) where the qc is 0, else undef (:882-884)
 *   own[n] ==  0 (another subdomain's)         untouched
 * Every other row is untouched.  The operator is letkf_obsope_dev's in obsmake_cal's mode, which differs from obsope_cal:
 *   no USE_OBS test (op->use_obs is checked for presence, not read) and no RADAR_ZMAX test;
 *   qc 11 is NOT turned into 0 (:488 has no counterpart in :864-884): a reflectivity or Doppler-velocity row whose
 *   simulated reflectivity is below MIN_RADAR_REF becomes undef;
 *   so undef covers qc 10 (PS beyond ps_adjust_thres), 11, 20, 21, 98 and 90 (an element the operator does not cover).
 * op->rotc, where given, is indexed per FILE row here (there are no obsda rows).  counts (dev int64 [2], or NULL) =
 * {rows in the slot, rows processed}: nslot and nobs_slot of :826, :841, summed over the files.
 *
 * letkf_obsmake_noise_dev.  error = com_randn(nobsall) over all rows of all files in file order (:1002); per row n:
 *   err[n] by element (:1014-1037): U obserr_u, V obserr_v, T and Tv obserr_t, Q obserr_q, RH obserr_rh, PS obserr_ps,
 *   REF and RE0 obserr_radar_ref, Vr obserr_radar_vr; any other element: err[n] is left as it is;
 *   dat[n] = dat[n] + err[n] * error[n] where dat[n] != undef and err[n] != undef (:1039-1041), product and sum rounded
 *   separately.  A row that is skipped still owns its deviate.
 *
 * REFUSED with LETKF_E_INVALID and a letkf_amd_last_error() message, nothing written (and no uniform consumed):
 *   letkf_obsmake_slot_dev: whatever letkf_obsope_dev refuses (the report type of a processed row outside 1..nobtype
 *     among it, checked on the device before anything is written: the call's one read-back); f->nmem != 1; NULL s /
 *     s->dif / files->dat; slot_lb or slot_ub not finite, or slot_lb >= slot_ub.
 *   letkf_obsmake_noise_dev: NULL e / files / r; nfile outside 1..16, off NULL or descending; NULL files->elm / dat /
 *     err where there are rows.
 *   letkf_randn_dev, letkf_rand_res53: NULL r; n < 0; NULL out where n > 0.  letkf_rand_create: NULL r.
 *   letkf_rand_set_chunk: NULL r; pairs < 1.
 * Apart from the slot entry's read-back and the waits on the staging events everything is asynchronous on the context's
 * stream; every element has one writer and results are bitwise equal from call to call for the same seed.
 */
#ifndef LETKF_AMD_OBSMAKE_H
#define LETKF_AMD_OBSMAKE_H

#include "letkf_amd_obsope.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LETKF_AMD_OBSMAKE_VERSION 1

typedef struct letkf_rand letkf_rand;

int letkf_rand_create(int32_t seed, letkf_rand **r);
int letkf_rand_destroy(letkf_rand *r);
int letkf_rand_set_chunk(letkf_rand *r, int64_t pairs);
int letkf_rand_res53(letkf_rand *r, int64_t n, double *out);
int letkf_randn_dev(letkf_ctx *ctx, letkf_rand *r, int64_t n, double *out);

typedef struct {            /* one time slot of obsmake_cal */
  double slot_lb, slot_ub;  /* (islot - SLOT_BASE -+ 0.5) * SLOT_TINTERVAL: the rows with slot_lb < dif <= slot_ub */
  const double *dif;        /* dev, per file row: obs%dif */
  const int32_t *own;       /* dev, per file row, or NULL (all 1): 1 this subdomain's, 0 another's, -1 outside the domain */
  int32_t outside_undef;    /* myrank_d == 0: rows outside the global domain get undef */
  int32_t reserved0;
} letkf_obsmake_slot;

int letkf_obsmake_slot_dev(letkf_ctx *ctx, const letkf_obsmake_slot *s, const letkf_obsope_params *op,
                           const letkf_obs_file_rows *files, const letkf_obsope_fields *f, int64_t *counts);

typedef struct {            /* OBSERR_* of the namelist */
  double obserr_u, obserr_v, obserr_t, obserr_q, obserr_rh, obserr_ps, obserr_radar_ref, obserr_radar_vr;
} letkf_obsmake_err;

int letkf_obsmake_noise_dev(letkf_ctx *ctx, const letkf_obsmake_err *e, const letkf_obs_file_rows *files, letkf_rand *r);

#ifdef __cplusplus
}
#endif
#endif
