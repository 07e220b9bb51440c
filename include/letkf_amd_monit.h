/* letkf_amd_monit.h -- the departure monitor monit_obs on the device: the mean state to history fields, then O-B / O-A.
 *
 * Companion of letkf_amd_obsope.h (which it includes for the operator's structures).  Two device entries and one host
 * helper stand where write_ensmean(..., monit_step=1) and write_ens_mpi(..., monit_step=2) call monit_obs
 * (scale/common/common_mpi_scale.f90:1481-1633, scale/common/common_obs_scale.f90:1370-1844) under DEPARTURE_STAT:
 *   letkf_state_to_history_dev   state_to_history (common_scale.f90:1292-1400) with scale_calc_z (:1434-1459)
 *   letkf_monit_obs_dev          the loop of monit_obs (common_obs_scale.f90:1467-1599) and its monit_dep (:1819)
 *   letkf_monit_type             the list of monitored elements (:1821-1837)
 * DESIGN.md section 13 has the details.  The ranks' MPI_ALLREDUCE of the statistics, the MPI_GATHERV of the records,
 * write_obs_dep, the LOG_LEVEL >= 3 prints, DEPARTURE_STAT_H08 and the TC vitals stay the host's (the H08 operator itself is
 * letkf_amd_h08.h).
 *
 * letkf_state_to_history_dev.  Writes member slot 0 of the layout `layout` describes (dimensions, halos, the strides
 * s3k .. s3v and s2i .. s2v, nv3dd >= 13, nv2dd >= 7) into v3d / v2d; layout->v3d, v2d, nmem, m0, s3m and s2m are not read.
 *   interior, 3-D   the 11 state variables (iv3d_* order u v w t p q qc qr qi qs qg) into their iv3dd_* slots (:1316-1326);
 *                   height (slot 13) = ((ztop - topo) / ztop) * cz[k] + topo, evaluated in that order without contraction
 *                   (:1452); RH (slot 12) = 0
 *   2-D             topo = the height of the first model level (:1342); ps, u10m, v10m, t2m, q2m = level-1 p, u, v, t, q
 *                   (:1345-1349); rain = 0; slots beyond the seventh are not written
 *   vertical halo   levels below khalo repeat the first model level, levels above the last one, all 13 slots (:1371-1379)
 *   lateral halo    on a side whose edge_fill bit is set (bit 0 west = low i, 1 east, 2 south = low j, 3 north) the halo
 *                   columns -- all levels, both arrays, a corner where both of its sides are set -- repeat the nearest
 *                   interior column; on a side whose bit is clear nothing is written, so the host's own halo exchange
 *                   can fill those columns before or after the call.
 * THE LATERAL HALO IS THE LIBRARY'S DEFINITION: the reference calls COMM_vars8 / COMM_wait of SCALE-RM there
 * (:1385-1397), which are not part of the reference tree; replication is what a domain boundary without a neighbour
 * needs for the operator's clamped reads, and a periodic or nested boundary is the host's exchange.
 *
 * letkf_monit_obs_dev.  For n = 0 .. nn - 1: r = key[n] (key NULL: r = n), the file row fr = (set[r], idx[r]) of `files`.
 * `op` and `f` are letkf_obsope_dev's arguments and are honoured as given (monit_obs passes stggrd = 1; use_obs and
 * radar_zmax cannot bite on rows that passed set_letkf_obs); f->nmem must be 1.  Per row (:1529-1581):
 *   t_range > 0 and |dif[fr]| > t_range     this step's qc -1, departure undef (-9.99e33)
 *   else qc = 90, then                       conventional file: the operator's qc and H(x)
 *                                            radar file: the operator's (qc 11 becomes 0) where departure_stat_radar != 0
 *   qc == 0: departure = files->dat[fr] - H(x); else undef (qc 10 PS beyond ps_adjust_thres, 20 / 21 / 98, 90)
 * files->dat is read as letkf_set_obs_dev left it (reflectivities in dBZ): call after it.
 *   step 1   rec->set[n] = set[r], rec->idx[n] = idx[r], rec->qc[n] = qc, rec->omb[n] = departure
 *   step 2   rec->oma[n] = departure; rec->qc[n] = qc only where rec->qc[n] == 0 (:1577-1579)
 * nobs, bias, rmse (dev [nid]) are monit_dep over THIS step's qc and departures with element files->elm[fr], Tv counted as
 * T and RE0 as REF, summed in letkf_monit_dep_dev's order.  nn == 0: counts 0, bias and rmse undef, nothing else written.
 * key indexes set / idx (and op->rotc, which is per obsda row like them), whose length the library does not know: an entry
 * beyond them is the caller's error.
 *
 * WHERE THE REFERENCE IS UNDEFINED.  (1) state_to_history leaves the RH slot and the rain slot uninitialised: they are 0
 * here.  (2) monit_obs leaves obsdep_qc / obsdep_omb / obsdep_oma of a row outside DEPARTURE_STAT_T_RANGE uninitialised:
 * here step 1 writes qc -1 and omb undef, step 2 writes oma undef.
 *
 * REFUSED with LETKF_E_INVALID and a letkf_amd_last_error() message, nothing written.
 *   letkf_state_to_history_dev: a NULL argument (s, layout, v3d, v2d, x, topo, cz); a zero stride; nv3d < 11; edge_fill
 *     outside 0..15; ztop not finite or <= 0; khalo < 1; nlev, nlon, nlat < 1 or a negative halo; nv3dd < 13 or nv2dd < 7.
 *   letkf_monit_obs_dev: whatever letkf_obsope_dev refuses; f->nmem != 1; step outside 1..2; nid outside 1..32; NULL mp /
 *     elem_uid / rec or any of its five arrays / nobs / bias / rmse; files->dat NULL; t_range > 0 with dif NULL; nn < 0;
 *     and, on the device before anything is written, folded into the operator's one read-back: a negative key entry.
 * Apart from that read-back everything is asynchronous on the context's stream, every element has one writer, and
 * results are bitwise equal from call to call.
 */
#ifndef LETKF_AMD_MONIT_H
#define LETKF_AMD_MONIT_H

#include "letkf_amd_obsope.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LETKF_AMD_MONIT_VERSION 1

typedef struct {            /* one state (the ensemble mean) on the device, and what scale_calc_z needs */
  int32_t nv3d;             /* >= 11, the reference's iv3d_* order: u v w t p q qc qr qi qs qg */
  int32_t edge_fill;        /* bit 0 west, 1 east, 2 south, 3 north: that side is a domain boundary */
  const double *x;          /* dev; element (i, j, lev, v) at x[i*si + j*sj + lev*sl + v*sv], 0-based */
  int64_t si, sj, sl, sv;   /* none 0.  gues3d(ij,lev,mmean,v): 1, nlon, nij1, nij1*nlev*nens, x = base + mmean*sm */
  const double *topo;       /* dev [nlat][nlon], i fastest */
  const double *cz;         /* HOST [nlev]: GRID_CZ(k + KHALO) */
  double ztop;              /* GRID_FZ(KE) - GRID_FZ(KS-1) */
} letkf_hist_state;

int letkf_state_to_history_dev(letkf_ctx *ctx, const letkf_hist_state *s, const letkf_obsope_fields *layout,
                               double *v3d, double *v2d);

typedef struct {
  int32_t step;                  /* 1 = guess (O-B), 2 = analysis (O-A) */
  int32_t departure_stat_radar;  /* DEPARTURE_STAT_RADAR */
  int32_t nid, reserved0;
  const int32_t *elem_uid;       /* HOST [nid], as letkf_monit_dep_dev */
  double t_range;                /* DEPARTURE_STAT_T_RANGE; <= 0: every row */
  const double *dif;             /* dev, per file row: obs%dif; may be NULL when t_range <= 0 */
} letkf_monit_params;

typedef struct { int32_t *set, *idx, *qc; double *omb, *oma; } letkf_obsdep;   /* dev [nn] each; INOUT across the two steps */

int letkf_monit_obs_dev(letkf_ctx *ctx, const letkf_monit_params *mp, const letkf_obsope_params *op,
                        const letkf_obs_file_rows *files, const letkf_obsope_fields *f,
                        int64_t nn, const int32_t *key, const int32_t *set, const int32_t *idx,
                        const letkf_obsdep *rec, int32_t *nobs, double *bias, double *rmse);

int letkf_monit_type(int32_t nid, const int32_t *elem_uid, int32_t departure_stat_radar, int32_t departure_stat_h08,
                     int32_t *monit_type);          /* HOST only: common_obs_scale.f90:1821-1837 */

#ifdef __cplusplus
}
#endif
#endif
