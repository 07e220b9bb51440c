/* letkf_amd_obsscan.h -- obsope_cal's first scan on the device: the subdomain and the time slot of every row of every
 * observation file, the bucket sort by (subdomain, slot) that makes obsda's set / idx, the count tables bsn / bsna and the qc of
 * the rows outside the window or the domain -- scale/obs/obsope_tools.f90:140-427 (all file:line below are in that file unless
 * noted) and rij_rank (scale/common/common_scale.f90:1728-1779).
 *
 * Companion of letkf_amd_obsope.h (which it includes for the operator's structs, and through it letkf_amd.h for letkf_ctx and
 * letkf_obs_file_rows).  The entries are exported by a library of their own, libletkf_amd_obsscan.so, which links against
 * libletkf_amd.so for the context, its stream and scratch buffer, letkf_amd_last_error() and the operator.  With it CALL
 * obsope_cal is replaced whole apart from file I/O and phys2ij / MPRJ_rotcoef, which are SCALE-RM's.  DESIGN.md section 18.
 *
 * letkf_obsscan_dev: ONE CALL covers all files and all subdomains.
 * INPUTS.  `files` as the operator takes it; only nfile (1..16), off (HOST), ri and rj are read.  dif: a device array per file
 * row.  The subdomain layout nlon, nlat, ihalo, jhalo, prc_num_x, prc_num_y (nprocs_d = prc_num_x * prc_num_y), the slots
 * slot_start, slot_end, slot_base, slot_tinterval (nslots = slot_end - slot_start + 1), HOST obsda_run[nfile] (non-zero = true)
 * or NULL for all true.
 *
 * PER FILE ROW, for every file whatever obsda_run says (:173-221)
 *   rank  rij_rank: -1 when ig < 1 + IHALO, ig > nlon * PRC_NUM_X + IHALO or the same test fails on jg; otherwise
 *         rank_i = ceiling((ig - IHALO - 0.5) / nlon) - 1, rank_j likewise, rank = rank_j * PRC_NUM_X + rank_i -- in double, in
 *         that order of operations, the division correctly rounded, no contraction.  NEW: a NaN coordinate gives -1 (the
 *         reference's CEILING is undefined there, and the operator gives such rows qc 98).
 *   slot  ceiling(dif / SLOT_TINTERVAL - 0.5) + SLOT_BASE (:256); outside SLOT_START .. SLOT_END it becomes SLOT_END + 1;
 *         rank == -1 gives SLOT_END + 2 and books the row under subdomain 0 (:251-262).  NEW: a non-finite dif, or
 *         |dif / T - 0.5| >= 2^30, gives SLOT_END + 1.
 * LISTS, over the rows of the files with obsda_run true: set / idx (dev, 1-based file and row, as letkf_obsope_dev and
 * letkf_set_obs_dev read them) in the order of the reference's obset_bufs / obidx_bufs: subdomain-major, then slot SLOT_START ..
 * SLOT_END + 2, and inside a bucket file order, then row order -- the scatter loop of :279-298 is stable.  qc (dev) per list
 * row is what the operator expects as INOUT: 0 in a slot, 97 (iqc_time) in the out-of-time bucket, 98 (iqc_out_h) in the
 * out-of-domain bucket (:413-427).  Their capacity is the number of rows of the obsda_run files.
 * TABLES, written to HOST memory, int32 as in the reference: bsn[nprocs_d][nslots + 2], bsna[nprocs_d][nslots + 3]; bsna[ip][0] is
 * bsna(SLOT_START-1, ip), the running offsets carry from one subdomain to the next (:269-277).  This is the entry's single
 * read-back and synchronisation; everything else is asynchronous on the context's stream.
 * OPTIONAL device outputs per file row (NULL allowed): rank (obs%rank), slot, and own for the subdomain myrank_d in the encoding
 * letkf_amd_obsmake.h documents: 1 when rank == myrank_d, -1 when rank < 0, 0 otherwise.
 * (obsmake_cal tests slot_lb < dif <= slot_ub (:825), which rounds differently from the ceiling formula:
 * letkf_obsmake_slot_dev keeps its own test.)
 *
 * HOW.  A lane per file row computes rank and the key ip * (nslots + 2) + bucket (rows of files that do not run: a key behind
 * all buckets); a stable radix sort of (key, flat row) over bit_length(buckets) bits; a lane per sorted position writes set, idx
 * and qc, and a lane per bucket finds bsna as the upper bound of its key in the sorted keys.  No counter is shared and every
 * value has one writer: results are bitwise equal from call to call.  No buffer is sized by rows x buckets; the workspace (16
 * bytes per file row, 4 per bucket and the sort's scratch) is the context's scratch buffer.
 *
 * REFUSED with LETKF_E_INVALID and a letkf_amd_last_error() message that names the argument, nothing written: a NULL ctx / p /
 * files / o, NULL off, bsn or bsna, a NULL ri / rj / dif with file rows, a NULL set / idx / qc with list rows; nfile outside
 * 1..16; nlon, nlat, prc_num_x or prc_num_y < 1; a negative halo; nlon * prc_num_x + ihalo or nlat * prc_num_y + jhalo of 2^31
 * or more; slot_start < 1 (slot 0 names the whole subdomain in letkf_obsscan_rows); slot_end < slot_start; slot_tinterval not
 * finite or <= 0; off not starting at 0, or decreasing; 2^31 file rows or more (idx is int32); nprocs_d * (nslots + 2) above
 * LETKF_OBSSCAN_MAX_BUCKETS; myrank_d outside 0 .. nprocs_d - 1 when own is asked for; a device output that overlaps a device
 * input.  With zero file rows the device arrays may be NULL and the tables come back all zero.
 *
 * letkf_obsscan_rows (host only): the list rows of subdomain ip in slot islot (SLOT_START .. SLOT_END + 2) as *first (0-based, in
 * the global lists) and *count; islot = 0 gives the whole subdomain -- the displacements and counts of the SCATTERV of :361-364.
 * letkf_obsscan_slot_bounds (host only): slot_lb / slot_ub [nslots] of :315-319.
 * letkf_obsope_slot_dev: the operator (letkf_obsope_dev's checks, kernel and read-back) on the list rows of subdomain ip in slot
 * islot (SLOT_START .. SLOT_END) of a scan's lists; p (ri_off / rj_off of that subdomain) and f are the operator's.  ensval is
 * indexed by the global list row, [row * kld + m0 + m].  A host that holds one slot's history fields at a time writes one call
 * per slot: the loop of :431-509.  An empty slot is no error and launches nothing.
 */
#ifndef LETKF_AMD_OBSSCAN_H
#define LETKF_AMD_OBSSCAN_H

#include "letkf_amd_obsope.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LETKF_AMD_OBSSCAN_VERSION 1
#define LETKF_OBSSCAN_MAX_BUCKETS 4194304   /* 2^22: nprocs_d * (nslots + 2); the sort key and a 16 MB table stay 32-bit */
#define LETKF_OBSSCAN_QC_TIME 97
#define LETKF_OBSSCAN_QC_OUT_H 98

typedef struct {          /* a host struct */
  const double *dif;                                  /* dev, per file row */
  const int32_t *obsda_run;                           /* HOST [nfile], or NULL: every file runs */
  int32_t nlon, nlat, ihalo, jhalo, prc_num_x, prc_num_y;
  int32_t slot_start, slot_end, slot_base, myrank_d;  /* myrank_d is read only when own is asked for */
  double slot_tinterval;
} letkf_obsscan_params;

typedef struct {
  int32_t *set, *idx, *qc;                            /* dev [rows of the obsda_run files] */
  int32_t *bsn;                                       /* HOST [nprocs_d][nslots + 2] */
  int32_t *bsna;                                      /* HOST [nprocs_d][nslots + 3] */
  int32_t *rank, *slot, *own;                         /* dev [file rows], each may be NULL */
} letkf_obsscan_out;

typedef struct {          /* what a scan left, as letkf_obsope_slot_dev takes it */
  int32_t nprocs_d, slot_start, slot_end, reserved0;
  const int32_t *bsna;                                /* HOST [nprocs_d][nslots + 3] */
  const int32_t *set, *idx;                           /* dev, the global lists */
  int32_t *qc;                                        /* dev, INOUT */
} letkf_obsscan_lists;

int letkf_obsscan_dev(letkf_ctx *ctx, const letkf_obsscan_params *p, const letkf_obs_file_rows *files, const letkf_obsscan_out *o);

int letkf_obsscan_rows(const int32_t *bsna, int32_t nprocs_d, int32_t slot_start, int32_t slot_end, int32_t ip, int32_t islot,
                       int64_t *first, int64_t *count);
int letkf_obsscan_slot_bounds(int32_t slot_start, int32_t slot_end, int32_t slot_base, double slot_tinterval, double *slot_lb,
                              double *slot_ub);

int letkf_obsope_slot_dev(letkf_ctx *ctx, const letkf_obsscan_lists *l, int32_t ip, int32_t islot, const letkf_obsope_params *p,
                          const letkf_obs_file_rows *files, const letkf_obsope_fields *f, double *ensval, int64_t kld);

#ifdef __cplusplus
}
#endif
#endif
