/* letkf_amd_superob.h -- superob on the device: the raw observations of all time slots reduced to at most one per grid cell
 * (or to the best ones), before the operator sees them.
 *
 * Companion of letkf_amd.h (which it includes for letkf_ctx).  The entries are exported by a library of their own,
 * libletkf_amd_superob.so, which links against libletkf_amd.so for the context, its stream and scratch buffer and
 * letkf_amd_last_error().  One call of letkf_superob_dev is the four stages of scale/obs/superob.f90 (all file:line below are
 * in that file unless noted) restated for SCALE's regional grid; the reference itself is bound to common_gfs, which is not in
 * its tree, and is in no PROGS list.  DESIGN.md section 16 has the details.
 *
 * INPUTS.  nobs rows as device arrays: elm (raw element id), typ (1..nobtype), lon, lat, lev, dat, err and the grid coordinates
 * ri, rj, rk (cell centres are the integers 1..nlon, 1..nlat, 1..nlevx; phys2ij / phys2ijk stay the host's, as in the operator).
 * HOST slot_off[nslots + 1]: the rows of slot s (1-based) are slot_off[s-1] .. slot_off[s]-1, the slot-by-slot read of :254-266.
 * HOST elem_uid[nid]: an id that is not in it has uid 0.  surface_typ_mask: bit t-1 set makes report type t a surface type
 * (the reference's set {8,9,10,11,15}, :289-291, is 0x4780).  Four HOST method tables method_g/v/t/h[nid * nobtype], element
 * (uid-1) * nobtype + (typ-1): the memory order of obmethod_*(nobtype, nid_obs).
 *
 * STAGE 1, per row, in this order (:281-379)
 *   1. a non-finite ri / rj / rk, or one of magnitude >= 2^30: qc 6 (NEW: the reference's floor() is undefined there)
 *   2. i, j, k = floor(r + 0.5)                                                                           (:281-283)
 *   3. a surface type or elm > 9999: k = 0; otherwise k < 1 becomes 1 and ceiling(rk) > nlevx gives qc 3  (:289-307)
 *   4. still 0: ceiling(rj) < 2 or > nlat gives qc 2                                                      (:309, :326)
 *   5. still 0: the same test on ri with nlon gives qc 2 (replaces the global longitude wrap of :285-286, which a regional
 *      domain does not have)
 *   6. still 0: a valid typ / uid with method_g == 1 gives qc 4                                           (:344)
 *   7. still 0: typ outside 1..nobtype or uid 0 gives qc 5 (:362).  The reference indexes its tables out of bounds for such
 *      rows; here their method lookups read 0 and they never join a record.
 * STAGE 2, vertical (:383-523).  A record is a maximal run of >= 2 consecutive rows of one slot in which every row after the
 *   first has method_v > 0 and equals the first row in lon, lat (as doubles), uid and typ (:384-386).  For k = 0..nlevx
 *   ascending, the record's rows with that k and qc 0, in row order, are one group (:395-410); a group of more than one row goes
 *   through superob_select with method_v and the first row's i, j (:411-421).  The mm resulting rows overwrite lon, lat, lev, dat,
 *   err, ri, rj, rk, k of the record's first mm positions (:429-437; i and j are NOT rewritten, as in the reference); every row of
 *   the record gets qc 9 (:425, those that had 2 or 3 too) and the first mm then qc 0 (:438).
 *   A result that lands on a position whose own i / j lies outside the grid gets qc 2 and counts in nobsrdc_bd (NEW: possible
 *   only where rows of one lon / lat carry different ri / rj, which phys2ij never makes; the reference indexes nobsgrd out of
 *   bounds there).
 *   REPAIR 1: the flush at the end of a slot ends at the slot's last row; the reference's recend = nn + n (:464) is one past it.
 *   REPAIR 2: there is no max_platform_reclen; the reference overflows tmp3* above 1000 rows.
 * superob_select(m, i, j, k, method), superob_tools.f90:21-140, literally.  err_min and dist_min start at the SINGLE-precision
 *   literal 1.e20 widened to double (:49, :56, :69).  Method 2 uses all rows, err_min = the smallest err below that start.
 *   Methods 1 and 3 use the rows whose err == the running minimum, a strictly smaller err restarts the list (:57-66).  Method 1
 *   keeps the first row of strictly smallest dist = sqrt(dx*dx + dy*dy [+ dz*dz unless k == 0]), dx = ri - i ... (:70-85).
 *   n_use > 1: the means of ri, rj, rk, lon, lat, lev, dat, each a sequential sum from 0.0 in list order divided by
 *   real(n_use), and err = err_min (:101-125).  n_use == 1: that row's own values (:126-134).  n_use == 0 (every err >= 1e20f
 *   or NaN) leaves the group's first row unchanged; for method 1 the reference reads an unset n_min there.  Method 0 keeps the
 *   group whole.  The result is bitwise the statement's: no contraction, correctly rounded division and sqrt.
 * STAGE 3, temporal (:571-761).  The qc-0 rows in (typ, uid, slot, k, j, i, row) order; for (typ, uid) with method_t > 0, per
 *   cell (typ, uid, k, j, i): under method 2 every row outside the first-priority slot is flagged 2 (:657-659); every other row
 *   is flagged 1 if an earlier row of the cell -- by slot priority, then by row, flagged or not; under method 2 only the
 *   first-priority slot's rows -- has identical lon, lat and lev as doubles (:679-709).
 * STAGE 4, all grid (:770-948).  The rows still at 0; for each cell (typ, uid, slot, k, j, i) with method_h > 0, m > 1 goes
 *   through superob_select centred on the cell's own i, j, k, and the output row carries the cell's i, j, k (:849-884).
 *   method_h == 0 keeps the rows as they are.
 *   REPAIR 3: the reference's copy at :909 starts from a stale loop index i; here the window is the rows :907 counts.
 *
 * OUTPUTS, device arrays of capacity nobs.  The surviving rows in (slot, typ, uid, k, j, i, in-cell row) order -- the
 * reference's supTT.dat files one after another: elm (the raw id elem_uid[uid-1]), typ, slot (1-based), lon, lat, lev, dat, err,
 * ri, rj, rk, i, j, k; nout [1]; and, each optional (NULL): slot_off_out [nslots + 1]; qc1 [nobs], the qc by position after
 * stages 1-2; counts [7] = nobsrdc_bd, _g, _tp, _v, _t, _h as the reference prints them (:555-558, :757, :950) and the number of
 * qc 6 rows; obsnum [4][nid][nobtype], print_obsnum's tables at the program's four points (:544, :562, :761, :954) over valid
 * typ / uid only.
 * What stays the host's: the log files 81-85, the density grid, reading files, and the unit conversions and single-precision
 * records of :964-1000.
 *
 * REFUSED with LETKF_E_INVALID and a letkf_amd_last_error() message, nothing written: a NULL ctx / p / o or a NULL array other
 * than the optional outputs (with nobs = 0 the row arrays may be NULL); nobs outside 0..2^31-1; an extent < 1; nslots outside
 * 1..64; nbslot outside 1..nslots; nobtype or nid outside 1..32; a method outside its range (g 0..1, v and h 0..3, t 0..2);
 * slot_off not starting at 0, decreasing, or not ending at nobs; nslots * nobtype * nid * (nlevx+1) * nlat * nlon of 2^62 or
 * more (the cell key); an output overlapping an input.
 * There is no read-back and no synchronisation: every stage runs over nobs-sized buffers with device-side counts, asynchronous
 * on the context's stream.  No buffer is sized by the number of cells.  The workspace is the context's scratch buffer.  Every
 * value has one writer, the counters are integer sums: results are bitwise equal from call to call.
 */
#ifndef LETKF_AMD_SUPEROB_H
#define LETKF_AMD_SUPEROB_H

#include "letkf_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LETKF_AMD_SUPEROB_VERSION 1
#define LETKF_SUPEROB_MAX_SLOTS 64
#define LETKF_SUPEROB_MAX_TYPES 32

typedef struct {          /* a host struct; slot_off, elem_uid and the method tables are HOST arrays, the rest device arrays */
  int64_t nobs;
  const int32_t *elm, *typ;                                   /* dev [nobs] */
  const double *lon, *lat, *lev, *dat, *err, *ri, *rj, *rk;   /* dev [nobs] */
  const int64_t *slot_off;                                    /* HOST [nslots + 1] */
  int32_t nlon, nlat, nlevx, nslots, nbslot, nobtype, nid, surface_typ_mask;
  const int32_t *elem_uid;                                    /* HOST [nid] */
  const int32_t *method_g, *method_v, *method_t, *method_h;   /* HOST [nid * nobtype] */
} letkf_superob_params;

typedef struct {          /* device arrays */
  int32_t *elm, *typ, *slot;                                  /* [nobs] */
  double *lon, *lat, *lev, *dat, *err, *ri, *rj, *rk;         /* [nobs] */
  int32_t *i, *j, *k;                                         /* [nobs] */
  int64_t *nout;                                              /* [1] */
  int64_t *slot_off_out;                                      /* [nslots + 1], or NULL */
  int32_t *qc1;                                               /* [nobs], or NULL */
  int64_t *counts;                                            /* [7], or NULL */
  int64_t *obsnum;                                            /* [4][nid][nobtype], or NULL */
} letkf_superob_out;

int letkf_superob_dev(letkf_ctx *ctx, const letkf_superob_params *p, const letkf_superob_out *o);

/* Host only: the reference's hard-coded tables (:120-151) for report types 1..nobtype and nid elements, each [nid * nobtype];
 * a type the tables name beyond nobtype is left out. */
int letkf_superob_default_methods(int32_t nobtype, int32_t nid, int32_t *method_g, int32_t *method_v, int32_t *method_t, int32_t *method_h);
/* Host only: slot_priority[nslots] (:164-175, 1-based slots): the nearest slot to nbslot first, the lower slot on ties. */
int letkf_superob_slot_priority(int32_t nslots, int32_t nbslot, int32_t *slot_priority);

#ifdef __cplusplus
}
#endif
#endif
