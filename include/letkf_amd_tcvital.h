/* letkf_amd_tcvital.h -- TC vitals on the device: the background cyclone's centre and central pressure for every member, the link
 * of the observation operator that letkf_obsope_dev leaves at qc 90.  The reference's version is search_tc_subdom + wgt_ave2d
 * (scale/common/common_obs_scale.f90:2686-2768) and the block around it in obsope_cal (scale/obs/obsope_tools.f90:118-204,
 * :650-710); it is commented out there and marked tentative, so this header states the mathematics it computes.  DESIGN.md
 * section 22.
 *
 * Companion of letkf_amd_obsope.h (which it includes for letkf_obsope_fields).  The entries are exported by a library of their
 * own, libletkf_amd_tcvital.so, which links against libletkf_amd.so for the context, its stream, its scratch buffer and
 * letkf_amd_last_error().
 *
 * THE ORDER OF CALLS for a file with a TC triplet: the record codec's decode (x / y in metres, OBSERR_TCX/TCY/TCP), the
 * projection's phys2ij, the first scan, the operator for all members (the three rows get qc 90), then
 *   letkf_tcvital_rows_dev    which rows, and whether they are a report of this slot        (obsope_tools.f90:154-204, :651-656)
 *   letkf_tcvital_search_dev  per rank: the candidate of every member in that subdomain     (search_tc_subdom)
 *   (the host's all-gather of the ranks' candidates)
 *   letkf_tcvital_fill_dev    the pick among the ranks and the three obsda rows             (:678-703)
 * and set_letkf_obs, which applies GROSS_ERROR_TCX/TCY/TCP.
 *
 * letkf_tcvital_rows_dev(ctx, n, elm, dif, slot_lb, slot_ub, rows, valid)
 *   elm    dev int32 [n], dif dev double [n]: the decoded columns of one file
 *   rows   HOST int64 [3]: the LAST 1-based row whose element is 99991 (TCX), 99992 (TCY), 99993 (TCP), or 0
 *   valid  HOST int32: 1 only when all three rows exist, dif(x) == dif(y) == dif(p) and slot_lb < dif(x) <= slot_ub
 *   One pass over elm (a maximum of three row numbers), a gather of the three dif, one read-back.  n = 0 is legal: rows 0, valid 0.
 *
 * letkf_tcvital_search_dev(ctx, p, f, ritc, rjtc, cand)
 *   p      HOST: dx, dy, cxg1, cyg1 as in letkf_amd_mapproj.h; i_off, j_off (rank_i * nlon, rank_j * nlat); tc_search_dis (m)
 *   f      of which only v2d, its strides, nlon, nlat, ihalo, jhalo, nv2dd and nmem are read; nv2dd >= 7 (topo = 1, ps = 2,
 *          t2m = 6, q2m = 7, the reference's order)
 *   ritc, rjtc   DEVICE pointers to one double each: the global grid coordinates of the TCX row, as phys2ij left them (no
 *          read-back: the entry is asynchronous on the context's stream)
 *   cand   dev [nmem][3] = (tcx m, tcy m, mslp Pa)
 *   Per member:
 *   slp of an array cell:  p = ps; dz = -1.0 * topo; if (dz != 0) { tv = t2m * (1 + 0.608 q2m);
 *          p = p * pow((-gamma * dz + tv) / tv, gg / (gamma * rd)) }, gamma = 5e-3, gg = 9.81, rd = 287.05 (prsadj; topo = 0
 *          leaves ps bit for bit)
 *   s of an interior cell (i, j), 1 <= i <= nlon, 1 <= j <= nlat, array element (i + ihalo, j + jhalo):  with ihalo >= 2 and
 *          jhalo >= 2, s = (c * 5 + (S3 - c) * 3 + (S5 - S3)) / 45 with c the cell's slp and S3, S5 the sums of slp over the 3 x 3
 *          and 5 x 5 blocks around it, each summed row by row in array order; otherwise s = slp
 *   disc:  ig = i + i_off, jg = j + j_off; xdis = |ig - ritc| * dx, ydis = |jg - rjtc| * dy, rdis = sqrt(xdis * xdis + ydis * ydis),
 *          every operation rounded on its own; the cell is out where rdis > tc_search_dis, or where ritc or rjtc is a NaN
 *   winner:  the lowest s below 9.99e33; among equal s the lowest j, then the lowest i; a NaN s never wins
 *   result:  tcx = (ig - 1) * dx + cxg1, tcy = (jg - 1) * dy + cyg1 (rounded term by term), mslp = s; no winner: 9.99e33 thrice
 *   WHERE THE REFERENCE IS NOT FOLLOWED.  (1) It reads v2d(il, jl) with il = 1..nlon on the array with halo and hands the same il
 *   to ij_l2g: the field is shifted by the halo against the coordinates; here the cell is read at (i + ihalo, j + jhalo), as
 *   obssim_cal does (obsope_tools.f90:1105).  (2) It searches IHALO+1 .. nlon-IHALO only; here every interior cell is searched and
 *   the stencil reaches into the halo, which the host fills as for the operator, so a decomposed grid gives the bits of the
 *   undivided one.  (3) With a NaN centre every cell is inside its disc (NaN > x is false); here none is.  (4) bTC_proc is
 *   uninitialised when no rank is below 1100 hPa; here the values are undef and the rows qc 50 (fill, below).  (5) Its
 *   MPI_ALLREDUCE(MIN) over bTC is an all-gather, each column having one writer: the host gathers, the library picks.
 *   Two kernels, no atomics: a partial per tile and member, then one reduction per member in a fixed order; results are
 *   bitwise equal from call to call.  A tile wholly outside the disc is left after the centre is read, on the device.
 *
 * letkf_tcvital_fill_dev(ctx, nproc, nmem, m0, cand_all, rows, qc_replace, qc, ensval, kld)
 *   cand_all  dev [nproc][nmem][3]: every rank's cand, rank-major (nproc = 1: cand itself)
 *   rows      HOST int64 [3]: the 0-based obsda rows of TCX, TCY, TCP on this rank; negative: not on this rank, nothing written
 *   Per member the best starts at 1100.0e2 and the first rank n = 0..nproc-1 with mslp < best takes over (ties: the lowest
 *   rank).  ensval[rows[c] * kld + m0 + m] is the picked rank's component c, or undef (-9.99e33) when no rank qualified.
 *   qc of the three rows: t = 50 (iqc_obs_bad) if any member of the call had no rank below the cap, else 0; qc = t with
 *   qc_replace != 0 (the call that takes over from the operator's 90), qc = max(qc, t) otherwise (member by member).
 *   One kernel, asynchronous, one writer per value.
 *
 * REFUSED with LETKF_E_INVALID and a letkf_amd_last_error() message, nothing written: a NULL argument; nmem < 1; m0 < 0 or
 * m0 + nmem > kld; nproc < 1; a zero stride; nlon or nlat < 1 or a negative halo; nv2dd < 7; dx, dy or tc_search_dis not
 * finite, dx or dy <= 0, tc_search_dis < 0; n < 0; slot_lb > slot_ub; more tiles times members than one grid holds (2^31 - 1).
 */
#ifndef LETKF_AMD_TCVITAL_H
#define LETKF_AMD_TCVITAL_H

#include "letkf_amd_obsope.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LETKF_AMD_TCVITAL_VERSION 1
#define LETKF_TCVITAL_ID_TCX 99991
#define LETKF_TCVITAL_ID_TCY 99992
#define LETKF_TCVITAL_ID_TCP 99993
#define LETKF_TCVITAL_QC_BAD 50

typedef struct {          /* a host struct */
  double dx, dy, cxg1, cyg1;          /* as in letkf_mapproj_params */
  int32_t i_off, j_off;               /* rank_i * nlon, rank_j * nlat */
  double tc_search_dis;               /* TC_SEARCH_DIS, metres */
} letkf_tcvital_params;

int letkf_tcvital_rows_dev(letkf_ctx *ctx, int64_t n, const int32_t *elm, const double *dif, double slot_lb, double slot_ub,
                           int64_t *rows, int32_t *valid);

int letkf_tcvital_search_dev(letkf_ctx *ctx, const letkf_tcvital_params *p, const letkf_obsope_fields *f, const double *ritc,
                             const double *rjtc, double *cand);

int letkf_tcvital_fill_dev(letkf_ctx *ctx, int32_t nproc, int32_t nmem, int32_t m0, const double *cand_all, const int64_t *rows,
                           int32_t qc_replace, int32_t *qc, double *ensval, int64_t kld);

#ifdef __cplusplus
}
#endif
#endif
