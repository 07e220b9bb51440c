/* letkf_amd_interp_window.h -- weight interpolation on a tile of a larger domain: one coarse lattice for the whole domain,
 * a call analyses a window of it.
 *
 * Second companion of letkf_amd.h, beside letkf_amd_interp.h (which it includes and whose semantics it keeps: GRID, COARSE
 * SOLVES, FINE POINTS and OUTPUTS there hold here word for word unless stated otherwise).  letkf_das_interp_dev anchors
 * its coarse set on the rectangle it is given, so two tiles of one domain get two lattices and the stitched analysis
 * changes with the decomposition.  Here the lattice belongs to the domain and the stitched analysis is the single-domain
 * one bit for bit ("Tiles").
 *
 * ARRAYS.  interp->nx, ny, nlev are the extents of the arrays the call is handed -- rig / rjg / rlev / rz, beta, infl,
 * the strided state, npts = nx*ny*nlev: the owned rectangle plus whatever halo the host chose.  Everything in
 * letkf_das_args and letkf_interp_args keeps its meaning.  The window places the arrays in the domain (array column
 * (0, 0) is global column (gi0, gj0)) and names the owned rectangle [oi0, oi0+onx) x [oj0, oj0+ony) in array indices.
 *
 * LATTICE.  Along x the global coarse lines are L = letkf_interp_coarse_axis(gnx, stride_x), along y the same with gny
 * and stride_y.  With the owned global range [p, q] = [gi0+oi0, gi0+oi0+onx-1] the call's coarse lines are
 *   { l in L : p <= l <= q },  plus the predecessor of p in L if p is not in L,  plus the successor of q in L if q is not:
 * a contiguous run of L, exactly the lines that carry non-zero weight at some owned point.  letkf_interp_window_axis
 * returns them as ascending array indices (global - g0).  Applying the cell rule of letkf_amd_interp.h to this run (the
 * lines i = b belong to the next cell, except in the last cell of the run) gives every owned point the corners, the
 * weight values and the corner order it has on the global lattice; every cell of the run holds an owned point.
 *
 * COARSE SOLVES happen at the call's coarse columns (ncx_w x ncy_w of them), all levels, exactly as in
 * letkf_das_interp_dev: column search on them, dense gather, cold letkf_core, rho from the coarse point's own slot.
 * Outside the owned rectangle the call READS ONLY COARSE COLUMNS: rig, rjg, rlev, rz, the inflation slots and, when
 * q_update_top > 0, the mean of variable iv_p.  No other halo element is touched, so the host fills nothing else.  The
 * search tables must hold every observation within the cut-off of those columns: with per-rank tables, the extended
 * subdomain reaches the cut-off plus stride-1 columns.
 *
 * FINE POINTS.  Only owned points are analysed: anal, rtps_infl_out and status are written at owned points only (array
 * indexing, p = i + nx*j + nx*ny*lev).  nobs_coarse is [ncx_w*ncy_w*nlev] over the call's own coarse set.  anal == gues
 * stays allowed: halo coarse columns are read, never written.
 *
 * REFUSED with LETKF_E_INVALID, nothing written: everything letkf_das_interp_dev refuses; a window extent < 1; the array
 * rectangle not inside the domain (gi0 < 0 or gi0 + nx > gnx, y likewise); the owned rectangle not inside the arrays; a
 * needed coarse line outside the arrays (letkf_amd_last_error names the axis and the global line).
 *
 * window == NULL is the whole array as the whole domain: letkf_das_interp_dev, which is a call of this entry with that
 * window.  Results are bitwise equal from call to call, for any slab cut and for any window that owns the point.
 */
#ifndef LETKF_AMD_INTERP_WINDOW_H
#define LETKF_AMD_INTERP_WINDOW_H

#include "letkf_amd_interp.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LETKF_AMD_INTERP_WINDOW_VERSION 1

typedef struct {
  int32_t gnx, gny;   /* columns of the whole domain */
  int32_t gi0, gj0;   /* global index of the arrays' column (0, 0): 0 <= gi0, gi0 + nx <= gnx (y likewise) */
  int32_t oi0, oj0;   /* first owned column, in array indices */
  int32_t onx, ony;   /* owned extent: the points this call analyses */
} letkf_interp_window;

/* Host only.  The coarse lines of one axis that a window needs, as ascending array indices idx[0 .. *count): gn the
 * domain's extent, g0 the global index of array index 0, n the arrays' extent, [o0, o0 + on) the owned range in array
 * indices.  idx holds on + 2 entries at the most; idx may be NULL to ask for the count alone.  LETKF_E_INVALID for
 * gn, stride, n or on < 1, g0 < 0, g0 + n > gn, o0 < 0, o0 + on > n, or a needed line outside [0, n). */
int letkf_interp_window_axis(int32_t gn, int32_t stride, int32_t g0, int32_t n, int32_t o0, int32_t on, int32_t *idx,
                             int32_t *count);

/* The analysis of the window by weight interpolation on the domain's lattice.  letkf_ctx_last_path names the route as
 * letkf_das_interp_dev does. */
int letkf_das_interp_window_dev(letkf_ctx *ctx, const letkf_das_args *args, const letkf_search_tables *tables,
                                const letkf_interp_args *interp, const letkf_interp_window *window);

#ifdef __cplusplus
}
#endif
#endif
