/* letkf_amd_interp.h -- weight interpolation: letkf_core on every s-th column, the analysis at every point.
 *
 * Companion of letkf_amd.h (which it includes for letkf_ctx, letkf_das_args and letkf_search_tables).  The reference has
 * no such switch: these semantics are this library's own (Yang et al. 2009, QJRMS 135: the transform T and the mean
 * weights w-bar vary smoothly in space, so they are solved on a coarse set and interpolated).  DESIGN.md section 11 has
 * the derivations.
 *
 * GRID.  A rectangular tile of nx x ny columns and nlev levels; point p = i + nx*j + nx*ny*lev (i fastest), so
 * nij1 = nx*ny and args->npts = nx*ny*nlev.  rig / rjg [nx*ny], rlev / rz [npts], beta, infl and the strided state are
 * exactly what letkf_das_columns_dev takes.
 *
 * COARSE SET.  Along x the coarse indices are {0, s_x, 2 s_x, ...} united with {nx-1}, along y likewise with s_y
 * (letkf_interp_coarse_axis; ncx and ncy of them).  Every level is solved: no vertical interpolation.  A stride larger
 * than the extent leaves the two ends, or the one column where the extent is 1.
 *
 * COARSE SOLVES.  At every coarse point (cx, cy, lev) the library runs obs_local (the column search of
 * letkf_obs_search_columns_dev on the coarse columns) and letkf_core (the solver routes of letkf_core_batch_dev, every
 * solve cold) and keeps T [k][k], w-bar [k] and, under det_run, w-bar_det [k].  rho is the coarse point's own inflation
 * slot: that of its first updated variable (var_mask, Q_UPDATE_TOP on its own mean pressure), 1 where it updates none.
 * beta is taken as 1 there: a coarse point with beta = 0 is solved like any other, since its neighbours may need it.
 * The levels go in slabs whose lists (20 B per entry), kept results ((k*k + 2k) doubles per coarse point) and gathered
 * observation rows fit ws_bytes of library workspace (0: 8 GiB); a slab has at least one level.
 *
 * FINE POINTS.  A cell is the rectangle between coarse neighbours a <= i <= b, c <= j <= d.  With
 *   wx = (i - a) / (b - a)  (0 where b == a),  wy = (j - c) / (d - c)  (0 where d == c)
 * the four corners (a,c), (b,c), (a,d), (b,d) weigh (1-wx)(1-wy), wx (1-wy), (1-wx) wy, wx wy.  A corner of weight 0
 * is not read (a point on a coarse line uses two corners, a coarse point one).  T~ = sum w_c T_c, and w-bar,
 * w-bar_det are blended with the same weights.  Every fine point belongs to one cell: the lines i = b and j = d belong
 * to the next cell, except in the last cell of a direction.
 * Then the rules of the das_letkf loop body apply at the fine point with its own data: Q_UPDATE_TOP on its own mean
 * pressure, relax_parm from its own inflation slot, RTPP as in letkf_das_points_dev, RTPS with var_g = |x'|^2 and
 * var_a = |T~^T x'|^2 / (k-1) (T^2 = (k-1) Pa, so this is x'^T Pa x' at stride 1, to rounding), beta, the analysis
 * value, the deterministic member and the q-spread clamp.  beta = 0 points copy the first guess.
 *
 * OUTPUTS.  anal (anal == gues allowed), rtps_infl_out, status[npts] = the largest letkf_core status among the
 * corners used with non-zero weight (0 at beta = 0 points), optional nobs_coarse.
 *
 * REFUSED with LETKF_E_INVALID, nothing written: infl_adaptive; trans_out / transm_out / pa_out / nsweep non-NULL;
 * a stride < 1 or > 8; k > 128; npts != nx*ny*nlev.  var_mask works as in letkf_das_args (one class per call).
 * Results are bitwise equal from call to call and for any slab cut.
 */
#ifndef LETKF_AMD_INTERP_H
#define LETKF_AMD_INTERP_H

#include "letkf_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LETKF_AMD_INTERP_VERSION 1

typedef struct {
  int32_t nx, ny, nlev;      /* the tile: point p = i + nx*j + nx*ny*lev */
  int32_t stride_x, stride_y;/* 1..8 */
  int32_t reserved0;         /* 0 */
  int64_t ws_bytes;          /* library workspace of a slab of levels; 0 = 8 GiB */
  const double *rig;         /* dev [nx*ny] */
  const double *rjg;         /* dev [nx*ny] */
  const double *rlev;        /* dev [nx*ny*nlev] */
  const double *rz;          /* dev [nx*ny*nlev] */
  int32_t *nobs_coarse;      /* dev [ncx*ncy*nlev] or NULL: local observations of coarse point cx + ncx*cy + ncx*ncy*lev */
} letkf_interp_args;

/* Host only.  The coarse indices of an axis of n points at the given stride, ascending: idx[0 .. *count).  idx holds
 * n entries at the most; idx may be NULL to ask for the count alone.  LETKF_E_INVALID for n < 1 or stride < 1. */
int letkf_interp_coarse_axis(int32_t n, int32_t stride, int32_t *idx, int32_t *count);

/* The analysis of the tile by weight interpolation.  letkf_ctx_last_path names the route ("interp: ... +
 * letkf_interp_apply_kernel<..>"); stride (1, 1) runs the same kernels, every point being a coarse point. */
int letkf_das_interp_dev(letkf_ctx *ctx, const letkf_das_args *args, const letkf_search_tables *tables,
                         const letkf_interp_args *interp);

#ifdef __cplusplus
}
#endif
#endif
