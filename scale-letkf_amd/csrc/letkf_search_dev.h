// letkf_search_dev.h -- obs_local's device functions, written once for every kernel that searches: the per-point and column
// kernels, the ring and survivor kernels (letkf_search.hip) and the fused search and column-survivor mode of the wave kernel
// (letkf_wave_dev.h).  The lists are bit-equal whichever route builds them, the list-free route is bit-equal to the lists and
// the LDS and ring kernels select the same sets because they evaluate these functions; the few sites that restate one (where
// the call cost registers or time: profiles/r10_README.md) say so in a comment that names it.
//   the walk      cell_rect (obs_local_range, scale/letkf/letkf_tools.f90:1775-1778, with ij_obsgrd_ext,
//                 scale/letkf/letkf_obs.f90:1209-1227) and row_span (obs_choose_ext's prefix sums, :1262);
//   the weights   obs_local_cal (letkf_tools.f90:1793-1906): whole (local_cal_v), its horizontal half (horizontal_nd,
//                 inside_cutoff, vertical_obs_coord) and its vertical half (column_vertical_cal);
//   the hand-over the survivor entry that carries a row from the horizontal half to the vertical half in another kernel;
//   the single-precision cut-off literals of letkf_obs.f90:27-28.
// The loops stay in the kernels (a flush round, an overflow exit, a prefetch, three passes wrap them differently).
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/letkf_amd.h"

namespace letkf {
namespace search_dev {

constexpr double kDistZeroFac = (double)3.651483717f;          // letkf_obs.f90:27 (single-precision literal)
constexpr double kDistZeroFacSq = (double)13.33333333f;        // :28
constexpr double kTiny = 2.2250738585072014e-308;              // tiny(var_local)

// The horizontal distance of a point from table row `row`, in units of the type's scale hloc (:1876-1878).  No multiply-add
// fusion: every route evaluates exactly these roundings.  (local_cal_v below has the observation's coordinates in registers
// and keeps its own copy of the three lines: through this function the per-point kernel's search was 3 % slower.)
__device__ __forceinline__ double horizontal_nd(const letkf_search_tables& t, const double hloc, const double ri,
                                                const double rj, const int row) {
#pragma clang fp contract(off)
  const double rdx = (ri - t.ob_ri[row]) * t.dx;
  const double rdy = (rj - t.ob_rj[row]) * t.dy;
  return sqrt(rdx * rdx + rdy * rdy) / hloc;
}
// the cut-off of a normalised distance, horizontal (:1881) or vertical (:1869); a NaN stays inside, as in the reference
__device__ __forceinline__ bool inside_cutoff(const double nd) { return !(nd > kDistZeroFac); }

// An observation's vertical coordinate as its type's mode compares it (:1851-1865): lev (vm 1), ln dat (2), ln lev (0);
// nothing where the type has no vertical localisation or compares the rain base (3).
__device__ __forceinline__ double vertical_obs_coord(const letkf_search_tables& t, const int vm, const double vloc,
                                                     const int row) {
#pragma clang fp contract(off)
  double v_obs = 0.0;
  if (vloc != 0.0) {
    if (vm == 1) v_obs = t.ob_lev[row];
    else if (vm == 2) v_obs = log(t.ob_dat[row]);
    else if (vm != 3) v_obs = log(t.ob_lev[row]);
  }
  return v_obs;
}

struct CalOut {
  double rloc, rdiag, ndist;
};

// scale/letkf/letkf_tools.f90:1793-1906, on the observation's metadata already in registers
__device__ __forceinline__ CalOut local_cal_v(const letkf_search_tables& t, int ic, double ri, double rj, double rlev,
                                              double rz, double ob_lev, double ob_dat, double ob_ri, double ob_rj,
                                              double ob_err) {
  // no multiply-add fusion here: the function is inlined into two different kernels (the stand-alone search and the
  // fused search of the wave kernel), and their weights must agree to the last bit for the two paths to be identical
#pragma clang fp contract(off)
  CalOut o{0.0, -1.0, -1.0};
  double nrloc = t.varloc[ic];                                 // :1840
  if (nrloc < kTiny) return o;                                 // :1843
  const double vloc = t.vert_loc[ic];
  double nd_v;
  const int vm = t.vmode[ic];
  if (vloc == 0.0) nd_v = 0.0;                                 // :1851-1865
  else if (vm == 2) nd_v = fabs(log(ob_dat) - log(rlev)) / vloc;
  else if (vm == 3) nd_v = fabs(log(t.rain_base) - log(rlev)) / vloc;
  else if (vm == 1) nd_v = fabs(ob_lev - rz) / vloc;
  else nd_v = fabs(log(ob_lev) - log(rlev)) / vloc;
  if (nd_v > kDistZeroFac) return o;                           // :1869
  const double rdx = (ri - ob_ri) * t.dx;                      // :1876-1878 (horizontal_nd restated)
  const double rdy = (rj - ob_rj) * t.dy;
  const double nd_h = sqrt(rdx * rdx + rdy * rdy) / t.hori_loc[ic];
  if (nd_h > kDistZeroFac) return o;                           // :1881
  const double nd = nd_h * nd_h + nd_v * nd_v;                 // :1888
  if (nd > kDistZeroFacSq) return o;                           // :1891
  nrloc = nrloc * exp(-0.5 * nd);                              // :1899
  o.rloc = nrloc;
  o.rdiag = ob_err * ob_err / nrloc;                           // :1903
  o.ndist = nd;
  return o;
}

// The vertical half of obs_local_cal for an observation whose horizontal half is done (the column search: nd_h and the
// observation's vertical coordinate v_obs -- lev, ln lev or ln dat by the ctype's mode -- are the same for every level of a
// column).  v_z = the point's height, v_p = ln of its pressure, l_rain = ln VERT_LOCAL_RAIN_BASE.  rloc = 0: rejected.
// Shared by the column search (lists) and the wave kernel's column-survivor mode (no lists): same weights to the last bit.
struct ColVert {
  double rloc, rdiag;
};
__device__ __forceinline__ ColVert column_vertical_cal(const int vm, const double vloc, const double varloc, const double nd_h,
                                                const double v_obs, const double err, const double v_z, const double v_p,
                                                const double l_rain) {
#pragma clang fp contract(off)
  ColVert o{0.0, 0.0};
  double nd_v;
  if (vloc == 0.0) nd_v = 0.0;                                 // :1851-1865
  else if (vm == 3) nd_v = fabs(l_rain - v_p) / vloc;
  else nd_v = fabs(v_obs - (vm == 1 ? v_z : v_p)) / vloc;
  if (nd_v > kDistZeroFac) return o;                           // :1869
  const double nd = nd_h * nd_h + nd_v * nd_v;                 // :1888
  if (nd > kDistZeroFacSq) return o;                           // :1891
  o.rloc = varloc * exp(-0.5 * nd);                            // :1899
  o.rdiag = err * err / o.rloc;                                // :1903
  return o;
}

__device__ __forceinline__ CalOut local_cal(const letkf_search_tables& t, int ic, double ri, double rj, double rlev,
                                            double rz, int row) {
  const int vm = t.vmode[ic];
  return local_cal_v(t, ic, ri, rj, rlev, rz, (vm == 2 || vm == 3) ? 1.0 : t.ob_lev[row], vm == 2 ? t.ob_dat[row] : 1.0,
                     t.ob_ri[row], t.ob_rj[row], t.ob_err[row]);
}

__device__ __forceinline__ void ij_obsgrd_ext(const letkf_search_tables& t, int ic, double ri, double rj, int& ogi,
                                              int& ogj) {       // letkf_obs.f90:1221-1224
  ogi = (int)ceil((ri - t.i_org) * (double)t.ngrd_i[ic] / (double)t.nlon) + t.ngrdsch_i[ic];
  ogj = (int)ceil((rj - t.j_org) * (double)t.ngrd_j[ic] / (double)t.nlat) + t.ngrdsch_j[ic];
}

// The rectangle of sorting-mesh cells of type ic that covers the horizontal cut-off around (ri, rj): obs_local_range
// (letkf_tools.f90:1775-1778).  The reference requires the extended mesh to cover the rectangle (DEBUG check :1780); clamped
// defensively here.  acb / ld address the type's prefix sums: row_span.
struct CellRect {
  int imin, imax, jmin, jmax;
  long acb;
  int ld;
  __device__ __forceinline__ bool empty() const { return imin > imax || jmin > jmax; }
};
__device__ __forceinline__ CellRect cell_rect(const letkf_search_tables& t, const int ic, const double ri, const double rj) {
  const double dzi = t.hori_loc[ic] * kDistZeroFac / t.dx;
  const double dzj = t.hori_loc[ic] * kDistZeroFac / t.dy;
  CellRect r;
  ij_obsgrd_ext(t, ic, ri - dzi, rj - dzj, r.imin, r.jmin);
  ij_obsgrd_ext(t, ic, ri + dzi, rj + dzj, r.imax, r.jmax);
  r.imin = max(r.imin, 1);
  r.jmin = max(r.jmin, 1);
  r.imax = min(r.imax, t.ngrdext_i[ic]);
  r.jmax = min(r.jmax, t.ngrdext_j[ic]);
  r.acb = t.ac_off[ic];
  r.ld = t.ngrdext_i[ic] + 1;
  return r;
}
// the table rows [lo, hi) of mesh row j inside the rectangle (obs_choose_ext, letkf_obs.f90:1262)
__device__ __forceinline__ int row_lo(const letkf_search_tables& t, const CellRect& r, const int j) {
  return t.ac_ext[r.acb + (r.imin - 1) + (long)r.ld * (j - 1)];
}
__device__ __forceinline__ int row_hi(const letkf_search_tables& t, const CellRect& r, const int j) {
  return t.ac_ext[r.acb + r.imax + (long)r.ld * (j - 1)];
}
__device__ __forceinline__ void row_span(const letkf_search_tables& t, const CellRect& r, const int j, int& lo, int& hi) {
  lo = row_lo(t, r, j);
  hi = row_hi(t, r, j);
}

// The survivor entry: a row inside the horizontal cut-off of a column, handed from the kernel that did the horizontal half
// (letkf_survivors_kernel, letkf_ring_survivors_kernel) to the one that does the vertical half per level
// (letkf_search_rings_kernel, the wave kernel's mode 3).  Four doubles, read as two double2:
//   (row | ctype << 32 as bits, nd_h) (v_obs, err)     v_obs = vertical_obs_coord of the row
// The pad entry (ctype << 32, 1e30) (0, 1) lies outside every cut-off; it fills a type's segment to whole chunks of 64.
__device__ __forceinline__ void survivor_store(double* sv, const long e, const int row, const int ic, const double nd_h,
                                               const double v_obs, const double err) {
  *reinterpret_cast<double2*>(&sv[4 * e]) = double2{__longlong_as_double((long)row | ((long)ic << 32)), nd_h};
  *reinterpret_cast<double2*>(&sv[4 * e + 2]) = double2{v_obs, err};
}
__device__ __forceinline__ void survivor_store_pad(double* sv, const long e, const int ic) {
  *reinterpret_cast<double2*>(&sv[4 * e]) = double2{__longlong_as_double((long)ic << 32), 1e30};
  *reinterpret_cast<double2*>(&sv[4 * e + 2]) = double2{0.0, 1.0};
}
__device__ __forceinline__ long survivor_bits(const double first) { return __double_as_longlong(first); }
__device__ __forceinline__ int survivor_row(const long bits) { return (int)(bits & 0xffffffffL); }
__device__ __forceinline__ int survivor_ctype(const long bits) { return (int)(bits >> 32); }

}  // namespace search_dev
}  // namespace letkf
