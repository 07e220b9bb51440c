// letkf_interp_dev.h -- argument blocks and launchers of the weight-interpolation route (letkf_interp.hip), shared with the
// host entry letkf_das_interp_dev (letkf_api_das.hip).  Internal: the public interface is include/letkf_amd_interp.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "letkf_device.h"

namespace letkf {

// The arrays of the call and its coarse set: point p = i + nx * j + nx * ny * lev; coarse column cc = cx + ncx * cy is fine
// column ix[cx] + nx * iy[cy]; coarse point cc + ncx * ncy * lev.  ix / iy are the call's run of the domain's coarse lines
// (include/letkf_amd_interp_window.h) in array indices; the owned points are [ox0, ox1) x [oy0, oy1), the whole arrays where
// the call has no window.
struct InterpGrid {
  int nx, ny, nlev, ncx, ncy;
  int ox0, ox1, oy0, oy1;
  const int* ix;   // dev [ncx]
  const int* iy;   // dev [ncy]
};

// The fine lines of one direction that cell c of a run of nc coarse lines owns, clipped to the owned range [o0, o1): the
// cell [a, b] owns [a, b), its far line too where it is the last of the run.  Host and device share this one statement.
__host__ __device__ inline void interp_cell_lines(int c, int nc, int a, int b, int o0, int o1, int* lo, int* hi) {
  const int ncel = nc > 1 ? nc - 1 : 1;
  const int end = (c == ncel - 1) ? b : b - 1;
  *lo = a > o0 ? a : o0;
  *hi = end < o1 - 1 ? end : o1 - 1;
}

// letkf_interp_window_axis with the global line that fell outside the arrays handed back (*bad; untouched otherwise)
int interp_window_axis(int32_t gn, int32_t stride, int32_t g0, int32_t n, int32_t o0, int32_t on, int32_t* idx, int32_t* count,
                       int32_t* bad);

// the coordinates of the coarse columns and points, gathered for the column search
struct InterpCoordArgs {
  InterpGrid G;
  const double *rig, *rjg, *rlev, *rz;   // the tile's
  double *crig, *crjg, *crlev, *crz;     // [ncx * ncy] / [ncx * ncy * nlev]
};
hipError_t launch_interp_coords(const InterpCoordArgs& a, int num_cu, hipStream_t st);

// One slab of levels [l0, l0 + nl): the local lists of its coarse points (global offsets, shifted bases) to the dense
// problems letkf_core's batch form takes -- problem b = cc + ncx * ncy * (lev - l0), nobs rows each -- and the rho of each.
struct InterpGatherArgs {
  InterpGrid G;
  PointArgs A;            // the rules' switches, infl, gues and strides of the call (solve_inflation, q_update_skipped)
  int l0, nl, nobs;
  const long* obs_off;    // [ncx * ncy * nlev + 1], all levels
  const int* obs_idx;
  const double *rdiag_l, *rloc_l;
  int* nobsl;             // [nb]
  double *hdxb, *rdiag, *rloc, *dep, *depd;   // [nb][k][nobs], [nb][nobs] ... (depd null without det_run)
  double* rho;            // [nb]
};
hipError_t launch_interp_gather(const InterpGatherArgs& a, int num_cu, hipStream_t st);

// The blend and the apply for the fine points of the slab's cells.
struct InterpApplyArgs {
  InterpGrid G;
  PointArgs A;            // k, nv, the rules' switches, beta, infl, gues, anal, strides, status, rtps_out of the call
  int l0, nl;
  const double* T;        // [nb][k * k]
  const double* wbar;     // [nb][k]
  const double* wbard;    // [nb][k] or null
  const int* cstatus;     // [nb]
};
int interp_apply_nct(int k);                 // column tiles of 16 of the instantiation that serves k (1, 2, 4, 8)
size_t interp_apply_lds_bytes(int k);
std::string interp_apply_kernel_name(int k);
hipError_t launch_interp_apply(const InterpApplyArgs& a, hipStream_t st);

}  // namespace letkf
