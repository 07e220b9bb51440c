// letkf_interp_dev.h -- argument blocks and launchers of the weight-interpolation route (letkf_interp.hip), shared with the
// host entry letkf_das_interp_dev (letkf_api.hip).  Internal: the public interface is include/letkf_amd_interp.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "letkf_device.h"

namespace letkf {

// The tile and its coarse set: point p = i + nx * j + nx * ny * lev; coarse column cc = cx + ncx * cy is fine column
// ix[cx] + nx * iy[cy]; coarse point cc + ncx * ncy * lev.
struct InterpGrid {
  int nx, ny, nlev, ncx, ncy;
  const int* ix;   // dev [ncx]
  const int* iy;   // dev [ncy]
};

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
