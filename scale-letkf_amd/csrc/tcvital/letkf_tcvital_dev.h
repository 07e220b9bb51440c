// letkf_tcvital_dev.h -- the kernels of the TC vitals (letkf_tcvital.hip) as the host entries (letkf_tcvital_entry.hip) call them.
// Internal: the public interface is include/letkf_amd_tcvital.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../../include/letkf_amd_tcvital.h"

namespace letkf {

constexpr int kTcTileI = 32, kTcTileJ = 8;   // interior cells of a workgroup's tile: one per thread, a wave is two rows
constexpr int kTcRowsBlock = 256;            // threads of a block of the row scan
constexpr int kTcRowsMaxBlocks = 1024;       // ... and the most blocks it is launched with

// letkf_tcvital_search_dev as its kernels take it (by value)
struct TcSearchArgs {
  const double* v2d;
  int64_t s2i, s2j, s2v, s2m;
  int32_t nlon, nlat, ihalo, jhalo, nmem;
  int32_t i_off, j_off;
  int32_t tiles_i, tiles_j;    // ceil(nlon / kTcTileI), ceil(nlat / kTcTileJ)
  double dx, dy, cxg1, cyg1, dis;
  const double *ritc, *rjtc;   // dev, one double each
  double* part_s;              // [nmem][tiles_i * tiles_j]: the tile's lowest s, 9.99e33 where it has none
  int32_t* part_ij;            // [nmem][tiles_i * tiles_j][2]: its global (ig, jg)
  double* cand;                // [nmem][3]
};

// bytes of part_s (256-byte aligned, part_ij follows) and of both
size_t tc_search_part_s_bytes(const TcSearchArgs& a);
size_t tc_search_ws_bytes(const TcSearchArgs& a);

// Every argument was checked by the entry; all are asynchronous on st.
hipError_t launch_tc_search(const TcSearchArgs& a, hipStream_t st);
// part [nblock][3] int64 (nblock = tc_rows_blocks(n)); out6: rows[3] as int64 (1-based, 0: none), then their dif as 3 doubles
int tc_rows_blocks(int64_t n);
hipError_t launch_tc_rows(int64_t n, const int32_t* elm, const double* dif, int64_t* part, int64_t* out6, hipStream_t st);
hipError_t launch_tc_fill(int nproc, int nmem, int m0, const double* cand_all, int64_t r0, int64_t r1, int64_t r2, int qc_replace,
                          int32_t* qc, double* ensval, int64_t kld, hipStream_t st);

}  // namespace letkf
