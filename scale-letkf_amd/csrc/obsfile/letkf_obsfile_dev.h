// letkf_obsfile_dev.h -- the record codec's unit (letkf_obsfile.hip) as the host entries (letkf_obsfile_entry.hip) call it.
// Internal: the public interface is include/letkf_amd_obsfile.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../../include/letkf_amd_obsfile.h"

namespace letkf {
namespace obsfile {

constexpr int kBlockRows = 256;                              // rows of a block of the row-wise kernels
constexpr int kTileRows = LETKF_OBSFILE_TILE_ROWS;           // the assemble kernel's tile
constexpr int kTileMembers = LETKF_OBSFILE_TILE_MEMBERS;
constexpr int kRadarHeadWords = 9;                           // three records of one float

// one image of an assemble call, as the kernel reads it from the table the entry uploads
struct ImageRef {
  const uint32_t* words;
  int32_t col, is_member;
};

inline int64_t row_blocks(int64_t n) { return (n + kBlockRows - 1) / kBlockRows; }
inline int64_t row_tiles(int64_t n) { return (n + kTileRows - 1) / kTileRows; }

// The launches on st, asynchronous.  Every argument was checked by the entry; n > 0.  A `cnt` is an int32 count per block (or
// tile, `ncnt` of them per block) that count_total_run sums into total[ncnt] (int64) with one block: integers, so any order.
hipError_t count_total_run(hipStream_t st, const int32_t* cnt, int64_t nblock, int ncnt, int64_t* total);

// rows of a conventional or radar image (behind its head) to the columns; cnt (bad markers per block) may be nullptr
hipError_t decode_run(hipStream_t st, const letkf_obsfile_params& p, const letkf_mapproj* proj, const uint32_t* rows, int64_t n,
                      const letkf_obsfile_cols& o, int32_t* cnt);
// the radar head: three records from three float32 values already narrowed by the entry (bits), written by one lane each
hipError_t radar_head_run(hipStream_t st, uint32_t* image, uint32_t b0, uint32_t b1, uint32_t b2, int big_endian);
// survivors per block of kBlockRows rows into counts [row_blocks(n)]
hipError_t encode_count_run(hipStream_t st, int64_t n, const double* dat, int32_t* counts);
// the records; off (block offsets from the scan) nullptr = every row, at its own place
hipError_t encode_run(hipStream_t st, const letkf_obsfile_params& p, int64_t n, const letkf_obsfile_cols& in, const int64_t* off,
                      uint32_t* rows);

// the assemble kernel; tab: dev [p.nmem]; cnt: dev [row_tiles(nobs)][2] (bad records, inconsistent rows) or nullptr
hipError_t assemble_run(hipStream_t st, const letkf_obsda_params& p, const ImageRef* tab, const letkf_obsda_cols& o, int32_t* cnt);
hipError_t obsda_encode_run(hipStream_t st, int nrec, int big_endian, int64_t n, const int32_t* set, const int32_t* idx, const int32_t* qc,
                            const double* value, int64_t stride, const double* lev, const double* val2, uint32_t* image);

// departures: rows outside the files per block into cnt [row_blocks(n)]; then the records.  off: dev [nfile + 1]
hipError_t obsdep_check_run(hipStream_t st, int64_t n, const int32_t* set, const int32_t* idx, int nfile, const int64_t* off, int32_t* cnt);
hipError_t obsdep_encode_run(hipStream_t st, int big_endian, int64_t n, const int32_t* set, const int32_t* idx, const int32_t* qc,
                             const double* omb, const double* oma, const letkf_obsfile_rows& f, const int64_t* off, uint32_t* image);

}  // namespace obsfile
}  // namespace letkf
