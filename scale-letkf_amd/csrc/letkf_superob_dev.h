// letkf_superob_dev.h -- superob's unit (letkf_superob.hip) as the host entry letkf_superob_dev (letkf_superob_entry.hip) calls
// it.  Internal: the public interface is include/letkf_amd_superob.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/letkf_amd_superob.h"

namespace letkf {

// the eight doubles of a row that superob_select reads and writes
struct SuperobRows {
  double *lon, *lat, *lev, *dat, *err, *ri, *rj, *rk;
};

// A call as the kernels take it (by value, 2 KB of kernel arguments): the host tables are in here.
struct SuperobArgs {
  int64_t n;
  const int32_t *elm, *typ;
  SuperobRows in;              // the caller's rows (read only)
  int32_t nlon, nlat, nlevx, nslots, nobtype, nid;
  uint32_t surf_mask;
  int32_t any_v, any_t;        // some method_v / method_t is > 0: stage 2 / stage 3 has work
  int64_t slot_off[LETKF_SUPEROB_MAX_SLOTS + 1];
  int32_t elem_uid[LETKF_SUPEROB_MAX_TYPES];
  uint8_t meth[LETKF_SUPEROB_MAX_TYPES * LETKF_SUPEROB_MAX_TYPES];   // g | v << 1 | t << 3 | h << 5 at (uid-1) * nobtype + typ-1
  uint8_t prio[LETKF_SUPEROB_MAX_SLOTS];                             // rank of slot s (0-based) in slot_priority
  letkf_superob_out out;
};

// Bytes of workspace a call of n rows needs (0: a rocprim size query failed).
size_t superob_ws_bytes(const SuperobArgs& a, hipStream_t st);
// The kernels on st; every argument was checked by the entry.  ws: superob_ws_bytes() bytes, 256-byte aligned.
hipError_t superob_run(hipStream_t st, const SuperobArgs& a, void* ws);

}  // namespace letkf
