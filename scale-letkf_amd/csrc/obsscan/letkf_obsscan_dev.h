// letkf_obsscan_dev.h -- the first scan's unit (letkf_obsscan.hip) as the host entry letkf_obsscan_dev (letkf_obsscan_entry.hip)
// calls it.  Internal: the public interface is include/letkf_amd_obsscan.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../../include/letkf_amd_obsscan.h"

namespace letkf {

// A call as the kernels take it (by value): the host tables are in here.
struct ObsscanArgs {
  int64_t n;                   // file rows of all files
  int64_t nlist;               // ... of the files that run: the length of the lists
  const double *ri, *rj, *dif;
  int64_t off[LETKF_OBSOPE_MAX_FILES + 1];   // off[q] for q > nfile: INT64_MAX (no row reaches it)
  uint32_t run_mask;           // bit f: file f runs
  int32_t nlon, nlat, ihalo, jhalo, px, py;
  int32_t slot_start, slot_end, slot_base, myrank_d;
  int32_t nb;                  // buckets of a subdomain, nslots + 2
  int32_t nbucket;             // px * py * nb, also the key of the rows that do not run
  double tint;
  int32_t *set, *idx, *qc, *rank, *slot, *own;
};

// Bytes of workspace a call needs (0: a rocprim size query failed).
size_t obsscan_ws_bytes(const ObsscanArgs& a, hipStream_t st);
// The kernels on st and the copy of the buckets' upper bounds into ub_host [nbucket], asynchronous: the caller synchronises.
// Every argument was checked by the entry.  ws: obsscan_ws_bytes() bytes, 256-byte aligned.
hipError_t obsscan_run(hipStream_t st, const ObsscanArgs& a, void* ws, int32_t* ub_host);

}  // namespace letkf
