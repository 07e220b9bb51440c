// letkf_obssim_dev.h -- the model-to-observation simulator's unit (letkf_obssim.hip) as the host entry letkf_obssim_dev
// (letkf_obssim_entry.hip) calls it.  Internal: the public interface is include/letkf_amd_obssim.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

#include "../../include/letkf_amd_obssim.h"

namespace letkf {

// Bytes of workspace a call needs (the per-column azimuth and distance of a radar element; 0 where no list names one).
size_t obssim_ws_bytes(const letkf_obssim_params* p, const letkf_obsope_fields* f);
// The kernels on st; every argument was checked by the entry.  ws: obssim_ws_bytes() bytes, 16-byte aligned (not read where that is 0).
hipError_t obssim_run(hipStream_t st, const letkf_obssim_params* p, const letkf_obsope_fields* f, const letkf_obssim_out* o,
                      void* ws);

}  // namespace letkf
