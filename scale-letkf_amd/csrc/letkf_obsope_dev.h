// letkf_obsope_dev.h -- the observation operator's unit (letkf_obsope.hip) as the host entry letkf_obsope_dev (letkf_api_obs.hip)
// calls it.  Internal: the public interface is include/letkf_amd_obsope.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "../../include/letkf_amd_obsope.h"

namespace letkf {

// Argument checks that need no device; LETKF_OK or LETKF_E_INVALID with *msg.
int obsope_check(const letkf_obsope_params* p, const letkf_obs_file_rows* files, const letkf_obsope_fields* f, int64_t row0,
                 int64_t nrows, const int32_t* set, const int32_t* idx, const int32_t* qc, const double* ensval, int64_t kld,
                 std::string* msg);
// The row check (one read-back of flag, a device int32 of the caller's) and the operator kernel on st.
// keep_ref_low: the mode of obsmake_cal (obsope_tools.f90:864-884) -- qc 11 is not turned into 0 (:488 has no counterpart
// there), use_obs counts as all ones and the lev > radar_zmax test is skipped.  nrows_dev (dev, or NULL): rows the caller
// compacted on the device -- min(nrows, *nrows_dev) of them are taken, nrows bounds the launch.
int obsope_run(hipStream_t st, const letkf_obsope_params* p, const letkf_obs_file_rows* files, const letkf_obsope_fields* f,
               int64_t row0, int64_t nrows, const int32_t* set, const int32_t* idx, int32_t* qc, double* ensval, int64_t kld,
               int32_t* flag, std::string* msg, bool keep_ref_low = false, const int64_t* nrows_dev = nullptr);

}  // namespace letkf
