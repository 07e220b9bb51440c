// letkf_monit_dev.h -- the departure monitor's unit (letkf_monit.hip) as the host entries of letkf_monit_entry.hip call it.
// Internal: the public interface is include/letkf_amd_monit.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "../../include/letkf_amd_monit.h"

namespace letkf {

// Argument checks that need no device; LETKF_OK or LETKF_E_INVALID with *msg.
int hist_check(const letkf_hist_state* s, const letkf_obsope_fields* layout, const double* v3d, const double* v2d, std::string* msg);
// Bytes of device workspace state_to_history needs (the levels' cz).
size_t hist_ws_bytes(const letkf_obsope_fields* layout);
// The kernels of state_to_history on st: cz to the workspace, the transposing copy, height / RH, the 2-D slots, the lateral halo.
hipError_t hist_run(hipStream_t st, const letkf_hist_state* s, const letkf_obsope_fields* layout, double* v3d, double* v2d, void* ws);

// The workspace of one letkf_monit_obs_dev call over nn rows, every part 256-byte aligned: the gathered rows the operator
// reads (set, idx, rotc), its one-column value buffer and qc, this step's element / qc / departure for the statistics.
struct MonitWs {
  int32_t *flag, *set, *idx, *oqc, *elm, *qc;
  double *val, *dep, *rotc;
  void* stat;             // launch_monit_dep's partial sums
};
size_t monit_ws_bytes(int64_t nn, size_t stat_bytes);
void monit_ws_layout(void* base, int64_t nn, size_t stat_bytes, MonitWs* w);
// set / idx / rotc (may be NULL) gathered by key (a negative key entry gives set 0, which the operator's row check refuses); qc
// zeroed.
hipError_t monit_gather(hipStream_t st, int64_t nn, const int32_t* key, const int32_t* set, const int32_t* idx, const double* rotc,
                        const MonitWs& w);
// The rules of monit_obs around the operator's value and qc (w.val, w.oqc), the records of this step, and w.elm / w.qc / w.dep.
hipError_t monit_finish(hipStream_t st, const letkf_monit_params* mp, const letkf_obsope_params* op, const letkf_obs_file_rows* files,
                        int64_t nn, const letkf_obsdep* rec, const MonitWs& w);

}  // namespace letkf
