// letkf_nobsout_dev.h -- the kernels of NOBS_OUT (letkf_nobsout.hip) as the host entries (letkf_nobsout_entry.hip) call them.
// Internal: the public interface is include/letkf_amd_nobsout.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../../include/letkf_amd_nobsout.h"

namespace letkf {

// letkf_nobs_fields_dev as its kernel takes it (by value): the host tables are in here, resolved to 0-based indices.
struct NobsFieldsArgs {
  int64_t npts;
  int32_t nctype, nobtype;
  const int32_t* nobs_ctype;   // [npts][nctype]
  const double* cutd_ctype;    // [npts][nctype] or null
  double* work3dn;             // [npts][nobtype + 6] or null
  double* fields;              // (p, f) at p * sp + f * sv, or null
  int64_t sp, sv;
  int32_t ic_radar[3];         // the combined type of (uid_ref | uid_re0 | uid_vr, typ_radar), -1: none
  int32_t row_field[LETKF_NOBSOUT_NFIELDS];   // the row of work3dn (0-based) that is field f
  // the combined types of every report type: typ_member[typ_start[r] .. typ_start[r + 1])
  uint8_t typ_start[LETKF_NOBSOUT_MAX_OBTYPE + 1];
  uint8_t typ_member[LETKF_NOBSOUT_MAX_CTYPE];
};

// Every argument was checked by the entry; all three are asynchronous on st.
hipError_t launch_nobs_fields(const NobsFieldsArgs& a, int num_cu, hipStream_t st);
// cutd [npts][nctype] of tables without a limit: criterion 1 hori_loc * dist_zero_fac on every group's master, 0 elsewhere
// (letkf_tools.f90:1384-1389); criterion 2 / 3: 0
hipError_t launch_nobs_cutd_default(const letkf_search_tables& t, int64_t npts, double* cutd_ctype, int num_cu, hipStream_t st);
// rows of the points with beta = 0 to zero (either array may be null)
hipError_t launch_nobs_zero_unanalysed(int64_t npts, int32_t nctype, const double* beta, int32_t* nobs_ctype, double* cutd_ctype,
                                       int num_cu, hipStream_t st);

}  // namespace letkf
