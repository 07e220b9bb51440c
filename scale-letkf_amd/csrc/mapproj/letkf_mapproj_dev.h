// letkf_mapproj_dev.h -- the map projection's unit (letkf_mapproj.hip) as the host entries (letkf_mapproj_entry.hip) call it.
// Internal: the public interface is include/letkf_amd_mapproj.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../../include/letkf_amd_mapproj.h"

namespace letkf {

// The launches on st, asynchronous.  Every argument was checked by the entry; n > 0; rotc may be nullptr.
hipError_t phys2ij_run(hipStream_t st, const letkf_mapproj& p, int64_t n, const double* lon, const double* lat, double* ri, double* rj,
                       double* rotc);
hipError_t ij2phys_run(hipStream_t st, const letkf_mapproj& p, int64_t n, const double* ri, const double* rj, double* lon, double* lat,
                       double* rotc);
// A subdomain's points, row j of nlon points after row j - 1; each output may be nullptr.
hipError_t mapproj_grid_run(hipStream_t st, const letkf_mapproj& p, int32_t nlon, int32_t nlat, int32_t ihalo, int32_t jhalo, double cx1,
                            double cy1, double* lon2d, double* lat2d, double* rotc2d);

}  // namespace letkf
