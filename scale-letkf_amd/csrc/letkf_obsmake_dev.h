// letkf_obsmake_dev.h -- the kernels of obsmake_cal (letkf_obsmake.hip) as the host entries of letkf_obsmake_entry.hip call them.
// Internal: the public interface is include/letkf_amd_obsmake.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/letkf_amd_obsmake.h"

namespace letkf {

// Box-Muller over npairs pairs of uniforms u (dev, [2 npairs]): out[2 i], out[2 i + 1] for the pairs i of this chunk, whose
// first element is out's; the element beyond nout (the cosine of an odd count's last pair) is not written.
hipError_t randn_pairs(hipStream_t st, int64_t npairs, const double* u, double* out, int64_t nout);

// The tail of the slot entry's scan workspace over n file rows, every part 256-byte aligned: the compacted rows the operator
// reads (set, idx, rotc), its one-column value buffer and qc, its read-back flag and the slot's two counters.
struct ObsmakeWs {
  int32_t *flag, *set, *idx, *qc;
  double *val, *rotc;
  unsigned long long* nslot;
};
size_t obsmake_ws_bytes(int64_t n);
void obsmake_ws_layout(char* tail, int64_t n, ObsmakeWs* w);

struct ObsmakeRows {      // the file rows of one slot call
  int nfile;
  long off[LETKF_OBSOPE_MAX_FILES + 1];
  long n;
  const double* dif;
  const int* own;
  double lb, ub;
  int outside_undef;
};
// count pass: sel[row] = 1 where the row is in the slot and this subdomain's, else 0; *w.nslot = rows in the slot (zeroed here)
hipError_t obsmake_count(hipStream_t st, const ObsmakeRows& R, int32_t* sel, const ObsmakeWs& w);
// fill pass: the selected rows at their offsets: set / idx (1-based), rotc gathered per file row (rotc may be NULL), qc zeroed
hipError_t obsmake_fill(hipStream_t st, const ObsmakeRows& R, const int32_t* sel, const int64_t* off, const double* rotc,
                        const ObsmakeWs& w);
// scatter: dat of the processed rows from the operator's value and qc, undef for the rows outside the domain, counts (may be NULL)
hipError_t obsmake_scatter(hipStream_t st, const ObsmakeRows& R, const int32_t* sel, const int64_t* off, const ObsmakeWs& w,
                           double* dat, int64_t* counts);

// err by element and dat += err * error (obsope_tools.f90:1013-1042) over n rows
hipError_t obsmake_noise(hipStream_t st, const letkf_obsmake_err* e, int64_t n, const int32_t* elm, const double* error, double* dat,
                         double* err);

}  // namespace letkf
