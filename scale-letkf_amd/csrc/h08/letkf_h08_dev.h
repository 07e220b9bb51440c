// letkf_h08_dev.h -- the kernels of the Himawari-8 radiances (letkf_h08.hip) as the host entries (letkf_h08_entry.hip) call them.
// Internal: the public interface is include/letkf_amd_h08.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../../include/letkf_amd_h08.h"

namespace letkf {
namespace h08 {

constexpr int kNch = LETKF_H08_NCH;
constexpr int kRecWords = 4 + kNch + 2;      // marker, wk(1 : 4 + nch), marker
constexpr int kBlock = 256;                  // threads of every block; profiles of a block of the record kernels
constexpr int kWaves = kBlock / 64;          // (profile, member) or (row, member) pairs a block has in flight

inline int64_t blocks_of(int64_t n) { return (n + kBlock - 1) / kBlock; }

// letkf_h08_profiles_dev as its kernel takes it (by value)
struct ProfileArgs {
  const double *v3d, *v2d;
  int64_t s3k, s3i, s3j, s3v, s3m, s2i, s2j, s2v, s2m;
  int32_t nlev, nlonh, nlath, khalo, nmem, nsel;
  int64_t nprof_file;          // entries of ri, rj, lon, lat, rotc
  int32_t top_down, stggrd, rttov_units;
  double ri_off, rj_off, rd, repsb, q_ppmv, qmin, minq, cfrac_cnst, sub_lon, r_pol, r_sat, ell_tan, ell_ecc;
  const int32_t* prof_list;
  const double *ri, *rj, *lon, *lat, *rotc;
  double *lev3, *sfc, *cloud;
  int32_t* pflag;
};

// letkf_h08_rows_dev as its kernel takes it
struct RowArgs {
  int64_t row0, nrows, nsel, kld, nprof_file;
  const int32_t *set, *idx, *slot_of_prof, *pflag;
  int32_t h08_set, nmem, m0, nlev, top_down, rttov_units, reject_land, use_obs23, finish, member, qc_replace;
  uint32_t ch_mask;            // bit c: ch_use[c] == 1
  double cldsky_thrs, bris, brie, brjs, brje;
  const double *lev3, *sfc, *btall, *btclr, *trans, *rig, *rjg;
  int32_t* qc;
  double *ensval, *lev, *val2;
};

// Every argument was checked by the entry; all are asynchronous on st.
// cnt: per-block counts of records with a wrong marker [blocks_of(nprof)], or NULL; total: their sum (count_total)
hipError_t launch_decode(int be, const uint32_t* image, int64_t nprof, const double (&obserr)[kNch], const letkf_obsfile_cols& o,
                         int32_t* cnt, hipStream_t st);
hipError_t launch_count_total(const int32_t* cnt, int64_t nblock, int64_t* total, hipStream_t st);
hipError_t launch_encode(int be, int64_t nprof, const letkf_obsfile_cols& in, uint32_t* image, hipStream_t st);
// flag [nprof_file] int32, zeroed by the caller; then off = its exclusive scan
hipError_t launch_select_mark(const int32_t* set, const int32_t* idx, int64_t row0, int64_t nrows, int h08_set, int64_t nprof_file,
                              int32_t* flag, hipStream_t st);
hipError_t launch_select_fill(int64_t nprof_file, const int32_t* flag, const int64_t* off, int32_t* prof_list, int32_t* slot_of_prof,
                              hipStream_t st);
hipError_t launch_profiles(const ProfileArgs& a, hipStream_t st);
hipError_t launch_rows(const RowArgs& a, hipStream_t st);

}  // namespace h08
}  // namespace letkf
