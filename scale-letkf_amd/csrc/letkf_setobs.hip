// letkf_setobs.hip -- set_letkf_obs behind one call (include/letkf_amd.h section 9; scale/letkf/letkf_obs.f90):
//   pre-processing of the obs files  :268-305   one thread per file row, in place; ctype_use as an LDS bitmap per block
//   combined-type tables             :307-342   host (16 x nobtype bits in, a few hundred integers out)
//   sorting-mesh sizes               :657-677   host (letkf_obs_mesh_dims)
//   row gather + ctype               obs(obsda%set(n))%...(obsda%idx(n)), ctype_elmtyp(uid_obs(elm), typ) (:744-748)
//   departure + QC, bucket sort      letkf_obsprep.hip (unchanged)
//   count tables                     :744-760   LDS histogram per block, integer atomics: exact
//   send buffer                      :993-1010  the sorted rows, packed ensval | val | lev | set | idx
//   obsda_sort assembly              :1036-1100 one launch for every column through the plan's row map
// Every result but the converted reflectivities is bit-identical to the reference's loops; 10 log10 is the device's log10.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../include/letkf_amd.h"
#include "letkf_device.h"

namespace {

// common_obs_scale.f90:48-77 (elem_uid order = uid_obs 1..16, :171-211)
constexpr int kIdU = 2819, kIdV = 2820, kIdT = 3073, kIdTv = 3074, kIdQ = 3330, kIdRh = 3331, kIdPs = 14593,
              kIdRain = 19999, kIdRadarRef = 4001, kIdRadarRefZero = 4004, kIdRadarVr = 4002, kIdRadarPrh = 4003,
              kIdH08IR = 8800, kIdTclon = 99991, kIdTclat = 99992, kIdTcmip = 99993;
constexpr int kElemUid[LETKF_NID_OBS] = {kIdU,        kIdV,           kIdT,       kIdTv,       kIdQ,     kIdRh,
                                         kIdPs,       kIdRain,        kIdRadarRef, kIdRadarRefZero, kIdRadarVr,
                                         kIdRadarPrh, kIdH08IR,       kIdTclon,   kIdTclat,    kIdTcmip};
constexpr int kTypPharad = 22, kTypH08 = 23;
constexpr double kUndef = -9.99e33;                       // common/common.f90:38
constexpr double kDistZeroFac = (double)3.651483717f;     // letkf_obs.f90:27, a single-precision literal

__host__ __device__ inline int uid_obs(int id) {
  switch (id) {
    case kIdU: return 1;
    case kIdV: return 2;
    case kIdT: return 3;
    case kIdTv: return 4;
    case kIdQ: return 5;
    case kIdRh: return 6;
    case kIdPs: return 7;
    case kIdRain: return 8;
    case kIdRadarRef: return 9;
    case kIdRadarRefZero: return 10;
    case kIdRadarVr: return 11;
    case kIdRadarPrh: return 12;
    case kIdH08IR: return 13;
    case kIdTclon: return 14;
    case kIdTclat: return 15;
    case kIdTcmip: return 16;
    default: return -1;
  }
}

struct PrepParams {
  double min_radar_ref;      // 10**(MIN_RADAR_REF_DBZ/10), computed on the host as common_obs_scale.f90:251 does
  double low_dbz;            // MIN_RADAR_REF_DBZ + LOW_REF_SHIFT
  double obserr_ref, obserr_vr;
  int use_err_ref, use_err_vr, nobtype;
};

// letkf_obs.f90:268-305.  use[uid-1] bit typ-1 = ctype_use(uid, typ); bad: a row outside uid_obs / 1..nobtype.
__global__ void __launch_bounds__(256) preprocess_kernel(const PrepParams P, const long nrows, int* __restrict__ elm,
                                                         const int* __restrict__ typ, double* __restrict__ dat,
                                                         double* __restrict__ err, unsigned* __restrict__ use,
                                                         int* __restrict__ bad) {
  __shared__ unsigned s_use[LETKF_NID_OBS];
  if (threadIdx.x < LETKF_NID_OBS) s_use[threadIdx.x] = 0u;
  __syncthreads();
  for (long n = (long)blockIdx.x * blockDim.x + threadIdx.x; n < nrows; n += (long)gridDim.x * blockDim.x) {
    int el = elm[n];
    if (el == kIdRadarRef) {
      const double d = dat[n];
      if (d >= 0.0 && d < 1.0e10) {
        if (d < P.min_radar_ref) {
          el = kIdRadarRefZero;
          elm[n] = el;
          dat[n] = P.low_dbz;
        } else {
          dat[n] = 10.0 * log10(d);
        }
      } else {
        dat[n] = kUndef;
      }
      if (P.use_err_ref) err[n] = P.obserr_ref;
    } else if (el == kIdRadarRefZero) {
      dat[n] = P.low_dbz;
      if (P.use_err_ref) err[n] = P.obserr_ref;
    } else if (el == kIdRadarVr) {
      if (P.use_err_vr) err[n] = P.obserr_vr;
    }
    const int u = uid_obs(el), t = typ[n];
    if (u < 1 || t < 1 || t > P.nobtype)
      atomicOr(bad, 1);
    else
      atomicOr(&s_use[u - 1], 1u << (t - 1));
  }
  __syncthreads();
  if (threadIdx.x < LETKF_NID_OBS && s_use[threadIdx.x]) atomicOr(&use[threadIdx.x], s_use[threadIdx.x]);
}

struct FileDev {
  int nfile;
  const long* off;           // dev [nfile + 1]
  const int* elm;
  const int* typ;
  const double *lev, *dat, *err, *ri, *rj;
};

// obs(set)%...(idx) per obsda row and ctype_elmtyp(uid_obs(elm), typ) - 1; bad: set / idx outside the files
__global__ void __launch_bounds__(256) row_gather_kernel(const FileDev F, const long nobs, const int* __restrict__ set,
                                                         const int* __restrict__ idx, const int* __restrict__ ctype_elmtyp,
                                                         int* __restrict__ o_elm, int* __restrict__ o_ctype,
                                                         double* __restrict__ o_dat, double* __restrict__ o_err,
                                                         double* __restrict__ o_ri, double* __restrict__ o_rj,
                                                         double* __restrict__ o_lev, int* __restrict__ bad) {
  for (long n = (long)blockIdx.x * blockDim.x + threadIdx.x; n < nobs; n += (long)gridDim.x * blockDim.x) {
    const int f = set[n] - 1;
    const long i = (long)idx[n] - 1;
    long r = -1;
    if (f >= 0 && f < F.nfile && i >= 0 && i < F.off[f + 1] - F.off[f]) r = F.off[f] + i;
    if (r < 0) {
      atomicOr(bad, 1);
      o_elm[n] = 0;
      o_ctype[n] = 0;
      o_dat[n] = o_err[n] = o_ri[n] = o_rj[n] = o_lev[n] = 0.0;
      continue;
    }
    const int el = F.elm[r];
    o_elm[n] = el;
    o_ctype[n] = ctype_elmtyp[(F.typ[r] - 1) * LETKF_NID_OBS + uid_obs(el) - 1] - 1;   // every file row is marked (preprocess)
    o_dat[n] = F.dat[r];
    o_err[n] = F.err[r];
    o_ri[n] = F.ri[r];
    o_rj[n] = F.rj[r];
    o_lev[n] = F.lev[r];
  }
}

// obsgrd(ic)%tot_sub, :744-760: tot[2 ic] rows of ctype ic, tot[2 ic + 1] those with qc == iqc_good
__global__ void __launch_bounds__(256) counts_kernel(const long nobs, const int nctype, const int* __restrict__ ctype,
                                                     const int* __restrict__ qc, int* __restrict__ tot) {
  extern __shared__ int hist[];                          // [2 nctype]
  for (int t = threadIdx.x; t < 2 * nctype; t += blockDim.x) hist[t] = 0;
  __syncthreads();
  for (long n = (long)blockIdx.x * blockDim.x + threadIdx.x; n < nobs; n += (long)gridDim.x * blockDim.x) {
    const int ic = ctype[n];
    atomicAdd(&hist[2 * ic], 1);
    if (qc[n] == 0) atomicAdd(&hist[2 * ic + 1], 1);
  }
  __syncthreads();
  for (int t = threadIdx.x; t < 2 * nctype; t += blockDim.x)
    if (hist[t]) atomicAdd(&tot[t], hist[t]);
}

// the rank's sorted rows (obsbufs, :993-1010): consecutive threads walk along a send row, coalesced on the write side and
// along the ensval row on the read side
__global__ void __launch_bounds__(256) pack_send_kernel(const long ns, const int kld, const int* __restrict__ key,
                                                        const double* __restrict__ ensval, const double* __restrict__ val,
                                                        const double* __restrict__ lev, const int* __restrict__ set,
                                                        const int* __restrict__ idx, double* __restrict__ send) {
  const int ld = kld + 4;
  const long tot = ns * (long)ld;
  for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < tot; t += (long)gridDim.x * blockDim.x) {
    const long r = t / ld;
    const int c = (int)(t - r * ld);
    const long n = key[r];
    double v;
    if (c < kld) v = ensval[n * kld + c];
    else if (c == kld) v = val[n];
    else if (c == kld + 1) v = lev ? lev[n] : 0.0;
    else if (c == kld + 2) v = (double)set[n];
    else v = (double)idx[n];
    send[t] = v;
  }
}

// obsda_sort and the metadata, :1036-1100, in one launch: ensval element-wise (coalesced on both sides), the per-row
// columns by the threads t < nt.  -DH08: type-23 rows carry obsda%lev (the sensitive height) in ob_lev.
__global__ void __launch_bounds__(256) assemble_kernel(const FileDev F, const long nt, const int kld, const int h08,
                                                       const int* __restrict__ src_row, const double* __restrict__ recv,
                                                       double* __restrict__ ens, double* __restrict__ val,
                                                       int* __restrict__ qc, double* __restrict__ ob_ri,
                                                       double* __restrict__ ob_rj, double* __restrict__ ob_lev,
                                                       double* __restrict__ ob_dat, double* __restrict__ ob_err) {
  const long ld = kld + 4;
  const long tot = nt * (long)kld;
  const long stride = (long)gridDim.x * blockDim.x;
  for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < tot; t += stride) {
    const long r = t / kld;
    const int c = (int)(t - r * kld);
    ens[t] = recv[(long)src_row[r] * ld + c];
  }
  for (long r = (long)blockIdx.x * blockDim.x + threadIdx.x; r < nt; r += stride) {
    const double* row = recv + (long)src_row[r] * ld + kld;
    val[r] = row[0];
    qc[r] = 0;                                           // the send buffers hold accepted rows only
    const int f = (int)row[2] - 1;
    const long ii = (long)row[3] - 1;
    if (f < 0 || f >= F.nfile || ii < 0 || ii >= F.off[f + 1] - F.off[f]) {   // a foreign send row outside the files
      ob_ri[r] = ob_rj[r] = ob_lev[r] = ob_dat[r] = ob_err[r] = kUndef;
      continue;
    }
    const long i = F.off[f] + ii;
    ob_ri[r] = F.ri[i];
    ob_rj[r] = F.rj[i];
    ob_lev[r] = (h08 && F.typ[i] == kTypH08) ? row[1] : F.lev[i];
    ob_dat[r] = F.dat[i];
    ob_err[r] = F.err[i];
  }
}

}  // namespace

// ---------------------------------------------------------------------------------------------------------------------
struct letkf_obs_table {
  int device = -1;
  bool finished = false;
  letkf_setobs_params p{};
  letkf_qc_params qc{};
  std::vector<double> hori_local, vert_local, sort_spacing, min_spacing;
  std::vector<int> max_nobs, ctype_merge;
  std::vector<long> off;
  // the caller's file rows (device pointers; they must live until the finish half)
  letkf_obs_file_rows files{};
  long nrows = 0, nobs = 0, nsorted = 0, nobstotal = 0, ncell = 0, nacx = 0;
  int kld = 0, nctype = 0;
  const int* set = nullptr;
  const int* idx = nullptr;
  // host tables
  std::vector<int> elm_ctype, elm_u_ctype, typ_ctype, ctype_elmtyp, ngrd_i, ngrd_j, ngrdsch_i, ngrdsch_j, ngrdext_i,
      ngrdext_j, tot_sub, tot_g, group_start, group_member, vmode, max_nobs_ctype;
  std::vector<double> hori_loc_ctype, vert_loc_ctype, grdspc_i, grdspc_j;
  std::vector<long> ac_off;
  // device buffers
  std::vector<void*> allocs;
  long* d_off = nullptr;
  int *d_ctype_elmtyp = nullptr, *d_row_elm = nullptr, *d_row_ctype = nullptr, *d_n_cell = nullptr, *d_key = nullptr,
      *d_flags = nullptr, *d_tot = nullptr;
  double *d_row_dat = nullptr, *d_row_err = nullptr, *d_row_ri = nullptr, *d_row_rj = nullptr, *d_row_lev = nullptr,
         *d_val = nullptr, *d_send = nullptr;
  void* d_scratch = nullptr;
  // after the finish half
  int *d_ac_ext = nullptr, *d_src_row = nullptr, *d_qc_sort = nullptr;
  double *d_ens_sort = nullptr, *d_val_sort = nullptr, *d_ob[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
  int *d_small_i = nullptr;        // group_start | group_member | vmode | max_nobs | ngrd_i .. ngrdext_j
  double* d_small_d = nullptr;     // hori_loc | vert_loc | varloc
  long* d_ac_off = nullptr;

  ~letkf_obs_table() {
    int prev = -1;
    (void)hipGetDevice(&prev);
    if (device >= 0) (void)hipSetDevice(device);
    for (void* a : allocs) (void)hipFree(a);
    if (prev >= 0) (void)hipSetDevice(prev);                // the caller's current device stays current
  }
};

namespace letkf {

namespace {

template <class T>
hipError_t dalloc(letkf_obs_table* t, T** out, size_t n) {
  void* v = nullptr;
  hipError_t e = hipMalloc(&v, sizeof(T) * (n > 0 ? n : 1));
  if (e != hipSuccess) return e;
  t->allocs.push_back(v);
  *out = static_cast<T*>(v);
  return hipSuccess;
}

FileDev file_dev(const letkf_obs_table* t) {
  return FileDev{t->files.nfile, t->d_off, t->files.elm, t->files.typ, t->files.lev, t->files.dat, t->files.err,
                 t->files.ri, t->files.rj};
}

// letkf_tools.f90:1851-1865 (letkf_vmode of letkf_tools_amd.f90)
int vmode_of(int elm, int typ) {
  if (elm == kIdPs) return 2;
  if (elm == kIdRain) return 3;
  if (typ == kTypPharad) return 1;
  return 0;
}

#define SO_TRY(expr)                                                                                    \
  do {                                                                                                  \
    hipError_t _e = (expr);                                                                             \
    if (_e != hipSuccess) {                                                                             \
      *msg = std::string(#expr) + ": " + hipGetErrorString(_e);                                         \
      return LETKF_E_HIP;                                                                               \
    }                                                                                                   \
  } while (0)

}  // namespace

int obs_mesh_dims(int nctype, const int* typ_ctype, const double* hori_loc_ctype, int nobtype, const double* spacing,
                  const int* max_nobs, const double* min_spacing, double dx, double dy, int nlon, int nlat, int* ngrd_i,
                  int* ngrd_j, double* grdspc_i, double* grdspc_j, int* ngrdsch_i, int* ngrdsch_j, int* ngrdext_i,
                  int* ngrdext_j) {
  for (int ic = 0; ic < nctype; ++ic) {
    const int ityp = typ_ctype[ic];
    if (ityp < 1 || ityp > nobtype) return 1;
    double target;
    if (spacing[ityp - 1] > 0.0)
      target = spacing[ityp - 1];
    else if (max_nobs[ityp - 1] > 0)
      target = 0.1 * std::sqrt((double)max_nobs[ityp - 1]) * min_spacing[ityp - 1];
    else
      target = hori_loc_ctype[ic] * kDistZeroFac / 6.0;
    const double gi = std::ceil(dx * (double)nlon / target), gj = std::ceil(dy * (double)nlat / target);
    ngrd_i[ic] = gi < (double)nlon ? (int)gi : nlon;
    ngrd_j[ic] = gj < (double)nlat ? (int)gj : nlat;
    grdspc_i[ic] = dx * (double)nlon / (double)ngrd_i[ic];
    grdspc_j[ic] = dy * (double)nlat / (double)ngrd_j[ic];
    ngrdsch_i[ic] = (int)std::ceil(hori_loc_ctype[ic] * kDistZeroFac / grdspc_i[ic]);
    ngrdsch_j[ic] = (int)std::ceil(hori_loc_ctype[ic] * kDistZeroFac / grdspc_j[ic]);
    ngrdext_i[ic] = ngrd_i[ic] + ngrdsch_i[ic] * 2;
    ngrdext_j[ic] = ngrd_j[ic] + ngrdsch_j[ic] * 2;
    if (ngrd_i[ic] < 1 || ngrd_j[ic] < 1) return 2;
  }
  return LETKF_OK;
}

int set_obs_local(int device, hipStream_t st, int num_cu, size_t lds_max, const letkf_setobs_params* p,
                  const letkf_qc_params* qcp, const letkf_obs_file_rows* f,
                  long nobs, const int* set, const int* idx, int* qc, double* ensval, long kld, letkf_obs_table** out,
                  std::string* msg) {
  if (!out) return *msg = "tab is NULL", LETKF_E_INVALID;
  *out = nullptr;
  if (!p) return *msg = "p is NULL", LETKF_E_INVALID;
  if (!qcp) return *msg = "qcp is NULL", LETKF_E_INVALID;
  if (!f) return *msg = "files is NULL", LETKF_E_INVALID;
  const letkf_qc_params& q = *qcp;
  if (p->nobtype < 1 || p->nobtype > 32) return *msg = "nobtype must be 1..32", LETKF_E_INVALID;
  if (!p->hori_local) return *msg = "p->hori_local is NULL", LETKF_E_INVALID;
  if (!p->vert_local) return *msg = "p->vert_local is NULL", LETKF_E_INVALID;
  if (!p->obs_sort_grid_spacing) return *msg = "p->obs_sort_grid_spacing is NULL", LETKF_E_INVALID;
  if (!p->obs_min_spacing) return *msg = "p->obs_min_spacing is NULL", LETKF_E_INVALID;
  if (!p->max_nobs_per_grid) return *msg = "p->max_nobs_per_grid is NULL", LETKF_E_INVALID;
  if (p->nlon < 1) return *msg = "nlon must be positive", LETKF_E_INVALID;
  if (p->nlat < 1) return *msg = "nlat must be positive", LETKF_E_INVALID;
  if (p->nprocs < 1) return *msg = "nprocs must be positive", LETKF_E_INVALID;
  if (p->prc_num_x < 1 || p->nprocs % p->prc_num_x != 0) return *msg = "prc_num_x must be positive and divide nprocs", LETKF_E_INVALID;
  if (p->myrank < 0 || p->myrank >= p->nprocs) return *msg = "myrank outside 0..nprocs-1", LETKF_E_INVALID;
  if (!(p->dx > 0.0)) return *msg = "dx must be positive", LETKF_E_INVALID;
  if (!(p->dy > 0.0)) return *msg = "dy must be positive", LETKF_E_INVALID;
  if (f->nfile < 0) return *msg = "files->nfile is negative", LETKF_E_INVALID;
  if (f->nfile > 0 && !f->off) return *msg = "files->off is NULL", LETKF_E_INVALID;
  if (nobs < 0 || nobs >= (1L << 31)) return *msg = "nobs outside 0..2^31-1", LETKF_E_INVALID;
  if (q.member < 1) return *msg = "qcp->member must be positive", LETKF_E_INVALID;
  if (kld < q.member + (q.det_run ? 1 : 0)) return *msg = "kld must hold MEMBER (+1 with DET_RUN) columns", LETKF_E_INVALID;
  if (kld >= (1L << 20)) return *msg = "kld must be below 2^20", LETKF_E_INVALID;
  if (nobs > 0 && !set) return *msg = "set is NULL", LETKF_E_INVALID;
  if (nobs > 0 && !idx) return *msg = "idx is NULL", LETKF_E_INVALID;
  if (nobs > 0 && !qc) return *msg = "qc is NULL", LETKF_E_INVALID;
  if (nobs > 0 && !ensval) return *msg = "ensval is NULL", LETKF_E_INVALID;
  if (nobs > 0 && f->nfile == 0) return *msg = "nobs > 0 with files->nfile = 0: obsda rows without observation files", LETKF_E_INVALID;
  if (q.h08 && nobs > 0 && !q.h08_lev) return *msg = "h08 = 1 needs qcp->h08_lev", LETKF_E_INVALID;

  letkf_obs_table* t = new letkf_obs_table();
  std::unique_ptr<letkf_obs_table> guard(t);
  t->device = device;
  t->p = *p;
  t->qc = q;
  const int nt_ = p->nobtype;
  t->hori_local.assign(p->hori_local, p->hori_local + nt_);
  t->vert_local.assign(p->vert_local, p->vert_local + nt_);
  t->sort_spacing.assign(p->obs_sort_grid_spacing, p->obs_sort_grid_spacing + nt_);
  t->min_spacing.assign(p->obs_min_spacing, p->obs_min_spacing + nt_);
  t->max_nobs.assign(p->max_nobs_per_grid, p->max_nobs_per_grid + nt_);
  t->ctype_merge.assign((size_t)LETKF_NID_OBS * nt_, 0);
  if (p->ctype_merge) t->ctype_merge.assign(p->ctype_merge, p->ctype_merge + (size_t)LETKF_NID_OBS * nt_);
  t->files = *f;
  t->off.assign(f->nfile + 1, 0);
  for (int i = 0; i <= f->nfile && f->nfile > 0; ++i) t->off[i] = f->off[i];
  if (t->off[0] != 0) return *msg = "files->off must start at 0", LETKF_E_INVALID;
  for (int i = 0; i < f->nfile; ++i)
    if (t->off[i + 1] < t->off[i]) return *msg = "files->off must not decrease", LETKF_E_INVALID;
  t->nrows = t->off[f->nfile];
  if (t->nrows > 0) {
    const void* arr[] = {f->elm, f->typ, f->lev, f->dat, f->err, f->ri, f->rj};
    const char* name[] = {"elm", "typ", "lev", "dat", "err", "ri", "rj"};
    for (int i = 0; i < 7; ++i)
      if (!arr[i]) return *msg = std::string("files->") + name[i] + " is NULL", LETKF_E_INVALID;
  }
  t->nobs = nobs;
  t->kld = (int)kld;
  t->set = set;
  t->idx = idx;

  SO_TRY(dalloc(t, &t->d_off, (size_t)f->nfile + 1));
  SO_TRY(dalloc(t, &t->d_flags, 2 + LETKF_NID_OBS));     // [0] bad file row, [1] bad obsda row, [2..] ctype_use
  SO_TRY(hipMemcpyAsync(t->d_off, t->off.data(), sizeof(long) * t->off.size(), hipMemcpyHostToDevice, st));
  SO_TRY(hipMemsetAsync(t->d_flags, 0, sizeof(int) * (2 + LETKF_NID_OBS), st));

  // ---- pre-processing + ctype_use (:268-305)
  unsigned* d_use = reinterpret_cast<unsigned*>(t->d_flags + 2);
  if (t->nrows > 0) {
    PrepParams pp{std::pow(10.0, p->min_radar_ref_dbz / 10.0), p->min_radar_ref_dbz + p->low_ref_shift, p->obserr_radar_ref,
                  p->obserr_radar_vr, p->use_obserr_radar_ref != 0, p->use_obserr_radar_vr != 0, p->nobtype};
    hipLaunchKernelGGL(preprocess_kernel, dim3(grid_for(t->nrows, 256, num_cu)), dim3(256), 0, st, pp, t->nrows, f->elm,
                       f->typ, f->dat, f->err, d_use, t->d_flags);
    SO_TRY(hipGetLastError());
  }
  int hflags[2 + LETKF_NID_OBS];
  SO_TRY(hipMemcpyAsync(hflags, t->d_flags, sizeof(hflags), hipMemcpyDeviceToHost, st));
  SO_TRY(hipStreamSynchronize(st));
  if (hflags[0]) return *msg = "files: a row's elm lies outside uid_obs or its typ outside 1..nobtype", LETKF_E_INVALID;

  // ---- combined-type tables (:307-342): types outer, elements inner, so the ctypes come in ascending order
  t->ctype_elmtyp.assign((size_t)LETKF_NID_OBS * nt_, 0);
  for (int ityp = 1; ityp <= nt_; ++ityp)
    for (int u = 1; u <= LETKF_NID_OBS; ++u) {
      if (!((unsigned)hflags[2 + u - 1] >> (ityp - 1) & 1u)) continue;
      t->ctype_elmtyp[(size_t)(ityp - 1) * LETKF_NID_OBS + u - 1] = (int)t->elm_ctype.size() + 1;
      const int el = kElemUid[u - 1];
      t->elm_ctype.push_back(el);
      t->elm_u_ctype.push_back(u);
      t->typ_ctype.push_back(ityp);
      t->hori_loc_ctype.push_back(el == kIdRadarRefZero ? p->hori_local_radar_obsnoref
                                  : el == kIdRadarVr    ? p->hori_local_radar_vr
                                                        : t->hori_local[ityp - 1]);
      t->vert_loc_ctype.push_back(el == kIdRadarVr ? p->vert_local_radar_vr : t->vert_local[ityp - 1]);
    }
  const int nc = t->nctype = (int)t->elm_ctype.size();

  // ---- sorting-mesh sizes (:657-677)
  for (auto* v : {&t->ngrd_i, &t->ngrd_j, &t->ngrdsch_i, &t->ngrdsch_j, &t->ngrdext_i, &t->ngrdext_j}) v->assign(nc, 0);
  t->grdspc_i.assign(nc, 0.0);
  t->grdspc_j.assign(nc, 0.0);
  if (obs_mesh_dims(nc, t->typ_ctype.data(), t->hori_loc_ctype.data(), nt_, t->sort_spacing.data(), t->max_nobs.data(),
                    t->min_spacing.data(), p->dx, p->dy, p->nlon, p->nlat, t->ngrd_i.data(), t->ngrd_j.data(),
                    t->grdspc_i.data(), t->grdspc_j.data(), t->ngrdsch_i.data(), t->ngrdsch_j.data(), t->ngrdext_i.data(),
                    t->ngrdext_j.data()))
    return *msg = "a sorting mesh came out empty (check hori_local / obs_sort_grid_spacing / dx / dy)", LETKF_E_INVALID;
  t->ac_off.assign(nc, 0);
  for (int ic = 0; ic < nc; ++ic) {
    t->ncell += (long)t->ngrd_i[ic] * t->ngrd_j[ic];
    if (ic + 1 < nc) t->ac_off[ic + 1] = t->ac_off[ic] + (long)(t->ngrdext_i[ic] + 1) * t->ngrdext_j[ic];
    t->nacx += (long)(t->ngrdext_i[ic] + 1) * t->ngrdext_j[ic];
  }

  // ---- row gather + ctype
  const long n1 = nobs > 0 ? nobs : 1;
  SO_TRY(dalloc(t, &t->d_ctype_elmtyp, t->ctype_elmtyp.size()));
  SO_TRY(dalloc(t, &t->d_row_elm, n1));
  SO_TRY(dalloc(t, &t->d_row_ctype, n1));
  SO_TRY(dalloc(t, &t->d_row_dat, n1));
  SO_TRY(dalloc(t, &t->d_row_err, n1));
  SO_TRY(dalloc(t, &t->d_row_ri, n1));
  SO_TRY(dalloc(t, &t->d_row_rj, n1));
  SO_TRY(dalloc(t, &t->d_row_lev, n1));
  SO_TRY(dalloc(t, &t->d_val, n1));
  SO_TRY(dalloc(t, &t->d_key, n1));
  SO_TRY(dalloc(t, &t->d_n_cell, t->ncell));
  SO_TRY(dalloc(t, &t->d_tot, 2 * (size_t)nc));
  SO_TRY(hipMemcpyAsync(t->d_ctype_elmtyp, t->ctype_elmtyp.data(), sizeof(int) * t->ctype_elmtyp.size(),
                        hipMemcpyHostToDevice, st));
  SO_TRY(hipMemsetAsync(t->d_val, 0, sizeof(double) * n1, st));
  if (nc > 0) SO_TRY(hipMemsetAsync(t->d_tot, 0, sizeof(int) * 2 * (size_t)nc, st));
  SO_TRY(hipMemsetAsync(t->d_n_cell, 0, sizeof(int) * (size_t)(t->ncell > 0 ? t->ncell : 1), st));
  if (nobs > 0) {
    hipLaunchKernelGGL(row_gather_kernel, dim3(grid_for(nobs, 256, num_cu)), dim3(256), 0, st, file_dev(t), nobs, set, idx,
                       t->d_ctype_elmtyp, t->d_row_elm, t->d_row_ctype, t->d_row_dat, t->d_row_err, t->d_row_ri,
                       t->d_row_rj, t->d_row_lev, t->d_flags + 1);
    SO_TRY(hipGetLastError());
    SO_TRY(hipMemcpyAsync(hflags, t->d_flags, sizeof(int) * 2, hipMemcpyDeviceToHost, st));
    SO_TRY(hipStreamSynchronize(st));
    if (hflags[1]) return *msg = "an obsda row's set / idx lies outside files", LETKF_E_INVALID;

    // ---- departure + QC (:361-561), counts (:744-760), bucket sort (:762-822)
    SO_TRY(launch_obs_departure(t->qc, nobs, t->d_row_elm, t->d_row_dat, t->d_row_err, ensval, kld, t->d_val, qc, num_cu, lds_max,
                                st));
    hipLaunchKernelGGL(counts_kernel, dim3(grid_for(nobs, 256, num_cu)), dim3(256), sizeof(int) * 2 * nc, st, nobs, nc,
                       t->d_row_ctype, qc, t->d_tot);
    SO_TRY(hipGetLastError());
    letkf_mesh m{nc, p->nlon, p->nlat, p->ihalo, p->jhalo, p->myrank % p->prc_num_x, p->myrank / p->prc_num_x,
                 p->fix_ij_obsgrd, t->ngrd_i.data(), t->ngrd_j.data()};
    size_t need = 0;
    long ns = 0;
    bool bad = false;                                      // every ctype here is ctype_elmtyp's: never set
    SO_TRY(obs_mesh_sort(m, nobs, t->d_row_ctype, t->d_row_ri, t->d_row_rj, qc, t->d_n_cell, t->d_key, &ns, &bad, nullptr,
                         &need, num_cu, st));
    char* scratch = nullptr;
    SO_TRY(dalloc(t, &scratch, need));
    SO_TRY(obs_mesh_sort(m, nobs, t->d_row_ctype, t->d_row_ri, t->d_row_rj, qc, t->d_n_cell, t->d_key, &ns, &bad, scratch,
                         &need, num_cu, st));
    t->nsorted = ns;
  }
  // ---- the rank's send buffer
  SO_TRY(dalloc(t, &t->d_send, (size_t)t->nsorted * (kld + 4)));
  if (t->nsorted > 0) {
    hipLaunchKernelGGL(pack_send_kernel, dim3(grid_for(t->nsorted * (kld + 4), 256, num_cu)), dim3(256), 0, st, t->nsorted,
                       (int)kld, t->d_key, ensval, t->d_val, q.h08 ? q.h08_lev : nullptr, set, idx, t->d_send);
    SO_TRY(hipGetLastError());
  }
  t->tot_sub.assign(2 * (size_t)nc, 0);
  if (nc > 0) SO_TRY(hipMemcpyAsync(t->tot_sub.data(), t->d_tot, sizeof(int) * 2 * nc, hipMemcpyDeviceToHost, st));
  SO_TRY(hipStreamSynchronize(st));
  *out = guard.release();
  return LETKF_OK;
}

int set_obs_finish(hipStream_t st, int num_cu, letkf_obs_table* t, const int* n_all, const int* tot_g, long nrecv,
                   const double* recv, std::string* msg) {
  if (!t) return *msg = "tab is NULL", LETKF_E_INVALID;
  if (t->finished) return *msg = "tab: the finish half already ran on this table", LETKF_E_INVALID;
  const int nc = t->nctype, np = t->p.nprocs, kld = t->kld;
  if (nc > 0 && t->ncell > 0 && !n_all) return *msg = "n_all is NULL", LETKF_E_INVALID;
  if (nrecv < 0) return *msg = "nrecv is negative", LETKF_E_INVALID;
  if (nrecv > 0 && !recv) return *msg = "recv is NULL", LETKF_E_INVALID;
  // the row map indexes the receive buffer: its rows must be exactly the cell counts' total
  long total = 0;
  if (nc > 0 && t->ncell > 0) {
    std::vector<int> h((size_t)np * t->ncell);
    SO_TRY(hipMemcpyAsync(h.data(), n_all, sizeof(int) * h.size(), hipMemcpyDeviceToHost, st));
    SO_TRY(hipStreamSynchronize(st));
    for (int v : h) {
      if (v < 0) return *msg = "n_all holds a negative cell count", LETKF_E_INVALID;
      total += v;
    }
  }
  if (total >= (1L << 31)) return *msg = "the total of n_all reaches 2^31 rows", LETKF_E_INVALID;
  if (total != nrecv) return *msg = "nrecv differs from the total of n_all", LETKF_E_INVALID;
  SO_TRY(dalloc(t, &t->d_ac_ext, t->nacx));
  SO_TRY(dalloc(t, &t->d_src_row, nrecv));
  long nt = 0;
  if (nc > 0) {
    letkf_halo_layout l{nc, np, t->p.prc_num_x, t->p.myrank, t->ngrd_i.data(), t->ngrd_j.data(), t->ngrdsch_i.data(),
                        t->ngrdsch_j.data()};
    const char* refused = nullptr;
    hipError_t e = obs_halo_plan(l, n_all, t->d_ac_ext, t->d_src_row, nrecv, &nt, &refused, num_cu, st);
    if (refused) return *msg = refused, LETKF_E_INVALID;
    SO_TRY(e);
  }
  t->nobstotal = nt;
  SO_TRY(dalloc(t, &t->d_ens_sort, (size_t)nt * kld));
  SO_TRY(dalloc(t, &t->d_val_sort, nt));
  SO_TRY(dalloc(t, &t->d_qc_sort, nt));
  for (auto& o : t->d_ob) SO_TRY(dalloc(t, &o, nt));
  if (nt > 0) {
    hipLaunchKernelGGL(assemble_kernel, dim3(grid_for(nt * kld, 256, num_cu)), dim3(256), 0, st, file_dev(t), nt, kld,
                       t->qc.h08, t->d_src_row, recv, t->d_ens_sort, t->d_val_sort, t->d_qc_sort, t->d_ob[0], t->d_ob[1],
                       t->d_ob[2], t->d_ob[3], t->d_ob[4]);
    SO_TRY(hipGetLastError());
  }
  t->tot_g = t->tot_sub;
  if (tot_g && nc > 0) SO_TRY(hipMemcpyAsync(t->tot_g.data(), tot_g, sizeof(int) * 2 * nc, hipMemcpyDeviceToHost, st));

  // ---- the search tables' small per-ctype arrays (letkf_tools.f90:167-192 groups, :1851-1865 vertical mode)
  t->group_start.assign(nc + 1, 0);
  t->group_member.assign(nc > 0 ? nc : 1, 0);
  int ngroup = 0;
  if (nc > 0 && letkf_ctype_merge_groups(nc, t->elm_u_ctype.data(), t->typ_ctype.data(), LETKF_NID_OBS, t->p.nobtype,
                                         t->ctype_merge.data(), t->group_start.data(), t->group_member.data(), &ngroup))
    return *msg = "letkf_ctype_merge_groups failed", LETKF_E_INVALID;
  t->group_start.resize(ngroup + 1);
  t->vmode.assign(nc, 0);
  t->max_nobs_ctype.assign(nc, 0);
  for (int ic = 0; ic < nc; ++ic) {
    t->vmode[ic] = vmode_of(t->elm_ctype[ic], t->typ_ctype[ic]);
    t->max_nobs_ctype[ic] = t->max_nobs[t->typ_ctype[ic] - 1];
  }
  std::vector<int> si;
  for (auto* v : {&t->group_start, &t->group_member, &t->vmode, &t->max_nobs_ctype, &t->ngrd_i, &t->ngrd_j, &t->ngrdsch_i,
                  &t->ngrdsch_j, &t->ngrdext_i, &t->ngrdext_j})
    si.insert(si.end(), v->begin(), v->end());
  std::vector<double> sd(t->hori_loc_ctype);
  sd.insert(sd.end(), t->vert_loc_ctype.begin(), t->vert_loc_ctype.end());
  sd.insert(sd.end(), (size_t)nc, 1.0);
  SO_TRY(dalloc(t, &t->d_small_i, si.size()));
  SO_TRY(dalloc(t, &t->d_small_d, sd.size()));
  SO_TRY(dalloc(t, &t->d_ac_off, (size_t)nc));
  if (!si.empty()) SO_TRY(hipMemcpyAsync(t->d_small_i, si.data(), sizeof(int) * si.size(), hipMemcpyHostToDevice, st));
  if (!sd.empty()) SO_TRY(hipMemcpyAsync(t->d_small_d, sd.data(), sizeof(double) * sd.size(), hipMemcpyHostToDevice, st));
  if (nc > 0) SO_TRY(hipMemcpyAsync(t->d_ac_off, t->ac_off.data(), sizeof(long) * nc, hipMemcpyHostToDevice, st));
  SO_TRY(hipStreamSynchronize(st));
  t->finished = true;
  return LETKF_OK;
}

int obs_table_search(const letkf_obs_table* t, letkf_search_tables* s) {
  if (!t || !s || !t->finished) return LETKF_E_INVALID;
  const int nc = t->nctype;
  const int ng = (int)t->group_start.size() - 1;
  std::memset(s, 0, sizeof(*s));
  s->nctype = nc;
  s->ngroup = ng;
  s->criterion = t->p.criterion;
  s->nlon = t->p.nlon;
  s->nlat = t->p.nlat;
  bool lim = false;
  for (int v : t->max_nobs_ctype) lim = lim || v > 0;
  s->limit_hint = lim ? 2 : 1;
  s->dx = t->p.dx;
  s->dy = t->p.dy;
  s->i_org = (double)t->p.ihalo + 0.5 + (double)((t->p.myrank % t->p.prc_num_x) * t->p.nlon);   // ij_obsgrd_ext, :1221
  s->j_org = (double)t->p.jhalo + 0.5 + (double)((t->p.myrank / t->p.prc_num_x) * t->p.nlat);
  s->rain_base = t->p.rain_base;
  const int* b = t->d_small_i;
  s->group_start = b;
  s->group_member = b + (ng + 1);
  const int* c = b + (ng + 1) + nc;
  s->vmode = c;
  s->max_nobs = c + nc;
  s->ngrd_i = c + 2 * nc;
  s->ngrd_j = c + 3 * nc;
  s->ngrdsch_i = c + 4 * nc;
  s->ngrdsch_j = c + 5 * nc;
  s->ngrdext_i = c + 6 * nc;
  s->ngrdext_j = c + 7 * nc;
  s->hori_loc = t->d_small_d;
  s->vert_loc = t->d_small_d + nc;
  s->varloc = t->d_small_d + 2 * nc;
  s->ac_off = reinterpret_cast<const int64_t*>(t->d_ac_off);
  s->ac_ext = t->d_ac_ext;
  s->ob_ri = t->d_ob[0];
  s->ob_rj = t->d_ob[1];
  s->ob_lev = t->d_ob[2];
  s->ob_dat = t->d_ob[3];
  s->ob_err = t->d_ob[4];
  return LETKF_OK;
}

int obs_table_set_varloc(hipStream_t st, letkf_obs_table* t, const double* varloc, std::string* msg) {
  if (!t) return *msg = "tab is NULL", LETKF_E_INVALID;
  if (!t->finished) return *msg = "tab: the finish half has not run", LETKF_E_INVALID;
  if (t->nctype > 0 && !varloc) return *msg = "varloc is NULL", LETKF_E_INVALID;
  if (t->nctype > 0)
    SO_TRY(hipMemcpyAsync(t->d_small_d + 2 * t->nctype, varloc, sizeof(double) * t->nctype, hipMemcpyHostToDevice, st));
  SO_TRY(hipStreamSynchronize(st));
  return LETKF_OK;
}

int obs_table_info(const letkf_obs_table* t, letkf_obs_table_info* i) {
  if (!t || !i) return LETKF_E_INVALID;
  std::memset(i, 0, sizeof(*i));
  i->nctype = t->nctype;
  i->kld = t->kld;
  i->finished = t->finished ? 1 : 0;
  i->nobtype = t->p.nobtype;
  i->nobs = t->nobs;
  i->nsorted = t->nsorted;
  i->ncell = t->ncell;
  i->nacx = t->nacx;
  i->nobstotal = t->nobstotal;
  i->ld_send = t->kld + 4;
  i->elm_ctype = t->elm_ctype.data();
  i->elm_u_ctype = t->elm_u_ctype.data();
  i->typ_ctype = t->typ_ctype.data();
  i->hori_loc_ctype = t->hori_loc_ctype.data();
  i->vert_loc_ctype = t->vert_loc_ctype.data();
  i->ctype_elmtyp = t->ctype_elmtyp.data();
  i->ngrd_i = t->ngrd_i.data();
  i->ngrd_j = t->ngrd_j.data();
  i->ngrdsch_i = t->ngrdsch_i.data();
  i->ngrdsch_j = t->ngrdsch_j.data();
  i->ngrdext_i = t->ngrdext_i.data();
  i->ngrdext_j = t->ngrdext_j.data();
  i->grdspc_i = t->grdspc_i.data();
  i->grdspc_j = t->grdspc_j.data();
  i->ac_off = reinterpret_cast<const int64_t*>(t->ac_off.data());
  i->tot_sub = t->tot_sub.data();
  i->tot_g = t->finished ? t->tot_g.data() : nullptr;
  i->n_cell = t->d_n_cell;
  i->key = t->d_key;
  i->sendbuf = t->d_send;
  i->row_elm = t->d_row_elm;
  i->row_ctype = t->d_row_ctype;
  i->row_dat = t->d_row_dat;
  i->row_err = t->d_row_err;
  i->row_ri = t->d_row_ri;
  i->row_rj = t->d_row_rj;
  i->row_lev = t->d_row_lev;
  i->val = t->d_val;
  i->ensval = t->d_ens_sort;
  i->val_sort = t->d_val_sort;
  i->qc_sort = t->d_qc_sort;
  return LETKF_OK;
}

void obs_table_destroy(letkf_obs_table* t) { delete t; }

int obs_table_download(hipStream_t st, const letkf_obs_table* t, double* ensval, double* val, int* qc, double* ob[5],
                       int* ac_ext, std::string* msg) {
  if (!t) return *msg = "tab is NULL", LETKF_E_INVALID;
  if (!t->finished) return *msg = "tab: the finish half has not run", LETKF_E_INVALID;
  const size_t nt = (size_t)t->nobstotal;
  if (ensval && nt) SO_TRY(hipMemcpyAsync(ensval, t->d_ens_sort, sizeof(double) * nt * t->kld, hipMemcpyDeviceToHost, st));
  if (val && nt) SO_TRY(hipMemcpyAsync(val, t->d_val_sort, sizeof(double) * nt, hipMemcpyDeviceToHost, st));
  if (qc && nt) SO_TRY(hipMemcpyAsync(qc, t->d_qc_sort, sizeof(int) * nt, hipMemcpyDeviceToHost, st));
  for (int k = 0; k < 5; ++k)
    if (ob[k] && nt) SO_TRY(hipMemcpyAsync(ob[k], t->d_ob[k], sizeof(double) * nt, hipMemcpyDeviceToHost, st));
  if (ac_ext && t->nacx) SO_TRY(hipMemcpyAsync(ac_ext, t->d_ac_ext, sizeof(int) * t->nacx, hipMemcpyDeviceToHost, st));
  SO_TRY(hipStreamSynchronize(st));
  return LETKF_OK;
}

}  // namespace letkf
