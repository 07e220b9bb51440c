// letkf_nobsout.hip -- the kernels of NOBS_OUT (include/letkf_amd_nobsout.h): work3dn and the reference's eleven fields from the
// counts and cut-offs per combined type (scale/letkf/letkf_tools.f90:440-447, :768-778), the default cut-offs of tables without a
// limit (:1384-1389) and the zeros of the points the main loop does not analyse (:333-359).  All three are pure data movement.

#include "letkf_nobsout_dev.h"
#include "letkf_search_dev.h"

namespace letkf {

namespace {

constexpr int kBlock = 128;   // threads of a workgroup, and the points of its tile
constexpr int kRadar = 3;     // ref, re0, vr

// A tile of kBlock consecutive points per workgroup.  nobs_ctype is point-major with a short row, and the rows of consecutive points
// are adjacent: the tile's rows are ONE contiguous run of kBlock * nctype ints, which the workgroup loads lane after lane into LDS
// (row stride odd: a lane per point then reads without bank conflicts).  Of cutd_ctype only the three radar columns are read.  The
// outputs are written in the order that is contiguous in memory: work3dn element after element of the tile's [kBlock][nobtype + 6]
// run, the fields point after point (sp <= sv) or field after field (the transposed layout).
__global__ void __launch_bounds__(kBlock) nobs_fields_kernel(const NobsFieldsArgs A) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_nobs[];
  __shared__ int s_start[LETKF_NOBSOUT_MAX_OBTYPE + 1], s_member[LETKF_NOBSOUT_MAX_CTYPE], s_rowf[LETKF_NOBSOUT_NFIELDS], s_icr[kRadar];
  const int tid = threadIdx.x;
  const int nct = A.nctype, stride = nct | 1, nobt = A.nobtype, nrow = nobt + 2 * kRadar;
  double* s_cut = reinterpret_cast<double*>(smem_nobs);           // [kRadar][kBlock]
  int* s_n = reinterpret_cast<int*>(s_cut + kRadar * kBlock);     // [kBlock][stride]
  if (tid <= nobt) s_start[tid] = A.typ_start[tid];
  if (tid < nct) s_member[tid] = A.typ_member[tid];
  if (tid < LETKF_NOBSOUT_NFIELDS) s_rowf[tid] = A.row_field[tid];
  if (tid < kRadar) s_icr[tid] = A.ic_radar[tid];
  __syncthreads();

  // row r of work3dn at point pt of the tile
  auto value = [&](const int pt, const int r) -> double {
    if (r < nobt) {                                               // sum(nobsl_t, dim=1), :441
      int s = 0;
      for (int m = s_start[r]; m < s_start[r + 1]; ++m) s += s_n[pt * stride + s_member[m]];
      return (double)s;
    }
    const int q = r - nobt;
    if (q >= kRadar) return s_cut[(q - kRadar) * kBlock + pt];    // cutd_t(uid, 22), :445-447
    const int ic = s_icr[q];                                      // nobsl_t(uid, 22), :442-444
    return ic >= 0 ? (double)s_n[pt * stride + ic] : 0.0;
  };

  const int64_t ntile = (A.npts + kBlock - 1) / kBlock;
  for (int64_t tile = blockIdx.x; tile < ntile; tile += gridDim.x) {
    const int64_t p0 = tile * kBlock;
    const int npt = (int)(A.npts - p0 < kBlock ? A.npts - p0 : kBlock);
    const int32_t* gn = A.nobs_ctype + p0 * nct;
    for (int e = tid; e < npt * nct; e += kBlock) {
      const int pt = e / nct;
      s_n[pt * stride + (e - pt * nct)] = gn[e];
    }
    if (tid < npt)
      for (int q = 0; q < kRadar; ++q) {
        const int ic = s_icr[q];
        s_cut[q * kBlock + tid] = (ic >= 0 && A.cutd_ctype) ? A.cutd_ctype[(p0 + tid) * nct + ic] : 0.0;
      }
    __syncthreads();
    if (A.work3dn) {
      double* gw = A.work3dn + p0 * nrow;
      for (int e = tid; e < npt * nrow; e += kBlock) {
        const int pt = e / nrow;
        gw[e] = value(pt, e - pt * nrow);
      }
    }
    if (A.fields) {
      if (A.sp <= A.sv) {
        if (tid < npt)
          for (int f = 0; f < LETKF_NOBSOUT_NFIELDS; ++f) A.fields[(p0 + tid) * A.sp + f * A.sv] = value(tid, s_rowf[f]);
      } else {
        for (int e = tid; e < npt * LETKF_NOBSOUT_NFIELDS; e += kBlock) {
          const int pt = e / LETKF_NOBSOUT_NFIELDS, f = e - pt * LETKF_NOBSOUT_NFIELDS;
          A.fields[(p0 + pt) * A.sp + f * A.sv] = value(pt, s_rowf[f]);
        }
      }
    }
    __syncthreads();                                              // (the next tile overwrites s_n / s_cut)
  }
}

// n = npts * nctype elements, element e of combined type e mod nctype
__global__ void __launch_bounds__(256) nobs_cutd_default_kernel(const letkf_search_tables t, const int64_t n, double* cutd) {
  extern __shared__ __attribute__((aligned(16))) double s_def[];  // [nctype]
  for (int ic = threadIdx.x; ic < t.nctype; ic += 256) s_def[ic] = 0.0;
  __syncthreads();
  if (t.criterion == 1)
    for (int g = threadIdx.x; g < t.ngroup; g += 256) {
      const int icm = t.group_member[t.group_start[g]];           // the master
      if (icm >= 0 && icm < t.nctype) s_def[icm] = t.hori_loc[icm] * search_dev::kDistZeroFac;
    }
  __syncthreads();
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (int64_t)gridDim.x * 256) cutd[e] = s_def[e % t.nctype];
}

__global__ void __launch_bounds__(256) nobs_zero_unanalysed_kernel(const int64_t n, const int nctype, const double* beta, int32_t* nobs,
                                                                   double* cutd) {
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (int64_t)gridDim.x * 256)
    if (beta[e / nctype] == 0.0) {
      if (nobs) nobs[e] = 0;
      if (cutd) cutd[e] = 0.0;
    }
}

unsigned grid_of(const int64_t nblock, const int num_cu, const int per_cu) {
  const int64_t g = (int64_t)num_cu * per_cu;
  return (unsigned)(nblock < g ? (nblock > 0 ? nblock : 1) : g);
}

}  // namespace

hipError_t launch_nobs_fields(const NobsFieldsArgs& a, int num_cu, hipStream_t st) {
  if (a.npts <= 0) return hipSuccess;
  const size_t lds = (size_t)kRadar * kBlock * sizeof(double) + (size_t)kBlock * (a.nctype | 1) * sizeof(int);   // <= 36352 B
  hipLaunchKernelGGL(nobs_fields_kernel, dim3(grid_of((a.npts + kBlock - 1) / kBlock, num_cu, 16)), dim3(kBlock), lds, st, a);
  return hipGetLastError();
}

hipError_t launch_nobs_cutd_default(const letkf_search_tables& t, int64_t npts, double* cutd_ctype, int num_cu, hipStream_t st) {
  const int64_t n = npts * t.nctype;
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(nobs_cutd_default_kernel, dim3(grid_of((n + 255) / 256, num_cu, 16)), dim3(256), (size_t)t.nctype * sizeof(double), st,
                     t, n, cutd_ctype);
  return hipGetLastError();
}

hipError_t launch_nobs_zero_unanalysed(int64_t npts, int32_t nctype, const double* beta, int32_t* nobs_ctype, double* cutd_ctype,
                                       int num_cu, hipStream_t st) {
  const int64_t n = npts * nctype;
  if (n <= 0 || !beta || (!nobs_ctype && !cutd_ctype)) return hipSuccess;
  hipLaunchKernelGGL(nobs_zero_unanalysed_kernel, dim3(grid_of((n + 255) / 256, num_cu, 16)), dim3(256), 0, st, n, nctype, beta, nobs_ctype,
                     cutd_ctype);
  return hipGetLastError();
}

}  // namespace letkf
