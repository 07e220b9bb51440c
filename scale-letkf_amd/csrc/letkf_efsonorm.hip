// letkf_efsonorm.hip -- the two ends of EFSO around das_efso (scale/letkf/efso.f90):
//   the forecast-error norm: the fcer assembly of efso.f90:100-117 and lnorm (scale/letkf/efso_tools.f90:52-156) in
//     SCALE's frame -- ensemble mean and perturbations, the layer weight sqrt(dp/ps) * wg1, the energy-norm factor of
//     each variable, the target region -- in one pass over the forecast ensemble (two small passes before it build
//     dp/ps from the mean pressure when the caller gives no layer weights);
//   the impact summary: print_obsense's table (efso_tools.f90:232-253) -- per region x observation type x element the
//     count, the summed impact and the number of negative impacts of every term.
//   No multiply-add fusion (the pragma below) and no floating-point atomics: every value is the formula evaluated one
//   IEEE operation at a time in the order of include/letkf_amd.h section 13, as numpy evaluates it.
#include <hip/hip_runtime.h>
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/iterator/counting_iterator.hpp>

#include "letkf_device.h"

#pragma clang fp contract(off)

namespace letkf {

namespace {

constexpr int kNormRegK = 64;   // members held in registers by the one-read norm kernel (k <= 64); larger k reads twice

// lnorm's ensmn3d: a sequential sum over the members starting from 0, times rinbv = 1/k
__device__ inline double member_mean(const double* __restrict__ x, long sm, int k, double rinbv) {
  double s = 0.0;
  for (int m = 0; m < k; ++m) s += x[m * sm];
  return s * rinbv;
}

// Mean pressure of every point (variable iv_p), for the half-level rule
__global__ void __launch_bounds__(256) efso_pmean_kernel(long npts, int k, const double* __restrict__ fcst, long sp, long sm,
                                                         double rinbv, double* __restrict__ pbar) {
  for (long p = (long)blockIdx.x * blockDim.x + threadIdx.x; p < npts; p += (long)gridDim.x * blockDim.x)
    pbar[p] = member_mean(fcst + p * sp, sm, k, rinbv);
}

// dp/ps of every level of a column from the mean pressure (levels bottom first), by the half-level rule of the header;
// a column with dp <= 0, ps <= 0 or a non-finite value at any level counts in *bad
__global__ void __launch_bounds__(256) efso_dpw_kernel(long nij1, int nlev, const double* __restrict__ pb,
                                                       double* __restrict__ w, unsigned* __restrict__ bad) {
  unsigned nbad = 0;
  for (long ij = (long)blockIdx.x * blockDim.x + threadIdx.x; ij < nij1; ij += (long)gridDim.x * blockDim.x) {
    if (nlev == 1) {
      w[ij] = 1.0;
      continue;
    }
    const double p1 = pb[ij], p2 = pb[ij + nij1];
    const double ps = p1 + 0.5 * (p1 - p2);
    bool ok = ps > 0.0 && isfinite(ps);
    double lo = ps;                                            // p_{l-1/2}
    for (int l = 0; l < nlev; ++l) {
      const double pl = pb[ij + nij1 * l];
      double hi;                                               // p_{l+1/2}
      if (l + 1 < nlev) {
        hi = 0.5 * (pl + pb[ij + nij1 * (l + 1)]);
      } else {
        const double t = pl - 0.5 * (pb[ij + nij1 * (l - 1)] - pl);
        hi = t > 0.0 ? t : 0.0;
      }
      const double dp = lo - hi;
      const double r = dp / ps;
      ok = ok && dp > 0.0 && isfinite(r);                      // (false for NaN)
      w[ij + nij1 * l] = r;
      lo = hi;
    }
    nbad += ok ? 0u : 1u;
  }
  if (nbad) atomicAdd(bad, nbad);
}

// The norm: one thread per point p = ij + nij1*lev.  Variables of class 0 (and every variable outside the target region)
// are written as zeros without their inputs being read, unless fmean asks for the mean.
template <int KR>
__global__ void __launch_bounds__(256) efso_norm_kernel(const EfsoNormArgs a) {
  const int k = a.k;
  const long sm = a.sm;
  for (long p = (long)blockIdx.x * blockDim.x + threadIdx.x; p < a.npts; p += (long)gridDim.x * blockDim.x) {
    const long ij = p % a.nij1, lev = p / a.nij1;
    bool in = lev >= a.lev0 && lev <= a.lev1;
    if (in && a.lon) {
      const double lo = a.lon[ij], la = a.lat[ij];
      in = !(lo < a.minlon || lo > a.maxlon || la < a.minlat || la > a.maxlat);
    }
    double sw = 0.0;
    if (in) {
      sw = sqrt(a.wl[p]);
      if (a.wg1) sw = sw * a.wg1[ij];
    }
    double* xp = a.fcst + p * a.sp;
    for (int v = 0; v < a.nv; ++v) {
      const int c = in ? a.cls[v] : 0;
      const double f = c == 1 ? sw : c == 2 ? a.cptr * sw : a.qweight * sw;
      double* x = xp + v * a.sv;
      if (c == 0 && !a.fmean) {
        for (int m = 0; m < k; ++m) x[m * sm] = 0.0;
        continue;
      }
      double mean;
      if constexpr (KR > 0) {
        double r[KR];
        const double* y = x;
#pragma unroll
        for (int m = 0; m < KR; ++m)
          if (m < k) {
            r[m] = *y;
            y += sm;
          }
        double s = 0.0;
#pragma unroll
        for (int m = 0; m < KR; ++m)
          if (m < k) s += r[m];
        mean = s * a.rinbv;
        if (a.fmean) a.fmean[p + a.npts * v] = mean;
        double* z = x;
#pragma unroll
        for (int m = 0; m < KR; ++m)
          if (m < k) {
            *z = c == 0 ? 0.0 : f * (r[m] - mean);
            z += sm;
          }
      } else {
        mean = member_mean(x, sm, k, a.rinbv);
        if (a.fmean) a.fmean[p + a.npts * v] = mean;
        for (int m = 0; m < k; ++m) x[m * sm] = c == 0 ? 0.0 : f * (x[m * sm] - mean);
      }
    }
    for (int v = 0; v < a.nv; ++v) {
      const int c = in ? a.cls[v] : 0;
      const long q = p * a.fsp + v * a.fsv;
      if (c == 0) {
        a.fcer[q] = 0.0;
        continue;
      }
      const double f = c == 1 ? sw : c == 2 ? a.cptr * sw : a.qweight * sw;
      const double e = a.xf ? (0.5 * (a.xf[q] + a.xg[q]) - a.xa[q]) / a.km1 : a.fcer[q];
      a.fcer[q] = f * e;
    }
  }
}

// ---- the summary (print_obsense)
constexpr int kMaxElem = 32;
struct ElemTable {
  int n;
  int id[kMaxElem];
};

// Bin of every row: (region * (nobtype + 1) + type - 1) * nid + element, regions NH = 0, TR = 1, SH = 2; a skipped row
// (qc != 0, element not in the table, type outside 1..nobtype+1) gets the key nbins and sorts behind every bin.
__global__ void __launch_bounds__(256) efso_bin_kernel(long nobs, const int* __restrict__ elm, const int* __restrict__ typ,
                                                       const double* __restrict__ lat, const int* __restrict__ qc,
                                                       const ElemTable T, int nobtype, double latbound, unsigned nbins,
                                                       int* __restrict__ cnt, unsigned* __restrict__ keys) {
  for (long n = (long)blockIdx.x * blockDim.x + threadIdx.x; n < nobs; n += (long)gridDim.x * blockDim.x) {
    unsigned key = nbins;
    const int e = elm[n], ot = typ[n];
    int oid = -1;
    for (int u = 0; u < T.n; ++u)
      if (T.id[u] == e) {
        oid = u;
        break;
      }
    if ((!qc || qc[n] == 0) && oid >= 0 && ot >= 1 && ot <= nobtype + 1) {
      const double y = lat[n];
      const int reg = y > latbound ? 0 : (y < -latbound ? 2 : 1);
      key = (unsigned)((reg * (nobtype + 1) + ot - 1) * T.n + oid);
      atomicAdd(cnt + key, 1);
    }
    keys[n] = key;
  }
}

// One thread per (term, bin): the bin's rows in ascending row order, summed from 0 one after the other
__global__ void __launch_bounds__(256) efso_binsum_kernel(int nterm, unsigned nbins, const long* __restrict__ start,
                                                          const unsigned* __restrict__ perm, const double* __restrict__ obsense,
                                                          int* __restrict__ count, double* __restrict__ sum,
                                                          int* __restrict__ nneg) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long)nterm * nbins) return;
  const int t = (int)(i / nbins);
  const long b = i - (long)t * nbins;
  const long q0 = start[b], q1 = start[b + 1];
  double s = 0.0;
  int neg = 0;
  for (long q = q0; q < q1; ++q) {
    const double x = obsense[(long)perm[q] * nterm + t];
    s += x;
    neg += x < 0.0 ? 1 : 0;
  }
  sum[i] = s;
  nneg[i] = neg;
  if (t == 0) count[b] = (int)(q1 - q0);
}

int key_bits(unsigned nkeys) {   // bits that hold the keys 0 .. nkeys
  int b = 1;
  while (b < 31 && (1u << b) <= nkeys) ++b;
  return b;
}

hipError_t sort_bins(void* temp, size_t* temp_bytes, const unsigned* keys, unsigned* keys_out, unsigned* perm, size_t n,
                     unsigned nbins, hipStream_t st) {
  return rocprim::radix_sort_pairs(temp, *temp_bytes, keys, keys_out, rocprim::counting_iterator<unsigned>(0u), perm, n, 0u,
                                   (unsigned)key_bits(nbins), st);
}

}  // namespace

hipError_t launch_efso_dpw(long nij1, int nlev, int k, const double* fcst_p, long sp, long sm, double rinbv, double* pbar,
                           double* w, unsigned* bad, int num_cu, hipStream_t st) {
  const long npts = nij1 * nlev;
  hipLaunchKernelGGL(efso_pmean_kernel, dim3(grid_for(npts, 256, num_cu)), dim3(256), 0, st, npts, k, fcst_p, sp, sm, rinbv, pbar);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(efso_dpw_kernel, dim3(grid_for(nij1, 256, num_cu)), dim3(256), 0, st, nij1, nlev, pbar, w, bad);
  return hipGetLastError();
}

hipError_t launch_efso_norm(const EfsoNormArgs& a, int num_cu, hipStream_t st) {
  if (a.npts <= 0) return hipSuccess;
  if (a.k <= kNormRegK)
    hipLaunchKernelGGL(efso_norm_kernel<kNormRegK>, dim3(grid_for(a.npts, 256, num_cu)), dim3(256), 0, st, a);
  else
    hipLaunchKernelGGL(efso_norm_kernel<0>, dim3(grid_for(a.npts, 256, num_cu)), dim3(256), 0, st, a);
  return hipGetLastError();
}

const char* efso_norm_path_name(int k) {
  return k <= kNormRegK ? "efso_norm_kernel<64>" : "efso_norm_kernel<0>";
}

// Workspace of the summary: keys [nobs] | keys_out [nobs] | perm [nobs] | cnt [nbins+1] | start [nbins+1] | sort | scan
size_t efso_summary_ws(long nobs, unsigned nbins, hipStream_t st, size_t* sort_bytes, size_t* scan_bytes) {
  auto al = [](size_t b) { return (b + 255) & ~(size_t)255; };
  const size_t n1 = (size_t)(nobs > 0 ? nobs : 1);
  *sort_bytes = *scan_bytes = 0;
  if (sort_bins(nullptr, sort_bytes, nullptr, nullptr, nullptr, n1, nbins, st) != hipSuccess) return 0;
  if (count_scan(nullptr, scan_bytes, nullptr, nullptr, (size_t)nbins + 1, st) != hipSuccess) return 0;
  return 3 * al(n1 * 4) + al(((size_t)nbins + 1) * 4) + al(((size_t)nbins + 1) * 8) + al(*sort_bytes) + al(*scan_bytes) + 256;
}

hipError_t launch_efso_summary(int nterm, long nobs, const double* obsense, const int* elm, const int* typ, const double* lat,
                               const int* qc, int nid, const int* elem_uid, int nobtype, double latbound, int* count,
                               double* sum, int* nneg, char* ws, size_t sort_bytes, size_t scan_bytes, int num_cu,
                               hipStream_t st) {
  auto al = [](size_t b) { return (b + 255) & ~(size_t)255; };
  if (nid < 1 || nid > kMaxElem) return hipErrorInvalidValue;
  const unsigned nbins = 3u * (unsigned)(nobtype + 1) * (unsigned)nid;
  const size_t n1 = (size_t)(nobs > 0 ? nobs : 1);
  unsigned* keys = reinterpret_cast<unsigned*>(ws);
  unsigned* keys_out = reinterpret_cast<unsigned*>(ws + al(n1 * 4));
  unsigned* perm = reinterpret_cast<unsigned*>(ws + 2 * al(n1 * 4));
  int* cnt = reinterpret_cast<int*>(ws + 3 * al(n1 * 4));
  long* start = reinterpret_cast<long*>(ws + 3 * al(n1 * 4) + al(((size_t)nbins + 1) * 4));
  char* sort_ws = ws + 3 * al(n1 * 4) + al(((size_t)nbins + 1) * 4) + al(((size_t)nbins + 1) * 8);
  char* scan_ws = sort_ws + al(sort_bytes);
  ElemTable T;
  T.n = nid;
  for (int i = 0; i < kMaxElem; ++i) T.id[i] = i < nid ? elem_uid[i] : 0;
  hipError_t e = hipMemsetAsync(cnt, 0, ((size_t)nbins + 1) * 4, st);
  if (e != hipSuccess) return e;
  if (nobs > 0) {
    hipLaunchKernelGGL(efso_bin_kernel, dim3(grid_for(nobs, 256, num_cu)), dim3(256), 0, st, nobs, elm, typ, lat, qc, T, nobtype,
                       latbound, nbins, cnt, keys);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    size_t sb = sort_bytes;
    if ((e = sort_bins(sort_ws, &sb, keys, keys_out, perm, (size_t)nobs, nbins, st)) != hipSuccess) return e;
  }
  size_t cb = scan_bytes;
  if ((e = count_scan(scan_ws, &cb, cnt, start, (size_t)nbins + 1, st)) != hipSuccess) return e;
  const long nth = (long)nterm * nbins;
  hipLaunchKernelGGL(efso_binsum_kernel, dim3((unsigned)((nth + 255) / 256)), dim3(256), 0, st, nterm, nbins, start, perm,
                     obsense, count, sum, nneg);
  return hipGetLastError();
}

}  // namespace letkf
