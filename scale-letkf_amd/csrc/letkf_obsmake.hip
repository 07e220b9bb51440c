// letkf_obsmake.hip -- the kernels of obsmake_cal (include/letkf_amd_obsmake.h; scale/obs/obsope_tools.f90:767-1058) around
// the operator of letkf_obsope.hip:
//   randn_pairs_kernel      Box-Muller of com_randn (common/common.f90:278-295), one lane per pair of uniforms
//   obsmake_count / fill    the rows of one time slot that this subdomain processes, compacted for the operator
//   obsmake_scatter         dat = H(x) where qc is 0, else undef; undef for the rows outside the global domain; nslot / nobs_slot
//   obsmake_noise           err by element, dat += err * error
// The unit is compiled without floating-point contraction (Makefile): the deviate's product and err * error + dat round as
// the reference's expressions do, term by term.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>

#include "letkf_obsmake_dev.h"

namespace {

constexpr int kIdU = 2819, kIdV = 2820, kIdT = 3073, kIdTv = 3074, kIdQ = 3330, kIdRh = 3331, kIdPs = 14593,
              kIdRadarRef = 4001, kIdRadarRefZero = 4004, kIdRadarVr = 4002;                       // common_obs_scale.f90:48-67
constexpr double kPi = 3.1415926535, kUndef = -9.99e33;                                            // common.f90:28, :38

__global__ void __launch_bounds__(256) randn_pairs_kernel(const long npairs, const double* __restrict__ u, double* __restrict__ out,
                                                          const long nout) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < npairs; i += (long)gridDim.x * blockDim.x) {
    const double u1 = u[2 * i], u2 = u[2 * i + 1];
    const double r = sqrt(-2.0 * log(u1)), th = (2.0 * kPi) * u2;
    out[2 * i] = r * sin(th);
    if (2 * i + 1 < nout) out[2 * i + 1] = r * cos(th);
  }
}

__device__ inline bool in_slot(const letkf::ObsmakeRows& R, long n) { return R.dif[n] > R.lb && R.dif[n] <= R.ub; }   // :825

__global__ void __launch_bounds__(256) obsmake_count_kernel(const letkf::ObsmakeRows R, int* __restrict__ sel,
                                                            unsigned long long* __restrict__ nslot) {
  unsigned mine = 0;
  for (long n = (long)blockIdx.x * blockDim.x + threadIdx.x; n < R.n; n += (long)gridDim.x * blockDim.x) {
    const bool in = in_slot(R, n);
    sel[n] = (in && (!R.own || R.own[n] == 1)) ? 1 : 0;
    mine += in ? 1u : 0u;
  }
  // the rows in the slot: an integer sum, whatever its order
  for (int o = 32; o > 0; o >>= 1) mine += __shfl_down(mine, o);
  if ((threadIdx.x & 63) == 0 && mine) atomicAdd(nslot, (unsigned long long)mine);
}

__global__ void __launch_bounds__(256) obsmake_fill_kernel(const letkf::ObsmakeRows R, const int* __restrict__ sel,
                                                           const long* __restrict__ off, const double* __restrict__ rotc,
                                                           int* __restrict__ gset, int* __restrict__ gidx, int* __restrict__ qc,
                                                           double* __restrict__ grotc) {
  for (long n = (long)blockIdx.x * blockDim.x + threadIdx.x; n < R.n; n += (long)gridDim.x * blockDim.x) {
    if (!sel[n]) continue;
    int f = 0;
    while (f + 1 < R.nfile && n >= R.off[f + 1]) ++f;
    const long j = off[n];                                          // < R.n: the lists hold R.n rows
    gset[j] = f + 1;
    gidx[j] = (int)(n - R.off[f]) + 1;
    qc[j] = 0;
    if (rotc) grotc[2 * j] = rotc[2 * n], grotc[2 * j + 1] = rotc[2 * n + 1];
  }
}

__global__ void __launch_bounds__(256) obsmake_scatter_kernel(const letkf::ObsmakeRows R, const int* __restrict__ sel,
                                                              const long* __restrict__ off, const int* __restrict__ qc,
                                                              const double* __restrict__ val, const unsigned long long* __restrict__ nslot,
                                                              double* __restrict__ dat, long* __restrict__ counts) {
  for (long n = (long)blockIdx.x * blockDim.x + threadIdx.x; n < R.n; n += (long)gridDim.x * blockDim.x) {
    if (sel[n]) {
      const long j = off[n];
      dat[n] = qc[j] == 0 ? val[j] : kUndef;                        // :882-884
    } else if (R.outside_undef && R.own && R.own[n] == -1 && in_slot(R, n)) {
      dat[n] = kUndef;                                              // :835-837
    }
  }
  if (counts && blockIdx.x == 0 && threadIdx.x == 0) counts[0] = (long)*nslot, counts[1] = off[R.n];
}

__global__ void __launch_bounds__(256) obsmake_noise_kernel(const letkf_obsmake_err E, const long n, const int* __restrict__ elm,
                                                            const double* __restrict__ error, double* __restrict__ dat,
                                                            double* __restrict__ err) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const int e = elm[i];
    double s = err[i];
    bool set = true;
    if (e == kIdU) s = E.obserr_u;
    else if (e == kIdV) s = E.obserr_v;
    else if (e == kIdT || e == kIdTv) s = E.obserr_t;
    else if (e == kIdQ) s = E.obserr_q;
    else if (e == kIdRh) s = E.obserr_rh;
    else if (e == kIdPs) s = E.obserr_ps;
    else if (e == kIdRadarRef || e == kIdRadarRefZero) s = E.obserr_radar_ref;
    else if (e == kIdRadarVr) s = E.obserr_radar_vr;
    else set = false;
    if (set) err[i] = s;
    const double d = dat[i];
    if (d != kUndef && s != kUndef) dat[i] = d + s * error[i];      // :1039-1041
  }
}

unsigned grid1d(long tot) { return (unsigned)std::min<long>(std::max<long>((tot + 255) / 256, 1), 65536); }
size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

}  // namespace

namespace letkf {

static_assert(sizeof(long) == sizeof(int64_t), "the kernels index with long");

hipError_t randn_pairs(hipStream_t st, int64_t npairs, const double* u, double* out, int64_t nout) {
  if (npairs <= 0) return hipSuccess;
  hipLaunchKernelGGL(randn_pairs_kernel, dim3(grid1d(npairs)), dim3(256), 0, st, (long)npairs, u, out, (long)nout);
  return hipGetLastError();
}

size_t obsmake_ws_bytes(int64_t n) {
  const size_t m = (size_t)std::max<int64_t>(n, 1);
  return 512 + 3 * align256(m * sizeof(int32_t)) + 3 * align256(m * sizeof(double));
}

void obsmake_ws_layout(char* p, int64_t n, ObsmakeWs* w) {
  const size_t m = (size_t)std::max<int64_t>(n, 1), ai = align256(m * sizeof(int32_t)), ad = align256(m * sizeof(double));
  w->flag = reinterpret_cast<int32_t*>(p), p += 256;
  w->nslot = reinterpret_cast<unsigned long long*>(p), p += 256;
  w->val = reinterpret_cast<double*>(p), p += ad;
  w->rotc = reinterpret_cast<double*>(p), p += 2 * ad;
  w->set = reinterpret_cast<int32_t*>(p), p += ai;
  w->idx = reinterpret_cast<int32_t*>(p), p += ai;
  w->qc = reinterpret_cast<int32_t*>(p);
}

hipError_t obsmake_count(hipStream_t st, const ObsmakeRows& R, int32_t* sel, const ObsmakeWs& w) {
  hipError_t e = hipMemsetAsync(w.nslot, 0, sizeof(unsigned long long), st);
  if (e != hipSuccess || R.n <= 0) return e;
  hipLaunchKernelGGL(obsmake_count_kernel, dim3(grid1d(R.n)), dim3(256), 0, st, R, sel, w.nslot);
  return hipGetLastError();
}

hipError_t obsmake_fill(hipStream_t st, const ObsmakeRows& R, const int32_t* sel, const int64_t* off, const double* rotc,
                        const ObsmakeWs& w) {
  if (R.n <= 0) return hipSuccess;
  hipLaunchKernelGGL(obsmake_fill_kernel, dim3(grid1d(R.n)), dim3(256), 0, st, R, sel, reinterpret_cast<const long*>(off), rotc, w.set,
                     w.idx, w.qc, w.rotc);
  return hipGetLastError();
}

hipError_t obsmake_scatter(hipStream_t st, const ObsmakeRows& R, const int32_t* sel, const int64_t* off, const ObsmakeWs& w,
                           double* dat, int64_t* counts) {
  hipLaunchKernelGGL(obsmake_scatter_kernel, dim3(grid1d(R.n)), dim3(256), 0, st, R, sel, reinterpret_cast<const long*>(off), w.qc,
                     w.val, w.nslot, dat, reinterpret_cast<long*>(counts));
  return hipGetLastError();
}

hipError_t obsmake_noise(hipStream_t st, const letkf_obsmake_err* e, int64_t n, const int32_t* elm, const double* error, double* dat,
                         double* err) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(obsmake_noise_kernel, dim3(grid1d(n)), dim3(256), 0, st, *e, (long)n, elm, error, dat, err);
  return hipGetLastError();
}

}  // namespace letkf
