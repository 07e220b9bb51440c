// letkf_efso.hip -- ensemble forecast sensitivity to observations (EFSO) on the local-observation lists:
//   the loop of das_efso, scale/letkf/letkf_tools.f90:1158-1302 (commented out in the reference; ported from the
//   SPEEDY/GFS system of efso.f90), for SCALE's point layout p = ij + nij1*lev.
//
//   w_p(t, m)   = sum over v with term(v) = t of  fcst[p, m, v] * fcer[p, v]                    ("work1", :1221-1249)
//   djdy(t, j) += sum over p with j in L_p of  (rloc / rdiag)_{p,j} * sum_m ya[j, m] * w_p(t, m)    ("djdy", :1251-1264)
//   obsense(t, j) = djdy(t, j) * dep[j]                                                          (:1283-1290)
//
// Bitwise deterministic, no floating-point atomics.  Three steps per slab of list entries:
//   1. efso_pairs_kernel: one wave per point builds w_p in LDS (lane = member), then every lane takes one list entry,
//      reads its table row and writes the nterm contributions of the pair at the entry's slab index.
//   2. a stable radix sort of the entry indices by observation row (rocprim; stable, so the entries of one row stay in
//      ascending list order = ascending p), and the per-row counts (integer atomics) turned into row offsets by
//      count_scan.  Entries whose row lies outside [0, nobs) are keyed nobs, so they sort behind every row's window.
//   3. efso_reduce_kernel: one thread per observation row adds its contributions to djdy(:, j) one after the other in
//      ascending p.  Since every slab continues the same sequence of additions, the result does not depend on how the
//      points are cut into slabs.  Rows no entry reaches are not written.
#include <hip/hip_runtime.h>
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/iterator/counting_iterator.hpp>

#include "letkf_device.h"

namespace letkf {

namespace {

constexpr int kEfsoWaves = 4;   // waves per workgroup of the pair kernel (each its own points, its own w_p slice of LDS)

// Pass 1.  Points p0 + wave, p0 + wave + nwave, ... of the slab; entry e of point p is list entry obs_off[p] + i and
// goes to contribution slot (e - e_base) * NT + t.  Entries outside [e_base, e_end) are skipped (memory safety against a
// malformed obs_off); rows outside [0, nobs) contribute 0.
template <int NT>
__global__ void __launch_bounds__(64 * kEfsoWaves) efso_pairs_kernel(EfsoArgs a, long npts, long e_base, long e_end,
                                                                      double* __restrict__ contrib) {
  extern __shared__ double lds_w[];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int k = a.k;
  double* w = lds_w + (size_t)wv * NT * k;          // w[t * k + m]
  const long nwave = (long)gridDim.x * kEfsoWaves;
  for (long p = (long)blockIdx.x * kEfsoWaves + wv; p < npts; p += nwave) {
    long o0 = a.obs_off[p], o1 = a.obs_off[p + 1];
    o0 = o0 < e_base ? e_base : o0;
    o1 = o1 > e_end ? e_end : o1;
    if (o1 <= o0) continue;                         // (wave-uniform)
    // w_p: lane = member, variables in ascending order
    const double* fc = a.fcst + p * a.sp;
    const double* fe = a.fcer + p * a.fsp;
    for (int m = lane; m < k; m += 64) {
      double acc[NT];
#pragma unroll
      for (int t = 0; t < NT; ++t) acc[t] = 0.0;
      for (int v = 0; v < a.nv; ++v) {
        const int tv = a.term[v];                   // (-1: not in this class / no term)
        if (tv < 0) continue;
        const double x = fc[m * a.sm + v * a.sv] * fe[v * a.fsv];
#pragma unroll
        for (int t = 0; t < NT; ++t)
          if (t == tv) acc[t] += x;
      }
#pragma unroll
      for (int t = 0; t < NT; ++t) w[t * k + m] = acc[t];
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    // the list: one entry per lane; w is read as an LDS broadcast
    for (long e = o0 + lane; e < o1; e += 64) {
      const int j = a.obs_idx[e];
      double s[NT];
#pragma unroll
      for (int t = 0; t < NT; ++t) s[t] = 0.0;
      double coef = 0.0;
      if ((unsigned long)(long)j < (unsigned long)a.nobs) {
        const double* row = a.ensval + (long)j * a.kld;
        int m = 0;
        for (; m + 4 <= k; m += 4) {
          const double y0 = row[m], y1 = row[m + 1], y2 = row[m + 2], y3 = row[m + 3];
#pragma unroll
          for (int t = 0; t < NT; ++t) {
            s[t] = fma(y0, w[t * k + m], s[t]);
            s[t] = fma(y1, w[t * k + m + 1], s[t]);
            s[t] = fma(y2, w[t * k + m + 2], s[t]);
            s[t] = fma(y3, w[t * k + m + 3], s[t]);
          }
        }
        for (; m < k; ++m) {
          const double y = row[m];
#pragma unroll
          for (int t = 0; t < NT; ++t) s[t] = fma(y, w[t * k + m], s[t]);
        }
        coef = a.rloc_l[e] / a.rdiag_l[e];
      }
      double* out = contrib + (e - e_base) * NT;
#pragma unroll
      for (int t = 0; t < NT; ++t) out[t] = coef * s[t];
    }
    // (w is rewritten for the next point only after every lane has read it)
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  }
}

// Sort keys and per-row counts of the slab's entries.  A row outside [0, nobs) gets the key nobs: it sorts behind every
// real row, past start[nobs], where no row's window reaches it.
__global__ void efso_key_kernel(const int* __restrict__ idx, long n, long nobs, int* __restrict__ cnt,
                                unsigned* __restrict__ keys) {
  for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (long)gridDim.x * blockDim.x) {
    const int j = idx[e];
    const bool live = (unsigned long)(long)j < (unsigned long)nobs;
    keys[e] = live ? (unsigned)j : (unsigned)nobs;
    if (live) atomicAdd(cnt + j, 1);
  }
}

// Pass 3.  Row j's entries are perm[start[j] .. start[j+1]) in ascending list order.
template <int NT>
__global__ void efso_reduce_kernel(long nobs, const long* __restrict__ start, const unsigned* __restrict__ perm,
                                   const double* __restrict__ contrib, double* __restrict__ djdy) {
  const long j = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= nobs) return;
  const long q0 = start[j], q1 = start[j + 1];
  if (q1 <= q0) return;
  double acc[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) acc[t] = djdy[j * NT + t];
  for (long q = q0; q < q1; ++q) {
    const double* c = contrib + (long)perm[q] * NT;
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[t] += c[t];
  }
#pragma unroll
  for (int t = 0; t < NT; ++t) djdy[j * NT + t] = acc[t];
}

__global__ void efso_obsense_kernel(int nterm, long nobs, const double* __restrict__ djdy, const double* __restrict__ dep,
                                    double* __restrict__ obsense) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < nobs * nterm) obsense[i] = djdy[i] * dep[i / nterm];
}

// bits that hold the keys 0 .. nobs (nobs: the key of a row outside the table)
int key_bits(long nobs) {
  int b = 1;
  while (b < 31 && (1L << b) <= nobs) ++b;
  return b;
}

hipError_t sort_entries(void* temp, size_t* temp_bytes, const unsigned* keys, unsigned* keys_out, unsigned* perm, size_t n,
                        long nobs, hipStream_t st) {
  return rocprim::radix_sort_pairs(temp, *temp_bytes, keys, keys_out, rocprim::counting_iterator<unsigned>(0u), perm, n, 0u,
                                   (unsigned)key_bits(nobs), st);
}

}  // namespace

size_t efso_pair_lds(int k, int nterm) { return (size_t)kEfsoWaves * nterm * k * sizeof(double); }

// Workspace of a slab of up to n entries over nobs rows: contrib [n][nterm] | keys [n] | keys_out [n] | perm [n] | cnt [nobs+1] |
// start [nobs+1] | sort scratch | scan scratch, every part 256-byte aligned.
hipError_t efso_ws_layout(long n, long nobs, int nterm, hipStream_t st, EfsoWs* ws) {
  auto al = [](size_t b) { return (b + 255) & ~(size_t)255; };
  const size_t n1 = (size_t)(n > 0 ? n : 1);
  ws->o_contrib = 0;
  ws->o_keys_in = ws->o_contrib + al(n1 * nterm * 8);
  ws->o_keys = ws->o_keys_in + al(n1 * 4);
  ws->o_perm = ws->o_keys + al(n1 * 4);
  ws->o_cnt = ws->o_perm + al(n1 * 4);
  ws->o_start = ws->o_cnt + al((size_t)(nobs + 1) * 4);
  ws->o_sort = ws->o_start + al((size_t)(nobs + 1) * 8);
  ws->sort_bytes = 0;
  hipError_t e = sort_entries(nullptr, &ws->sort_bytes, nullptr, nullptr, nullptr, n1, nobs, st);
  if (e != hipSuccess) return e;
  ws->o_scan = ws->o_sort + al(ws->sort_bytes);
  ws->scan_bytes = 0;
  e = count_scan(nullptr, &ws->scan_bytes, nullptr, nullptr, (size_t)nobs + 1, st);
  if (e != hipSuccess) return e;
  ws->total = ws->o_scan + al(ws->scan_bytes) + 256;
  return hipSuccess;
}

// One slab: the points [0, npts) of a (list offsets already shifted to the slab's points), their entries
// [e_base, e_end) of the list arrays; ws laid out by efso_ws_layout for at least e_end - e_base entries.
hipError_t efso_slab(const EfsoArgs& a, long npts, long e_base, long e_end, char* base, const EfsoWs& ws, int num_cu,
                     hipStream_t st) {
  const long n = e_end - e_base;
  if (npts <= 0 || n <= 0) return hipSuccess;
  double* contrib = reinterpret_cast<double*>(base + ws.o_contrib);
  unsigned* keys = reinterpret_cast<unsigned*>(base + ws.o_keys_in);
  unsigned* keys_out = reinterpret_cast<unsigned*>(base + ws.o_keys);
  unsigned* perm = reinterpret_cast<unsigned*>(base + ws.o_perm);
  int* cnt = reinterpret_cast<int*>(base + ws.o_cnt);
  long* start = reinterpret_cast<long*>(base + ws.o_start);
  // 1. contributions of every pair
  const size_t lds = efso_pair_lds(a.k, a.nterm);
  const long nwg_need = (npts + kEfsoWaves - 1) / kEfsoWaves;
  const long nwg = nwg_need < (long)num_cu * 16 ? nwg_need : (long)num_cu * 16;
  hipError_t e = hipSuccess;
  switch (a.nterm) {
#define EFSO_PAIRS(NT)                                                                                                   \
  case NT:                                                                                                               \
    e = lds_opt_in(efso_pairs_kernel<NT>, lds);                                                                          \
    if (e != hipSuccess) return e;                                                                                       \
    hipLaunchKernelGGL(efso_pairs_kernel<NT>, dim3((unsigned)nwg), dim3(64 * kEfsoWaves), lds, st, a, npts, e_base, e_end, \
                       contrib);                                                                                         \
    break;
    EFSO_PAIRS(1)
    EFSO_PAIRS(2)
    EFSO_PAIRS(3)
    EFSO_PAIRS(4)
#undef EFSO_PAIRS
    default: return hipErrorInvalidValue;
  }
  if ((e = hipGetLastError()) != hipSuccess) return e;
  // 2. rows of the entries: counts -> offsets, and the entries in (row, list order) order
  if ((e = hipMemsetAsync(cnt, 0, (size_t)(a.nobs + 1) * 4, st)) != hipSuccess) return e;
  const long nb = (n + 255) / 256;
  hipLaunchKernelGGL(efso_key_kernel, dim3((unsigned)(nb < (long)num_cu * 32 ? nb : (long)num_cu * 32)), dim3(256), 0, st,
                     a.obs_idx + e_base, n, a.nobs, cnt, keys);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  size_t scan_b = ws.scan_bytes;
  if ((e = count_scan(base + ws.o_scan, &scan_b, cnt, start, (size_t)a.nobs + 1, st)) != hipSuccess) return e;
  size_t sort_b = ws.sort_bytes;
  if ((e = sort_entries(base + ws.o_sort, &sort_b, keys, keys_out, perm, (size_t)n, a.nobs, st)) != hipSuccess)
    return e;
  // 3. per row, in ascending p
  const unsigned nr = (unsigned)((a.nobs + 255) / 256);
  switch (a.nterm) {
    case 1: hipLaunchKernelGGL(efso_reduce_kernel<1>, dim3(nr), dim3(256), 0, st, a.nobs, start, perm, contrib, a.djdy); break;
    case 2: hipLaunchKernelGGL(efso_reduce_kernel<2>, dim3(nr), dim3(256), 0, st, a.nobs, start, perm, contrib, a.djdy); break;
    case 3: hipLaunchKernelGGL(efso_reduce_kernel<3>, dim3(nr), dim3(256), 0, st, a.nobs, start, perm, contrib, a.djdy); break;
    default: hipLaunchKernelGGL(efso_reduce_kernel<4>, dim3(nr), dim3(256), 0, st, a.nobs, start, perm, contrib, a.djdy); break;
  }
  return hipGetLastError();
}

hipError_t launch_efso_obsense(int nterm, long nobs, const double* djdy, const double* dep, double* obsense, hipStream_t st) {
  const long n = nobs * nterm;
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(efso_obsense_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, nterm, nobs, djdy, dep, obsense);
  return hipGetLastError();
}

const char* efso_path_name(int nterm) {
  switch (nterm) {
    case 1: return "efso_pairs_kernel<1> + rocprim radix_sort_pairs + efso_reduce_kernel<1>";
    case 2: return "efso_pairs_kernel<2> + rocprim radix_sort_pairs + efso_reduce_kernel<2>";
    case 3: return "efso_pairs_kernel<3> + rocprim radix_sort_pairs + efso_reduce_kernel<3>";
    default: return "efso_pairs_kernel<4> + rocprim radix_sort_pairs + efso_reduce_kernel<4>";
  }
}

}  // namespace letkf
