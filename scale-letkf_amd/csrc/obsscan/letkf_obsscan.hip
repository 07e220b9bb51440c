// letkf_obsscan.hip -- obsope_cal's first scan (scale/obs/obsope_tools.f90:140-427) on the device, three steps over nobs-sized
// buffers:
//   obsscan_key_kernel   a lane per file row: rij_rank (common_scale.f90:1728-1779) and the slot of :256 in the reference's double
//                        arithmetic, the optional rank / slot / own, and the key ip * (nslots + 2) + bucket with the flat row as its
//                        value; rows of files that do not run get the key behind all buckets (24 B read, 8 B written per row)
//   rocprim radix sort   stable, over bit_length(buckets) bits: inside a bucket the flat rows ascend, which is file order, then
//                        row order -- the order the serial scatter loop of :279-298 leaves
//   obsscan_fill_kernel  a lane per sorted position: the file from off (at most 16), set / idx / qc; a lane per bucket: the upper
//                        bound of its key in the sorted keys, which is bsna
// No counter is shared: one subdomain with one slot, which puts every row into one bucket, costs what any other layout costs.
// Built with -ffp-contract=off: (ig - IHALO - 0.5) / nlon and dif / T - 0.5 round operation by operation.
#include <hip/hip_runtime.h>

#include <rocprim/device/device_radix_sort.hpp>

#include "letkf_obsscan_dev.h"

namespace letkf {
namespace {

constexpr int kBlock = 256;

struct Ws {
  uint32_t *kA, *kB, *vA, *vB;
  int32_t* ub;
  char* temp;
  size_t temp_bytes, total;
};

// The file of flat row r and that file's first row.  off is non-decreasing and INT64_MAX behind the last file, so the files
// whose first row r has reached are a prefix; every index is a constant (the table stays in scalar registers, no scratch).
__device__ inline int file_of(const ObsscanArgs& a, int64_t r, int64_t* first) {
  int f = 0;
  int64_t base = 0;
#pragma unroll
  for (int q = 1; q < LETKF_OBSOPE_MAX_FILES; ++q)
    if (r >= a.off[q]) f = q, base = a.off[q];
  *first = base;
  return f;
}

// rij_rank on one axis: -1 outside [1 + halo, n * prc + halo] (a NaN is outside), else ceiling((g - halo - 0.5) / n) - 1
__device__ inline int axis_rank(double g, int halo, int n, int prc) {
  const double lo = (double)(1 + halo), hi = (double)(n * prc + halo);
  if (!(g >= lo) || !(g <= hi)) return -1;
  return (int)ceil((g - (double)halo - 0.5) / (double)n) - 1;
}

__global__ void __launch_bounds__(kBlock) obsscan_key_kernel(ObsscanArgs a, Ws w) {
  const int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (r >= a.n) return;
  int64_t first;
  const int f = file_of(a, r, &first);
  const int ri = axis_rank(a.ri[r], a.ihalo, a.nlon, a.px);
  const int rj = axis_rank(a.rj[r], a.jhalo, a.nlat, a.py);
  const int rank = ri < 0 || rj < 0 ? -1 : rj * a.px + ri;
  int slot = a.slot_end + 2;                                                // outside the domain
  if (rank >= 0) {
    const double x = a.dif[r] / a.tint - 0.5;
    slot = a.slot_end + 1;                                                  // outside the window
    if (fabs(x) < 1073741824.0) {                                           // (a NaN or an infinity is not)
      const int64_t s = (int64_t)ceil(x) + a.slot_base;
      if (s >= a.slot_start && s <= a.slot_end) slot = (int)s;
    }
  }
  if (a.rank) a.rank[r] = rank;
  if (a.slot) a.slot[r] = slot;
  if (a.own) a.own[r] = rank < 0 ? -1 : rank == a.myrank_d ? 1 : 0;
  const bool runs = (a.run_mask >> f) & 1u;
  w.kA[r] = runs ? (uint32_t)((rank < 0 ? 0 : rank) * a.nb + (slot - a.slot_start)) : (uint32_t)a.nbucket;
  w.vA[r] = (uint32_t)r;
}

__global__ void __launch_bounds__(kBlock) obsscan_fill_kernel(ObsscanArgs a, Ws w) {
  const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (t < a.nlist) {
    const int64_t r = w.vB[t];
    int64_t first;
    const int f = file_of(a, r, &first);
    const int bucket = (int)(w.kB[t] % (uint32_t)a.nb);
    a.set[t] = f + 1;
    a.idx[t] = (int32_t)(r - first + 1);
    a.qc[t] = bucket < a.nb - 2 ? 0 : bucket == a.nb - 2 ? LETKF_OBSSCAN_QC_TIME : LETKF_OBSSCAN_QC_OUT_H;
  }
  if (t < a.nbucket) {                                  // the first sorted position whose key is above bucket t
    const uint32_t key = (uint32_t)t;
    int64_t lo = 0, hi = a.nlist;
    while (lo < hi) {
      const int64_t mid = lo + (hi - lo) / 2;
      if (w.kB[mid] <= key) lo = mid + 1;
      else hi = mid;
    }
    w.ub[t] = (int32_t)lo;
  }
}

int bit_length(uint32_t v) {
  int b = 0;
  while (v) ++b, v >>= 1;
  return b > 0 ? b : 1;
}

// the workspace of a call, carved from base (nullptr: only the size)
hipError_t carve(const ObsscanArgs& a, hipStream_t st, char* base, Ws* w) {
  const size_t n = (size_t)(a.n > 0 ? a.n : 1);
  size_t off = 0;
  auto take = [&](size_t bytes) {
    char* p = base + off;
    off += (bytes + 255) & ~(size_t)255;
    return p;
  };
  uint32_t** u4[4] = {&w->kA, &w->kB, &w->vA, &w->vB};
  for (auto f : u4) *f = reinterpret_cast<uint32_t*>(take(n * 4));
  w->ub = reinterpret_cast<int32_t*>(take((size_t)a.nbucket * 4));
  size_t t = 0;
  const hipError_t e = rocprim::radix_sort_pairs(nullptr, t, (const uint32_t*)nullptr, (uint32_t*)nullptr, (const uint32_t*)nullptr,
                                                 (uint32_t*)nullptr, n, 0u, (unsigned)bit_length((uint32_t)a.nbucket), st);
  if (e != hipSuccess) return e;
  w->temp_bytes = t;
  w->temp = take(t);
  w->total = off + 256;
  return hipSuccess;
}

}  // namespace

size_t obsscan_ws_bytes(const ObsscanArgs& a, hipStream_t st) {
  Ws w = {};
  return carve(a, st, nullptr, &w) == hipSuccess ? w.total : 0;
}

hipError_t obsscan_run(hipStream_t st, const ObsscanArgs& a, void* ws, int32_t* ub_host) {
  Ws w = {};
  hipError_t e = carve(a, st, static_cast<char*>(ws), &w);
  if (e != hipSuccess) return e;
  const dim3 block(kBlock);
  if (a.n > 0) {
    hipLaunchKernelGGL(obsscan_key_kernel, dim3((unsigned)((a.n + kBlock - 1) / kBlock)), block, 0, st, a, w);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  if (a.nlist > 0) {                                     // (without list rows every upper bound is 0: the entry's tables start so)
    size_t bytes = w.temp_bytes;
    e = rocprim::radix_sort_pairs(w.temp, bytes, w.kA, w.kB, w.vA, w.vB, (size_t)a.n, 0u, (unsigned)bit_length((uint32_t)a.nbucket), st);
    if (e != hipSuccess) return e;
    const int64_t lanes = a.nlist > a.nbucket ? a.nlist : a.nbucket;
    hipLaunchKernelGGL(obsscan_fill_kernel, dim3((unsigned)((lanes + kBlock - 1) / kBlock)), block, 0, st, a, w);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if ((e = hipMemcpyAsync(ub_host, w.ub, (size_t)a.nbucket * 4, hipMemcpyDeviceToHost, st)) != hipSuccess) return e;
  }
  return hipSuccess;
}

}  // namespace letkf
