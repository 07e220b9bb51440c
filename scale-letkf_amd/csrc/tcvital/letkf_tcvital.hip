// letkf_tcvital.hip -- the kernels of the TC vitals (include/letkf_amd_tcvital.h): search_tc_subdom + wgt_ave2d
// (scale/common/common_obs_scale.f90:2686-2768) for every member of a subdomain, the scan for the three rows of a file
// (scale/obs/obsope_tools.f90:154-204) and the pick among the ranks with the three obsda rows (:678-703).  Compiled without
// floating-point contraction (Makefile): the disc test, the smoothing and the position round term by term.

#include "letkf_tcvital_dev.h"
#include "letkf_obsope_point_dev.h"

namespace letkf {

namespace {

using obsope_point_dev::kGg;
using obsope_point_dev::kRd;
using obsope_point_dev::kUndef;
using obsope_point_dev::V2_PS;
using obsope_point_dev::V2_Q2M;
using obsope_point_dev::V2_T2M;
using obsope_point_dev::V2_TOPO;

constexpr int kBlock = kTcTileI * kTcTileJ;   // 256 threads: four waves, each two rows of the tile
constexpr int kWaves = kBlock / 64;
constexpr int kRim = 2;                       // of the 5 x 5 stencil
constexpr double kNone = 9.99e33;             // the reference's "nothing found", and the bound a winner stays below
constexpr double kCap = 1100.0e2;             // obsope_tools.f90:679
constexpr int kNoIndex = 0x7fffffff;

// the key of the arg-min: the lowest s, then the lowest j, then the lowest i -- the reference's loop order under its strict <
struct Key {
  double s;
  int j, i;
};

__device__ inline bool better(const Key& a, const Key& b) {
  return a.s < b.s || (a.s == b.s && (a.j < b.j || (a.j == b.j && a.i < b.i)));
}

__device__ inline Key wave_min(Key k) {
  for (int off = 32; off > 0; off >>= 1) {
    Key o;
    o.s = __shfl_down(k.s, off, 64);
    o.j = __shfl_down(k.j, off, 64);
    o.i = __shfl_down(k.i, off, 64);
    if (better(o, k)) k = o;
  }
  return k;   // (lane 0's is the wave's)
}

// |g - c| * d for both axes and the root of the squares, as the reference writes them
__device__ inline double disc_distance(double gi, double gj, double ritc, double rjtc, double dx, double dy) {
  const double xdis = fabs(gi - ritc) * dx, ydis = fabs(gj - rjtc) * dy;
  return sqrt(xdis * xdis + ydis * ydis);
}

// One workgroup: a tile of kTcTileI x kTcTileJ interior cells of one member.  slp of the tile and its rim goes into LDS once (one
// pow per array cell of the block), s is formed from LDS, and the block's key is reduced by wave shuffles and across its four waves.
__global__ void __launch_bounds__(kBlock) tc_search_tile_kernel(const TcSearchArgs A) {
  __shared__ double s_slp[(kTcTileJ + 2 * kRim) * (kTcTileI + 2 * kRim)];
  __shared__ double s_ws[kWaves];
  __shared__ int s_wj[kWaves], s_wi[kWaves];
  const int tid = threadIdx.x;
  const int ntile = A.tiles_i * A.tiles_j;
  const int m = blockIdx.x / ntile, tile = blockIdx.x - m * ntile;
  const int tj = tile / A.tiles_i, ti = tile - tj * A.tiles_i;
  const int i0 = ti * kTcTileI, j0 = tj * kTcTileJ;                               // the tile's first interior cell, 0-based
  const int i1 = min(i0 + kTcTileI, A.nlon), j1 = min(j0 + kTcTileJ, A.nlat);     // ... and one past its last
  const double ritc = *A.ritc, rjtc = *A.rjtc, kinf = kNone;
  const int64_t pidx = (int64_t)m * ntile + tile;

  // The tile against the disc: the point of the tile's rectangle nearest the centre is no farther than any of its cells, and every
  // operation of the distance is monotone, so a rectangle outside the disc has no cell inside it.
  {
    const double ci = fmin(fmax(ritc, (double)(i0 + 1 + A.i_off)), (double)(i1 + A.i_off));
    const double cj = fmin(fmax(rjtc, (double)(j0 + 1 + A.j_off)), (double)(j1 + A.j_off));
    const bool nan_centre = ritc != ritc || rjtc != rjtc;
    if (nan_centre || disc_distance(ci, cj, ritc, rjtc, A.dx, A.dy) > A.dis) {
      if (tid == 0) {
        A.part_s[pidx] = kinf;
        A.part_ij[2 * pidx] = kNoIndex;
        A.part_ij[2 * pidx + 1] = kNoIndex;
      }
      return;
    }
  }

  const bool smooth = A.ihalo >= kRim && A.jhalo >= kRim;
  const int rim = smooth ? kRim : 0;
  const int w = kTcTileI + 2 * rim, h = kTcTileJ + 2 * rim;
  const int nlonh = A.nlon + 2 * A.ihalo, nlath = A.nlat + 2 * A.jhalo;
  const double* vm = A.v2d + (int64_t)m * A.s2m;
  for (int e = tid; e < w * h; e += kBlock) {
    const int lj = e / w, li = e - lj * w;
    const int ai = i0 + li - rim + A.ihalo, aj = j0 + lj - rim + A.jhalo;         // 0-based array element (>= 0: the halo holds the rim)
    double p = 0.0;
    if (ai < nlonh && aj < nlath) {                                               // (beyond: only cells outside the interior read it)
      const double* c = vm + (int64_t)ai * A.s2i + (int64_t)aj * A.s2j;
      p = c[V2_PS * A.s2v];
      const double dz = -1.0 * c[V2_TOPO * A.s2v];
      if (dz != 0.0) {                                                            // prsadj, common_obs_scale.f90:600-616
        const double gamma = 5.0e-3, tv = c[V2_T2M * A.s2v] * (1.0 + 0.608 * c[V2_Q2M * A.s2v]);
        p = p * pow((-gamma * dz + tv) / tv, kGg / (gamma * kRd));
      }
    }
    s_slp[e] = p;
  }
  __syncthreads();

  const int li = tid & (kTcTileI - 1), lj = tid / kTcTileI;
  const int i = i0 + li, j = j0 + lj;
  Key k = {kinf, kNoIndex, kNoIndex};
  if (i < A.nlon && j < A.nlat) {
    const int ig = i + 1 + A.i_off, jg = j + 1 + A.j_off;
    const double* c = s_slp + (lj + rim) * w + (li + rim);
    double s = c[0];
    if (smooth) {                                                                 // wgt_ave2d
      double s3 = 0.0, s5 = 0.0;
#pragma unroll
      for (int dj = -1; dj <= 1; ++dj)
#pragma unroll
        for (int di = -1; di <= 1; ++di) s3 = (dj == -1 && di == -1) ? c[dj * w + di] : s3 + c[dj * w + di];
#pragma unroll
      for (int dj = -2; dj <= 2; ++dj)
#pragma unroll
        for (int di = -2; di <= 2; ++di) s5 = (dj == -2 && di == -2) ? c[dj * w + di] : s5 + c[dj * w + di];
      s = (c[0] * 5.0 + (s3 - c[0]) * 3.0 + (s5 - s3)) / 45.0;
    }
    const bool out = disc_distance((double)ig, (double)jg, ritc, rjtc, A.dx, A.dy) > A.dis;
    if (!out && s < kinf) k = Key{s, jg, ig};
  }
  k = wave_min(k);
  if ((tid & 63) == 0) {
    s_ws[tid >> 6] = k.s;
    s_wj[tid >> 6] = k.j;
    s_wi[tid >> 6] = k.i;
  }
  __syncthreads();
  if (tid == 0) {
    for (int q = 1; q < kWaves; ++q) {
      const Key o = {s_ws[q], s_wj[q], s_wi[q]};
      if (better(o, k)) k = o;
    }
    A.part_s[pidx] = k.s;
    A.part_ij[2 * pidx] = k.i;
    A.part_ij[2 * pidx + 1] = k.j;
  }
}

// One wave per member: the tiles' partials in a fixed order, then cand
__global__ void __launch_bounds__(64) tc_search_pick_kernel(const TcSearchArgs A) {
  const int m = blockIdx.x, lane = threadIdx.x;
  const int ntile = A.tiles_i * A.tiles_j;
  Key k = {kNone, kNoIndex, kNoIndex};
  for (int t = lane; t < ntile; t += 64) {
    const int64_t pidx = (int64_t)m * ntile + t;
    const Key o = {A.part_s[pidx], A.part_ij[2 * pidx + 1], A.part_ij[2 * pidx]};
    if (better(o, k)) k = o;
  }
  k = wave_min(k);
  if (lane == 0) {
    double* out = A.cand + (int64_t)m * 3;
    if (k.s < kNone) {
      out[0] = ((double)k.i - 1.0) * A.dx + A.cxg1;
      out[1] = ((double)k.j - 1.0) * A.dy + A.cyg1;
      out[2] = k.s;
    } else {
      out[0] = out[1] = out[2] = kNone;
    }
  }
}

__device__ inline long long wave_max(long long v) {
  for (int off = 32; off > 0; off >>= 1) {
    const long long o = __shfl_down(v, off, 64);
    v = o > v ? o : v;
  }
  return v;
}

// the last 1-based row of each of the three ids among the rows a block strides over: part [gridDim.x][3]
__global__ void __launch_bounds__(kTcRowsBlock) tc_rows_scan_kernel(const int64_t n, const int32_t* elm, int64_t* part) {
  __shared__ long long s_w[kTcRowsBlock / 64][3];
  long long last[3] = {0, 0, 0};
  for (int64_t r = (int64_t)blockIdx.x * kTcRowsBlock + threadIdx.x; r < n; r += (int64_t)gridDim.x * kTcRowsBlock) {
    const int e = elm[r];
    if (e == LETKF_TCVITAL_ID_TCX) last[0] = r + 1;        // (r grows along a thread's walk: the last assignment is its maximum)
    if (e == LETKF_TCVITAL_ID_TCY) last[1] = r + 1;
    if (e == LETKF_TCVITAL_ID_TCP) last[2] = r + 1;
  }
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    const long long v = wave_max(last[q]);
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6][q] = v;
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    long long v = s_w[0][threadIdx.x];
    for (int wv = 1; wv < kTcRowsBlock / 64; ++wv) v = s_w[wv][threadIdx.x] > v ? s_w[wv][threadIdx.x] : v;
    part[(int64_t)blockIdx.x * 3 + threadIdx.x] = v;
  }
}

// one wave: the blocks' partials, then the three rows and their dif
__global__ void __launch_bounds__(64) tc_rows_pick_kernel(const int nblock, const int64_t* part, const double* dif, int64_t* out6) {
  double* out_dif = reinterpret_cast<double*>(out6 + 3);
  for (int q = 0; q < 3; ++q) {
    long long v = 0;
    for (int b = threadIdx.x; b < nblock; b += 64) v = part[(int64_t)b * 3 + q] > v ? part[(int64_t)b * 3 + q] : v;
    v = wave_max(v);
    if (threadIdx.x == 0) {
      out6[q] = v;
      out_dif[q] = v > 0 ? dif[v - 1] : 0.0;
    }
  }
}

// the pick among the ranks for every member and the three obsda rows: member m's three values have one writer, thread m mod 256;
// the rows' qc has one each, after the block knows whether any member found no rank
__global__ void __launch_bounds__(256) tc_fill_kernel(const int nproc, const int nmem, const int m0, const double* cand_all, const int64_t r0,
                                                      const int64_t r1, const int64_t r2, const int qc_replace, int32_t* qc, double* ensval,
                                                      const int64_t kld) {
  const int64_t row[3] = {r0, r1, r2};
  int none = 0;
  for (int m = threadIdx.x; m < nmem; m += 256) {
    double best = kCap;
    int pick = -1;
    for (int n = 0; n < nproc; ++n) {
      const double v = cand_all[((int64_t)n * nmem + m) * 3 + 2];
      if (v < best) {
        best = v;
        pick = n;
      }
    }
    if (pick < 0) none = 1;
#pragma unroll
    for (int c = 0; c < 3; ++c)
      if (row[c] >= 0) ensval[row[c] * kld + m0 + m] = pick >= 0 ? cand_all[((int64_t)pick * nmem + m) * 3 + c] : kUndef;
  }
  none = __syncthreads_or(none);
  if (threadIdx.x < 3) {
    const int64_t r = threadIdx.x == 0 ? r0 : (threadIdx.x == 1 ? r1 : r2);
    if (r >= 0) {
      const int t = none ? LETKF_TCVITAL_QC_BAD : 0;
      qc[r] = qc_replace ? t : max(qc[r], t);
    }
  }
}

}  // namespace

size_t tc_search_part_s_bytes(const TcSearchArgs& a) {
  const size_t n = (size_t)a.nmem * a.tiles_i * a.tiles_j;
  return (n * sizeof(double) + 255) & ~(size_t)255;
}

size_t tc_search_ws_bytes(const TcSearchArgs& a) {
  return tc_search_part_s_bytes(a) + (size_t)a.nmem * a.tiles_i * a.tiles_j * 2 * sizeof(int32_t);
}

hipError_t launch_tc_search(const TcSearchArgs& a, hipStream_t st) {
  const unsigned nblock = (unsigned)a.nmem * (unsigned)(a.tiles_i * a.tiles_j);
  hipLaunchKernelGGL(tc_search_tile_kernel, dim3(nblock), dim3(kBlock), 0, st, a);
  if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
  hipLaunchKernelGGL(tc_search_pick_kernel, dim3((unsigned)a.nmem), dim3(64), 0, st, a);
  return hipGetLastError();
}

int tc_rows_blocks(int64_t n) {
  const int64_t b = (n + kTcRowsBlock - 1) / kTcRowsBlock;
  return (int)(b < 1 ? 1 : (b > kTcRowsMaxBlocks ? kTcRowsMaxBlocks : b));
}

hipError_t launch_tc_rows(int64_t n, const int32_t* elm, const double* dif, int64_t* part, int64_t* out6, hipStream_t st) {
  const int nblock = tc_rows_blocks(n);
  hipLaunchKernelGGL(tc_rows_scan_kernel, dim3(nblock), dim3(kTcRowsBlock), 0, st, n, elm, part);
  if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
  hipLaunchKernelGGL(tc_rows_pick_kernel, dim3(1), dim3(64), 0, st, nblock, part, dif, out6);
  return hipGetLastError();
}

hipError_t launch_tc_fill(int nproc, int nmem, int m0, const double* cand_all, int64_t r0, int64_t r1, int64_t r2, int qc_replace,
                          int32_t* qc, double* ensval, int64_t kld, hipStream_t st) {
  hipLaunchKernelGGL(tc_fill_kernel, dim3(1), dim3(256), 0, st, nproc, nmem, m0, cand_all, r0, r1, r2, qc_replace, qc, ensval, kld);
  return hipGetLastError();
}

}  // namespace letkf
