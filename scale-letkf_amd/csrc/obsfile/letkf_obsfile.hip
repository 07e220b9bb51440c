// letkf_obsfile.hip -- the record codec on the device (include/letkf_amd_obsfile.h).  A record is W = nrec + 2 dwords: marker,
// wk(1:nrec), marker.
//   decode_kernel / encode_kernel / obsda_encode_kernel / obsdep_encode_kernel
//       256 rows per block, a lane per row.  The block's records pass through LDS so that the image is read and written with
//       coalesced dword accesses (lane l touches dword l, l + 256, ..), while a lane reads or writes its own record at a pitch of
//       W | 1 dwords, an odd number: no bank conflict.  Without `missing` the encoder is a stable compaction: encode_count_kernel
//       counts a block's survivors, the main library's scan turns the counts into block offsets, and inside the block a row's
//       place is its rank among the survivors (ballot + popcount); no shared counter.
//   assemble_kernel
//       the hot path: nmem obsda images into the member-fastest ensval table.  A block owns 64 rows and walks the images 16 at a
//       time.  Load: wave w takes images w, w + 4, ..; its lanes read the 64 records of one image as W coalesced dwords each
//       (the records of a member are contiguous).  The tile lies in LDS as [image][row][W | 1] + 2 dwords per image: a half
//       wave then reads 16 images x 2 rows on 32 distinct banks.  Lanes (image fastest) write ensval as 128-byte row segments,
//       and the same pass takes the qc max, the set / idx comparison and the marker check from the tile, per lane; the 16 lanes
//       of a row meet once, after the last image (shuffles).
//       Every output has one writer; lev / val2 (nrec 6) are summed sequentially in image order by value.
//   count_total_kernel   per-block int32 counts to int64 totals, one block
// Built with -ffp-contract=off (the projection's point functions) and without fast-math; float32 denormals are kept (hipcc's
// default for gfx950).
#include <hip/hip_runtime.h>

#include <climits>

#include "letkf_obsfile_dev.h"
#include "mapproj/letkf_mapproj_point.h"

namespace letkf {
namespace obsfile {
namespace {

constexpr int kBlock = 256;
static_assert(kBlock == kBlockRows && kBlock == 4 * kTileRows && kTileMembers == 16 && kTileRows == 64, "the lane maps below");
constexpr double kUndef = -9.99e33;               // common/common.f90:38
constexpr float kTiny = 1.17549435e-38f;          // tiny(1.0_r_sngl)

enum : int32_t {                                  // common_obs_scale.f90:48-61
  kIdU = 2819, kIdV = 2820, kIdT = 3073, kIdTv = 3074, kIdQ = 3330, kIdRh = 3331, kIdPs = 14593,
  kIdTcLon = 99991, kIdTcLat = 99992, kIdTcMip = 99993
};

__device__ inline uint32_t wd(uint32_t w, int be) { return be ? __builtin_bswap32(w) : w; }
__device__ inline uint32_t fw(float f, int be) { return wd(__float_as_uint(f), be); }

// NINT of a float32: half away from zero (roundf is exact: the statement's trunc(x + copysign(0.5, x)) in double adds 0.5 to a
// float32 without rounding); NaN gives 0, beyond int32 saturates
__device__ inline int32_t nint32(float x) {
  if (x != x) return 0;
  const float r = roundf(x);
  if (r >= 2147483648.0f) return INT_MAX;
  if (r <= -2147483648.0f) return INT_MIN;
  return (int32_t)r;
}

// write_obs' test (:2236): in double, tiny of the single kind
__device__ inline bool defined_dat(double dat) { return fabs(dat - kUndef) > (double)kTiny; }

// the block's nr records between the image (W dwords each, contiguous) and LDS (pitch W | 1)
template <int W>
__device__ inline void stage_in(const uint32_t* __restrict__ src, int nr, uint32_t* rec) {
  for (int j = threadIdx.x; j < nr * W; j += kBlock) rec[(j / W) * (W | 1) + j % W] = src[j];
}
template <int W>
__device__ inline void stage_out(uint32_t* __restrict__ dst, int nr, const uint32_t* rec) {
  for (int j = threadIdx.x; j < nr * W; j += kBlock) dst[j] = rec[(j / W) * (W | 1) + j % W];
}

// the sum of v over the block; sh: 4 ints of LDS that nothing else uses
__device__ inline int block_sum(int v, int32_t* sh) {
  for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  return sh[0] + sh[1] + sh[2] + sh[3];
}

// read_obs' SELECT CASE (:2162-2198) on wk(1:8), 1-based, in float32
__device__ inline void scale_read(float* wk, const letkf_obsfile_params& p, const letkf_mapproj& proj) {
  switch (nint32(wk[1])) {
    case kIdU: case kIdV: case kIdT: case kIdTv: case kIdQ:
      wk[4] = wk[4] * 100.0f;
      break;
    case kIdPs:
      wk[5] = wk[5] * 100.0f;
      wk[6] = wk[6] * 100.0f;
      break;
    case kIdRh:
      wk[4] = wk[4] * 100.0f;
      wk[5] = wk[5] * 0.01f;
      wk[6] = wk[6] * 0.01f;
      break;
    case kIdTcMip:
      wk[4] = wk[4] * 100.0f;
      wk[5] = wk[5] * 100.0f;
      wk[6] = (float)p.obserr_tcp;
      break;
    case kIdTcLon: case kIdTcLat: {
      const bool is_lon = nint32(wk[1]) == kIdTcLon;
      double x = NAN, y = NAN, cs, sn;
      if (p.proj_given)
        mapproj::lc_forward(proj, (double)wk[2] * mapproj::kPiRef / 180.0, (double)wk[3] * mapproj::kPiRef / 180.0, &x, &y, &cs, &sn);
      wk[4] = wk[4] * 100.0f;
      wk[5] = (float)(is_lon ? x : y);
      wk[6] = (float)(is_lon ? p.obserr_tcx : p.obserr_tcy);
      break;
    }
    default:
      break;
  }
}

// write_obs' and write_obs_dep's SELECT CASE (:2245-2266, :2382-2403)
__device__ inline void scale_write(float* wk) {
  switch (nint32(wk[1])) {
    case kIdU: case kIdV: case kIdT: case kIdTv: case kIdQ:
      wk[4] = wk[4] * 0.01f;
      break;
    case kIdPs: case kIdTcMip:
      wk[5] = wk[5] * 0.01f;
      wk[6] = wk[6] * 0.01f;
      break;
    case kIdRh:
      wk[4] = wk[4] * 0.01f;
      wk[5] = wk[5] * 100.0f;
      wk[6] = wk[6] * 100.0f;
      break;
    default:
      break;
  }
}

template <int W>
__global__ void __launch_bounds__(kBlock) decode_kernel(letkf_obsfile_params p, letkf_mapproj proj, const uint32_t* __restrict__ rows,
                                                        int64_t n, letkf_obsfile_cols o, int32_t* __restrict__ cnt) {
  constexpr int NREC = W - 2, WP = W | 1;
  __shared__ uint32_t rec[kBlock * WP];
  __shared__ int32_t sh[4];
  const int64_t row0 = (int64_t)blockIdx.x * kBlock;
  const int nr = (int)(n - row0 < kBlock ? n - row0 : kBlock), be = p.big_endian;
  stage_in<W>(rows + row0 * W, nr, rec);
  __syncthreads();
  int bad = 0;
  if ((int)threadIdx.x < nr) {
    const uint32_t* r = rec + threadIdx.x * WP;
    const int64_t row = row0 + threadIdx.x;
    bad = wd(r[0], be) != 4u * NREC || wd(r[W - 1], be) != 4u * NREC;
    float wk[9];
    wk[8] = 0.0f;
#pragma unroll
    for (int k = 1; k <= NREC; ++k) wk[k] = __uint_as_float(wd(r[k], be));
    const bool radar = p.format == LETKF_OBSFILE_RADAR;
    if (!radar) scale_read(wk, p, proj);
    if (o.elm) o.elm[row] = nint32(wk[1]);
    if (o.lon) o.lon[row] = (double)wk[2];
    if (o.lat) o.lat[row] = (double)wk[3];
    if (o.lev) o.lev[row] = (double)wk[4];
    if (o.dat) o.dat[row] = (double)wk[5];
    if (o.err) o.err[row] = (double)wk[6];
    if (o.typ) o.typ[row] = radar ? LETKF_OBSFILE_TYP_RADAR : nint32(wk[7]);
    if (o.dif) o.dif[row] = NREC == 8 ? (double)wk[8] : 0.0;
  }
  if (cnt) {                                       // (uniform)
    const int total = block_sum(bad, sh);
    if (threadIdx.x == 0) cnt[blockIdx.x] = total;
  }
}

__global__ void radar_head_kernel(uint32_t* image, uint32_t b0, uint32_t b1, uint32_t b2, int be) {
  const int t = threadIdx.x;
  if (t < kRadarHeadWords) image[t] = wd(t % 3 != 1 ? 4u : t == 1 ? b0 : t == 4 ? b1 : b2, be);
}

__global__ void __launch_bounds__(kBlock) encode_count_kernel(int64_t n, const double* __restrict__ dat, int32_t* __restrict__ counts) {
  __shared__ int32_t sh[4];
  const int64_t row = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  const int total = block_sum(row < n && defined_dat(dat[row]), sh);
  if (threadIdx.x == 0) counts[blockIdx.x] = total;
}

template <int W>
__global__ void __launch_bounds__(kBlock) encode_kernel(letkf_obsfile_params p, int64_t n, letkf_obsfile_cols in,
                                                        const int64_t* __restrict__ off, uint32_t* __restrict__ rows) {
  constexpr int NREC = W - 2, WP = W | 1;
  __shared__ uint32_t rec[kBlock * WP];
  __shared__ int32_t wtot[4];
  const int64_t row0 = (int64_t)blockIdx.x * kBlock, row = row0 + threadIdx.x;
  const int nr = (int)(n - row0 < kBlock ? n - row0 : kBlock), be = p.big_endian;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const bool keep = row < n && (!off || defined_dat(in.dat[row]));
  // the row's place among the block's survivors: those of the waves before it, then of the lanes before it
  const unsigned long long votes = __ballot(keep);
  if (lane == 0) wtot[wave] = __popcll(votes);
  __syncthreads();
  int place = __popcll(votes & ((1ull << lane) - 1ull)), total = 0;
  for (int w = 0; w < 4; ++w) {
    if (w < wave) place += wtot[w];
    total += wtot[w];
  }
  if (keep) {
    float wk[9];
    wk[1] = (float)in.elm[row];
    wk[2] = (float)in.lon[row];
    wk[3] = (float)in.lat[row];
    wk[4] = (float)in.lev[row];
    wk[5] = (float)in.dat[row];
    wk[6] = (float)in.err[row];
    wk[7] = (float)in.typ[row];
    wk[8] = NREC == 8 ? (float)in.dif[row] : 0.0f;
    if (p.format != LETKF_OBSFILE_RADAR) scale_write(wk);
    uint32_t* r = rec + place * WP;
    r[0] = r[W - 1] = wd(4u * NREC, be);
#pragma unroll
    for (int k = 1; k <= NREC; ++k) r[k] = fw(wk[k], be);
  }
  __syncthreads();
  stage_out<W>(rows + (off ? off[blockIdx.x] : row0) * W, off ? total : nr, rec);
}

template <int W>
__global__ void __launch_bounds__(kBlock) obsda_encode_kernel(int be, int64_t n, const int32_t* __restrict__ set, const int32_t* __restrict__ idx,
                                                              const int32_t* __restrict__ qc, const double* __restrict__ value, int64_t stride,
                                                              const double* __restrict__ lev, const double* __restrict__ val2,
                                                              uint32_t* __restrict__ image) {
  constexpr int NREC = W - 2, WP = W | 1;
  __shared__ uint32_t rec[kBlock * WP];
  const int64_t row0 = (int64_t)blockIdx.x * kBlock, row = row0 + threadIdx.x;
  const int nr = (int)(n - row0 < kBlock ? n - row0 : kBlock);
  if (row < n) {
    uint32_t* r = rec + threadIdx.x * WP;
    r[0] = r[W - 1] = wd(4u * NREC, be);
    r[1] = fw((float)set[row], be);                // (:2335-2336: rounds above 2^24)
    r[2] = fw((float)idx[row], be);
    r[3] = fw((float)value[row * stride], be);
    r[4] = fw((float)qc[row], be);
    if (NREC == 6) {
      r[5] = fw((float)lev[row], be);
      r[6] = fw((float)val2[row], be);
    }
  }
  __syncthreads();
  stage_out<W>(image + row0 * W, nr, rec);
}

// is (set, idx), 1-based, a row of the files?
__device__ inline bool file_row(int32_t s, int32_t i, int nfile, const int64_t* __restrict__ off, int64_t* g) {
  if (s < 1 || s > nfile || i < 1) return false;
  const int64_t first = off[s - 1];
  if ((int64_t)i > off[s] - first) return false;
  *g = first + i - 1;
  return true;
}

__global__ void __launch_bounds__(kBlock) obsdep_check_kernel(int64_t n, const int32_t* __restrict__ set, const int32_t* __restrict__ idx, int nfile,
                                                              const int64_t* __restrict__ off, int32_t* __restrict__ cnt) {
  __shared__ int32_t sh[4];
  const int64_t row = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  int64_t g;
  const int total = block_sum(row < n && !file_row(set[row], idx[row], nfile, off, &g), sh);
  if (threadIdx.x == 0) cnt[blockIdx.x] = total;
}

__global__ void __launch_bounds__(kBlock) obsdep_encode_kernel(int be, int64_t n, const int32_t* __restrict__ set, const int32_t* __restrict__ idx,
                                                               const int32_t* __restrict__ qc, const double* __restrict__ omb,
                                                               const double* __restrict__ oma, letkf_obsfile_rows f,
                                                               const int64_t* __restrict__ off, uint32_t* __restrict__ image) {
  constexpr int W = 13, NREC = 11, WP = 13;
  __shared__ uint32_t rec[kBlock * WP];
  const int64_t row0 = (int64_t)blockIdx.x * kBlock, row = row0 + threadIdx.x;
  const int nr = (int)(n - row0 < kBlock ? n - row0 : kBlock);
  int64_t g;
  if (row < n && file_row(set[row], idx[row], f.nfile, off, &g)) {        // (the check kernel found every row inside)
    float wk[12];
    wk[1] = (float)f.elm[g];
    wk[2] = (float)f.lon[g];
    wk[3] = (float)f.lat[g];
    wk[4] = (float)f.lev[g];
    wk[5] = (float)f.dat[g];
    wk[6] = (float)f.err[g];
    wk[7] = (float)f.typ[g];
    wk[8] = (float)f.dif[g];
    wk[9] = (float)qc[row];
    wk[10] = (float)omb[row];
    wk[11] = (float)oma[row];
    scale_write(wk);
    uint32_t* r = rec + threadIdx.x * WP;
    r[0] = r[W - 1] = wd(4u * NREC, be);
#pragma unroll
    for (int k = 1; k <= NREC; ++k) r[k] = fw(wk[k], be);
  }
  __syncthreads();
  stage_out<W>(image + row0 * W, nr, rec);
}

// ---- the assemble kernel.  Lane l of wave w: image mi = l & 15 of the tile, row r = pass * 16 + w * 4 + (l >> 4), pass 0..3.
template <int W>
__global__ void __launch_bounds__(kBlock) assemble_kernel(letkf_obsda_params p, const ImageRef* __restrict__ tab, letkf_obsda_cols o,
                                                          int32_t* __restrict__ cnt) {
  constexpr int NREC = W - 2, WP = W | 1, P = kTileRows * WP + 2;          // P = 2 (mod 32), WP odd: see above
  static_assert((kTileRows * WP) % 32 == 0 && kTileRows * W == 64 * W, "bank map; W loads per lane and image");
  __shared__ uint32_t tile[kTileMembers * P];
  __shared__ int32_t sh_bad[4], sh_inc[4];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), mi = lane & 15, rr = lane >> 4;
  const int64_t r0 = (int64_t)blockIdx.x * kTileRows;
  const int nr = (int)(p.nobs - r0 < kTileRows ? p.nobs - r0 : kTileRows), be = p.big_endian, nw = nr * W;

  int32_t qcacc[4], set0[4], idx0[4], incons[4];
  double levacc[4], v2acc[4];
  int bad = 0;
#pragma unroll
  for (int ps = 0; ps < 4; ++ps) {
    const int r = ps * 16 + wave * 4 + rr;
    qcacc[ps] = INT_MIN, set0[ps] = idx0[ps] = incons[ps] = 0;
    levacc[ps] = NREC == 6 && o.lev && r < nr ? o.lev[r0 + r] : 0.0;
    v2acc[ps] = NREC == 6 && o.val2 && r < nr ? o.val2[r0 + r] : 0.0;
  }

  for (int m0 = 0; m0 < p.nmem; m0 += kTileMembers) {
    const int nm = p.nmem - m0 < kTileMembers ? p.nmem - m0 : kTileMembers;
    if (m0) __syncthreads();                       // the tile of the images before is read
    for (int i = wave; i < nm; i += 4) {           // (uniform per wave: the image's pointer is a scalar)
      const uint32_t* __restrict__ src = tab[m0 + i].words + r0 * W;
      uint32_t* dst = tile + i * P;
#pragma unroll
      for (int t = 0; t < W; ++t) {
        const int j = lane + 64 * t;
        if (j < nw) dst[(j / W) * WP + j % W] = src[j];
      }
    }
    __syncthreads();

    const bool mval = mi < nm;
    const int32_t mycol = mval ? tab[m0 + mi].col : 0;
#pragma unroll
    for (int ps = 0; ps < 4; ++ps) {
      const int r = ps * 16 + wave * 4 + rr;
      const bool valid = mval && r < nr;
      uint32_t w[W];
#pragma unroll
      for (int k = 0; k < W; ++k) w[k] = valid ? wd(tile[mi * P + r * WP + k], be) : 0u;
      if (valid) {
        o.ensval[(r0 + r) * p.kld + mycol] = (double)__uint_as_float(w[3]);
        bad += w[0] != 4u * NREC || w[W - 1] != 4u * NREC;
      }
      const int32_t s = nint32(__uint_as_float(w[1])), ix = nint32(__uint_as_float(w[2]));
      if (m0 == 0) {                               // image 0 is lane mi = 0 of the first tile (:214-216)
        set0[ps] = __shfl(s, lane & 48);
        idx0[ps] = __shfl(ix, lane & 48);
      }
      const int32_t q = valid ? nint32(__uint_as_float(w[4])) : INT_MIN;       // (:1865) per lane here, over the lanes below
      qcacc[ps] = q > qcacc[ps] ? q : qcacc[ps];
      incons[ps] |= valid && (s != set0[ps] || ix != idx0[ps]);
      if (NREC == 6) {                             // (:1867-1870) image after image, as the reference adds them
        const float f5 = valid ? __uint_as_float(w[NREC == 6 ? 5 : 0]) : 0.0f, f6 = valid ? __uint_as_float(w[NREC == 6 ? 6 : 0]) : 0.0f;
        for (int j = 0; j < nm; ++j) {
          const float a = __shfl(f5, (lane & 48) + j), b = __shfl(f6, (lane & 48) + j);
          if (tab[m0 + j].is_member) {
            levacc[ps] += (double)a;
            v2acc[ps] += (double)b;
          }
        }
      }
    }
  }

  // a row's 16 lanes hold the maxima and flags of their own images: once over the lanes
#pragma unroll
  for (int ps = 0; ps < 4; ++ps) {
#pragma unroll
    for (int d = 1; d < 16; d <<= 1) {
      const int32_t q2 = __shfl_xor(qcacc[ps], d);
      qcacc[ps] = q2 > qcacc[ps] ? q2 : qcacc[ps];
      incons[ps] |= __shfl_xor(incons[ps], d);
    }
  }
  // the per-row results through LDS, so that set, idx and qc are written by consecutive lanes
  __syncthreads();
  int32_t* res = reinterpret_cast<int32_t*>(tile);
#pragma unroll
  for (int ps = 0; ps < 4; ++ps) {
    const int r = ps * 16 + wave * 4 + rr;
    if (mi == 0) {
      res[r] = set0[ps], res[64 + r] = idx0[ps], res[128 + r] = qcacc[ps], res[192 + r] = incons[ps];
      if (NREC == 6 && r < nr) {
        const double div = p.finish ? (double)p.member : 1.0;
        if (o.lev) o.lev[r0 + r] = p.finish ? levacc[ps] / div : levacc[ps];
        if (o.val2) o.val2[r0 + r] = p.finish ? v2acc[ps] / div : v2acc[ps];
      }
    }
  }
  __syncthreads();
  const int r = threadIdx.x & 63, what = threadIdx.x >> 6;
  if (r < nr) {
    const int64_t n = r0 + r;
    if (what == 0) o.set[n] = res[r];
    if (what == 1) o.idx[n] = res[64 + r];
    if (what == 2) o.qc[n] = o.qc[n] > res[128 + r] ? o.qc[n] : res[128 + r];       // (:1865)
  }
  if (cnt) {                                       // (uniform)
    const int nbad = block_sum(bad, sh_bad), ninc = block_sum(what == 3 && r < nr && res[192 + r], sh_inc);
    if (threadIdx.x == 0) cnt[2 * (int64_t)blockIdx.x] = nbad, cnt[2 * (int64_t)blockIdx.x + 1] = ninc;
  }
}

__global__ void __launch_bounds__(kBlock) count_total_kernel(const int32_t* __restrict__ cnt, int64_t nblock, int ncnt, int64_t* __restrict__ total) {
  __shared__ long long sh[4];
  for (int c = 0; c < ncnt; ++c) {
    long long v = 0;
    for (int64_t i = threadIdx.x; i < nblock; i += kBlock) v += cnt[i * ncnt + c];
    for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) total[c] = sh[0] + sh[1] + sh[2] + sh[3];
  }
}

dim3 grid_of(int64_t blocks) { return dim3((unsigned)blocks); }

}  // namespace

hipError_t count_total_run(hipStream_t st, const int32_t* cnt, int64_t nblock, int ncnt, int64_t* total) {
  hipLaunchKernelGGL(count_total_kernel, dim3(1), dim3(kBlock), 0, st, cnt, nblock, ncnt, total);
  return hipGetLastError();
}

hipError_t decode_run(hipStream_t st, const letkf_obsfile_params& p, const letkf_mapproj* proj, const uint32_t* rows, int64_t n,
                      const letkf_obsfile_cols& o, int32_t* cnt) {
  const letkf_mapproj pr = p.proj_given && proj ? *proj : letkf_mapproj{};
  letkf_obsfile_params q = p;
  q.proj_given = p.proj_given && proj;
  if (p.nrec == 8)
    hipLaunchKernelGGL(decode_kernel<10>, grid_of(row_blocks(n)), dim3(kBlock), 0, st, q, pr, rows, n, o, cnt);
  else
    hipLaunchKernelGGL(decode_kernel<9>, grid_of(row_blocks(n)), dim3(kBlock), 0, st, q, pr, rows, n, o, cnt);
  return hipGetLastError();
}

hipError_t radar_head_run(hipStream_t st, uint32_t* image, uint32_t b0, uint32_t b1, uint32_t b2, int big_endian) {
  hipLaunchKernelGGL(radar_head_kernel, dim3(1), dim3(64), 0, st, image, b0, b1, b2, big_endian);
  return hipGetLastError();
}

hipError_t encode_count_run(hipStream_t st, int64_t n, const double* dat, int32_t* counts) {
  hipLaunchKernelGGL(encode_count_kernel, grid_of(row_blocks(n)), dim3(kBlock), 0, st, n, dat, counts);
  return hipGetLastError();
}

hipError_t encode_run(hipStream_t st, const letkf_obsfile_params& p, int64_t n, const letkf_obsfile_cols& in, const int64_t* off,
                      uint32_t* rows) {
  if (p.nrec == 8)
    hipLaunchKernelGGL(encode_kernel<10>, grid_of(row_blocks(n)), dim3(kBlock), 0, st, p, n, in, off, rows);
  else
    hipLaunchKernelGGL(encode_kernel<9>, grid_of(row_blocks(n)), dim3(kBlock), 0, st, p, n, in, off, rows);
  return hipGetLastError();
}

hipError_t assemble_run(hipStream_t st, const letkf_obsda_params& p, const ImageRef* tab, const letkf_obsda_cols& o, int32_t* cnt) {
  if (p.nrec == 6)
    hipLaunchKernelGGL(assemble_kernel<8>, grid_of(row_tiles(p.nobs)), dim3(kBlock), 0, st, p, tab, o, cnt);
  else
    hipLaunchKernelGGL(assemble_kernel<6>, grid_of(row_tiles(p.nobs)), dim3(kBlock), 0, st, p, tab, o, cnt);
  return hipGetLastError();
}

hipError_t obsda_encode_run(hipStream_t st, int nrec, int big_endian, int64_t n, const int32_t* set, const int32_t* idx, const int32_t* qc,
                            const double* value, int64_t stride, const double* lev, const double* val2, uint32_t* image) {
  if (nrec == 6)
    hipLaunchKernelGGL(obsda_encode_kernel<8>, grid_of(row_blocks(n)), dim3(kBlock), 0, st, big_endian, n, set, idx, qc, value, stride, lev, val2,
                       image);
  else
    hipLaunchKernelGGL(obsda_encode_kernel<6>, grid_of(row_blocks(n)), dim3(kBlock), 0, st, big_endian, n, set, idx, qc, value, stride, lev, val2,
                       image);
  return hipGetLastError();
}

hipError_t obsdep_check_run(hipStream_t st, int64_t n, const int32_t* set, const int32_t* idx, int nfile, const int64_t* off, int32_t* cnt) {
  hipLaunchKernelGGL(obsdep_check_kernel, grid_of(row_blocks(n)), dim3(kBlock), 0, st, n, set, idx, nfile, off, cnt);
  return hipGetLastError();
}

hipError_t obsdep_encode_run(hipStream_t st, int big_endian, int64_t n, const int32_t* set, const int32_t* idx, const int32_t* qc,
                             const double* omb, const double* oma, const letkf_obsfile_rows& f, const int64_t* off, uint32_t* image) {
  hipLaunchKernelGGL(obsdep_encode_kernel, grid_of(row_blocks(n)), dim3(kBlock), 0, st, big_endian, n, set, idx, qc, omb, oma, f, off, image);
  return hipGetLastError();
}

}  // namespace obsfile
}  // namespace letkf
