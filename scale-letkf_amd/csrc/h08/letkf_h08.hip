// letkf_h08.hip -- the Himawari-8 radiances on the device (include/letkf_amd_h08.h).
//   decode_kernel / encode_kernel
//       256 profiles per block.  A record is 16 dwords (marker, wk(1:14), marker); the block's records pass through LDS at a pitch
//       of 17 dwords so that the image is read and written with coalesced dword accesses, and the ten rows of a profile are
//       written (read) with the block's threads along the ROWS: coalesced columns.  The small helpers (byte order, NINT of a
//       float32) restate those of obsfile/letkf_obsfile.hip, which lives in another library.
//   count_total_kernel    per-block int32 counts to one int64, one block, a fixed order
//   select_mark_kernel / select_fill_kernel
//       a 0 / 1 flag per file profile (every writer writes 1), the main library's scan between them, then one writer per
//       position of prof_list / slot_of_prof
//   profiles_kernel
//       one wave per (member, selected profile), lanes along the level (a loop when nlev > 64): the four corner columns of p, t,
//       q, qc, qi, qs, qg are unit-stride loads where s3k = 1, the outputs level-fastest stores in either direction.  The cloud
//       layers take the neighbouring level from the next lane.  Lanes 0..6 interpolate one surface field each, lane 7 has the
//       zenith angle.
//   rows_kernel
//       one block per obsda row; its four waves take the members in turn, lanes along the layer of one (row, member).  The first
//       maximum of the weights: per lane in ascending j with >, then wave_max of the value and wave_min of the lowest j among the
//       lanes that hold it (letkf_lane_dev.h) -- the sequential statement's result.  Members' plev / btclr / qc go through LDS 64 at
//       a time and thread 0 adds them in member order: lev / val2 / qc have one writer.
// Built with -ffp-contract=off: every product and sum rounds on its own, as the reference's expressions do.  No atomics.
#include <hip/hip_runtime.h>

#include <climits>

#include "letkf_h08_dev.h"
#include "letkf_lane_dev.h"
#include "letkf_obsope_point_dev.h"

namespace letkf {
namespace h08 {
namespace {

using namespace letkf::obsope_point_dev;   // ceil_split, term2, kQcOutH, kQcOtype, kUndef, the iv3dd slots
using namespace letkf::lane_dev;

constexpr int W = kRecWords, WP = kRecWords | 1;
constexpr int kBatch = 64;                                   // members whose results wait in LDS for thread 0
constexpr double kD2R = 3.14159265358979 / 180.0;            // SCALE-RM's CONST_D2R
enum { V2_U10M = 3, V2_V10M = 4, V2_LSMASK = 7, V2_SKINT = 8 };   // iv2dd_* - 1 (common_scale.f90:82-88)

struct Obserr {
  double v[kNch];
};

__device__ inline uint32_t wd(uint32_t w, int be) { return be ? __builtin_bswap32(w) : w; }
__device__ inline uint32_t fw(float f, int be) { return wd(__float_as_uint(f), be); }
// NINT of a float32: half away from zero; NaN gives 0, beyond int32 saturates (the rules of include/letkf_amd_obsfile.h)
__device__ inline int32_t nint32(float x) {
  if (x != x) return 0;
  const float r = roundf(x);
  if (r >= 2147483648.0f) return INT_MAX;
  if (r <= -2147483648.0f) return INT_MIN;
  return (int32_t)r;
}

__device__ inline int block_sum(int v, int32_t* sh) {
  for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  return sh[0] + sh[1] + sh[2] + sh[3];
}

__global__ void __launch_bounds__(kBlock) decode_kernel(int be, const uint32_t* __restrict__ image, int64_t nprof, Obserr e,
                                                        letkf_obsfile_cols o, int32_t* __restrict__ cnt) {
  __shared__ uint32_t rec[kBlock * WP];
  __shared__ int32_t sh[kWaves];
  const int64_t p0 = (int64_t)blockIdx.x * kBlock;
  const int np = (int)(nprof - p0 < kBlock ? nprof - p0 : kBlock);
  const uint32_t* src = image + p0 * W;
  for (int j = threadIdx.x; j < np * W; j += kBlock) rec[(j / W) * WP + j % W] = src[j];
  __syncthreads();
  for (int r = threadIdx.x; r < np * kNch; r += kBlock) {
    const int q = r / kNch, c = r % kNch;
    const uint32_t* w = rec + q * WP;
    const int64_t row = p0 * kNch + r;
    if (o.elm) o.elm[row] = nint32(__uint_as_float(wd(w[1], be)));
    if (o.typ) o.typ[row] = nint32(__uint_as_float(wd(w[2], be)));
    if (o.lon) o.lon[row] = (double)__uint_as_float(wd(w[3], be));
    if (o.lat) o.lat[row] = (double)__uint_as_float(wd(w[4], be));
    if (o.lev) o.lev[row] = (double)(c + 7);                       // ch + 6.0, ch = c + 1
    if (o.dat) o.dat[row] = (double)__uint_as_float(wd(w[5 + c], be));
    if (o.err) o.err[row] = e.v[c];
    if (o.dif) o.dif[row] = 0.0;
  }
  if (cnt) {                                                       // (uniform)
    int bad = 0;
    if ((int)threadIdx.x < np) {
      const uint32_t* w = rec + threadIdx.x * WP;
      bad = wd(w[0], be) != 4u * (W - 2) || wd(w[W - 1], be) != 4u * (W - 2);
    }
    const int total = block_sum(bad, sh);
    if (threadIdx.x == 0) cnt[blockIdx.x] = total;
  }
}

__global__ void __launch_bounds__(kBlock) count_total_kernel(const int32_t* __restrict__ cnt, int64_t nblock, int64_t* __restrict__ total) {
  __shared__ int64_t part[kBlock];
  int64_t s = 0;
  for (int64_t b = threadIdx.x; b < nblock; b += kBlock) s += cnt[b];
  part[threadIdx.x] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    int64_t t = 0;
    for (int k = 0; k < kBlock; ++k) t += part[k];
    *total = t;
  }
}

__global__ void __launch_bounds__(kBlock) encode_kernel(int be, int64_t nprof, letkf_obsfile_cols in, uint32_t* __restrict__ image) {
  __shared__ uint32_t rec[kBlock * WP];
  const int64_t p0 = (int64_t)blockIdx.x * kBlock;
  const int np = (int)(nprof - p0 < kBlock ? nprof - p0 : kBlock);
  for (int r = threadIdx.x; r < np * kNch; r += kBlock) {
    const int q = r / kNch, c = r % kNch;
    uint32_t* w = rec + q * WP;
    const int64_t row = p0 * kNch + r;
    w[5 + c] = fw((float)in.dat[row], be);
    if (c == 0) {
      w[0] = w[W - 1] = wd(4u * (W - 2), be);
      w[1] = fw((float)in.elm[row], be);
      w[2] = fw((float)in.typ[row], be);
      w[3] = fw((float)in.lon[row], be);
      w[4] = fw((float)in.lat[row], be);
    }
  }
  __syncthreads();
  uint32_t* dst = image + p0 * W;
  for (int j = threadIdx.x; j < np * W; j += kBlock) dst[j] = rec[(j / W) * WP + j % W];
}

__global__ void __launch_bounds__(kBlock) select_mark_kernel(const int32_t* __restrict__ set, const int32_t* __restrict__ idx, int64_t row0,
                                                             int64_t nrows, int h08_set, int64_t nprof_file, int32_t* __restrict__ flag) {
  const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (t >= nrows) return;
  const int64_t r = row0 + t, i1 = (int64_t)idx[r] - 1;
  if (set[r] == h08_set && i1 >= 0 && i1 < nprof_file * kNch) flag[i1 / kNch] = 1;
}

__global__ void __launch_bounds__(kBlock) select_fill_kernel(int64_t nprof_file, const int32_t* __restrict__ flag, const int64_t* __restrict__ off,
                                                             int32_t* __restrict__ prof_list, int32_t* __restrict__ slot_of_prof) {
  const int64_t fp = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (fp >= nprof_file) return;
  const bool sel = flag[fp] != 0;
  slot_of_prof[fp] = sel ? (int32_t)off[fp] : -1;
  if (sel) prof_list[off[fp]] = (int32_t)fp;
}

// (:551-572) every operation on its own, left to right
__device__ inline double zenith(const ProfileArgs& A, double lon, double lat) {
  const double rlat = lat * kD2R, rlon = lon * kD2R;
  const double c_lat = atan(A.ell_tan * tan(rlat));
  const double rl = A.r_pol / sqrt(1.0 - A.ell_ecc * cos(c_lat) * cos(c_lat));
  const double dl = rlon - A.sub_lon * kD2R;
  const double r1 = A.r_sat - rl * cos(c_lat) * cos(dl);
  const double r2 = -rl * cos(c_lat) * sin(dl);
  const double r3 = rl * sin(c_lat);
  const double rnps = sqrt(r1 * r1 + r2 * r2 + r3 * r3);
  const double r1ps = r1 * (-1.0), r2ps = r2 * (-1.0), r3ps = r3 * (-1.0);
  const double r1ep = r1 - A.r_sat, r2ep = r2, r3ep = r3;
  const double rnep = sqrt(r1ep * r1ep + r2ep * r2ep + r3ep * r3ep);
  double z = r1ps * r1ep + r2ps * r2ep + r3ps * r3ep;
  z = z / (rnps * rnep);
  z = fmax(-1.0, fmin(1.0, z));                                     // NOT FOLLOWED (1): the sub-satellite point
  return acos(z) / kD2R;
}

__global__ void __launch_bounds__(kBlock) profiles_kernel(ProfileArgs A) {
  const int lane = threadIdx.x & 63;
  const long task = (long)blockIdx.x * kWaves + (threadIdx.x >> 6);
  if (task >= (long)A.nmem * A.nsel) return;                        // (wave-uniform)
  const int nlev = A.nlev;
  const int m = (int)(task / A.nsel);
  const long s = task % A.nsel;
  const long fp = A.prof_list[s];
  const bool in_file = fp >= 0 && fp < A.nprof_file;                // (a list select did not make: flagged, not read)
  const double ril = in_file ? A.ri[fp] - A.ri_off : NAN, rjl = in_file ? A.rj[fp] - A.rj_off : NAN;
  const bool ok = ril >= 1.0 && ril <= (double)A.nlonh && rjl >= 1.0 && rjl <= (double)A.nlath;   // (a NaN fails)
  double* l3 = A.lev3 + task * 5 * nlev;
  double* sf = A.sfc + task * 8;
  double* cl = A.rttov_units ? A.cloud + task * 3 * (nlev - 1) : nullptr;
  if (m == 0 && lane == 0) A.pflag[s] = ok ? 0 : kQcOutH;
  if (!ok) {
    for (int q = lane; q < 5 * nlev; q += 64) l3[q] = kUndef;
    if (lane < 8) sf[lane] = kUndef;
    if (cl)
      for (int q = lane; q < 3 * (nlev - 1); q += 64) cl[q] = kUndef;
    return;
  }

  // ---- the surface: lane v < 7 one field, lane 7 the zenith angle
  double val = 0.0;
  if (lane < 7) {
    const int v2 = lane == 0 ? V2_SKINT : lane == 1 ? V2_Q2M : lane == 2 ? V2_PS : lane == 3 ? V2_U10M : lane == 4 ? V2_V10M
                   : lane == 5 ? V2_TOPO : V2_LSMASK;
    double ri_v = ril, rj_v = rjl;
    if (A.stggrd == 1 && lane == 3) ri_v -= 0.5;
    if (A.stggrd == 1 && lane == 4) rj_v -= 0.5;
    int i0, i1, j0, j1;
    double ai, aj;
    ceil_split(ri_v, A.nlonh, &i0, &i1, &ai);
    ceil_split(rj_v, A.nlath, &j0, &j1, &aj);
    const double* g = A.v2d + (long)m * A.s2m + (long)v2 * A.s2v;
    const double wa0 = 1.0 - ai, wb0 = 1.0 - aj;
    val = term2(g[i0 * A.s2i + j0 * A.s2j], wa0, wb0) + term2(g[i1 * A.s2i + j0 * A.s2j], ai, wb0) +
          term2(g[i0 * A.s2i + j1 * A.s2j], wa0, aj) + term2(g[i1 * A.s2i + j1 * A.s2j], ai, aj);
  }
  {
    const double u = wshfl(val, 3), v = wshfl(val, 4);
    if (A.rotc) {
      const double rc1 = A.rotc[2 * fp], rc2 = A.rotc[2 * fp + 1];
      if (lane == 3) val = u * rc1 - v * rc2;
      if (lane == 4) val = u * rc2 + v * rc1;
    }
    if (lane == 7) val = zenith(A, A.lon[fp], A.lat[fp]);
    if (A.rttov_units) {
      if (lane == 1) {
        val = val * A.q_ppmv;
        if (val < A.qmin) val = A.qmin + A.qmin * 0.01;
      }
      if (lane == 2) val = val * 0.01;
      if (lane == 5) val = val * 0.001;                             // (lane 6: the mask stays as interpolated, rows tests it)
    }
    if (lane < 8) sf[lane] = val;
  }

  // ---- the columns
  int i0, i1, j0, j1;
  double ai, aj;
  ceil_split(ril, A.nlonh, &i0, &i1, &ai);
  ceil_split(rjl, A.nlath, &j0, &j1, &aj);
  const double wa0 = 1.0 - ai, wb0 = 1.0 - aj;
  const double* v3 = A.v3d + (long)m * A.s3m;
  const long cb0 = i0 * A.s3i + j0 * A.s3j, cb1 = i1 * A.s3i + j0 * A.s3j, cb2 = i0 * A.s3i + j1 * A.s3j, cb3 = i1 * A.s3i + j1 * A.s3j;
  // x = p, t, q, qc, qi + qs + qg at model level k
  auto level = [&](int k, double(&x)[5]) {
    const long ko = (long)(A.khalo + k) * A.s3k;
    const int slot[4] = {V_P, V_T, V_Q, V_QC};
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const double* g = v3 + (long)slot[q] * A.s3v + ko;
      x[q] = term2(g[cb0], wa0, wb0) + term2(g[cb1], ai, wb0) + term2(g[cb2], wa0, aj) + term2(g[cb3], ai, aj);
    }
    const double *gi = v3 + (long)V_QI * A.s3v + ko, *gs = v3 + (long)V_QS * A.s3v + ko, *gg = v3 + (long)V_QG * A.s3v + ko;
    x[4] = term2(gi[cb0] + gs[cb0] + gg[cb0], wa0, wb0) + term2(gi[cb1] + gs[cb1] + gg[cb1], ai, wb0) +
           term2(gi[cb2] + gs[cb2] + gg[cb2], wa0, aj) + term2(gi[cb3] + gs[cb3] + gg[cb3], ai, aj);
  };
  // (:604-609) the liquid and ice contents in g m-3
  auto contents = [&](const double(&x)[5], double* liqc, double* icec) {
    const double tv = x[1] * (1.0 + x[2] * A.repsb) / (1.0 + x[2]);
    const double g = x[0] / (A.rd * tv) * 1000.0;
    *liqc = fmax(x[3], 0.0) * g;
    *icec = fmax(x[4], 0.0) * g;
  };
  const int nchunk = (nlev + 63) >> 6;
  for (int c = 0; c < nchunk; ++c) {
    const int k = c * 64 + lane;
    const bool in = k < nlev;
    double x[5];
    level(min(k, nlev - 1), x);
    const int l = A.top_down ? nlev - 1 - k : k;
    if (A.rttov_units) {
      double liqc, icec, liqn, icen;
      contents(x, &liqc, &icec);
      liqn = __shfl_down(liqc, 1, 64), icen = __shfl_down(icec, 1, 64);
      if (lane == 63 && k + 1 < nlev) {                             // the next chunk's first level
        double y[5];
        level(k + 1, y);
        contents(y, &liqn, &icen);
      }
      if (k + 1 < nlev) {
        const double liq = (liqc + liqn) * 0.5, ice = (icec + icen) * 0.5;
        double cf;
        if (A.cfrac_cnst <= 0.0) cf = (liq + ice) > A.minq ? 1.0 : 0.0;
        else cf = fmin((liq + ice) / A.cfrac_cnst, 1.0);
        const int ll = A.top_down ? nlev - 2 - k : k;
        cl[ll] = liq, cl[(nlev - 1) + ll] = ice, cl[2 * (nlev - 1) + ll] = cf;
      }
      x[0] = x[0] * 0.01;
      x[2] = x[2] * A.q_ppmv;
      if (x[2] < A.qmin) x[2] = A.qmin + A.qmin * 0.01;
    }
    if (in) {
#pragma unroll
      for (int q = 0; q < 5; ++q) l3[q * nlev + l] = x[q];
    }
  }
}

__global__ void __launch_bounds__(kBlock) rows_kernel(RowArgs A) {
  __shared__ double s_plev[kBatch], s_clr[kBatch];
  __shared__ int s_qc[kBatch];
  const long r = A.row0 + blockIdx.x;
  if (A.set[r] != A.h08_set) return;                                // (all block-uniform)
  const long i1 = (long)A.idx[r] - 1;
  if (i1 < 0 || i1 >= A.nprof_file * kNch) return;
  const long fp = i1 / kNch;
  const int ch = (int)(i1 % kNch);
  const long s = A.slot_of_prof[fp];
  if (s < 0 || s >= A.nsel) return;
  if (!A.use_obs23) {
    if (threadIdx.x == 0) A.qc[r] = A.qc_replace ? kQcOtype : max(A.qc[r], kQcOtype);
    return;
  }
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, nlev = A.nlev, nlayer = nlev - 1;
  const double rig = A.rig[fp], rjg = A.rjg[fp];
  const bool buffer = rig <= A.bris || rig >= A.brie || rjg <= A.brjs || rjg >= A.brje;   // NOT FOLLOWED (2)
  const int pf = A.pflag[s];
  const int qc_ch = ((A.ch_mask >> ch) & 1u) ? 0 : LETKF_H08_QC_BAD;
  double acc_lev = 0.0, acc_v2 = 0.0;
  int acc_qc = 0;
  if (threadIdx.x == 0) acc_lev = A.lev[r], acc_v2 = A.val2[r], acc_qc = A.qc_replace ? 0 : A.qc[r];

  for (int mb = 0; mb < A.nmem; mb += kBatch) {
    const int nb = min(kBatch, A.nmem - mb);
    for (int mm = wave; mm < nb; mm += kWaves) {                    // (wave-uniform)
      const int m = mb + mm;
      const long pm = (long)m * A.nsel + s;
      const double* prs = A.lev3 + pm * 5 * nlev;
      const double* tau = A.trans + (pm * kNch + ch) * nlev;
      auto P = [&](int k) {
        const double v = prs[A.top_down ? nlev - 1 - k : k];
        return A.rttov_units ? v * 100.0 : v;
      };
      auto T = [&](int k) { return tau[A.top_down ? nlev - 1 - k : k]; };
      double bw = -INFINITY;
      int bj = INT_MAX;
      bool nan1 = false;
      for (int c0 = 0; c0 < nlayer; c0 += 64) {
        const int j = 1 + c0 + lane;                                // the layer between levels j - 1 and j
        if (j <= nlayer) {
          const double p1 = P(j), p0 = P(j - 1), dt = T(j) - T(j - 1);
          const double w = j == 1 ? fabs(dt * (1.0 / (p1 - p0))) : dt * (1.0 / fabs(p1 - p0));
          if (j == 1) nan1 = w != w;
          if (w > bw) bw = w, bj = j;
        }
      }
      int jwin = 1;
      if (!(__ballot(nan1) & 1ull)) {                               // (a NaN w1 keeps the first layer)
        const double wmax = wave_max(bw);
        jwin = (int)fmin(wave_min(bw == wmax ? (double)bj : 1.0e300), (double)nlayer);   // (lane 0 holds w1 >= 0: some lane matches)
      }
      if (lane == 0) {
        const double plev = (P(jwin) + P(jwin - 1)) * 0.5;
        const double ball = A.btall[pm * kNch + ch], bclr = A.btclr[pm * kNch + ch];
        double yobs = ball;
        if (fabs(ball - bclr) > A.cldsky_thrs) yobs = yobs * (-1.0);
        int q = qc_ch;
        if (A.reject_land && A.sfc[pm * 8 + 6] > 0.5) q = LETKF_H08_QC_BAD;
        if (q == 0 && buffer) q = LETKF_H08_QC_BAD;
        q = max(q, pf);
        A.ensval[r * A.kld + A.m0 + m] = yobs;
        s_plev[mm] = plev, s_clr[mm] = bclr, s_qc[mm] = q;
      }
    }
    __syncthreads();
    if (threadIdx.x == 0)
      for (int mm = 0; mm < nb; ++mm) {
        acc_lev = acc_lev + s_plev[mm];
        acc_v2 = acc_v2 + s_clr[mm];
        acc_qc = max(acc_qc, s_qc[mm]);
      }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    if (A.finish) acc_lev = acc_lev / (double)A.member, acc_v2 = acc_v2 / (double)A.member;
    A.lev[r] = acc_lev, A.val2[r] = acc_v2, A.qc[r] = acc_qc;
  }
}

}  // namespace

hipError_t launch_decode(int be, const uint32_t* image, int64_t nprof, const double (&obserr)[kNch], const letkf_obsfile_cols& o,
                         int32_t* cnt, hipStream_t st) {
  Obserr e;
  for (int c = 0; c < kNch; ++c) e.v[c] = obserr[c];
  decode_kernel<<<dim3((unsigned)blocks_of(nprof)), dim3(kBlock), 0, st>>>(be, image, nprof, e, o, cnt);
  return hipGetLastError();
}

hipError_t launch_count_total(const int32_t* cnt, int64_t nblock, int64_t* total, hipStream_t st) {
  count_total_kernel<<<dim3(1), dim3(kBlock), 0, st>>>(cnt, nblock, total);
  return hipGetLastError();
}

hipError_t launch_encode(int be, int64_t nprof, const letkf_obsfile_cols& in, uint32_t* image, hipStream_t st) {
  encode_kernel<<<dim3((unsigned)blocks_of(nprof)), dim3(kBlock), 0, st>>>(be, nprof, in, image);
  return hipGetLastError();
}

hipError_t launch_select_mark(const int32_t* set, const int32_t* idx, int64_t row0, int64_t nrows, int h08_set, int64_t nprof_file,
                              int32_t* flag, hipStream_t st) {
  select_mark_kernel<<<dim3((unsigned)blocks_of(nrows)), dim3(kBlock), 0, st>>>(set, idx, row0, nrows, h08_set, nprof_file, flag);
  return hipGetLastError();
}

hipError_t launch_select_fill(int64_t nprof_file, const int32_t* flag, const int64_t* off, int32_t* prof_list, int32_t* slot_of_prof,
                              hipStream_t st) {
  select_fill_kernel<<<dim3((unsigned)blocks_of(nprof_file)), dim3(kBlock), 0, st>>>(nprof_file, flag, off, prof_list, slot_of_prof);
  return hipGetLastError();
}

hipError_t launch_profiles(const ProfileArgs& a, hipStream_t st) {
  const int64_t tasks = (int64_t)a.nmem * a.nsel;
  profiles_kernel<<<dim3((unsigned)((tasks + kWaves - 1) / kWaves)), dim3(kBlock), 0, st>>>(a);
  return hipGetLastError();
}

hipError_t launch_rows(const RowArgs& a, hipStream_t st) {
  rows_kernel<<<dim3((unsigned)a.nrows), dim3(kBlock), 0, st>>>(a);
  return hipGetLastError();
}

}  // namespace h08
}  // namespace letkf
