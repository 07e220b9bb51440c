// letkf_monit.hip -- the departure monitor monit_obs (include/letkf_amd_monit.h; scale/common/common_obs_scale.f90:1370-1844):
//   state_to_history   common_scale.f90:1292-1400 with scale_calc_z :1434-1459.  The state is point-fastest, the history fields
//                      are level-fastest (what the operator's level scan reads): a transposing copy through LDS that also
//                      forms height and RH, then the 2-D slots, then the lateral halo of the sides that are domain boundaries
//   monit_obs          :1467-1599 around the operator of letkf_obsope.hip: the rows gathered by key, the rules per row and the
//                      records of the step; the statistics are launch_monit_dep's (letkf_post.hip)
// The unit is compiled without floating-point contraction (Makefile): the height rounds as the reference's expression does.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <string>

#include "letkf_monit_dev.h"

namespace {

constexpr double kUndef = -9.99e33;
constexpr int kQcOtype = 90;                                          // common_obs_scale.f90:150
// iv3dd_* - 1 and iv2dd_* - 1 (common_scale.f90:60-85); the state's iv3d_* - 1 are the first eleven of the former
enum { V_U = 0, V_V, V_W, V_T, V_P, V_Q, V_RH = 11, V_HGT = 12, NV3DD = 13 };
enum { V2_TOPO = 0, V2_PS, V2_RAIN, V2_U10, V2_V10, V2_T2M, V2_Q2M, NV2DD = 7 };
constexpr int kNState = 11;

struct HistArgs {
  int nlon, nlat, nlev, khalo, ihalo, jhalo, edge_fill;
  const double* x;
  long si, sj, sl, sv;
  const double *topo, *cz;
  double ztop;
  double* v3d;
  long s3k, s3i, s3j, s3v;
  double* v2d;
  long s2i, s2j, s2v;
};

// The tile of the transposing copy: 64 points x 64 levels of one history slot.  Row pitch 65 doubles: the load phase writes a row
// of 64 consecutive doubles per wave; the store phase reads one point's levels, lane = level: dword address 130 kk + 2 pp = 2 kk +
// 2 pp (mod 64), so the distinct kk of a 32-lane half sit on distinct even banks, every 8-byte read on its own pair, and the lanes
// of the vertical halo, which repeat a level, read one address.
constexpr int kTilePts = 64, kTileLev = 64, kPitch = 65;

// blockIdx = (point tile, level chunk, history slot 0 .. 12).  Load: lanes are points (contiguous where si = 1 and sj = nlon); the
// eleven state variables are read, height (scale_calc_z, :1452) is computed and RH is 0.  Store: lanes are the levels of the
// history column, vertical halo included (:1371-1379: a level below / above the model levels repeats the first / last one), one
// point per wave and step -- contiguous where s3k = 1, a whole column in one store where nlevh <= 64.  The chunk with the first
// (last) model level also writes the halo below (above) it, so every element has one writer.  Any strides give the same result,
// only slower.
__global__ void __launch_bounds__(256) hist_copy_kernel(const HistArgs A) {
  __shared__ double tile[kTileLev * kPitch];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long p0 = (long)blockIdx.x * kTilePts, npt = (long)A.nlon * A.nlat;
  const int k0 = blockIdx.y * kTileLev, v = blockIdx.z;
  const long p = p0 + lane;
  if (p < npt) {
    if (v < kNState) {
      const double* src = A.x + (p % A.nlon) * A.si + (p / A.nlon) * A.sj + v * A.sv;
      for (int kk = wave; kk < kTileLev; kk += 4)
        if (k0 + kk < A.nlev) tile[kk * kPitch + lane] = src[(long)(k0 + kk) * A.sl];
    } else {
      const double topo = A.topo[p], f = (A.ztop - topo) / A.ztop;
      for (int kk = wave; kk < kTileLev; kk += 4)
        if (k0 + kk < A.nlev) tile[kk * kPitch + lane] = v == V_HGT ? f * A.cz[k0 + kk] + topo : 0.0;
    }
  }
  __syncthreads();
  const int nlevh = A.nlev + 2 * A.khalo;
  const int elo = k0 == 0 ? 0 : k0 + A.khalo, ehi = k0 + kTileLev >= A.nlev ? nlevh : k0 + kTileLev + A.khalo;
  for (int it = 0; it < kTilePts / 4; ++it) {
    const int pp = wave * (kTilePts / 4) + it;
    const long q = p0 + pp;
    if (q >= npt) break;
    double* dst = A.v3d + (q % A.nlon + A.ihalo) * A.s3i + (q / A.nlon + A.jhalo) * A.s3j + v * A.s3v;
    for (int kh = elo + lane; kh < ehi; kh += 64) {
      const int kk = min(max(kh - A.khalo, 0), A.nlev - 1) - k0;
      dst[(long)kh * A.s3k] = tile[kk * kPitch + pp];
    }
  }
}

// The 2-D slots of the interior columns (:1342-1349): topo = the height of the first model level, ps u10m v10m t2m q2m = the
// first level's p u v t q, rain = 0.
__global__ void __launch_bounds__(256) hist_surface_kernel(const HistArgs A) {
  const long npt = (long)A.nlon * A.nlat;
  for (long p = (long)blockIdx.x * blockDim.x + threadIdx.x; p < npt; p += (long)gridDim.x * blockDim.x) {
    const long i = p % A.nlon, j = p / A.nlon;
    const double topo = A.topo[p];
    const double* src = A.x + i * A.si + j * A.sj;
    double* d2 = A.v2d + (i + A.ihalo) * A.s2i + (j + A.jhalo) * A.s2j;
    d2[V2_TOPO * A.s2v] = (A.ztop - topo) / A.ztop * A.cz[0] + topo;
    d2[V2_PS * A.s2v] = src[V_P * A.sv];
    d2[V2_RAIN * A.s2v] = 0.0;
    d2[V2_U10 * A.s2v] = src[V_U * A.sv];
    d2[V2_V10 * A.s2v] = src[V_V * A.sv];
    d2[V2_T2M * A.s2v] = src[V_T * A.sv];
    d2[V2_Q2M * A.s2v] = src[V_Q * A.sv];
  }
}

// The lateral halo: a column outside the interior, all of whose outside directions are domain boundaries (edge_fill), repeats the
// nearest interior column.  Reads what the two kernels above wrote, writes only halo columns.
__global__ void __launch_bounds__(256) hist_halo_kernel(const HistArgs A) {
  const int nlevh = A.nlev + 2 * A.khalo, nlonh = A.nlon + 2 * A.ihalo, nlath = A.nlat + 2 * A.jhalo;
  const long tot = (long)nlonh * nlath * nlevh;
  for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < tot; t += (long)gridDim.x * blockDim.x) {
    const int kh = (int)(t % nlevh);
    const long c = t / nlevh;
    const int ie = (int)(c % nlonh), je = (int)(c / nlonh);
    const int need = (ie < A.ihalo ? 1 : 0) | (ie >= A.ihalo + A.nlon ? 2 : 0) | (je < A.jhalo ? 4 : 0) | (je >= A.jhalo + A.nlat ? 8 : 0);
    if (need == 0 || (need & ~A.edge_fill)) continue;
    const int ci = min(max(ie, A.ihalo), A.ihalo + A.nlon - 1), cj = min(max(je, A.jhalo), A.jhalo + A.nlat - 1);
    const long so = (long)ci * A.s3i + (long)cj * A.s3j + (long)kh * A.s3k, to = (long)ie * A.s3i + (long)je * A.s3j + (long)kh * A.s3k;
    for (int v = 0; v < NV3DD; ++v) A.v3d[to + v * A.s3v] = A.v3d[so + v * A.s3v];
    if (kh == 0)
      for (int v = 0; v < NV2DD; ++v)
        A.v2d[(long)ie * A.s2i + (long)je * A.s2j + v * A.s2v] = A.v2d[(long)ci * A.s2i + (long)cj * A.s2j + v * A.s2v];
  }
}

__global__ void __launch_bounds__(256) monit_gather_kernel(const long nn, const int* __restrict__ key, const int* __restrict__ set,
                                                           const int* __restrict__ idx, const double* __restrict__ rotc,
                                                           int* __restrict__ gset, int* __restrict__ gidx, int* __restrict__ oqc,
                                                           double* __restrict__ grotc) {
  for (long n = (long)blockIdx.x * blockDim.x + threadIdx.x; n < nn; n += (long)gridDim.x * blockDim.x) {
    const long r = key ? (long)key[n] : n;
    gset[n] = r < 0 ? 0 : set[r];                                   // set 0 is outside the files: the row check refuses the call
    gidx[n] = r < 0 ? 0 : idx[r];
    oqc[n] = 0;
    if (rotc) {                                                     // rotc is per obsda row, as set / idx are
      grotc[2 * n] = r < 0 ? 1.0 : rotc[2 * r];
      grotc[2 * n + 1] = r < 0 ? 0.0 : rotc[2 * r + 1];
    }
  }
}

struct FinishArgs {
  int nfile, step, stat_radar;
  long off[LETKF_OBSOPE_MAX_FILES + 1];
  int radar[LETKF_OBSOPE_MAX_FILES];
  const int* elm;
  const double *dat, *dif;
  double t_range;
  long nn;
  const int *gset, *gidx, *oqc;
  const double* val;
  int *w_elm, *w_qc;
  double* w_dep;
  int *r_set, *r_idx, *r_qc;
  double *r_omb, *r_oma;
};

// common_obs_scale.f90:1529-1581 below the operator (the rows passed its check: set / idx are inside the files)
__global__ void __launch_bounds__(256) monit_finish_kernel(const FinishArgs A) {
  for (long n = (long)blockIdx.x * blockDim.x + threadIdx.x; n < A.nn; n += (long)gridDim.x * blockDim.x) {
    const int f = A.gset[n] - 1;
    const long fr = A.off[f] + (A.gidx[n] - 1);
    int qc = -1;
    double dep = kUndef;
    if (A.t_range <= 0.0 || fabs(A.dif[fr]) <= A.t_range) {
      qc = (A.radar[f] >= 0 && !A.stat_radar) ? kQcOtype : A.oqc[n];
      if (qc == 0) dep = A.dat[fr] - A.val[n];
    }
    A.w_elm[n] = A.elm[fr];
    A.w_qc[n] = qc;
    A.w_dep[n] = dep;
    if (A.step == 1) {
      A.r_set[n] = A.gset[n];
      A.r_idx[n] = A.gidx[n];
      A.r_qc[n] = qc;
      A.r_omb[n] = dep;
    } else {
      if (A.r_qc[n] == 0) A.r_qc[n] = qc;                           // the QC value of y_a only if the QC of y_b is good
      A.r_oma[n] = dep;
    }
  }
}

unsigned grid1d(long tot) { return (unsigned)std::min<long>(std::max<long>((tot + 255) / 256, 1), 65536); }
size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

}  // namespace

namespace letkf {

int hist_check(const letkf_hist_state* s, const letkf_obsope_fields* l, const double* v3d, const double* v2d, std::string* msg) {
  auto bad = [&](const char* m) { return *msg = m, LETKF_E_INVALID; };
  if (!s || !l || !v3d || !v2d) return bad("state / layout / v3d / v2d is NULL");
  if (!s->x || !s->topo || !s->cz) return bad("x / topo / cz is NULL");
  if (!s->si || !s->sj || !s->sl || !s->sv) return bad("a stride of the state is zero");
  if (s->nv3d < kNState) return bad("nv3d must be >= 11");
  if (s->edge_fill < 0 || s->edge_fill > 15) return bad("edge_fill must be 0..15");
  if (!std::isfinite(s->ztop) || !(s->ztop > 0.0)) return bad("ztop must be finite and > 0");
  if (l->khalo < 1) return bad("khalo must be >= 1");
  if (l->nlev < 1 || l->nlon < 1 || l->nlat < 1 || l->ihalo < 0 || l->jhalo < 0) return bad("bad grid extents");
  if (l->nv3dd < NV3DD || l->nv2dd < NV2DD) return bad("nv3dd must be >= 13 and nv2dd >= 7");
  if (!l->s3k || !l->s3i || !l->s3j || !l->s3v || !l->s2i || !l->s2j || !l->s2v) return bad("a stride of the layout is zero");
  if (((int64_t)l->nlon * l->nlat + kTilePts - 1) / kTilePts > 0x7fffffff) return bad("more than 2^37 points");
  return LETKF_OK;
}

size_t hist_ws_bytes(const letkf_obsope_fields* l) { return align256((size_t)l->nlev * sizeof(double)); }

hipError_t hist_run(hipStream_t st, const letkf_hist_state* s, const letkf_obsope_fields* l, double* v3d, double* v2d, void* ws) {
  HistArgs A = {};
  A.nlon = l->nlon, A.nlat = l->nlat, A.nlev = l->nlev, A.khalo = l->khalo, A.ihalo = l->ihalo, A.jhalo = l->jhalo;
  A.edge_fill = s->edge_fill;
  A.x = s->x, A.si = s->si, A.sj = s->sj, A.sl = s->sl, A.sv = s->sv;
  A.topo = s->topo, A.cz = static_cast<const double*>(ws), A.ztop = s->ztop;
  A.v3d = v3d, A.s3k = l->s3k, A.s3i = l->s3i, A.s3j = l->s3j, A.s3v = l->s3v;
  A.v2d = v2d, A.s2i = l->s2i, A.s2j = l->s2j, A.s2v = l->s2v;
  hipError_t e = hipMemcpyAsync(ws, s->cz, (size_t)l->nlev * sizeof(double), hipMemcpyHostToDevice, st);
  if (e != hipSuccess) return e;
  const long npt = (long)l->nlon * l->nlat;
  const int nlevh = l->nlev + 2 * l->khalo;
  const dim3 cgrid((unsigned)((npt + kTilePts - 1) / kTilePts), (unsigned)((l->nlev + kTileLev - 1) / kTileLev), NV3DD);
  hipLaunchKernelGGL(hist_copy_kernel, cgrid, dim3(256), 0, st, A);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  hipLaunchKernelGGL(hist_surface_kernel, dim3(grid1d(npt)), dim3(256), 0, st, A);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  if (A.edge_fill && (l->ihalo > 0 || l->jhalo > 0)) {
    const long tot = (long)(l->nlon + 2 * l->ihalo) * (l->nlat + 2 * l->jhalo) * nlevh;
    hipLaunchKernelGGL(hist_halo_kernel, dim3(grid1d(tot)), dim3(256), 0, st, A);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  return hipSuccess;
}

size_t monit_ws_bytes(int64_t nn, size_t stat_bytes) {
  const size_t n = (size_t)std::max<int64_t>(nn, 1);
  return align256(stat_bytes) + 256 + 5 * align256(n * sizeof(int32_t)) + 4 * align256(n * sizeof(double));
}

void monit_ws_layout(void* base, int64_t nn, size_t stat_bytes, MonitWs* w) {
  const size_t n = (size_t)std::max<int64_t>(nn, 1), ai = align256(n * sizeof(int32_t)), ad = align256(n * sizeof(double));
  char* p = static_cast<char*>(base);
  w->stat = p, p += align256(stat_bytes);
  w->flag = reinterpret_cast<int32_t*>(p), p += 256;
  w->val = reinterpret_cast<double*>(p), p += ad;
  w->dep = reinterpret_cast<double*>(p), p += ad;
  w->rotc = reinterpret_cast<double*>(p), p += 2 * ad;
  w->set = reinterpret_cast<int32_t*>(p), p += ai;
  w->idx = reinterpret_cast<int32_t*>(p), p += ai;
  w->oqc = reinterpret_cast<int32_t*>(p), p += ai;
  w->elm = reinterpret_cast<int32_t*>(p), p += ai;
  w->qc = reinterpret_cast<int32_t*>(p);
}

hipError_t monit_gather(hipStream_t st, int64_t nn, const int32_t* key, const int32_t* set, const int32_t* idx, const double* rotc,
                        const MonitWs& w) {
  if (nn <= 0) return hipSuccess;
  hipLaunchKernelGGL(monit_gather_kernel, dim3(grid1d(nn)), dim3(256), 0, st, (long)nn, key, set, idx, rotc, w.set, w.idx, w.oqc,
                     w.rotc);
  return hipGetLastError();
}

hipError_t monit_finish(hipStream_t st, const letkf_monit_params* mp, const letkf_obsope_params* op, const letkf_obs_file_rows* files,
                        int64_t nn, const letkf_obsdep* rec, const MonitWs& w) {
  if (nn <= 0) return hipSuccess;
  FinishArgs A = {};
  A.nfile = files->nfile, A.step = mp->step, A.stat_radar = mp->departure_stat_radar != 0;
  for (int i = 0; i <= files->nfile; ++i) A.off[i] = files->off[i];
  for (int i = 0; i < files->nfile; ++i) A.radar[i] = op->file_radar[i];
  A.elm = files->elm, A.dat = files->dat, A.dif = mp->dif, A.t_range = mp->t_range, A.nn = nn;
  A.gset = w.set, A.gidx = w.idx, A.oqc = w.oqc, A.val = w.val, A.w_elm = w.elm, A.w_qc = w.qc, A.w_dep = w.dep;
  A.r_set = rec->set, A.r_idx = rec->idx, A.r_qc = rec->qc, A.r_omb = rec->omb, A.r_oma = rec->oma;
  hipLaunchKernelGGL(monit_finish_kernel, dim3(grid1d(nn)), dim3(256), 0, st, A);
  return hipGetLastError();
}

}  // namespace letkf
