// letkf_obsope.hip -- the observation operator of obsope_cal (include/letkf_amd_obsope.h; scale/obs/obsope_tools.f90:454-507 and
// scale/common/common_obs_scale.f90) for nmem members in one launch.  A wave takes 64 (obsda row, member) pairs:
//   stage 1  vertical index   lanes are levels (chunks of 64): each lane forms plev(k) / zlev(k) from the four corner columns,
//                             ballots give the lowest valid level ks and the first crossing in scan order
//   stage 2  corner gather    lanes are (variable 0..15) x (column 0..3): two adjacent levels per lane, three weights, the four
//                             column lanes of a variable summed through DPP in a fixed order
//   stage 3  point physics    Trans_XtoY / Trans_XtoY_radar / calc_ref_vr, one lane per pair, once the wave has taken its 64
//                             pairs through stages 1 and 2 (the whole wave works on one pair at a time there)
// The unit is compiled without floating-point contraction (Makefile): the interpolations then round as the reference's
// expressions do, term by term.  A corner of weight exactly 0 never contributes and no index leaves the arrays (header:
// "where the reference is undefined").  Real literals the reference writes without a kind are widened from single precision (F).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <string>

#include "letkf_obsope_dev.h"
#include "letkf_obsope_point_dev.h"

namespace {

using namespace letkf::obsope_point_dev;   // ids, constants, ceil_split, term2 / term3, the radar angles, calc_ref_vr

struct ObsopeArgs {
  // files and rows
  int nfile;
  long off[LETKF_OBSOPE_MAX_FILES + 1];
  int radar[LETKF_OBSOPE_MAX_FILES];              // -1 conventional, else radar format
  double meta[LETKF_OBSOPE_MAX_FILES][3];         // the file's radar: lon, lat, z
  const int *elm, *typ;
  const double *lev, *ri, *rj, *lon, *lat, *rotc;
  const int *set, *idx;
  unsigned use_mask;                              // bit typ-1 = USE_OBS(typ)
  int nobtype, method, use_tv, stggrd;
  int keep_ref_low;                               // obsmake_cal's mode: qc 11 stays (obsope_tools.f90:864-884 has no :488)
  double min_ref, low_dbz, radar_zmax, ps_thres, ri_off, rj_off;
  // fields
  int nlev, khalo, nlevh, nlonh, nlath, nmem, m0;
  const double* v3d;
  long s3k, s3i, s3j, s3v, s3m;
  const double* v2d;
  long s2i, s2j, s2v, s2m;
  // outputs
  long row0, nrows, kld;
  const long* nrows_dev;                          // NULL, or the device's own row count (<= nrows, which then bounds the grid)
  int* qc;
  double* ensval;
};

// the rows of this call: nrows, or where the caller compacted them on the device the count it left there (wave-uniform)
__device__ inline long rows_of(const ObsopeArgs& A) { return A.nrows_dev ? min(A.nrows, *A.nrows_dev) : A.nrows; }

// set / idx outside the files, or a report type outside 1..nobtype
__global__ void __launch_bounds__(256) obsope_rows_check_kernel(const ObsopeArgs A, int* __restrict__ bad) {
  const long nrows = rows_of(A);
  for (long n = (long)blockIdx.x * blockDim.x + threadIdx.x; n < nrows; n += (long)gridDim.x * blockDim.x) {
    const int f = A.set[A.row0 + n] - 1;
    const long i = (long)A.idx[A.row0 + n] - 1;
    bool ok = f >= 0 && f < A.nfile;
    if (ok) ok = i >= 0 && i < A.off[f + 1] - A.off[f];
    if (ok) {
      const int t = A.typ[A.off[f] + i];
      ok = t >= 1 && t <= A.nobtype;
    }
    if (!ok) atomicOr(bad, 1);
  }
}

__device__ inline double rdlane(double x, int l) {   // l wave-uniform
  const int lo = __builtin_amdgcn_readlane(__double2loint(x), l), hi = __builtin_amdgcn_readlane(__double2hiint(x), l);
  return __hiloint2double(hi, lo);
}

template <int CTRL>
__device__ inline double quad_perm(double x) {
  const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(x), CTRL, 0xf, 0xf, false);
  const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(x), CTRL, 0xf, 0xf, false);
  return __hiloint2double(hi, lo);
}

// The file row behind an obsda row, as every stage reads it
struct TaskRow {
  long r, fr;
  int m, f, elm, typ;
  double lev, ril, rjl;
  bool is_radar;
};

__device__ inline TaskRow task_row(const ObsopeArgs& A, const long task) {
  TaskRow t;
  t.r = A.row0 + task / A.nmem;
  t.m = (int)(task % A.nmem);
  t.f = A.set[t.r] - 1;
  t.fr = A.off[t.f] + (A.idx[t.r] - 1);               // (the rows were checked before the launch)
  t.elm = A.elm[t.fr], t.typ = A.typ[t.fr];
  t.lev = A.lev[t.fr];
  t.ril = A.ri[t.fr] - A.ri_off, t.rjl = A.rj[t.fr] - A.rj_off;
  t.is_radar = A.radar[t.f] >= 0;
  return t;
}

// Stages 1 and 2 of one task, by the whole wave (task is wave-uniform): qc and rk of the coordinate search, and in lane 4 v the
// interpolated variable v (PS rows: t2m, q2m, topo, ps in lanes 0, 4, 8, 12)
__device__ inline void stages_1_2(const ObsopeArgs& A, const long task, const int lane, int* qc_out, double* rk_out, double* s_out) {
  const TaskRow R = task_row(A, task);
  const int m = R.m, elm = R.elm, typ = R.typ;
  const double lev = R.lev, ril = R.ril, rjl = R.rjl;
  const bool is_radar = R.is_radar;
  const double* v3 = A.v3d + (long)m * A.s3m;

  int qc = 0;
  double rk = 0.0, s = 0.0;

  if (!((A.use_mask >> (typ - 1)) & 1u)) {
    qc = kQcOtype;
  } else if (is_radar && lev > A.radar_zmax) {
    qc = kQcRadarVhi;
  } else if (!(ril >= 1.0 && ril <= (double)A.nlonh && rjl >= 1.0 && rjl <= (double)A.nlath)) {
    qc = kQcOutH;
  } else if (!is_radar && elm > 9999) {
    rk = lev;                                                       // surface observation
  } else {
    // ---- stage 1: phys2ijk / phys2ijkz.  0-based level kk = kb + 64 c + lane, kb .. ktop the model levels
    int i0, i1, j0, j1;
    double ai, aj;
    ceil_split(ril, A.nlonh, &i0, &i1, &ai);
    ceil_split(rjl, A.nlath, &j0, &j1, &aj);
    const double* col = v3 + (long)(is_radar ? V_HGT : V_P) * A.s3v;
    const long cb0 = i0 * A.s3i + j0 * A.s3j, cb1 = i1 * A.s3i + j0 * A.s3j, cb2 = i0 * A.s3i + j1 * A.s3j,
               cb3 = i1 * A.s3i + j1 * A.s3j;
    const int kb = A.khalo, ktop = A.khalo + A.nlev - 1;
    const int nchunk = (A.nlev + 63) >> 6;
    const double tl = is_radar ? lev : log(lev);
    // pass A: the lowest valid level of every column; chunk 0's values stay in registers for pass B
    double c00 = 0.0, c01 = 0.0, c02 = 0.0, c03 = 0.0;
    int first0 = ktop + 1, first1 = ktop + 1, first2 = ktop + 1, first3 = ktop + 1;
    for (int c = 0; c < nchunk; ++c) {
      const int kk = kb + c * 64 + lane;
      const bool inr = kk <= ktop;
      const long ko = (long)min(kk, ktop) * A.s3k;
      const double x0 = col[cb0 + ko], x1 = col[cb1 + ko], x2 = col[cb2 + ko], x3 = col[cb3 + ko];
      if (c == 0) c00 = x0, c01 = x1, c02 = x2, c03 = x3;
      const unsigned long long b0 = __ballot(inr && (is_radar ? (x0 > -300.0 && x0 < 10000.0) : (x0 >= 0.0)));
      const unsigned long long b1 = __ballot(inr && (is_radar ? (x1 > -300.0 && x1 < 10000.0) : (x1 >= 0.0)));
      const unsigned long long b2 = __ballot(inr && (is_radar ? (x2 > -300.0 && x2 < 10000.0) : (x2 >= 0.0)));
      const unsigned long long b3 = __ballot(inr && (is_radar ? (x3 > -300.0 && x3 < 10000.0) : (x3 >= 0.0)));
      if (first0 > ktop && b0) first0 = kb + c * 64 + __ffsll((long long)b0) - 1;
      if (first1 > ktop && b1) first1 = kb + c * 64 + __ffsll((long long)b1) - 1;
      if (first2 > ktop && b2) first2 = kb + c * 64 + __ffsll((long long)b2) - 1;
      if (first3 > ktop && b3) first3 = kb + c * 64 + __ffsll((long long)b3) - 1;
    }
    const int ks = __builtin_amdgcn_readfirstlane(max(max(first0, first1), max(first2, first3)));
    if (ks > ktop) {
      qc = kQcOutVlo;                                               // a corner column without a valid level
    } else {
      // pass B: plev(k) per lane, its values at the top and at ks, the first crossing above ks in scan order
      const double wa0 = 1.0 - ai, wb0 = 1.0 - aj;
      bool found = false;
      int kx = 0;
      double pl_k = 0.0, pl_km1 = 0.0, prev_last = 0.0, p_top = 0.0, p_ks = 0.0;
      for (int c = 0; c < nchunk; ++c) {
        const int base = kb + c * 64;
        const int kk = base + lane;
        const bool inr = kk <= ktop;
        double x0, x1, x2, x3;
        if (c == 0) {
          x0 = c00, x1 = c01, x2 = c02, x3 = c03;
        } else {
          const long ko = (long)min(kk, ktop) * A.s3k;
          x0 = col[cb0 + ko], x1 = col[cb1 + ko], x2 = col[cb2 + ko], x3 = col[cb3 + ko];
        }
        if (!is_radar) x0 = log(x0), x1 = log(x1), x2 = log(x2), x3 = log(x3);
        const double plv = term2(x0, wa0, wb0) + term2(x1, ai, wb0) + term2(x2, wa0, aj) + term2(x3, ai, aj);
        if (ktop >= base && ktop < base + 64) p_top = rdlane(plv, ktop - base);
        if (ks >= base && ks < base + 64) p_ks = rdlane(plv, ks - base);
        const unsigned long long b = __ballot(inr && kk > ks && (is_radar ? plv > tl : plv < tl));
        if (!found && b) {
          const int l = __builtin_amdgcn_readfirstlane(__ffsll((long long)b) - 1);
          found = true;
          kx = base + l;
          pl_k = rdlane(plv, l);
          pl_km1 = l > 0 ? rdlane(plv, l - 1) : prev_last;
        }
        prev_last = rdlane(plv, 63);
      }
      if (is_radar ? tl > p_top : tl < p_top) {
        qc = kQcOutVhi;
      } else if (is_radar ? tl < p_ks : tl > p_ks) {
        qc = kQcOutVlo;
      } else if (!found) {
        rk = (double)(ktop + 1);                                    // on the top level itself
      } else {
        rk = (double)kx + (tl - pl_km1) / (pl_k - pl_km1);          // REAL(k - 1) + ak, k = kx + 1
      }
    }
  }

  if (qc == 0) {
    // ---- stage 2: the corner gather.  lane = 4 * variable + column; column bit 0: i, bit 1: j
    const int var = lane >> 2, cc = lane & 3;
    const bool is_ps = !is_radar && elm == kIdPs;
    unsigned vmask;                                                  // the variables Trans_XtoY* interpolates
    if (is_radar) vmask = 0x7ffu;
    else if (elm == kIdU || elm == kIdV) vmask = (1u << V_U) | (1u << V_V);
    else if (elm == kIdT) vmask = 1u << V_T;
    else if (elm == kIdTv) vmask = (1u << V_T) | (1u << V_Q);
    else if (elm == kIdQ) vmask = 1u << V_Q;
    else if (elm == kIdRh) vmask = 1u << V_RH;
    else if (is_ps) vmask = 0xfu;                                    // t2m, q2m, topo, ps
    else vmask = 0u;
    if ((vmask >> var) & 1u) {
      double ri_v = ril, rj_v = rjl, rk_v = rk;
      if (A.stggrd == 1 && !is_ps) {
        if (var == V_U) ri_v -= 0.5;
        if (var == V_V) rj_v -= 0.5;
        if (var == V_W) rk_v -= 0.5;                                 // (W is gathered by the radar operator only)
      }
      int i0, i1, j0, j1;
      double ai, aj;
      ceil_split(ri_v, A.nlonh, &i0, &i1, &ai);
      ceil_split(rj_v, A.nlath, &j0, &j1, &aj);
      const int ii = (cc & 1) ? i1 : i0, jj = (cc & 2) ? j1 : j0;
      const double wi = (cc & 1) ? ai : 1.0 - ai, wj = (cc & 2) ? aj : 1.0 - aj;
      if (is_ps) {
        const int v2 = var == 0 ? V2_T2M : var == 1 ? V2_Q2M : var == 2 ? V2_TOPO : V2_PS;
        const double x = A.v2d[(long)m * A.s2m + (long)v2 * A.s2v + ii * A.s2i + jj * A.s2j];
        s = term2(x, wi, wj);
      } else {
        int k0, k1;
        double ak;
        ceil_split(rk_v, A.nlevh, &k0, &k1, &ak);
        const double* pv = v3 + (long)var * A.s3v + ii * A.s3i + jj * A.s3j;
        const double x0 = pv[k0 * A.s3k], x1 = pv[k1 * A.s3k];
        s = term3(x0, 1.0 - ak, wi, wj) + term3(x1, ak, wi, wj);
      }
    }
    s = s + quad_perm<0xB1>(s);                                      // lanes 0+1 | 2+3 of every quad
    s = s + quad_perm<0x4E>(s);                                      // (0+1) + (2+3)
  }
  *qc_out = qc, *rk_out = rk, *s_out = s;
}

// Stage 3 of one task, by one lane: Trans_XtoY / Trans_XtoY_radar below their interpolations, x[v] the interpolated variable v
__device__ inline void stage_3(const ObsopeArgs& A, const long task, int qc, const double rk, const double (&x)[12]) {
  const TaskRow R = task_row(A, task);
  const long r = R.r, fr = R.fr;
  const int m = R.m, f = R.f, elm = R.elm;
  const double lev = R.lev;
  const bool is_radar = R.is_radar, is_ps = !is_radar && elm == kIdPs;
  double val = 0.0;
  if (qc == 0) {
    double rc1 = 1.0, rc2 = 0.0;
    if (A.rotc) rc1 = A.rotc[2 * r], rc2 = A.rotc[2 * r + 1];
    if (!is_radar) {
      if (elm == kIdU || elm == kIdV) {
        const double u = x[V_U], v = x[V_V];
        val = elm == kIdU ? u * rc1 - v * rc2 : u * rc2 + v * rc1;
      } else if (elm == kIdT) {
        val = x[V_T];
      } else if (elm == kIdTv) {
        val = x[V_T] * (1.0 + kFvirt * x[V_Q]);
      } else if (elm == kIdQ) {
        val = x[V_Q];
      } else if (elm == kIdRh) {
        val = x[V_RH];
      } else if (is_ps) {
        const double t = x[0], q = x[1], topo = x[2];
        val = x[3];
        const double dz = rk - topo;
        if (dz != 0.0) {                                             // prsadj, :600-616
          const double gamma = 5.0e-3, tv = t * (1.0 + 0.608 * q);
          val = val * pow((-gamma * dz + tv) / tv, kGg / (gamma * kRd));
        }
        if (fabs(dz) > A.ps_thres) qc = kQcPsTer;
      } else {
        val = kUndef;
        qc = kQcOtype;
      }
    } else {
      const double ut = x[V_U], vt = x[V_V], wr = x[V_W], tr = x[V_T],
                   pr = x[V_P], qrr = x[V_QR], qsr = x[V_QS], qgr = x[V_QG];
      const double ur = ut * rc1 - vt * rc2, vr = ut * rc2 + vt * rc1;
      const double lon = A.lon[fr], lat = A.lat[fr];
      const double rlon = A.meta[f][0], rlat = A.meta[f][1], rz = A.meta[f][2];
      const double dlon = lon - rlon, dlat = lat - rlat;
      val = kUndef;
      if (dlon == 0.0 && dlat == 0.0) {
        qc = kQcOutH;
      } else {
        const double az = radar_azimuth(dlon, dlat, rlat);
        const double elev = radar_elevation(lev, rz, radar_distance(lon, lat, rlon, rlat));
        double ref, rv;
        calc_ref_vr(A.method, A.use_tv, qrr, qsr, qgr, ur, vr, wr, tr, pr, az, elev, &ref, &rv);
        if (elm == kIdRadarRef || elm == kIdRadarRefZero) {
          if (ref < A.min_ref) {
            qc = kQcRefLow;
            val = A.low_dbz;
          } else {
            val = 10.0 * log10(ref);
          }
        } else if (elm == kIdRadarVr) {
          if (ref < A.min_ref) qc = kQcRefLow;
          val = rv;
        } else {
          qc = kQcOtype;
        }
        if (qc == kQcRefLow && !A.keep_ref_low) qc = 0;              // obsope_tools.f90:488
      }
    }
  }
  A.ensval[r * A.kld + A.m0 + m] = val;
  if (qc > 0) atomicMax(&A.qc[r], qc);
}

// One wave takes 64 consecutive (row, member) pairs: stages 1 and 2 pair by pair with the whole wave, lane t keeping pair t's
// interpolated values in registers; then stage 3 once, one lane per pair.
__global__ void __launch_bounds__(256) letkf_obsope_kernel(const ObsopeArgs A) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const long base = ((long)blockIdx.x * 4 + wave) * 64, ntask = rows_of(A) * A.nmem;
  if (base >= ntask) return;
  const int cnt = (int)(ntask - base < 64 ? ntask - base : 64);
  int my_qc = 0;
  double my_rk = 0.0, x[12] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int t = 0; t < cnt; ++t) {
    int qc;
    double rk, s;
    stages_1_2(A, base + t, lane, &qc, &rk, &s);
    const bool mine = lane == t;
#pragma unroll
    for (int v = 0; v < 12; ++v) {
      const double sv = rdlane(s, 4 * v);
      if (mine) x[v] = sv;
    }
    if (mine) my_qc = qc, my_rk = rk;
  }
  if (lane < cnt) stage_3(A, base + lane, my_qc, my_rk, x);
}

}  // namespace

namespace letkf {

int obsope_check(const letkf_obsope_params* p, const letkf_obs_file_rows* files, const letkf_obsope_fields* f, int64_t row0,
                 int64_t nrows, const int32_t* set, const int32_t* idx, const int32_t* qc, const double* ensval, int64_t kld,
                 std::string* msg) {
  auto bad = [&](const char* m) { return *msg = m, LETKF_E_INVALID; };
  if (!p || !files || !f) return bad("params / files / fields is NULL");
  if (row0 < 0 || nrows < 0) return bad("row0 / nrows is negative");
  if (!set || !idx || !qc || !ensval) return bad("set / idx / qc / ensval is NULL");
  if (f->nmem < 1) return bad("nmem must be >= 1");
  if (f->m0 < 0 || (int64_t)f->m0 + f->nmem > kld) return bad("m0 + nmem must be <= kld");
  if (f->khalo < 1) return bad("khalo must be >= 1");
  if (f->nlev < 1 || f->nlon < 1 || f->nlat < 1 || f->ihalo < 0 || f->jhalo < 0) return bad("bad grid extents");
  if (f->nv3dd < 13 || f->nv2dd < 7) return bad("nv3dd must be >= 13 and nv2dd >= 7");
  if (!f->v3d || !f->v2d) return bad("v3d / v2d is NULL");
  if (!f->s3k || !f->s3i || !f->s3j || !f->s3v || !f->s3m || !f->s2i || !f->s2j || !f->s2v || !f->s2m) return bad("a stride is zero");
  if (p->method_ref_calc < 1 || p->method_ref_calc > 3) return bad("method_ref_calc must be 1..3");
  if (p->nobtype < 1 || p->nobtype > 32 || !p->use_obs) return bad("nobtype must be 1..32 and use_obs given");
  if (files->nfile < 1 || files->nfile > LETKF_OBSOPE_MAX_FILES || !files->off) return bad("nfile must be 1..16 and off given");
  if (!p->file_radar) return bad("file_radar is NULL");
  for (int i = 0; i < files->nfile; ++i) {
    if (files->off[i + 1] < files->off[i]) return bad("file offsets must ascend");
    if (p->file_radar[i] < -1) return bad("file_radar must be -1 or a radar_meta row");
    if (p->file_radar[i] >= 0 && !p->radar_meta) return bad("a radar file needs radar_meta");
  }
  if (files->off[files->nfile] > 0 && (!files->elm || !files->typ || !files->lev || !files->ri || !files->rj || !p->lon || !p->lat))
    return bad("a file row array is NULL (elm, typ, lev, ri, rj, lon, lat)");
  return LETKF_OK;
}

int obsope_run(hipStream_t st, const letkf_obsope_params* p, const letkf_obs_file_rows* files, const letkf_obsope_fields* f,
               int64_t row0, int64_t nrows, const int32_t* set, const int32_t* idx, int32_t* qc, double* ensval, int64_t kld,
               int32_t* flag, std::string* msg, bool keep_ref_low, const int64_t* nrows_dev) {
  if (nrows == 0) return LETKF_OK;
  ObsopeArgs A = {};
  A.nfile = files->nfile;
  for (int i = 0; i <= files->nfile; ++i) A.off[i] = files->off[i];
  for (int i = 0; i < files->nfile; ++i) {
    A.radar[i] = p->file_radar[i];
    if (A.radar[i] >= 0)
      for (int c = 0; c < 3; ++c) A.meta[i][c] = p->radar_meta[3 * (long)A.radar[i] + c];
  }
  A.elm = files->elm, A.typ = files->typ, A.lev = files->lev, A.ri = files->ri, A.rj = files->rj;
  A.lon = p->lon, A.lat = p->lat, A.rotc = p->rotc, A.set = set, A.idx = idx;
  for (int t = 0; t < p->nobtype; ++t)
    if (p->use_obs[t]) A.use_mask |= 1u << t;
  A.nobtype = p->nobtype, A.method = p->method_ref_calc, A.use_tv = p->use_terminal_velocity != 0, A.stggrd = p->stggrd;
  A.min_ref = pow(10.0, p->min_radar_ref_dbz / 10.0);                // common_obs_scale.f90:251, on the host as letkf_setobs does
  A.low_dbz = p->min_radar_ref_dbz + p->low_ref_shift;
  A.radar_zmax = p->radar_zmax, A.ps_thres = p->ps_adjust_thres, A.ri_off = p->ri_off, A.rj_off = p->rj_off;
  A.nlev = f->nlev, A.khalo = f->khalo, A.nlevh = f->nlev + 2 * f->khalo, A.nlonh = f->nlon + 2 * f->ihalo,
  A.nlath = f->nlat + 2 * f->jhalo, A.nmem = f->nmem, A.m0 = f->m0;
  A.v3d = f->v3d, A.s3k = f->s3k, A.s3i = f->s3i, A.s3j = f->s3j, A.s3v = f->s3v, A.s3m = f->s3m;
  A.v2d = f->v2d, A.s2i = f->s2i, A.s2j = f->s2j, A.s2v = f->s2v, A.s2m = f->s2m;
  A.row0 = row0, A.nrows = nrows, A.kld = kld, A.qc = qc, A.ensval = ensval;
  static_assert(sizeof(long) == sizeof(int64_t), "the device count is read as long");
  A.nrows_dev = reinterpret_cast<const long*>(nrows_dev);
  if (keep_ref_low) {                                                // obsmake_cal: no USE_OBS test, no RADAR_ZMAX test
    A.keep_ref_low = 1;
    A.use_mask = 0xffffffffu;
    A.radar_zmax = INFINITY;
  }
  const int64_t ntask = nrows * (int64_t)f->nmem;
  if ((ntask + 255) / 256 > 0x7fffffff) return *msg = "more than 2^39 (row, member) pairs in one call", LETKF_E_INVALID;

  auto hip = [&](hipError_t e, const char* what) {
    if (e == hipSuccess) return false;
    *msg = std::string(what) + ": " + hipGetErrorString(e);
    return true;
  };
  if (hip(hipMemsetAsync(flag, 0, sizeof(int32_t), st), "hipMemsetAsync")) return LETKF_E_HIP;
  const unsigned cgrid = (unsigned)std::min<int64_t>((nrows + 255) / 256, 4096);
  hipLaunchKernelGGL(obsope_rows_check_kernel, dim3(cgrid), dim3(256), 0, st, A, flag);
  if (hip(hipGetLastError(), "obsope_rows_check_kernel")) return LETKF_E_HIP;
  int32_t h_flag = 0;
  if (hip(hipMemcpyAsync(&h_flag, flag, sizeof(int32_t), hipMemcpyDeviceToHost, st), "hipMemcpyAsync")) return LETKF_E_HIP;
  if (hip(hipStreamSynchronize(st), "hipStreamSynchronize")) return LETKF_E_HIP;
  if (h_flag) return *msg = "an obsda row names a file row outside the files (set / idx) or a report type outside 1..nobtype", LETKF_E_INVALID;

  hipLaunchKernelGGL(letkf_obsope_kernel, dim3((unsigned)((ntask + 255) / 256)), dim3(256), 0, st, A);
  if (hip(hipGetLastError(), "letkf_obsope_kernel")) return LETKF_E_HIP;
  return LETKF_OK;
}

}  // namespace letkf
