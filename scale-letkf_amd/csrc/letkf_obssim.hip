// letkf_obssim.hip -- obssim_cal (include/letkf_amd_obssim.h; scale/obs/obsope_tools.f90:1063-1150): the observation operator at
// every interior grid point of nstate model states, and this subdomain's part of write_grd_mpi's records (:1184-1204).
//
// At a grid point the operator has nothing to search and nothing to interpolate: rk = k + KHALO, and the integer coordinates put
// weight 1 on one corner.  So this is a streaming kernel, one lane per point, with the point physics of the row operator
// (letkf_obsope_point_dev.h) behind it:
//   lanes      flattened over (level, column) inside a row j -- the level axis is the fastest axis of the reference layout, so the
//              loads are contiguous up to the halo gap and waves stay full when nlev is no multiple of 64; blockIdx.y is the
//              row, blockIdx.z the state
//   one evaluation per point: the lists are wave-uniform, the entry reduces them to the set of fields they need and to one kind
//              per entry; a point loads each needed field once, runs calc_ref_vr once and serves every entry from that
//   per column the azimuth and com_distll_1's distance of the radar operator come from a kernel in front (16 B per column in the
//              context's scratch buffer): they carry most of the trigonometry and do not depend on the level.  Computed by every
//              lane instead (same expressions, bitwise the same values) the radar lists ran 14 % slower
//   rec        is a transposition (reads level-fastest, records column-fastest) and is stored directly, one float per lane at a
//              stride of a record: turning a block of 1024 points in LDS to store runs of columns was measured 15 % slower
//              (DESIGN.md section 15).  No kernel here uses LDS.
// Compiled without floating-point contraction (Makefile): the staggered sums round as itpl_3d's expressions do.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>

#include "letkf_obsope_point_dev.h"
#include "letkf_obssim_dev.h"

namespace {

using namespace letkf::obsope_point_dev;

// what a list entry stores: one of the values a point evaluates, or undef
enum Kind { K_UNDEF = 0, K_U, K_V, K_T, K_TV, K_Q, K_RH, K_PS, K_REF, K_VR };
// what the lists need of a point
enum Need { N_UV = 1, N_T = 2, N_Q = 4, N_RH = 8, N_PS = 16, N_RADAR = 32 };

struct ObssimArgs {
  int nvar3, nvar2;
  unsigned char kind3[LETKF_OBSSIM_MAX_VARS], kind2[LETKF_OBSSIM_MAX_VARS];
  unsigned need;
  int method, use_tv, stggrd, round_single;
  double rlon, rlat, rz, min_ref, low_dbz, ps_thres, undef;
  const double *lon, *lat, *rotc;
  const double* azd;                              // [nlat][nlon][2] azimuth, distance (< 0: the point is on the radar)
  int nlev, nlon, nlat, khalo, ihalo, jhalo, nlevh, nlonh, nlath;
  const double* v3d;
  long s3k, s3i, s3j, s3v, s3m;
  const double* v2d;
  long s2i, s2j, s2v, s2m;
  double *v3, *v2;
  float* rec;
  long sm3, sm2;
};

struct PointVals {
  double u, v, t, tv, q, rh, ps, ref, vr;
};

__device__ inline double pick(const PointVals& x, const int kind, const double undef) {
  switch (kind) {
    case K_U: return x.u;
    case K_V: return x.v;
    case K_T: return x.t;
    case K_TV: return x.tv;
    case K_Q: return x.q;
    case K_RH: return x.rh;
    case K_PS: return x.ps;
    case K_REF: return x.ref;
    case K_VR: return x.vr;
    default: return undef;
  }
}

// the radar's azimuth and distance at column (i, j); a distance below 0 marks a point on the radar's own lon / lat (qc 98)
__device__ inline void column_angles(const ObssimArgs& A, const long c, double* az, double* dist) {
  const double lon = A.lon[c], lat = A.lat[c];
  const double dlon = lon - A.rlon, dlat = lat - A.rlat;
  if (dlon == 0.0 && dlat == 0.0) {
    *az = 0.0, *dist = -1.0;
  } else {
    *az = radar_azimuth(dlon, dlat, A.rlat);
    *dist = radar_distance(lon, lat, A.rlon, A.rlat);
  }
}

__global__ void __launch_bounds__(256) obssim_angles_kernel(const ObssimArgs A, double* __restrict__ azd) {
  const long c = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= (long)A.nlat * A.nlon) return;
  double az, dist;
  column_angles(A, c, &az, &dist);
  azd[2 * c] = az, azd[2 * c + 1] = dist;
}

// Trans_XtoY / Trans_XtoY_radar at the grid point (k, i, j) of state s (0-based interior indices): every value the lists need,
// undef where its qc is not 0.  A.need is wave-uniform: what no entry asks for is neither loaded nor computed.
__device__ inline void point_values(const ObssimArgs& A, const int s, const int k, const int i, const int j, PointVals* out) {
  const int kk = k + A.khalo, ii = i + A.ihalo, jj = j + A.jhalo;      // 0-based in the arrays with halo; rk = kk + 1, ...
  const double* v3 = A.v3d + (long)s * A.s3m;
  const long p0 = kk * A.s3k + ii * A.s3i + jj * A.s3j;
  const unsigned need = A.need;
  // itpl_3d at integer coordinates: seven corners of weight exactly 0, the eighth of weight 1 -- 0.0 + x, as the sum leaves it
  auto own = [&](int var) { return 0.0 + v3[p0 + var * A.s3v]; };
  PointVals x = {A.undef, A.undef, A.undef, A.undef, A.undef, A.undef, A.undef, A.undef, A.undef};

  double rc1 = 1.0, rc2 = 0.0;
  if (A.rotc && (need & (N_UV | N_RADAR))) {
    const long c = (long)j * A.nlon + i;
    rc1 = A.rotc[2 * c], rc2 = A.rotc[2 * c + 1];
  }
  double tr = 0.0, qv = 0.0, ur = 0.0, vr = 0.0;
  if (need & (N_UV | N_RADAR)) {
    double ut, vt;
    if (A.stggrd == 1) {                                               // U at ri - 0.5, V at rj - 0.5: two terms each
      int i0, i1, j0, j1;
      double ai, aj;
      ceil_split((double)(ii + 1) - 0.5, A.nlonh, &i0, &i1, &ai);
      ceil_split((double)(jj + 1) - 0.5, A.nlath, &j0, &j1, &aj);
      const double* pu = v3 + V_U * A.s3v + kk * A.s3k + jj * A.s3j;
      const double* pv = v3 + V_V * A.s3v + kk * A.s3k + ii * A.s3i;
      ut = 0.0 + term3(pu[i0 * A.s3i], 1.0, 1.0 - ai, 1.0) + term3(pu[i1 * A.s3i], 1.0, ai, 1.0);
      vt = 0.0 + term3(pv[j0 * A.s3j], 1.0, 1.0, 1.0 - aj) + term3(pv[j1 * A.s3j], 1.0, 1.0, aj);
    } else {
      ut = own(V_U), vt = own(V_V);
    }
    ur = ut * rc1 - vt * rc2, vr = ut * rc2 + vt * rc1;
    x.u = ur, x.v = vr;
  }
  if (need & (N_T | N_RADAR)) tr = own(V_T), x.t = tr;
  if (need & N_Q) qv = own(V_Q), x.q = qv;
  if ((need & N_T) && (need & N_Q)) x.tv = tr * (1.0 + kFvirt * qv);
  if (need & N_RH) x.rh = own(V_RH);
  if (need & N_PS) {                                                   // Trans_XtoY's PS with the rk it is given: a level index
    const double* v2 = A.v2d + (long)s * A.s2m + ii * A.s2i + jj * A.s2j;
    const double t = 0.0 + v2[V2_T2M * A.s2v], q = 0.0 + v2[V2_Q2M * A.s2v], topo = 0.0 + v2[V2_TOPO * A.s2v];
    double val = 0.0 + v2[V2_PS * A.s2v];
    const double dz = (double)(kk + 1) - topo;
    if (dz != 0.0) {                                                   // prsadj, common_obs_scale.f90:600-616
      const double gamma = 5.0e-3, tv = t * (1.0 + 0.608 * q);
      val = val * pow((-gamma * dz + tv) / tv, kGg / (gamma * kRd));
    }
    x.ps = fabs(dz) > A.ps_thres ? A.undef : val;                      // qc 10
  }
  if (need & N_RADAR) {
    double wr;
    if (A.stggrd == 1) {                                               // W at rk - 0.5
      int k0, k1;
      double ak;
      ceil_split((double)(kk + 1) - 0.5, A.nlevh, &k0, &k1, &ak);
      const double* pw = v3 + V_W * A.s3v + ii * A.s3i + jj * A.s3j;
      wr = 0.0 + term3(pw[k0 * A.s3k], 1.0 - ak, 1.0, 1.0) + term3(pw[k1 * A.s3k], ak, 1.0, 1.0);
    } else {
      wr = own(V_W);
    }
    const double pr = own(V_P), qrr = own(V_QR), qsr = own(V_QS), qgr = own(V_QG);
    const double lev = v3[p0 + V_HGT * A.s3v];
    const long c = (long)j * A.nlon + i;
    const double az = A.azd[2 * c], dist = A.azd[2 * c + 1];
    if (dist >= 0.0) {                                                 // (else qc 98: both stay undef)
      double ref, rv;
      calc_ref_vr(A.method, A.use_tv, qrr, qsr, qgr, ur, vr, wr, tr, pr, az, radar_elevation(lev, A.rz, dist), &ref, &rv);
      x.ref = ref < A.min_ref ? A.low_dbz : 10.0 * log10(ref);         // qc 11 -> 0, obsope_tools.f90:1108
      x.vr = rv;
    }
  }
  *out = x;
}

__global__ void __launch_bounds__(256) letkf_obssim_kernel(const ObssimArgs A) {
  const int j = blockIdx.y, s = blockIdx.z;
  const int nrow = A.nlev * A.nlon;                                    // points of a row
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= nrow) return;
  const long nrec = (long)A.nvar3 * A.nlev + A.nvar2;
  const int i = t / A.nlev, k = t - i * A.nlev;
  if (A.nvar3 == 0 && k != 0) return;                                  // a 2-D list alone: the lowest level's lanes
  PointVals x;
  point_values(A, s, k, i, j, &x);
  for (int n = 0; n < A.nvar3; ++n) {
    double val = pick(x, A.kind3[n], A.undef);
    if (A.round_single) val = (double)(float)val;
    if (A.v3) A.v3[s * A.sm3 + ((long)n * A.nlat + j) * nrow + t] = val;
    if (A.rec) A.rec[((s * nrec + (long)n * A.nlev + k) * A.nlat + j) * A.nlon + i] = (float)val;
  }
  if (k == 0) {                                                        // the 2-D list: Trans_XtoY at rk = 1 + KHALO, every id
    for (int n = 0; n < A.nvar2; ++n) {
      double val = pick(x, A.kind2[n], A.undef);
      if (A.round_single) val = (double)(float)val;
      if (A.v2) A.v2[s * A.sm2 + ((long)n * A.nlat + j) * A.nlon + i] = val;
      if (A.rec) A.rec[((s * nrec + (long)A.nvar3 * A.nlev + n) * A.nlat + j) * A.nlon + i] = (float)val;
    }
  }
}

// the kind an id stores in the 3-D list (Trans_XtoY_radar for the radar ids, Trans_XtoY else) or in the 2-D list (Trans_XtoY)
int kind_of(int id, bool list3) {
  switch (id) {
    case kIdU: return K_U;
    case kIdV: return K_V;
    case kIdT: return K_T;
    case kIdTv: return K_TV;
    case kIdQ: return K_Q;
    case kIdRh: return K_RH;
    case kIdPs: return K_PS;
    case kIdRadarRef:
    case kIdRadarRefZero: return list3 ? K_REF : K_UNDEF;
    case kIdRadarVr: return list3 ? K_VR : K_UNDEF;
    default: return K_UNDEF;                                           // the pseudo-RH id too: CASE DEFAULT of Trans_XtoY_radar, qc 90
  }
}

unsigned need_of(int kind) {
  switch (kind) {
    case K_U:
    case K_V: return N_UV;
    case K_T: return N_T;
    case K_TV: return N_T | N_Q;
    case K_Q: return N_Q;
    case K_RH: return N_RH;
    case K_PS: return N_PS;
    case K_REF:
    case K_VR: return N_RADAR;
    default: return 0;
  }
}

unsigned need_of_lists(const letkf_obssim_params* p) {
  unsigned need = 0;
  for (int n = 0; n < p->nvar3; ++n) need |= need_of(kind_of(p->vars3[n], true));
  for (int n = 0; n < p->nvar2; ++n) need |= need_of(kind_of(p->vars2[n], false));
  return need;
}

}  // namespace

namespace letkf {

size_t obssim_ws_bytes(const letkf_obssim_params* p, const letkf_obsope_fields* f) {
  if (!(need_of_lists(p) & N_RADAR)) return 0;
  return (size_t)f->nlat * f->nlon * 2 * sizeof(double);
}

hipError_t obssim_run(hipStream_t st, const letkf_obssim_params* p, const letkf_obsope_fields* f, const letkf_obssim_out* o,
                      void* ws) {
  ObssimArgs A = {};
  A.nvar3 = p->nvar3, A.nvar2 = p->nvar2;
  for (int n = 0; n < p->nvar3; ++n) A.kind3[n] = (unsigned char)kind_of(p->vars3[n], true);
  for (int n = 0; n < p->nvar2; ++n) A.kind2[n] = (unsigned char)kind_of(p->vars2[n], false);
  A.need = need_of_lists(p);
  A.method = p->method_ref_calc, A.use_tv = p->use_terminal_velocity != 0, A.stggrd = p->stggrd, A.round_single = p->round_single;
  A.rlon = p->radar_lon, A.rlat = p->radar_lat, A.rz = p->radar_z;
  A.min_ref = pow(10.0, p->min_radar_ref_dbz / 10.0);                  // common_obs_scale.f90:251, on the host as the operator does
  A.low_dbz = p->min_radar_ref_dbz + p->low_ref_shift;
  A.ps_thres = p->ps_adjust_thres;
  A.undef = p->round_single ? (double)(float)kUndef : kUndef;
  A.lon = p->lon, A.lat = p->lat, A.rotc = p->rotc;
  A.nlev = f->nlev, A.nlon = f->nlon, A.nlat = f->nlat, A.khalo = f->khalo, A.ihalo = f->ihalo, A.jhalo = f->jhalo;
  A.nlevh = f->nlev + 2 * f->khalo, A.nlonh = f->nlon + 2 * f->ihalo, A.nlath = f->nlat + 2 * f->jhalo;
  A.v3d = f->v3d, A.s3k = f->s3k, A.s3i = f->s3i, A.s3j = f->s3j, A.s3v = f->s3v, A.s3m = f->s3m;
  A.v2d = f->v2d, A.s2i = f->s2i, A.s2j = f->s2j, A.s2v = f->s2v, A.s2m = f->s2m;
  A.v3 = o->v3, A.v2 = o->v2, A.rec = o->rec, A.sm3 = o->sm3, A.sm2 = o->sm2;

  if (A.need & N_RADAR) {
    const long ncol = (long)f->nlat * f->nlon;
    hipLaunchKernelGGL(obssim_angles_kernel, dim3((unsigned)((ncol + 255) / 256)), dim3(256), 0, st, A, static_cast<double*>(ws));
    if (hipError_t e = hipGetLastError()) return e;
    A.azd = static_cast<const double*>(ws);
  }
  const long nrow = (long)f->nlev * f->nlon;
  const dim3 grid((unsigned)((nrow + 255) / 256), (unsigned)f->nlat, (unsigned)f->nmem);
  hipLaunchKernelGGL(letkf_obssim_kernel, grid, dim3(256), 0, st, A);
  return hipGetLastError();
}

}  // namespace letkf
