// letkf_obsope_point_dev.h -- the point physics of the observation operator as every kernel that evaluates H(x) at a point uses
// it: letkf_obsope.hip (the row operator of obsope_cal / monit_obs / obsmake_cal) and letkf_obssim.hip (obssim_cal, every grid
// point).  The element ids and qc values, the constants, the interpolation terms, the radar's azimuth / distance / elevation and
// calc_ref_vr exist once, here.  Units that include it are compiled without floating-point contraction (Makefile): the sums
// then round as the reference's expressions do, term by term.  Real literals the reference writes without a kind are widened
// from single precision (F, undefined again at the end of this header).
#pragma once
#include <hip/hip_runtime.h>

namespace letkf {
namespace obsope_point_dev {

#define F(x) ((double)x##f)

constexpr int kIdU = 2819, kIdV = 2820, kIdT = 3073, kIdTv = 3074, kIdQ = 3330, kIdRh = 3331, kIdPs = 14593,
              kIdRadarRef = 4001, kIdRadarRefZero = 4004, kIdRadarVr = 4002;                       // common_obs_scale.f90:48-67
constexpr int kQcPsTer = 10, kQcRefLow = 11, kQcRadarVhi = 19, kQcOutVhi = 20, kQcOutVlo = 21, kQcOtype = 90, kQcOutH = 98;   // :139-151
constexpr double kPi = 3.1415926535, kGg = 9.81, kRd = 287.05, kRv = 461.50, kRe = 6371.3e3, kUndef = -9.99e33;   // common.f90:28-38
constexpr double kFvirt = kRv / kRd - 1.0, kDeg2Rad = kPi / 180.0, kRad2Deg = 180.0 / kPi;
// com_gamma(4.8), (4.25), (4.5) (common.f90:861-912), the only arguments calc_ref_vr passes
constexpr double kGamma48 = 17.8378619818136, kGamma425 = 8.28508514183522, kGamma45 = 11.631728396567446;
// iv3dd_* - 1 (common_scale.f90:66-85): the gather's variable slots 0..11 are these, hgt (12) is stage 1's
enum { V_U = 0, V_V, V_W, V_T, V_P, V_Q, V_QC, V_QR, V_QI, V_QS, V_QG, V_RH, V_HGT };
enum { V2_TOPO = 0, V2_PS = 1, V2_T2M = 5, V2_Q2M = 6 };

// CEILING(r), the weight of the upper index and the two 0-based indices, clamped into [0, n - 1]
__device__ inline void ceil_split(double r, int n, int* lo, int* hi, double* a) {
  const int c = (int)ceil(r);
  *a = r - (double)(c - 1);
  *lo = min(max(c - 2, 0), n - 1);
  *hi = min(max(c - 1, 0), n - 1);
}

// one term of the reference's interpolation sums, v * w1 * w2 [* w3] left to right; a factor of exactly 0 drops the term
__device__ inline double term2(double v, double w1, double w2) { return (w1 != 0.0 && w2 != 0.0) ? v * w1 * w2 : 0.0; }
__device__ inline double term3(double v, double w1, double w2, double w3) {
  return (w1 != 0.0 && w2 != 0.0 && w3 != 0.0) ? v * w1 * w2 * w3 : 0.0;
}

// Trans_XtoY_radar's angles in degrees (common_obs_scale.f90:408-425).  The azimuth [0, 360) and com_distll_1's distance
// (common/common.f90:401-424) depend on the horizontal position only, the elevation on the height as well: a kernel that walks a
// column takes the first two once.
__device__ inline double radar_azimuth(double dlon, double dlat, double rlat) {
  double az = kRad2Deg * atan2(dlon * cos(rlat * kDeg2Rad), dlat);
  if (az < 0.0) az = 360.0 + az;
  return az;
}
__device__ inline double radar_distance(double lon, double lat, double rlon, double rlat) {
  const double r180 = 1.0 / 180.0;
  const double lon1 = lon * kPi * r180, lon2 = rlon * kPi * r180, lat1 = lat * kPi * r180, lat2 = rlat * kPi * r180;
  double cosd = sin(lat1) * sin(lat2) + cos(lat1) * cos(lat2) * cos(lon2 - lon1);
  cosd = fmax(-1.0, fmin(1.0, cosd));
  return acos(cosd) * kRe;
}
__device__ inline double radar_elevation(double lev, double rz, double dist) { return kRad2Deg * atan2(lev - rz, dist); }

// calc_ref_vr, common_obs_scale.f90:626-990
__device__ inline void calc_ref_vr(int method, int use_tv, double qr, double qs, double qg, double u, double v, double w,
                                   double t, double p, double az, double elev, double* ref_out, double* vr_out) {
  double zr = 0.0, zs = 0.0, zg = 0.0, zms = 0.0, zmg = 0.0, ref = 0.0, wt = 0.0;
  double ro = p / (kRd * t);
  const double pip = pow(kPi, 1.75);
  if (method == 1) {
    const double nor = 8.0e6, ror = 1000.0, cf = 10.0e18 * 72, p0 = 1.0e5;
    const double qt = qr + qs + qg;
    if (qt > 0.0) {
      ref = cf * pow(ro * qt, 1.75);
      ref = ref / (pip * pow(nor, 0.75) * pow(ror, 1.75));
      const double a = pow(p0 / p, F(0.4));
      wt = 5.40 * a * pow(qt, 0.125);
    }
  } else if (method == 2) {
    double nor = 8.0e6, nos = 3.0e6, nog = 4.0e4, ror = 1000.0, ros = 100.0, rog = 913.0, roo = 1.0;
    const double roi = 917.0, ki2 = 0.176, kr2 = 0.930, cf = 1.0e18 * 720;
    if (qr > 0.0) {
      zr = cf * pow(ro * qr, 1.75);
      zr = zr / (pip * pow(nor, 0.75) * pow(ror, 1.75));
    }
    if (qs > 0.0) {
      if (t <= F(273.16)) {
        zs = cf * ki2 * pow(ros, 0.25) * pow(ro * qs, 1.75);
        zs = zs / (pip * kr2 * pow(nos, 0.75) * (roi * roi));
      } else {
        zs = cf * pow(ro * qs, 1.75);
        zs = zs / (pip * pow(nos, 0.75) * pow(roi, 1.75));
      }
    }
    if (qg > 0.0) {
      zg = pow(cf / (pip * pow(nog, 0.75) * pow(rog, 1.75)), F(0.95));
      zg = zg * pow(ro * qg, F(1.6625));
    }
    ref = zr + zs + zg;
    if (ref > 0.0) {
      nor = nor * F(1e-3);
      nos = nos * F(1e-3);
      nog = nog * F(1e-3);
      ror = ror * F(1e-3);
      ros = ros * F(1e-3);
      rog = rog * F(1e-3);
      roo = roo * F(1e-3);
      ro = ro * F(1e-3);
      const double a = 2115.0, b = 0.8, c = 152.93, d = 0.25, Cd = 0.6;
      const double rofactor = pow(roo / ro, 0.25);
      double wr = 0.0, ws = 0.0, wg = 0.0;
      if (qr > 0.0) {
        const double lr = pow(kPi * ror * nor / (ro * qr), 0.25);
        wr = a * kGamma48 / (6.0 * pow(lr, b));
        wr = 1.0e-2 * wr * rofactor;
      }
      if (qs > 0.0) {
        const double ls = pow(kPi * ros * nos / (ro * qs), 0.25);
        ws = c * kGamma425 / (6.0 * pow(ls, d));
        ws = 1.0e-2 * ws * rofactor;
      }
      if (qg > 0.0) {
        const double lg = pow(kPi * rog * nog / (ro * qg), 0.25);
        wg = kGamma45 * pow((4.0 * kGg * 100.0 * rog) / (3.0 * Cd * ro), 0.5);
        wg = 1.0e-2 * wg / (6.0 * pow(lg, 0.5));
      }
      wt = (wr * zr + ws * zs + wg * zg) / (zr + zs + zg);
    }
  } else {
    const double maxf = 0.5;
    double Fg = 0.0, Fs = 0.0, fwg = 0.0, fws = 0.0;
    if (qr > 0.0 && qg > 0.0) {
      Fg = maxf * pow(fmin(qr / qg, qg / qr), 1.0 / 3.0);
      fwg = qr / (qr + qg);
    }
    if (qr > 0.0 && qs > 0.0) {
      Fs = maxf * pow(fmin(qr / qs, qs / qr), 1.0 / 3.0);
      fws = qr / (qr + qs);
    }
    const double qrp = (1.0 - Fs - Fg) * qr, qsp = (1.0 - Fs) * qs, qgp = (1.0 - Fg) * qg;
    const double qms = Fs * (qr + qs), qmg = Fg * (qr + qg);
    if (qrp > 0.0) zr = 2.53e4 * pow(ro * qrp * 1.0e3, F(1.84));
    if (qsp > 0.0) zs = 3.48e3 * pow(ro * qsp * 1.0e3, F(1.66));
    if (qgp > 0.0) zg = 5.54e3 * pow(ro * qgp * 1.0e3, F(1.70));
    if (qms > 0.0) {
      zms = (F(0.00491) + F(5.75) * fws - F(5.588) * (fws * fws)) * 1.0e5;
      zms = zms * pow(ro * qms * 1.0e3, F(1.67) - F(0.202) * fws + F(0.398) * (fws * fws));
    }
    if (qmg > 0.0) {
      zmg = (F(0.809) + F(10.13) * fwg - F(5.98) * (fwg * fwg)) * 1.0e5;
      zmg = zmg * pow(ro * qmg * 1.0e3, F(1.48) + F(0.0448) * fwg - F(0.0313) * (fwg * fwg));
    }
    ref = zr + zg + zs + zms + zmg;
    if (ref > 0.0) {
      const double nor = 8.0e-2, nos = 3.0e-2, nog = 4.0e-4, ror = 1.0, ros = 0.1, rog = 0.917, roo = 0.001;
      ro = 1.0e-3 * ro;
      const double a = 2115.0, b = 0.8, c = 152.93, d = 0.25, Cd = 0.6;
      const double rofactor = pow(roo / ro, 0.5);
      double wr = 0.0, ws = 0.0, wg = 0.0;
      if (qr > 0.0) {
        const double lr = pow(kPi * ror * nor / (ro * qr), 0.25);
        wr = a * kGamma48 / (6.0 * pow(lr, b));
        wr = 1.0e-2 * wr * rofactor;
      }
      if (qs > 0.0) {
        const double ls = pow(kPi * ros * nos / (ro * qs), 0.25);
        ws = c * kGamma425 / (6.0 * pow(ls, d));
        ws = 1.0e-2 * ws * rofactor;
      }
      if (qg > 0.0) {
        const double lg = pow(kPi * rog * nog / (ro * qg), 0.25);
        wg = kGamma45 * pow((4.0 * kGg * 100.0 * rog) / (3.0 * Cd * ro), 0.5);
        wg = 1.0e-2 * wg / (6.0 * pow(lg, 0.5));
      }
      wt = (wr * zr + ws * zs + ws * zms + wg * zg + wg * zmg) / (zr + zs + zg + zms + zmg);
    }
  }
  double vr = u * cos(elev * kDeg2Rad) * sin(az * kDeg2Rad);
  vr = vr + v * cos(elev * kDeg2Rad) * cos(az * kDeg2Rad);
  vr = vr + (use_tv ? (w - wt) : w) * sin(elev * kDeg2Rad);
  *ref_out = ref;
  *vr_out = vr;
}

#undef F

}  // namespace obsope_point_dev
}  // namespace letkf
