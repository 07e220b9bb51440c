// letkf_mapproj_entry.hip -- C ABI of the ninth companion header include/letkf_amd_mapproj.h: the map projection's derived
// constants, the three device entries and the two one-point host helpers.  Host side only, in the library of the projection
// (libletkf_amd_mapproj.so): the kernels are letkf_mapproj.hip's, the point functions letkf_mapproj_point.h's (compiled here for
// the host), the context, its stream and the error text the main library's.

#include "letkf_api_internal.h"
#include "letkf_mapproj_dev.h"
#include "letkf_mapproj_point.h"

#include <climits>

using namespace letkf::api;

namespace {

struct Range {
  const char* name;
  const void* p;
  size_t bytes;
};

bool overlap(const Range& a, const Range& b) {
  const char *x = static_cast<const char*>(a.p), *y = static_cast<const char*>(b.p);
  return x && y && a.bytes && b.bytes && x < y + b.bytes && y < x + a.bytes;
}

// no output on an input, no output on another output
int check_ranges(const Range* in, int nin, const Range* out, int nout) {
  for (int o = 0; o < nout; ++o) {
    for (int i = 0; i < nin; ++i)
      if (overlap(out[o], in[i])) return fail(LETKF_E_INVALID, std::string(out[o].name) + " overlaps " + in[i].name);
    for (int q = o + 1; q < nout; ++q)
      if (overlap(out[o], out[q])) return fail(LETKF_E_INVALID, std::string(out[o].name) + " overlaps " + out[q].name);
  }
  return LETKF_OK;
}

bool positive(double v) { return std::isfinite(v) && v > 0.0; }

// a proj as letkf_mapproj_setup leaves it
int check_proj(const letkf_mapproj* p) {
  if (!p) return fail(LETKF_E_INVALID, "proj is NULL");
  if (p->type != LETKF_MAPPROJ_LC) return fail(LETKF_E_INVALID, "proj->type must be 1 (LC)");
  if (p->hemisphere != 1.0 && p->hemisphere != -1.0) return fail(LETKF_E_INVALID, "proj->hemisphere must be +1 or -1");
  if (!positive(p->c) || !(p->c < 1.0)) return fail(LETKF_E_INVALID, "proj->c must be in (0, 1)");
  if (!positive(p->fact)) return fail(LETKF_E_INVALID, "proj->fact must be finite and > 0");
  if (!positive(p->radius)) return fail(LETKF_E_INVALID, "proj->radius must be finite and > 0");
  if (!positive(p->dx) || !positive(p->dy)) return fail(LETKF_E_INVALID, "proj->dx and proj->dy must be finite and > 0");
  if (!std::isfinite(p->lon0) || !std::isfinite(p->pole_x) || !std::isfinite(p->pole_y) || !std::isfinite(p->cxg1) || !std::isfinite(p->cyg1))
    return fail(LETKF_E_INVALID, "proj->lon0, pole_x, pole_y, cxg1 and cyg1 must be finite");
  return LETKF_OK;
}

int check_rotc(const double* rotc) {
  if (reinterpret_cast<uintptr_t>(rotc) % 16) return fail(LETKF_E_INVALID, "rotc must be 16-byte aligned");
  return LETKF_OK;
}

// the row-wise entries: a[0], a[1] in, b[0], b[1] and rotc out
int check_rows(int64_t n, const char* const names[4], const double* a0, const double* a1, double* b0, double* b1, double* rotc) {
  if (n < 0) return fail(LETKF_E_INVALID, "n must be >= 0");
  if (n > INT64_MAX / 16) return fail(LETKF_E_INVALID, "n must be <= 2^59");
  if (n == 0) return LETKF_OK;
  if (!a0 || !a1) return fail(LETKF_E_INVALID, std::string(names[0]) + " / " + names[1] + " is NULL");
  if (!b0 || !b1) return fail(LETKF_E_INVALID, std::string(names[2]) + " / " + names[3] + " is NULL");
  if (int rc = check_rotc(rotc)) return rc;
  const size_t b = (size_t)n * 8;
  const Range in[2] = {{names[0], a0, b}, {names[1], a1, b}};
  const Range out[3] = {{names[2], b0, b}, {names[3], b1, b}, {"rotc", rotc, 2 * b}};
  return check_ranges(in, 2, out, 3);
}

}  // namespace

extern "C" {

int letkf_mapproj_setup(const letkf_mapproj_params* p, letkf_mapproj* proj) try {
  if (!p || !proj) return fail(LETKF_E_INVALID, "params / proj is NULL");
  if (p->type != LETKF_MAPPROJ_LC) return fail(LETKF_E_INVALID, "type must be 1 (LC): NONE, PS, MER and EC are not built");
  if (!std::isfinite(p->basepoint_lon) || !std::isfinite(p->basepoint_x) || !std::isfinite(p->basepoint_y) || !std::isfinite(p->cxg1) ||
      !std::isfinite(p->cyg1))
    return fail(LETKF_E_INVALID, "basepoint_lon, basepoint_x, basepoint_y, cxg1 and cyg1 must be finite");
  if (!(std::fabs(p->lc_lat1) < 90.0) || !(std::fabs(p->lc_lat2) < 90.0)) return fail(LETKF_E_INVALID, "lc_lat1 and lc_lat2 must be inside (-90, 90)");
  if (!(std::fabs(p->basepoint_lat) < 90.0)) return fail(LETKF_E_INVALID, "basepoint_lat must be inside (-90, 90)");
  if (!(p->lc_lat1 < p->lc_lat2)) return fail(LETKF_E_INVALID, "lc_lat1 must be < lc_lat2");
  if (p->lc_lat1 + p->lc_lat2 == 0.0) return fail(LETKF_E_INVALID, "lc_lat1 + lc_lat2 must not be 0: the cone is a cylinder");
  if (!positive(p->radius)) return fail(LETKF_E_INVALID, "radius must be finite and > 0");
  if (!positive(p->dx) || !positive(p->dy)) return fail(LETKF_E_INVALID, "dx and dy must be finite and > 0");

  // Once, on the host, in the x87 extended format (64-bit significand) and rounded to double at the end: c is a quotient of two
  // differences of logarithms that cancel a digit and a half, and its error is multiplied by dlam in every sincos(c dlam) --
  // made in double it alone costs 20 * 2^-53 * rho at the cut.  So each constant is within an ulp of its real value.
  typedef long double real;
  const real kPi = 3.14159265358979323846264338327950288L, D = kPi / 180.0L;
  const real h = p->lc_lat1 + p->lc_lat2 > 0.0 ? 1.0L : -1.0L;
  const real psi1 = 0.5L * kPi - h * p->lc_lat1 * D, psi2 = 0.5L * kPi - h * p->lc_lat2 * D, psi0 = 0.5L * kPi - h * p->basepoint_lat * D;
  const real c = (std::log(std::sin(psi1)) - std::log(std::sin(psi2))) / (std::log(std::tan(0.5L * psi1)) - std::log(std::tan(0.5L * psi2)));
  const real fact = std::sin(psi1) / (c * std::pow(std::tan(0.5L * psi1), c));
  letkf_mapproj q = {};
  q.type = p->type, q.hemisphere = (double)h, q.lon0 = (double)(p->basepoint_lon * D), q.c = (double)c, q.fact = (double)fact;
  q.radius = p->radius, q.pole_x = p->basepoint_x;
  q.pole_y = (double)(p->basepoint_y + h * (fact * p->radius * std::pow(std::tan(0.5L * psi0), c)));
  q.cxg1 = p->cxg1, q.cyg1 = p->cyg1, q.dx = p->dx, q.dy = p->dy;
  if (int rc = check_proj(&q)) return rc;
  *proj = q;
  return LETKF_OK;
} LETKF_ENTRY_END(letkf_mapproj_setup)

int letkf_phys2ij_dev(letkf_ctx* c, const letkf_mapproj* proj, int64_t n, const double* lon, const double* lat, double* ri, double* rj,
                      double* rotc) try {
  if (!c) return fail(LETKF_E_INVALID, "ctx is NULL");
  if (int rc = check_ctx(c)) return rc;
  if (int rc = check_proj(proj)) return rc;
  static const char* const names[4] = {"lon", "lat", "ri", "rj"};
  if (int rc = check_rows(n, names, lon, lat, ri, rj, rotc)) return rc;
  if (n == 0) return LETKF_OK;
  HIP_TRY(letkf::phys2ij_run(c->stream, *proj, n, lon, lat, ri, rj, rotc));
  return LETKF_OK;
} LETKF_ENTRY_END(letkf_phys2ij_dev)

int letkf_ij2phys_dev(letkf_ctx* c, const letkf_mapproj* proj, int64_t n, const double* ri, const double* rj, double* lon, double* lat,
                      double* rotc) try {
  if (!c) return fail(LETKF_E_INVALID, "ctx is NULL");
  if (int rc = check_ctx(c)) return rc;
  if (int rc = check_proj(proj)) return rc;
  static const char* const names[4] = {"ri", "rj", "lon", "lat"};
  if (int rc = check_rows(n, names, ri, rj, lon, lat, rotc)) return rc;
  if (n == 0) return LETKF_OK;
  HIP_TRY(letkf::ij2phys_run(c->stream, *proj, n, ri, rj, lon, lat, rotc));
  return LETKF_OK;
} LETKF_ENTRY_END(letkf_ij2phys_dev)

int letkf_mapproj_grid_dev(letkf_ctx* c, const letkf_mapproj* proj, int32_t nlon, int32_t nlat, int32_t ihalo, int32_t jhalo, double cx1,
                           double cy1, double* lon2d, double* lat2d, double* rotc2d) try {
  if (!c) return fail(LETKF_E_INVALID, "ctx is NULL");
  if (int rc = check_ctx(c)) return rc;
  if (int rc = check_proj(proj)) return rc;
  if (nlon < 1 || nlat < 1) return fail(LETKF_E_INVALID, "nlon and nlat must be >= 1");
  if ((int64_t)nlon * nlat > INT_MAX) return fail(LETKF_E_INVALID, "nlon * nlat must be < 2^31");
  if (ihalo < 0 || jhalo < 0) return fail(LETKF_E_INVALID, "ihalo and jhalo must be >= 0");
  if ((int64_t)nlon + ihalo > INT_MAX || (int64_t)nlat + jhalo > INT_MAX) return fail(LETKF_E_INVALID, "nlon + ihalo and nlat + jhalo must be < 2^31");
  if (!std::isfinite(cx1) || !std::isfinite(cy1)) return fail(LETKF_E_INVALID, "cx1 and cy1 must be finite");
  if (!lon2d && !lat2d && !rotc2d) return fail(LETKF_E_INVALID, "lon2d, lat2d and rotc2d are all NULL");
  if (int rc = check_rotc(rotc2d)) return rc;
  const size_t b = (size_t)nlon * nlat * 8;
  const Range out[3] = {{"lon2d", lon2d, b}, {"lat2d", lat2d, b}, {"rotc2d", rotc2d, 2 * b}};
  if (int rc = check_ranges(nullptr, 0, out, 3)) return rc;
  HIP_TRY(letkf::mapproj_grid_run(c->stream, *proj, nlon, nlat, ihalo, jhalo, cx1, cy1, lon2d, lat2d, rotc2d));
  return LETKF_OK;
} LETKF_ENTRY_END(letkf_mapproj_grid_dev)

int letkf_phys2ij_host(const letkf_mapproj* proj, double lon, double lat, double* ri, double* rj, double* rotc) try {
  if (int rc = check_proj(proj)) return rc;
  if (!ri || !rj) return fail(LETKF_E_INVALID, "ri / rj is NULL");
  double r0, r1;
  letkf::mapproj::phys2ij_point(*proj, lon, lat, ri, rj, &r0, &r1);
  if (rotc) rotc[0] = r0, rotc[1] = r1;
  return LETKF_OK;
} LETKF_ENTRY_END(letkf_phys2ij_host)

int letkf_ij2phys_host(const letkf_mapproj* proj, double ri, double rj, double* lon, double* lat, double* rotc) try {
  if (int rc = check_proj(proj)) return rc;
  if (!lon || !lat) return fail(LETKF_E_INVALID, "lon / lat is NULL");
  letkf::mapproj::ij2phys_point(*proj, ri, rj, lon, lat);
  if (rotc) letkf::mapproj::rotc_at(*proj, *lon, *lat, &rotc[0], &rotc[1]);
  return LETKF_OK;
} LETKF_ENTRY_END(letkf_ij2phys_host)

}  // extern "C"
