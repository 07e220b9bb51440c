// letkf_nobsout_entry.hip -- C ABI of the eleventh companion header include/letkf_amd_nobsout.h: das_letkf's main loop with the
// NOBS_OUT diagnostics, and work3dn / the eleven fields from them.  Host side only, in the library of NOBS_OUT
// (libletkf_amd_nobsout.so): the kernels are letkf_nobsout.hip's; the context, its stream, the error text and the main loop itself
// (das_columns_impl of letkf_api_das.hip, reached as the library of the first scan reaches the operator) are the main library's.

#include "letkf_api_internal.h"
#include "letkf_nobsout_dev.h"

using namespace letkf::api;

namespace {

struct Range {
  const char* p;
  size_t bytes;
};

Range range_of(const void* p, size_t bytes) { return Range{reinterpret_cast<const char*>(p), bytes}; }

bool overlap(const Range& a, const Range& b) {
  return a.p && b.p && a.bytes && b.bytes && a.p < b.p + b.bytes && b.p < a.p + a.bytes;
}

}  // namespace

extern "C" {

int letkf_das_columns_nobs_dev(letkf_ctx* c, const letkf_das_args* g, const letkf_search_tables* t, int64_t nij1, int32_t nlev,
                               const double* rig, const double* rjg, const double* rlev, const double* rz, int64_t list_bytes,
                               int32_t* nobs_out, int32_t* nobs_ctype, double* cutd_ctype) try {
  if (int rc = check_ctx(c)) return rc;
  if (!nobs_ctype && !cutd_ctype) return das_columns_impl(c, g, t, nij1, nlev, rig, rjg, rlev, rz, list_bytes, nobs_out, nullptr);
  // (what the main loop refuses, it refuses below before anything is written; the overlaps need the extents it checks)
  if (g && t && g->npts > 0 && t->nctype >= 1) {
    const size_t np = (size_t)g->npts, ne = np * (size_t)t->nctype;
    const Range dn = range_of(nobs_ctype, ne * 4), dc = range_of(cutd_ctype, ne * 8);
    const Range others[2] = {range_of(nobs_out, np * 4), range_of(g->status, np * 4)};
    if (overlap(dn, dc)) return fail(LETKF_E_INVALID, "nobs_ctype overlaps cutd_ctype");
    for (const Range& o : others)
      if (overlap(dn, o) || overlap(dc, o)) return fail(LETKF_E_INVALID, "nobs_ctype / cutd_ctype overlaps nobs_out or args->status");
  }
  DasColumnsDiag d{nobs_ctype, cutd_ctype, false};
  if (int rc = das_columns_impl(c, g, t, nij1, nlev, rig, rjg, rlev, rz, list_bytes, nobs_out, &d)) return rc;
  if (d.cutd_from_tables) HIP_TRY(letkf::launch_nobs_cutd_default(*t, g->npts, cutd_ctype, c->num_cu, c->stream));
  if (g->beta) HIP_TRY(letkf::launch_nobs_zero_unanalysed(g->npts, t->nctype, g->beta, nobs_ctype, cutd_ctype, c->num_cu, c->stream));
  return LETKF_OK;
} LETKF_ENTRY_END(letkf_das_columns_nobs_dev)

int letkf_nobs_fields_dev(letkf_ctx* c, const letkf_nobsout_params* p, int64_t npts, const int32_t* nobs_ctype,
                          const double* cutd_ctype, double* work3dn, double* fields, int64_t sp, int64_t sv) try {
  if (int rc = check_ctx(c)) return rc;
  if (!p) return fail(LETKF_E_INVALID, "params is NULL");
  if (p->nctype < 1 || p->nctype > LETKF_NOBSOUT_MAX_CTYPE) return fail(LETKF_E_INVALID, "nctype must be 1 .. 64");
  if (p->nobtype < 1 || p->nobtype > LETKF_NOBSOUT_MAX_OBTYPE) return fail(LETKF_E_INVALID, "nobtype must be 1 .. 32");
  if (!p->elm_u_ctype || !p->typ_ctype) return fail(LETKF_E_INVALID, "elm_u_ctype / typ_ctype is NULL");
  if (npts < 0) return fail(LETKF_E_INVALID, "npts < 0");
  if (!nobs_ctype) return fail(LETKF_E_INVALID, "nobs_ctype is NULL");
  if (!work3dn && !fields) return fail(LETKF_E_INVALID, "work3dn and fields are both NULL");
  const int32_t uid[3] = {p->uid_ref, p->uid_re0, p->uid_vr};
  for (int q = 0; q < 3; ++q)
    if (uid[q] < 1 || uid[q] > 16) return fail(LETKF_E_INVALID, "uid_ref / uid_re0 / uid_vr must be 1 .. 16");
  if (p->typ_radar < 1 || p->typ_radar > p->nobtype) return fail(LETKF_E_INVALID, "typ_radar must be 1 .. nobtype");
  for (int f = 0; f < 5; ++f)
    if (p->pick[f] < 1 || p->pick[f] > p->nobtype) return fail(LETKF_E_INVALID, "pick must be 1 .. nobtype");
  for (int ic = 0; ic < p->nctype; ++ic) {
    if (p->elm_u_ctype[ic] < 1 || p->elm_u_ctype[ic] > 16) return fail(LETKF_E_INVALID, "elm_u_ctype must be 1 .. 16");
    if (p->typ_ctype[ic] < 1 || p->typ_ctype[ic] > p->nobtype) return fail(LETKF_E_INVALID, "typ_ctype must be 1 .. nobtype");
    for (int jc = 0; jc < ic; ++jc)
      if (p->elm_u_ctype[jc] == p->elm_u_ctype[ic] && p->typ_ctype[jc] == p->typ_ctype[ic])
        return fail(LETKF_E_INVALID, "two combined types with the same (elm_u, typ)");
  }
  const int nrow = p->nobtype + 6;
  size_t fext = 0;                                      // elements the fields span
  if (fields) {
    const int64_t last = npts > 0 ? npts - 1 : 0, lim = INT64_MAX / 16;
    const bool by_point = sp >= 1 && sp <= lim / (last + 1) && sv > last * sp && sv <= lim;
    const bool by_field = sv >= 1 && sv <= lim / 16 && sp > 10 * sv && sp <= lim / (last + 1);
    if (!by_point && !by_field)
      return fail(LETKF_E_INVALID, "strides: sp >= 1 with sv > (npts - 1) * sp, or sv >= 1 with sp > 10 * sv");
    fext = (size_t)(last * sp + 10 * sv + 1);
  }
  if (npts == 0) return LETKF_OK;
  {
    const size_t ne = (size_t)npts * (size_t)p->nctype;
    const Range in[2] = {range_of(nobs_ctype, ne * 4), range_of(cutd_ctype, ne * 8)};
    const Range out[2] = {range_of(work3dn, (size_t)npts * nrow * 8), range_of(fields, fext * 8)};
    for (const Range& x : out)
      for (const Range& y : in)
        if (overlap(x, y)) return fail(LETKF_E_INVALID, "an output overlaps an input");
    if (overlap(out[0], out[1])) return fail(LETKF_E_INVALID, "work3dn overlaps fields");
  }
  letkf::NobsFieldsArgs a = {};
  a.npts = npts, a.nctype = p->nctype, a.nobtype = p->nobtype;
  a.nobs_ctype = nobs_ctype, a.cutd_ctype = cutd_ctype, a.work3dn = work3dn, a.fields = fields, a.sp = sp, a.sv = sv;
  for (int q = 0; q < 3; ++q) {
    a.ic_radar[q] = -1;
    for (int ic = 0; ic < p->nctype; ++ic)
      if (p->elm_u_ctype[ic] == uid[q] && p->typ_ctype[ic] == p->typ_radar) a.ic_radar[q] = ic;
  }
  for (int f = 0; f < LETKF_NOBSOUT_NFIELDS; ++f) a.row_field[f] = f < 5 ? p->pick[f] - 1 : p->nobtype + (f - 5);   // :768-778
  int m = 0;
  for (int r = 0; r < p->nobtype; ++r) {
    a.typ_start[r] = (uint8_t)m;
    for (int ic = 0; ic < p->nctype; ++ic)
      if (p->typ_ctype[ic] == r + 1) a.typ_member[m++] = (uint8_t)ic;
  }
  a.typ_start[p->nobtype] = (uint8_t)m;
  HIP_TRY(letkf::launch_nobs_fields(a, c->num_cu, c->stream));
  return LETKF_OK;
} LETKF_ENTRY_END(letkf_nobs_fields_dev)

}  // extern "C"
