// letkf_tcvital_entry.hip -- C ABI of the twelfth companion header include/letkf_amd_tcvital.h: the rows of a TC vitals report,
// the background cyclone's centre and pressure per member and subdomain, and the pick among the ranks with the three obsda rows.
// Host side only, in the library of the TC vitals (libletkf_amd_tcvital.so): the kernels are letkf_tcvital.hip's; the context, its
// stream, its scratch buffer and the error text are the main library's.

#include "letkf_api_internal.h"
#include "letkf_tcvital_dev.h"

using namespace letkf::api;

extern "C" {

int letkf_tcvital_rows_dev(letkf_ctx* c, int64_t n, const int32_t* elm, const double* dif, double slot_lb, double slot_ub, int64_t* rows,
                           int32_t* valid) try {
  if (int rc = check_ctx(c)) return rc;
  if (!rows || !valid) return fail(LETKF_E_INVALID, "rows / valid is NULL");
  if (n < 0) return fail(LETKF_E_INVALID, "n < 0");
  if (n > 0 && (!elm || !dif)) return fail(LETKF_E_INVALID, "elm / dif is NULL");
  if (!(slot_lb <= slot_ub)) return fail(LETKF_E_INVALID, "slot_lb > slot_ub");
  if (n == 0) {
    rows[0] = rows[1] = rows[2] = 0;
    *valid = 0;
    return LETKF_OK;
  }
  // blocks' partials [nblock][3] int64 | the three rows int64 [3] | their dif double [3]
  const size_t o_out = align256((size_t)letkf::tc_rows_blocks(n) * 3 * sizeof(int64_t));
  if (int rc = grow(c, &c->scratch, o_out + 6 * sizeof(int64_t))) return rc;
  int64_t* part = reinterpret_cast<int64_t*>(c->scratch.p);
  int64_t* out6 = reinterpret_cast<int64_t*>(c->scratch.p + o_out);
  HIP_TRY(letkf::launch_tc_rows(n, elm, dif, part, out6, c->stream));
  int64_t back[6];
  HIP_TRY(hipMemcpyAsync(back, out6, sizeof(back), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  double d[3];
  std::memcpy(d, back + 3, sizeof(d));
  for (int q = 0; q < 3; ++q) rows[q] = back[q];
  const bool all = back[0] > 0 && back[1] > 0 && back[2] > 0;                          // obsope_tools.f90:651-656
  *valid = all && d[0] == d[1] && d[1] == d[2] && d[0] > slot_lb && d[0] <= slot_ub;
  return LETKF_OK;
} LETKF_ENTRY_END(letkf_tcvital_rows_dev)

int letkf_tcvital_search_dev(letkf_ctx* c, const letkf_tcvital_params* p, const letkf_obsope_fields* f, const double* ritc,
                             const double* rjtc, double* cand) try {
  if (int rc = check_ctx(c)) return rc;
  if (!p || !f || !ritc || !rjtc || !cand) return fail(LETKF_E_INVALID, "params / fields / ritc / rjtc / cand is NULL");
  if (!f->v2d) return fail(LETKF_E_INVALID, "fields->v2d is NULL");
  if (f->nmem < 1) return fail(LETKF_E_INVALID, "nmem < 1");
  if (f->nlon < 1 || f->nlat < 1 || f->ihalo < 0 || f->jhalo < 0) return fail(LETKF_E_INVALID, "nlon / nlat < 1 or a negative halo");
  if (f->nv2dd < 7) return fail(LETKF_E_INVALID, "nv2dd < 7");
  if (!f->s2i || !f->s2j || !f->s2v || !f->s2m) return fail(LETKF_E_INVALID, "a zero stride");
  if (!std::isfinite(p->dx) || !std::isfinite(p->dy) || p->dx <= 0.0 || p->dy <= 0.0)
    return fail(LETKF_E_INVALID, "dx / dy must be finite and positive");
  if (!std::isfinite(p->tc_search_dis) || p->tc_search_dis < 0.0) return fail(LETKF_E_INVALID, "tc_search_dis must be finite and >= 0");
  letkf::TcSearchArgs a = {};
  a.v2d = f->v2d, a.s2i = f->s2i, a.s2j = f->s2j, a.s2v = f->s2v, a.s2m = f->s2m;
  a.nlon = f->nlon, a.nlat = f->nlat, a.ihalo = f->ihalo, a.jhalo = f->jhalo, a.nmem = f->nmem;
  a.i_off = p->i_off, a.j_off = p->j_off;
  a.tiles_i = (f->nlon + letkf::kTcTileI - 1) / letkf::kTcTileI, a.tiles_j = (f->nlat + letkf::kTcTileJ - 1) / letkf::kTcTileJ;
  a.dx = p->dx, a.dy = p->dy, a.cxg1 = p->cxg1, a.cyg1 = p->cyg1, a.dis = p->tc_search_dis;
  a.ritc = ritc, a.rjtc = rjtc, a.cand = cand;
  if ((int64_t)a.tiles_i * a.tiles_j * (int64_t)a.nmem > (int64_t)INT32_MAX)
    return fail(LETKF_E_INVALID, "more tiles times members than one grid holds");
  if (int rc = grow(c, &c->scratch, letkf::tc_search_ws_bytes(a))) return rc;
  a.part_s = reinterpret_cast<double*>(c->scratch.p);
  a.part_ij = reinterpret_cast<int32_t*>(c->scratch.p + letkf::tc_search_part_s_bytes(a));
  HIP_TRY(letkf::launch_tc_search(a, c->stream));
  return LETKF_OK;
} LETKF_ENTRY_END(letkf_tcvital_search_dev)

int letkf_tcvital_fill_dev(letkf_ctx* c, int32_t nproc, int32_t nmem, int32_t m0, const double* cand_all, const int64_t* rows,
                           int32_t qc_replace, int32_t* qc, double* ensval, int64_t kld) try {
  if (int rc = check_ctx(c)) return rc;
  if (!cand_all || !rows || !qc || !ensval) return fail(LETKF_E_INVALID, "cand_all / rows / qc / ensval is NULL");
  if (nproc < 1) return fail(LETKF_E_INVALID, "nproc < 1");
  if (nmem < 1) return fail(LETKF_E_INVALID, "nmem < 1");
  if (m0 < 0 || (int64_t)m0 + nmem > kld) return fail(LETKF_E_INVALID, "m0 < 0 or m0 + nmem > kld");
  HIP_TRY(letkf::launch_tc_fill(nproc, nmem, m0, cand_all, rows[0], rows[1], rows[2], qc_replace, qc, ensval, kld, c->stream));
  return LETKF_OK;
} LETKF_ENTRY_END(letkf_tcvital_fill_dev)

}  // extern "C"
