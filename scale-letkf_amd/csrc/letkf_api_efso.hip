// letkf_api_efso.hip -- C ABI, observation impact (EFSO): the seven letkf_efso_* entries.

#include "letkf_api_internal.h"

using namespace letkf::api;

namespace letkf::api {

// ---- EFSO (letkf_efso.hip).  Workspace per list entry besides the lists: nterm contributions, the sort's keys (in and
// out) and entry numbers, and about as much again of sort scratch.
int64_t efso_entry_bytes(int nterm) { return 8 * (int64_t)nterm + 20; }
constexpr int64_t kEfsoMaxSlab = (int64_t)1 << 31;   // entry numbers of a slab are 32-bit in the sort

int efso_check(letkf_ctx* c, const letkf_efso_args* g, bool lists, letkf::EfsoArgs* a) {
  if (int rc = check_ctx(c)) return rc;
  if (!g) return fail(LETKF_E_INVALID, "args is NULL");
  if (g->nterm < 1 || g->nterm > 4) return fail(LETKF_E_INVALID, "nterm must be 1..4");
  if (g->k < 2) return fail(LETKF_E_INVALID, "ensemble size must be >= 2");
  if (g->nv < 1 || g->nv > 32) return fail(LETKF_E_INVALID, "nv must be 1..32");
  if (g->npts < 0 || g->nobs < 0) return fail(LETKF_E_INVALID, "negative npts / nobs");
  if (g->nobs > 0x7fffffff) return fail(LETKF_E_INVALID, "more than 2^31 observation rows");
  if (g->kld < g->k) return fail(LETKF_E_INVALID, "kld must be >= k");
  if (!g->term_of_var || !g->ensval || !g->fcst || !g->fcer || !g->djdy)
    return fail(LETKF_E_INVALID, "a required pointer is NULL (term_of_var, ensval, fcst, fcer, djdy)");
  if (lists && (!g->obs_off || !g->obs_idx || !g->rdiag_l || !g->rloc_l))
    return fail(LETKF_E_INVALID, "a list pointer is NULL (obs_off, obs_idx, rdiag_l, rloc_l)");
  if (letkf::efso_pair_lds(g->k, g->nterm) > c->lds_max) return fail(LETKF_E_INVALID, "ensemble size too large for the LDS of w_p");
  *a = letkf::EfsoArgs{};
  a->k = g->k;
  a->nv = g->nv;
  a->nterm = g->nterm;
  for (int v = 0; v < 32; ++v) a->term[v] = -1;
  for (int v = 0; v < g->nv; ++v) {
    const int t = g->term_of_var[v];
    if (t < -1 || t >= g->nterm) return fail(LETKF_E_INVALID, "term_of_var values must be -1..nterm-1");
    a->term[v] = (signed char)((g->var_mask == 0 || ((g->var_mask >> v) & 1u)) ? t : -1);
  }
  a->nobs = g->nobs;
  a->kld = g->kld;
  a->obs_off = reinterpret_cast<const long*>(g->obs_off);
  a->obs_idx = g->obs_idx;
  a->rdiag_l = g->rdiag_l;
  a->rloc_l = g->rloc_l;
  a->ensval = g->ensval;
  a->fcst = g->fcst;
  a->sp = g->sp;
  a->sm = g->sm;
  a->sv = g->sv;
  a->fcer = g->fcer;
  a->fsp = g->fsp;
  a->fsv = g->fsv;
  a->djdy = g->djdy;
  return LETKF_OK;
}

// One slab: points [p0, p0 + npts) of a, whose lists are entries [e0, e1) at the device offsets off -- of the slab ls, or of
// a's own lists without one
int efso_run_slab(letkf_ctx* c, letkf::EfsoArgs a, int64_t p0, int64_t npts, const int64_t* off, const ListSlab* ls, int64_t e0,
                  int64_t e1) {
  a.obs_off = reinterpret_cast<const long*>(off + p0);
  if (ls) {
    a.obs_idx = ls->idx;
    a.rdiag_l = ls->rd;
    a.rloc_l = ls->rl;
  }
  a.fcst += p0 * a.sp;
  a.fcer += p0 * a.fsp;
  if (npts <= 0 || e1 <= e0 || a.nobs == 0) return LETKF_OK;
  letkf::EfsoWs ws;
  HIP_TRY(letkf::efso_ws_layout(e1 - e0, a.nobs, a.nterm, c->stream, &ws));
  if (int rc = grow(c, &c->efso_ws, ws.total)) return rc;
  HIP_TRY(letkf::efso_slab(a, npts, e0, e1, c->efso_ws.p, ws, c->num_cu, c->stream));
  return LETKF_OK;
}

}  // namespace letkf::api

extern "C" {

// EFSO, das_efso's loop (scale/letkf/letkf_tools.f90:1158-1302) on caller-built lists: points in chunks whose pair
// workspace fits pair_bytes (the offsets are read back only when the lists do not fit at once)
int letkf_efso_points_dev(letkf_ctx* c, const letkf_efso_args* g) try {
  letkf::EfsoArgs a;
  if (int rc = efso_check(c, g, true, &a)) return rc;
  c->last_path = letkf::efso_path_name(g->nterm);
  if (g->npts == 0 || g->nobs == 0) return LETKF_OK;
  const int64_t budget = g->pair_bytes > 0 ? g->pair_bytes : ((int64_t)8 << 30);
  const int64_t cap = std::max<int64_t>(1, std::min(budget / efso_entry_bytes(g->nterm), kEfsoMaxSlab));
  int64_t ends[2];
  HIP_TRY(hipMemcpyAsync(&ends[0], g->obs_off, 8, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipMemcpyAsync(&ends[1], g->obs_off + g->npts, 8, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  if (ends[1] - ends[0] <= cap) return efso_run_slab(c, a, 0, g->npts, g->obs_off, nullptr, ends[0], ends[1]);
  std::vector<int64_t> off((size_t)g->npts + 1);
  HIP_TRY(hipMemcpyAsync(off.data(), g->obs_off, off.size() * 8, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  for (int64_t p0 = 0; p0 < g->npts;) {
    const int64_t p1 = chunk_end(off, p0, g->npts, 1, 1, cap);   // (the budget in entries: cap of them, 1 B each)
    if (off[p1] - off[p0] > kEfsoMaxSlab) return fail(LETKF_E_INVALID, "a point with more than 2^31 local observations");
    if (int rc = efso_run_slab(c, a, p0, p1 - p0, g->obs_off, nullptr, off[p0], off[p1])) return rc;
    p0 = p1;
  }
  return LETKF_OK;
} LETKF_ENTRY_END(letkf_efso_points_dev)

// EFSO for a whole subdomain: the column search (3a) by slabs of levels whose lists and pair workspace fit list_bytes,
// then the EFSO passes on each slab -- the list route of letkf_das_columns_dev
int letkf_efso_columns_dev(letkf_ctx* c, const letkf_efso_args* g, const letkf_search_tables* t, int64_t nij1, int32_t nlev,
                           const double* rig, const double* rjg, const double* rlev, const double* rz, int64_t list_bytes) try {
  letkf::EfsoArgs a;
  if (int rc = efso_check(c, g, false, &a)) return rc;
  if (!t) return fail(LETKF_E_INVALID, "tables is NULL");
  if (nij1 < 1 || nlev < 1 || g->npts != nij1 * (int64_t)nlev) return fail(LETKF_E_INVALID, "npts must be nij1 * nlev");
  if (!rig || !rjg || !rlev || !rz) return fail(LETKF_E_INVALID, "a point coordinate array is NULL");
  c->last_path = std::string("search_columns + ") + letkf::efso_path_name(g->nterm);
  if (list_bytes <= 0) list_bytes = (int64_t)8 << 30;
  const int64_t per_entry = 20 + efso_entry_bytes(g->nterm);
  RingKeep ring_keep_guard(c);
  // ---- count pass over all levels, prefix sum, level boundaries back to the host
  ScanWs sw;
  if (int rc = count_columns(c, t, nij1, nlev, rig, rjg, rlev, rz, &sw)) return rc;
  if (int rc = offsets_to_host(c, sw, (size_t)nij1)) return rc;
  const std::vector<int64_t>& lev_off = sw.hoff;
  // ---- slabs of levels whose lists and pair workspace fit: fill pass, EFSO passes
  int l0 = 0;
  while (l0 < nlev) {
    const int l1 = (int)chunk_end(lev_off, l0, nlev, 1, per_entry, list_bytes, kEfsoMaxSlab);
    const int64_t p0 = (int64_t)l0 * nij1, np = (int64_t)(l1 - l0) * nij1;
    if (lev_off[l1] - lev_off[l0] > kEfsoMaxSlab) return fail(LETKF_E_INVALID, "a level with more than 2^31 local observations");
    ListSlab ls;
    if (int rc = fill_columns(c, t, nij1, l0, l1, rig, rjg, rlev, rz, sw, &ls)) return rc;
    if (int rc = efso_run_slab(c, a, p0, np, sw.off, &ls, lev_off[l0], lev_off[l1])) return rc;
    l0 = l1;
  }
  return LETKF_OK;
} LETKF_ENTRY_END(letkf_efso_columns_dev)

// obsense(t, j) = djdy(t, j) * dep(j), das_efso :1283-1290
int letkf_efso_obsense_dev(letkf_ctx* c, int32_t nterm, int64_t nobs, const double* djdy, const double* dep, double* obsense) try {
  if (int rc = check_ctx(c)) return rc;
  if (nterm < 1 || nterm > 4) return fail(LETKF_E_INVALID, "nterm must be 1..4");
  if (nobs < 0) return fail(LETKF_E_INVALID, "negative nobs");
  if (nobs > 0 && (!djdy || !dep || !obsense)) return fail(LETKF_E_INVALID, "a required pointer is NULL (djdy, dep, obsense)");
  HIP_TRY(letkf::launch_efso_obsense(nterm, nobs, djdy, dep, obsense, c->stream));
  return LETKF_OK;
} LETKF_ENTRY_END(letkf_efso_obsense_dev)

// (12) das_efso's advection branch (letkf_tools.f90:1225-1229): loc_advection (efso_tools.f90:158-195) on SCALE's grid
int letkf_efso_locadv_dev(letkf_ctx* c, int64_t nij1, int32_t nlev, const double* rig, const double* rjg, const double* u0,
                          const double* v0, const double* u1, const double* v1, double locadv_rate, double eft, double dx,
                          double dy, double* ri, double* rj) try {
  if (int rc = check_ctx(c)) return rc;
  if (nij1 < 1 || nlev < 1) return fail(LETKF_E_INVALID, "nij1 and nlev must be >= 1");
  if (!rig || !rjg || !u0 || !v0 || !u1 || !v1 || !ri || !rj)
    return fail(LETKF_E_INVALID, "a required pointer is NULL (rig, rjg, u0, v0, u1, v1, ri, rj)");
  if (!(std::isfinite(dx) && dx > 0.0) || !(std::isfinite(dy) && dy > 0.0)) return fail(LETKF_E_INVALID, "dx and dy must be finite and > 0");
  if (!std::isfinite(locadv_rate) || !std::isfinite(eft)) return fail(LETKF_E_INVALID, "locadv_rate and eft must be finite");
  // the reference's rad2deg = locadv_rate*eft*3600*180/(pi*re), with the grid spacing in place of the arc per degree
  const double ci = locadv_rate * eft * 3600.0 / dx;
  const double cj = locadv_rate * eft * 3600.0 / dy;
  if (int rc = grow(c, &c->scratch, 256)) return rc;
  unsigned* bad = reinterpret_cast<unsigned*>(c->scratch.p);
  HIP_TRY(hipMemsetAsync(bad, 0, 4, c->stream));
  HIP_TRY(letkf::launch_efso_locadv(nij1, nij1 * (int64_t)nlev, rig, rjg, u0, v0, u1, v1, ci, cj, ri, rj, bad, c->num_cu,
                                    c->stream));
  unsigned nbad = 0;
  HIP_TRY(hipMemcpyAsync(&nbad, bad, 4, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  c->last_path = "efso_locadv_kernel";
  if (nbad)
    return fail(LETKF_E_INVALID, std::to_string(nbad) + " point(s) advected to a non-finite position or by more than 2^20 cells");
  return LETKF_OK;
} LETKF_ENTRY_END(letkf_efso_locadv_dev)

// (12) EFSO at per-point positions: the point search (3) and the EFSO passes in runs of consecutive points whose lists and
// pair workspace fit list_bytes -- the chunking of letkf_das_obs_dev
int letkf_efso_search_dev(letkf_ctx* c, const letkf_efso_args* g, const letkf_search_tables* t, int64_t npts, const double* ri,
                          const double* rj, const double* rlev, const double* rz, int64_t list_bytes) try {
  letkf::EfsoArgs a;
  if (int rc = efso_check(c, g, false, &a)) return rc;
  if (!t) return fail(LETKF_E_INVALID, "tables is NULL");
  if (npts != g->npts) return fail(LETKF_E_INVALID, "npts must equal args->npts");
  if (!ri || !rj || !rlev || !rz) return fail(LETKF_E_INVALID, "a point coordinate array is NULL");
  if (t->nctype < 1 || t->ngroup < 1 || t->criterion < 1 || t->criterion > 3)
    return fail(LETKF_E_INVALID, "bad nctype / ngroup / criterion");
  letkf_search_tables tab;
  if (int rc = tables_hinted(c, t, &tab)) return rc;
  c->last_path = std::string(tab.limit_hint == 2 ? "search_kernel (radix select) + " : "search_kernel + ") +
                 letkf::efso_path_name(g->nterm);
  if (npts == 0 || g->nobs == 0) return LETKF_OK;
  if (list_bytes <= 0) list_bytes = (int64_t)8 << 30;
  const int64_t per_entry = 20 + efso_entry_bytes(g->nterm);
  // ---- count pass over all points, prefix sum, the offsets back to the host (the one synchronisation)
  ScanWs sw;
  if (int rc = scan_ws(c, &c->scratch, (size_t)npts, 0, &sw)) return rc;
  HIP_TRY(zero_total(c, sw));
  if (int rc = letkf_obs_search_dev(c, &tab, npts, ri, rj, rlev, rz, 0, sw.counts, nullptr, nullptr, nullptr, nullptr)) return rc;
  HIP_TRY(scan_offsets(c, sw));
  if (int rc = offsets_to_host(c, sw)) return rc;
  // ---- runs of consecutive points in ascending order: fill pass, EFSO passes
  for (int64_t p0 = 0; p0 < npts;) {
    const int64_t p1 = chunk_end(sw.hoff, p0, npts, 1, per_entry, list_bytes, kEfsoMaxSlab);
    const int64_t nnz = sw.hoff[p1] - sw.hoff[p0];
    if (nnz > kEfsoMaxSlab) return fail(LETKF_E_INVALID, "a point with more than 2^31 local observations");
    ListSlab ls;
    if (int rc = list_slab(c, sw.hoff[p0], sw.hoff[p1], &ls)) return rc;
    if (nnz > 0) {
      if (int rc = letkf_obs_search_dev(c, &tab, p1 - p0, ri + p0, rj + p0, rlev + p0, rz + p0, 1, nullptr, sw.off + p0, ls.idx, ls.rd, ls.rl))
        return rc;
      if (int rc = efso_run_slab(c, a, p0, p1 - p0, sw.off, &ls, sw.hoff[p0], sw.hoff[p1])) return rc;
    }
    p0 = p1;
  }
  return LETKF_OK;
} LETKF_ENTRY_END(letkf_efso_search_dev)

// (13) EFSO's front end: the fcer assembly (efso.f90:100-117) and lnorm (efso_tools.f90:52-156) in SCALE's frame
int letkf_efso_norm_dev(letkf_ctx* c, const letkf_efso_norm_params* prm, int64_t nij1, int32_t nlev, double* fcst, int64_t sp,
                        int64_t sm, int64_t sv, double* fmean, double* fcer, int64_t fsp, int64_t fsv, const double* xf,
                        const double* xg, const double* xa, const double* wlev, const double* wg1, const double* lon,
                        const double* lat) try {
  if (int rc = check_ctx(c)) return rc;
  if (!prm || !fcst || !fcer) return fail(LETKF_E_INVALID, "prm, fcst and fcer must not be NULL");
  const letkf_efso_norm_params& q = *prm;
  if (nij1 < 1 || nlev < 1) return fail(LETKF_E_INVALID, "nij1 and nlev must be >= 1");
  if (q.k < 2) return fail(LETKF_E_INVALID, "k must be >= 2");
  if (q.nv < 1 || q.nv > 32) return fail(LETKF_E_INVALID, "nv must lie in 1..32");
  auto slot = [&](int32_t i) { return i >= 0 && i < q.nv; };
  if (!slot(q.iv_u) || !slot(q.iv_v) || !slot(q.iv_t) || !slot(q.iv_q))
    return fail(LETKF_E_INVALID, "iv_u, iv_v, iv_t and iv_q must lie in 0..nv-1");
  if (!wlev && !slot(q.iv_p)) return fail(LETKF_E_INVALID, "iv_p must lie in 0..nv-1 when wlev is NULL");
  if (q.tar_minlev > q.tar_maxlev) return fail(LETKF_E_INVALID, "tar_minlev > tar_maxlev");
  if ((xf != nullptr) != (xg != nullptr) || (xf != nullptr) != (xa != nullptr))
    return fail(LETKF_E_INVALID, "xf, xg and xa: all three or none");
  if ((lon != nullptr) != (lat != nullptr)) return fail(LETKF_E_INVALID, "lon and lat: both or none");
  if (!(std::isfinite(q.cp) && q.cp > 0.0) || !(std::isfinite(q.tref) && q.tref > 0.0))
    return fail(LETKF_E_INVALID, "cp and tref must be finite and > 0");
  if (!(std::isfinite(q.wmoist) && q.wmoist >= 0.0) || !std::isfinite(q.hvap))
    return fail(LETKF_E_INVALID, "wmoist must be finite and >= 0, hvap finite");
  letkf::EfsoNormArgs a{};
  a.k = q.k;
  a.nv = q.nv;
  a.nij1 = nij1;
  a.npts = nij1 * nlev;
  a.lev0 = (long)q.tar_minlev - 1;
  a.lev1 = (long)q.tar_maxlev - 1;
  for (int v = 0; v < q.nv; ++v)    // lnorm's IF / ELSE IF order
    a.cls[v] = (v == q.iv_u || v == q.iv_v) ? 1 : v == q.iv_t ? 2 : v == q.iv_q ? 3 : 0;
  a.rinbv = 1.0 / (double)q.k;
  a.cptr = std::sqrt(q.cp / q.tref);
  a.qweight = std::sqrt(q.wmoist / (q.cp * q.tref)) * q.hvap;
  a.km1 = (double)(q.k - 1);
  a.minlon = q.tar_minlon;
  a.maxlon = q.tar_maxlon;
  a.minlat = q.tar_minlat;
  a.maxlat = q.tar_maxlat;
  a.fcst = fcst;
  a.sp = sp;
  a.sm = sm;
  a.sv = sv;
  a.fmean = fmean;
  a.fcer = fcer;
  a.fsp = fsp;
  a.fsv = fsv;
  a.xf = xf;
  a.xg = xg;
  a.xa = xa;
  a.wg1 = wg1;
  a.lon = lon;
  a.lat = lat;
  a.wl = wlev;
  c->last_path = letkf::efso_norm_path_name(q.k);
  if (!wlev) {
    // dp/ps from the mean pressure; the bad-column count read back before any output is written
    const size_t nb = align256((size_t)a.npts * 8);
    if (int rc = grow(c, &c->scratch, 2 * nb + 256)) return rc;
    double* pbar = reinterpret_cast<double*>(c->scratch.p);
    double* w = reinterpret_cast<double*>(c->scratch.p + nb);
    unsigned* bad = reinterpret_cast<unsigned*>(c->scratch.p + 2 * nb);
    HIP_TRY(hipMemsetAsync(bad, 0, 4, c->stream));
    HIP_TRY(letkf::launch_efso_dpw(nij1, nlev, q.k, fcst + q.iv_p * sv, sp, sm, a.rinbv, pbar, w, bad, c->num_cu, c->stream));
    unsigned nbad = 0;
    HIP_TRY(hipMemcpyAsync(&nbad, bad, 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->last_path = std::string("efso_pmean_kernel + efso_dpw_kernel + ") + c->last_path;
    if (nbad)
      return fail(LETKF_E_INVALID, std::to_string(nbad) + " column(s) with dp <= 0, ps <= 0 or a non-finite mean pressure");
    a.wl = w;
  }
  HIP_TRY(letkf::launch_efso_norm(a, c->num_cu, c->stream));
  return LETKF_OK;
} LETKF_ENTRY_END(letkf_efso_norm_dev)

// (13) EFSO's back end: print_obsense's table (efso_tools.f90:232-253) for every term
int letkf_efso_summary_dev(letkf_ctx* c, int32_t nterm, int64_t nobs, const double* obsense, const int32_t* elm,
                           const int32_t* typ, const double* lat, const int32_t* qc, int32_t nid, const int32_t* elem_uid,
                           int32_t nobtype, double latbound, int32_t* count, double* sum, int32_t* nneg) try {
  if (int rc = check_ctx(c)) return rc;
  if (nterm < 1 || nterm > 4) return fail(LETKF_E_INVALID, "nterm must lie in 1..4");
  if (nobs < 0 || nobs > 0x7fffffffLL) return fail(LETKF_E_INVALID, "nobs must lie in 0..2^31-1");
  if (nid < 1 || nid > 32 || !elem_uid) return fail(LETKF_E_INVALID, "bad element table (nid 1..32, elem_uid)");
  if (nobtype < 1 || nobtype > 4096) return fail(LETKF_E_INVALID, "nobtype must lie in 1..4096");
  if (!std::isfinite(latbound)) return fail(LETKF_E_INVALID, "latbound must be finite");
  if (!count || !sum || !nneg) return fail(LETKF_E_INVALID, "an output (count, sum, nneg) is NULL");
  if (nobs > 0 && (!obsense || !elm || !typ || !lat)) return fail(LETKF_E_INVALID, "obsense, elm, typ or lat is NULL");
  const unsigned nbins = 3u * (unsigned)(nobtype + 1) * (unsigned)nid;
  size_t sort_b = 0, scan_b = 0;
  const size_t need = letkf::efso_summary_ws(nobs, nbins, c->stream, &sort_b, &scan_b);
  if (!need) return fail(LETKF_E_HIP, "rocprim workspace query failed");
  if (int rc = grow(c, &c->scratch, need)) return rc;
  HIP_TRY(letkf::launch_efso_summary(nterm, nobs, obsense, elm, typ, lat, qc, nid, elem_uid, nobtype, latbound, count, sum,
                                     nneg, c->scratch.p, sort_b, scan_b, c->num_cu, c->stream));
  c->last_path = "efso_bin_kernel + rocprim radix_sort_pairs + efso_binsum_kernel";
  return LETKF_OK;
} LETKF_ENTRY_END(letkf_efso_summary_dev)

}  // extern "C"
