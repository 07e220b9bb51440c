// letkf_api_das.hip -- C ABI, the analysis entries: das_letkf's loop body on lists, fused with the search, by columns, by weight
// interpolation, and at the observations (das_letkf_obs).

#include "letkf_api_internal.h"

using namespace letkf::api;

namespace letkf::api {

// the counts of a count pass to the caller's nobs_out, if it has one: as the list-free route of letkf_das_columns_dev reports
// them, zero where beta = 0 (the reference does not run obs_local there, letkf_tools.f90:333-359)
int report_counts(letkf_ctx* c, const int32_t* counts, int64_t n, const double* beta, int32_t* nobs_out) {
  if (!nobs_out) return LETKF_OK;
  HIP_TRY(hipMemcpyAsync(nobs_out, counts, (size_t)n * 4, hipMemcpyDeviceToDevice, c->stream));
  if (beta) HIP_TRY(letkf::launch_zero_counts_where_beta_is_zero(n, beta, nobs_out, c->stream));
  return LETKF_OK;
}

// the loop body's own argument checks (npts > 0); letkf_das_columns_dev runs them before its search writes anything
int das_args_check(const letkf_das_args* g, bool lists) {
  if (g->k < 2 || g->nv < 1 || g->npts < 0) return fail(LETKF_E_INVALID, "bad k/nv/npts");
  if ((lists && !g->obs_off) || !g->gues || !g->anal || !g->infl)
    return fail(LETKF_E_INVALID, "a required device pointer is NULL");
  if (g->kld < g->k + (g->det_run ? 1 : 0)) return fail(LETKF_E_INVALID, "kld too small for k (+1 with det_run)");
  if (g->iv_p < 0 || g->iv_p >= g->nv) {
    if (g->q_update_top > 0.0) return fail(LETKF_E_INVALID, "iv_p out of range");
  }
  return LETKF_OK;
}

// The rule switches and the state of a call, as every kernel of the loop body reads them (mode 0; the rest is zero)
static void point_args(const letkf_das_args* g, letkf::PointArgs* a) {
  std::memset(a, 0, sizeof(*a));
  a->k = g->k;
  a->nv = g->nv;
  a->npts = g->npts;
  a->ensval = g->ensval;
  a->kld = g->kld;
  a->dep = g->dep;
  a->det_run = g->det_run;
  a->infl_adaptive = g->infl_adaptive;
  a->relax_to_inflated_prior = g->relax_to_inflated_prior;
  a->iv_p = g->iv_p;
  a->iv_q_first = g->iv_q_first;
  a->iv_q_last = g->iv_q_last;
  a->relax_alpha = g->relax_alpha;
  a->relax_alpha_spread = g->relax_alpha_spread;
  a->q_update_top = g->q_update_top;
  a->q_sprd_max = g->q_sprd_max;
  a->beta = g->beta;
  a->infl = g->infl;
  a->infl_sv = g->infl_sv > 0 ? g->infl_sv : g->npts;
  a->gues = g->gues;
  a->anal = g->anal;
  a->sp = g->sp;
  a->sm = g->sm;
  a->sv = g->sv;
  a->status = g->status;
  a->rtps_out = g->rtps_infl_out;
  a->var_mask = g->var_mask ? g->var_mask : ~0u;
}

// shared by the list-driven and the fused-search entry
int das_points_impl(letkf_ctx* c, const letkf_das_args* g, const letkf_search_tables* t, const double* ri, const double* rj,
                    const double* rlev, const double* rz, int32_t* nobs_out, const SurvivorView* sview) {
  if (int rc = check_ctx(c)) return rc;
  if (!g) return fail(LETKF_E_INVALID, "args is NULL");
  if (g->npts == 0) return LETKF_OK;
  if (int rc = das_args_check(g, !t)) return rc;
  letkf::PointArgs a;
  point_args(g, &a);
  a.obs_off = reinterpret_cast<const long*>(g->obs_off);
  a.obs_idx = g->obs_idx;
  a.rdiag_l = g->rdiag_l;
  a.rloc_l = g->rloc_l;
  a.trans_out = g->trans_out;
  a.transm_out = g->transm_out;
  a.pa_out = g->pa_out;
  a.nsweep = g->nsweep;
  if (t && sview) {
    a.mode = 3;
    a.stab = *t;
    a.prlev = rlev;
    a.prz = rz;
    a.nobs_out = nobs_out;
    a.sv_off = reinterpret_cast<const long*>(sview->sv_off);
    a.surv = sview->sv;
    a.pt_stride = sview->pt_stride;
    a.pt0 = sview->pt0;
    a.sl_cap = (sview->cap + 3) & ~(int64_t)3;
  } else if (t) {
    if (!ri || !rj || !rlev || !rz) return fail(LETKF_E_INVALID, "a point coordinate array is NULL");
    if (t->nctype < 1 || t->ngroup < 1) return fail(LETKF_E_INVALID, "bad nctype / ngroup");
    if (!letkf::wave_kernel_supports(g->k, g->nv, 2))
      return fail(LETKF_E_INVALID, "the fused search needs the one-wave kernel (k <= 62, nv = 11): build lists with "
                                   "letkf_obs_search_dev and call letkf_das_points_dev instead");
    // only the no-limit mode of obs_local is fused (letkf_tools.f90:1438-1476)
    bool limited = false;
    if (int rc = tables_limited(c, t, &limited)) return rc;
    if (limited)
      return fail(LETKF_E_INVALID, "MAX_NOBS_PER_GRID > 0: build lists with letkf_obs_search_columns_dev / "
                                   "letkf_obs_search_dev (radix select) and call letkf_das_points_dev");
    if (g->trans_out || g->pa_out) return fail(LETKF_E_INVALID, "the fused search has no k x k outputs");
    a.mode = 2;
    a.stab = *t;
    a.pri = ri;
    a.prj = rj;
    a.prlev = rlev;
    a.prz = rz;
    a.nobs_out = nobs_out;
  }
  return launch(c, a, g->warm_run < 0 ? 0 : g->warm_run, g->warm_stride);
}

// das_letkf's main loop for a whole subdomain: column search + loop body by slabs of levels whose lists fit a workspace of the
// library (scale/letkf/letkf_tools.f90:313, the level loop).  letkf_das_columns_dev is this with d = NULL; with d
// (letkf_das_columns_nobs_dev, include/letkf_amd_nobsout.h) the searches this function runs anyway also write nobsl_t / cutd_t.
int das_columns_impl(letkf_ctx* c, const letkf_das_args* g, const letkf_search_tables* t, int64_t nij1, int32_t nlev,
                     const double* rig, const double* rjg, const double* rlev, const double* rz, int64_t list_bytes,
                     int32_t* nobs_out, DasColumnsDiag* d) {
  if (int rc = check_ctx(c)) return rc;
  if (!g || !t) return fail(LETKF_E_INVALID, "args / tables is NULL");
  if (nij1 < 1 || nlev < 1 || g->npts != nij1 * (int64_t)nlev) return fail(LETKF_E_INVALID, "npts must be nij1 * nlev");
  if (!rig || !rjg || !rlev || !rz) return fail(LETKF_E_INVALID, "a point coordinate array is NULL");
  if (g->trans_out || g->transm_out || g->pa_out) return fail(LETKF_E_INVALID, "per-point k x k / w-bar outputs: use letkf_das_points_dev");
  // (the loop body's checks, before the count pass of the list route copies its counts to nobs_out: a refused call writes nothing)
  if (int rc = das_args_check(g, false)) return rc;
  const int64_t npts = g->npts;
  if (list_bytes <= 0) list_bytes = (int64_t)8 << 30;
  // ---- the diagnostics, where asked for: nobsl_t from whichever search pass selects anyway, cutd_t from the limited kernels;
  // tables without a limit have the criterion's default cut-off everywhere, which the caller fills (d->cutd_from_tables)
  int32_t* const dn = d ? d->nobs_ctype : nullptr;
  double* dc = d ? d->cutd_ctype : nullptr;
  bool dlimited = false;
  if (dn || dc) {
    if (t->nctype < 1 || t->ngroup < 1 || t->criterion < 1 || t->criterion > 3)
      return fail(LETKF_E_INVALID, "bad nctype / ngroup / criterion");
    if (int rc = tables_limited(c, t, &dlimited)) return rc;
    if (!dlimited) {
      d->cutd_from_tables = dc != nullptr;
      dc = nullptr;
    }
  }
  // (the unlimited column kernel writes the types it walks: the others keep obs_local's initial zeros, :1380-1383)
  auto zero_diag = [&]() { return dn && !dlimited ? hipMemsetAsync(dn, 0, (size_t)npts * t->nctype * 4, c->stream) : hipSuccess; };
  // ---- the list-free route: where the one-wave kernel serves the call and no combined type has a limit, the horizontal half of
  // obs_local is done once per COLUMN (32 B per survivor) and the vertical half inside the loop body kernel -- no count pass
  // over the levels, no 20 B per (point, observation) written and read back.  Same weights, same order, same analysis to the
  // last bit as the lists give (tests/test_gpu_columns.py).  LETKF_OPT_COLUMN_SURVIVORS = 0 keeps the lists.
  if (c->col_survivors && g->k >= 2 && letkf::wave_kernel_supports(g->k, g->nv, 3) && nij1 <= 0x7fffffff) {
    if (t->nctype < 1 || t->ngroup < 1) return fail(LETKF_E_INVALID, "bad nctype / ngroup");
    bool limited = false;
    if (int rc = tables_limited(c, t, &limited)) return rc;
    if (!limited) {
      // ---- survivor count per column, prefix sum, the offsets back to the host
      ScanWs sw;
      if (int rc = scan_ws(c, &c->scratch, (size_t)nij1, 0, &sw)) return rc;
      HIP_TRY(zero_total(c, sw));
      HIP_TRY(letkf::launch_survivors(*t, 0, nij1, rig, rjg, 0, sw.counts, nullptr, nullptr, c->num_cu, c->stream));
      HIP_TRY(scan_offsets(c, sw));
      if (int rc = offsets_to_host(c, sw)) return rc;
      // (2 = automatic: the list-free route where the lists of all levels would not fit the workspace at once -- about half
      // of a column's horizontal survivors pass a level's vertical cut-off, 20 B each.  Where they fit, one fill pass for
      // the whole domain is cheaper than the vertical half inside the register-bound loop body kernel: C2, 203 local
      // observations per point, 384 against 394 ms per analysis; BASELINE configs[3], 4900 per point, 40 slabs: 7.45 against 6.11 s.)
      const bool take = c->col_survivors == 1 || (double)sw.hoff[nij1] * (double)nlev * 10.0 > (double)list_bytes;
      // batches of columns whose survivors fit the workspace (32 B each)
      int64_t c0 = take ? 0 : nij1;
      while (c0 < nij1) {
        const int64_t c1 = chunk_end(sw.hoff, c0, nij1, 1, 32, list_bytes);
        double* sv = nullptr;
        if (int rc = survivor_slab(c, &c->list_ws, sw.hoff[c0], sw.hoff[c1], &sv)) return rc;
        HIP_TRY(letkf::launch_survivors(*t, c0, c1 - c0, rig, rjg, 1, nullptr, reinterpret_cast<const long*>(sw.off + c0), sv, c->num_cu,
                                        c->stream));
        letkf_das_args a = *g;
        a.npts = (c1 - c0) * (int64_t)nlev;
        a.infl_sv = g->infl_sv > 0 ? g->infl_sv : npts;
        a.warm_stride = (int32_t)(c1 - c0);                   // runs up the columns
        int64_t cap = 0;
        for (int64_t cc = c0; cc < c1; ++cc) cap = std::max(cap, sw.hoff[cc + 1] - sw.hoff[cc]);
        SurvivorView sview{sw.off + c0, sv, nij1, c0, cap};
        if (int rc = das_points_impl(c, &a, t, nullptr, nullptr, rlev, rz, nobs_out, &sview)) return rc;
        c0 = c1;
      }
      if (take) {
        // (no search by point ran: the unlimited column kernel's count pass, its counts into the scratch buffer the loop is done with)
        if (dn) {
          ScanWs cw;
          if (int rc = scan_ws(c, &c->scratch, (size_t)npts, 0, &cw)) return rc;
          HIP_TRY(zero_diag());
          if (int rc = letkf_obs_search_columns_dev(c, t, nij1, nlev, rig, rjg, rlev, rz, 0, cw.counts, nullptr, nullptr, nullptr, nullptr,
                                                    dn, nullptr))
            return rc;
        }
        return LETKF_OK;
      }
    }
  }
  // (the searches below -- one count pass, a fill pass per slab -- share the ring-ordered survivors of the dense limited case)
  RingKeep ring_keep_guard(c);
  // ---- count pass over all levels, prefix sum, level boundaries back to the host
  ScanWs sw;
  if (int rc = count_columns(c, t, nij1, nlev, rig, rjg, rlev, rz, &sw)) return rc;
  if (int rc = report_counts(c, sw.counts, npts, g->beta, nobs_out)) return rc;
  if (int rc = offsets_to_host(c, sw, (size_t)nij1)) return rc;
  const std::vector<int64_t>& lev_off = sw.hoff;
  HIP_TRY(zero_diag());
  // ---- slabs of levels: as many as fit the list workspace (20 B per entry)
  int l0 = 0;
  while (l0 < nlev) {
    const int l1 = (int)chunk_end(lev_off, l0, nlev, 1, 20, list_bytes);
    const int64_t p0 = (int64_t)l0 * nij1, np = (int64_t)(l1 - l0) * nij1;
    ListSlab ls;
    if (!dn && !dc) {
      if (int rc = fill_columns(c, t, nij1, l0, l1, rig, rjg, rlev, rz, sw, &ls)) return rc;
    } else {   // (fill_columns with the diagnostics of the slab's points)
      if (int rc = list_slab(c, lev_off[(size_t)l0], lev_off[(size_t)l1], &ls)) return rc;
      if (int rc = letkf_obs_search_columns_dev(c, t, nij1, l1 - l0, rig, rjg, rlev + p0, rz + p0, 1, nullptr, sw.off + p0, ls.idx, ls.rd,
                                                ls.rl, dn ? dn + p0 * t->nctype : nullptr, dc ? dc + p0 * t->nctype : nullptr))
        return rc;
    }
    letkf_das_args a = *g;
    a.npts = np;
    a.obs_off = sw.off + p0;
    a.obs_idx = ls.idx;
    a.rdiag_l = ls.rd;
    a.rloc_l = ls.rl;
    a.gues = g->gues + p0 * g->sp;
    a.anal = g->anal + p0 * g->sp;
    if (g->beta) a.beta = g->beta + p0;
    a.infl = g->infl + p0;
    a.infl_sv = g->infl_sv > 0 ? g->infl_sv : npts;
    if (g->status) a.status = g->status + p0;
    if (g->nsweep) a.nsweep = g->nsweep + p0;
    if (g->rtps_infl_out) a.rtps_infl_out = g->rtps_infl_out + p0;
    a.warm_stride = (l1 - l0 > 1) ? (int32_t)nij1 : 0;      // runs up the columns of the slab
    if (nij1 > 0x7fffffff) a.warm_stride = 0;
    if (int rc = das_points_impl(c, &a, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr)) return rc;
    l0 = l1;
  }
  return LETKF_OK;
}

}  // namespace letkf::api

extern "C" {

int letkf_das_points_dev(letkf_ctx* c, const letkf_das_args* g) try {
  return das_points_impl(c, g, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
} LETKF_ENTRY_END(letkf_das_points_dev)

int letkf_das_points_fused_dev(letkf_ctx* c, const letkf_das_args* g, const letkf_search_tables* t, const double* ri,
                               const double* rj, const double* rlev, const double* rz, int32_t* nobs_out) try {
  if (!t) return fail(LETKF_E_INVALID, "tables is NULL");
  return das_points_impl(c, g, t, ri, rj, rlev, rz, nobs_out);
} LETKF_ENTRY_END(letkf_das_points_fused_dev)

// (3c) das_letkf's main loop for a whole subdomain (das_columns_impl above)
int letkf_das_columns_dev(letkf_ctx* c, const letkf_das_args* g, const letkf_search_tables* t, int64_t nij1, int32_t nlev,
                          const double* rig, const double* rjg, const double* rlev, const double* rz, int64_t list_bytes,
                          int32_t* nobs_out) try {
  return das_columns_impl(c, g, t, nij1, nlev, rig, rjg, rlev, rz, list_bytes, nobs_out, nullptr);
} LETKF_ENTRY_END(letkf_das_columns_dev)

// (3d) weight interpolation (include/letkf_amd_interp.h): letkf_core at the coarse points of a tile by slabs of levels -- the
// column search on the coarse columns, the lists gathered into the batch form of letkf_core_batch_dev, every solver route with
// T, w-bar (and w-bar_det) kept -- then the blend and the apply at every fine point of the slab (letkf_interp.hip)
int letkf_das_interp_dev(letkf_ctx* c, const letkf_das_args* g, const letkf_search_tables* t, const letkf_interp_args* ia) try {
  return letkf_das_interp_window_dev(c, g, t, ia, nullptr);
} LETKF_ENTRY_END(letkf_das_interp_dev)

// ... on the coarse lattice of a whole domain, for the window of it that the call owns (include/letkf_amd_interp_window.h);
// without a window the arrays are the domain
int letkf_das_interp_window_dev(letkf_ctx* c, const letkf_das_args* g, const letkf_search_tables* t, const letkf_interp_args* ia,
                                const letkf_interp_window* win) try {
  if (int rc = check_ctx(c)) return rc;
  if (!g || !t || !ia) return fail(LETKF_E_INVALID, "args / tables / interp is NULL");
  if (ia->nx < 1 || ia->ny < 1 || ia->nlev < 1 || g->npts != (int64_t)ia->nx * ia->ny * ia->nlev)
    return fail(LETKF_E_INVALID, "npts must be nx * ny * nlev");
  if (ia->stride_x < 1 || ia->stride_x > 8 || ia->stride_y < 1 || ia->stride_y > 8) return fail(LETKF_E_INVALID, "strides must be 1..8");
  if (g->k > 128) return fail(LETKF_E_INVALID, "weight interpolation serves k <= 128");
  if (g->infl_adaptive) return fail(LETKF_E_INVALID, "adaptive inflation belongs to solved points: not on the interpolation route");
  if (g->trans_out || g->transm_out || g->pa_out || g->nsweep)
    return fail(LETKF_E_INVALID, "trans_out / transm_out / pa_out / nsweep must be NULL on the interpolation route");
  if (!ia->rig || !ia->rjg || !ia->rlev || !ia->rz) return fail(LETKF_E_INVALID, "a point coordinate array is NULL");
  if (t->nctype < 1 || t->ngroup < 1) return fail(LETKF_E_INVALID, "bad nctype / ngroup");
  if (int rc = das_args_check(g, false)) return rc;
  if (g->nv > 32) return fail(LETKF_E_INVALID, "nv must be <= 32");
  const int k = g->k, nlev = ia->nlev;
  const int64_t budget = ia->ws_bytes > 0 ? ia->ws_bytes : ((int64_t)8 << 30);

  // ---- the coarse set (letkf_interp_coarse_axis / letkf_interp_window_axis and nothing else), its indices and coordinates on
  // the device
  letkf_interp_window whole = {ia->nx, ia->ny, 0, 0, 0, 0, ia->nx, ia->ny};
  const letkf_interp_window& W = win ? *win : whole;
  if (W.gnx < 1 || W.gny < 1 || W.onx < 1 || W.ony < 1) return fail(LETKF_E_INVALID, "window: extents must be >= 1");
  if (W.gi0 < 0 || (int64_t)W.gi0 + ia->nx > W.gnx || W.gj0 < 0 || (int64_t)W.gj0 + ia->ny > W.gny)
    return fail(LETKF_E_INVALID, "window: the array rectangle is not inside the domain");
  if (W.oi0 < 0 || (int64_t)W.oi0 + W.onx > ia->nx || W.oj0 < 0 || (int64_t)W.oj0 + W.ony > ia->ny)
    return fail(LETKF_E_INVALID, "window: the owned rectangle is not inside the arrays");
  std::vector<int32_t> hx((size_t)ia->nx + 2), hy((size_t)ia->ny + 2);
  int32_t ncx = 0, ncy = 0, bad = -1;
  if (win) {
    if (letkf::interp_window_axis(W.gnx, ia->stride_x, W.gi0, ia->nx, W.oi0, W.onx, hx.data(), &ncx, &bad))
      return fail(LETKF_E_INVALID, "window: the needed coarse line x = " + std::to_string(bad) + " (global) lies outside the arrays");
    if (letkf::interp_window_axis(W.gny, ia->stride_y, W.gj0, ia->ny, W.oj0, W.ony, hy.data(), &ncy, &bad))
      return fail(LETKF_E_INVALID, "window: the needed coarse line y = " + std::to_string(bad) + " (global) lies outside the arrays");
  } else if (letkf_interp_coarse_axis(ia->nx, ia->stride_x, hx.data(), &ncx) || letkf_interp_coarse_axis(ia->ny, ia->stride_y, hy.data(), &ncy)) {
    return fail(LETKF_E_INVALID, "bad extent / stride");
  }
  // every cell of the run holds an owned point (the run is the lines that weigh at one): the apply kernel's grid relies on it
  for (int d = 0; d < 2; ++d) {
    const std::vector<int32_t>& h = d ? hy : hx;
    const int nc = d ? ncy : ncx, o0 = d ? W.oj0 : W.oi0, o1 = o0 + (d ? W.ony : W.onx);
    for (int cl = 0; cl < (nc > 1 ? nc - 1 : 1); ++cl) {
      int lo, hi;
      letkf::interp_cell_lines(cl, nc, h[(size_t)cl], h[(size_t)std::min(cl + 1, nc - 1)], o0, o1, &lo, &hi);
      if (hi < lo) return fail(LETKF_E_INVALID, "window: a cell of the coarse run owns no point (internal)");
    }
  }
  const int64_t ncc = (int64_t)ncx * ncy, npc = ncc * nlev;
  const size_t o_iy = align256((size_t)ncx * 4), o_rig = o_iy + align256((size_t)ncy * 4), o_rjg = o_rig + align256((size_t)ncc * 8);
  const size_t o_rlev = o_rjg + align256((size_t)ncc * 8), o_rz = o_rlev + align256((size_t)npc * 8);
  if (int rc = grow(c, &c->interp_fix, o_rz + (size_t)npc * 8 + 256)) return rc;
  letkf::InterpGrid G;
  G.nx = ia->nx;
  G.ny = ia->ny;
  G.nlev = nlev;
  G.ncx = ncx;
  G.ncy = ncy;
  G.ox0 = W.oi0;
  G.ox1 = W.oi0 + W.onx;
  G.oy0 = W.oj0;
  G.oy1 = W.oj0 + W.ony;
  G.ix = reinterpret_cast<const int*>(c->interp_fix.p);
  G.iy = reinterpret_cast<const int*>(c->interp_fix.p + o_iy);
  HIP_TRY(hipMemcpyAsync(c->interp_fix.p, hx.data(), (size_t)ncx * 4, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(c->interp_fix.p + o_iy, hy.data(), (size_t)ncy * 4, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));   // (hx, hy are this call's own)
  letkf::InterpCoordArgs ca;
  ca.G = G;
  ca.rig = ia->rig;
  ca.rjg = ia->rjg;
  ca.rlev = ia->rlev;
  ca.rz = ia->rz;
  ca.crig = reinterpret_cast<double*>(c->interp_fix.p + o_rig);
  ca.crjg = reinterpret_cast<double*>(c->interp_fix.p + o_rjg);
  ca.crlev = reinterpret_cast<double*>(c->interp_fix.p + o_rlev);
  ca.crz = reinterpret_cast<double*>(c->interp_fix.p + o_rz);
  HIP_TRY(letkf::launch_interp_coords(ca, c->num_cu, c->stream));

  // ---- count pass over the coarse points of all levels, prefix sum; level boundaries and the counts back to the host
  RingKeep ring_keep_guard(c);
  ScanWs sw;
  if (int rc = count_columns(c, t, ncc, nlev, ca.crig, ca.crjg, ca.crlev, ca.crz, &sw)) return rc;
  if (ia->nobs_coarse) HIP_TRY(hipMemcpyAsync(ia->nobs_coarse, sw.counts, (size_t)npc * 4, hipMemcpyDeviceToDevice, c->stream));
  std::vector<int32_t> hcount((size_t)npc);
  if (int rc = offsets_to_host(c, sw, (size_t)ncc, hcount.data(), sw.counts, (size_t)npc * 4)) return rc;
  const std::vector<int64_t>& lev_off = sw.hoff;
  std::vector<int32_t> lev_max((size_t)nlev, 0);
  for (int l = 0; l < nlev; ++l)
    for (int64_t cc = 0; cc < ncc; ++cc) lev_max[(size_t)l] = std::max(lev_max[(size_t)l], hcount[(size_t)(l * ncc + cc)]);

  // the rules' switches and the state of the call, as the kernels of this route read them
  letkf::PointArgs P;
  point_args(g, &P);

  // ---- slabs of levels: the lists (20 B per entry), per coarse point the kept k * k + 2 k doubles, rho, count and status, and the
  // gathered rows of the slab's longest list (k + 4 doubles each)
  const int64_t kept = ((int64_t)k * k + 2 * (int64_t)k + 2) * 8;
  auto slab_bytes = [&](int l0, int l1, int nmax) {
    return 20 * (lev_off[(size_t)l1] - lev_off[(size_t)l0]) + (int64_t)(l1 - l0) * ncc * (kept + (int64_t)nmax * (k + 4) * 8);
  };
  std::string solve_path;
  int l0 = 0;
  while (l0 < nlev) {
    int l1 = l0 + 1, nmax = std::max(1, lev_max[(size_t)l0]);
    while (l1 < nlev) {
      const int nm = std::max(nmax, lev_max[(size_t)l1]);
      if (slab_bytes(l0, l1 + 1, nm) > budget) break;
      nmax = nm;
      ++l1;
    }
    const int nl = l1 - l0;
    const int64_t nb = (int64_t)nl * ncc;
    ListSlab ls;
    if (int rc = fill_columns(c, t, ncc, l0, l1, ca.crig, ca.crjg, ca.crlev, ca.crz, sw, &ls)) return rc;
    // T | w-bar | w-bar_det | rho | rdiag | rloc | dep | depd | hdxb | nobsl | status
    const size_t s_T = align256((size_t)nb * k * k * 8), s_w = align256((size_t)nb * k * 8), s_r = align256((size_t)nb * 8);
    const size_t s_o = align256((size_t)nb * nmax * 8), s_h = align256((size_t)nb * nmax * k * 8), s_i = align256((size_t)nb * 4);
    const size_t o_w = s_T, o_wd = o_w + s_w, o_rho = o_wd + s_w, o_rd = o_rho + s_r, o_rl = o_rd + s_o, o_dep = o_rl + s_o;
    const size_t o_depd = o_dep + s_o, o_h = o_depd + s_o, o_n = o_h + s_h, o_st = o_n + s_i;
    if (int rc = grow(c, &c->interp_ws, o_st + s_i + 256)) return rc;
    char* w = c->interp_ws.p;
    letkf::InterpGatherArgs ga;
    ga.G = G;
    ga.A = P;
    ga.l0 = l0;
    ga.nl = nl;
    ga.nobs = nmax;
    ga.obs_off = reinterpret_cast<const long*>(sw.off);
    ga.obs_idx = ls.idx;
    ga.rdiag_l = ls.rd;
    ga.rloc_l = ls.rl;
    ga.nobsl = reinterpret_cast<int*>(w + o_n);
    ga.hdxb = reinterpret_cast<double*>(w + o_h);
    ga.rdiag = reinterpret_cast<double*>(w + o_rd);
    ga.rloc = reinterpret_cast<double*>(w + o_rl);
    ga.dep = reinterpret_cast<double*>(w + o_dep);
    ga.depd = g->det_run ? reinterpret_cast<double*>(w + o_depd) : nullptr;
    ga.rho = reinterpret_cast<double*>(w + o_rho);
    HIP_TRY(letkf::launch_interp_gather(ga, c->num_cu, c->stream));
    // letkf_core at the slab's coarse points, as letkf_core_batch_dev runs it (letkf_tools.f90:420-447: rdiag carries the
    // localisation, transm and transmd are asked for).  Every solve is cold: a warm-start run would tie a point's rounding
    // to the slab it falls in.
    letkf::PointArgs a;
    std::memset(&a, 0, sizeof(a));
    a.k = k;
    a.nv = 0;
    a.var_mask = ~0u;
    a.mode = 1;
    a.npts = nb;
    a.nobsl = ga.nobsl;
    a.hdxb = ga.hdxb;
    a.rdiag = ga.rdiag;
    a.rloc = ga.rloc;
    a.depv = ga.dep;
    a.depd = ga.depd;
    a.nobs = nmax;
    a.rdiag_wloc = 1;
    a.infl = ga.rho;
    a.trans_out = reinterpret_cast<double*>(w);
    a.transm_out = reinterpret_cast<double*>(w + o_w);
    a.transmd_out = g->det_run ? reinterpret_cast<double*>(w + o_wd) : nullptr;
    a.status = reinterpret_cast<int*>(w + o_st);
    if (int rc = launch(c, a, 1, 1)) return rc;
    solve_path = c->last_path;
    letkf::InterpApplyArgs aa;
    aa.G = G;
    aa.A = P;
    aa.l0 = l0;
    aa.nl = nl;
    aa.T = a.trans_out;
    aa.wbar = a.transm_out;
    aa.wbard = a.transmd_out;
    aa.cstatus = a.status;
    HIP_TRY(letkf::launch_interp_apply(aa, c->stream));
    l0 = l1;
  }
  c->last_path = "interp: search_columns + " + solve_path + " + " + letkf::interp_apply_kernel_name(k);
  return LETKF_OK;
} LETKF_ENTRY_END(letkf_das_interp_window_dev)

// (11) das_letkf_obs (scale/letkf/letkf_tools.f90:933-1156): the loop body at every target observation's own location, on
// the two-variable pseudo-state of letkf_obsanal.hip (variable 0 the target, variable 1 its pressure for Q_UPDATE_TOP), in
// chunks of targets whose lists fit list_bytes
int letkf_das_obs_dev(letkf_ctx* c, const letkf_das_obs_args* g, const letkf_search_tables* t) try {
  if (int rc = check_ctx(c)) return rc;
  if (!g || !t) return fail(LETKF_E_INVALID, "args / tables is NULL");
  const int det = g->det_run ? 1 : 0;
  if (g->k < 2) return fail(LETKF_E_INVALID, "ensemble size must be >= 2");
  if (g->ntgt < 0) return fail(LETKF_E_INVALID, "negative ntgt");
  if (g->lda < g->k + det) return fail(LETKF_E_INVALID, "lda too small for k (+1 with det_run)");
  if (g->kld < g->k + det) return fail(LETKF_E_INVALID, "kld too small for k (+1 with det_run)");
  if (!g->ensval || !g->dep || !g->ya) return fail(LETKF_E_INVALID, "a required pointer is NULL (ensval, dep, ya)");
  if (g->ntgt == 0) return LETKF_OK;
  if (g->nobs < 1) return fail(LETKF_E_INVALID, "targets in a table without rows");
  if (g->nobs > 0x7fffffff) return fail(LETKF_E_INVALID, "more than 2^31 observation rows");
  if (t->nctype < 1 || t->ngroup < 1) return fail(LETKF_E_INVALID, "bad nctype / ngroup");
  const int64_t n = g->ntgt;
  const int k = g->k;
  const bool qvar = g->tvar >= 0 && g->tvar >= g->iv_q_first && g->tvar <= g->iv_q_last;
  const bool qtop = qvar && g->q_update_top > 0.0;
  const bool qsprd = g->tvar >= 0 && g->tvar == g->iv_q_first && g->q_sprd_max > 0.0;
  letkf_search_tables tab;
  if (int rc = tables_hinted(c, t, &tab)) return rc;
  // workspace: ri | rj | rlev | rz [n] | infl [2 n] | gues [2 (k + 2) n] | anal [2 (k + 2) n] | flag word
  const size_t nd = (size_t)n, ps = 2 * (size_t)(k + 2) * nd;
  const size_t o_flag = align256((6 * nd + 2 * ps) * 8);
  if (int rc = grow(c, &c->obsanal_ws, o_flag + 256)) return rc;
  double* w = reinterpret_cast<double*>(c->obsanal_ws.p);
  letkf::ObsAnalArgs o;
  std::memset(&o, 0, sizeof(o));
  o.tab = tab;
  o.k = k;
  o.det_run = det;
  o.q_top = qtop ? 1 : 0;
  o.ntgt = n;
  o.nobs = g->nobs;
  o.kld = g->kld;
  o.lda = g->lda;
  o.tgt_row = g->tgt_row;
  o.ensval = g->ensval;
  o.dep = g->dep;
  o.rlev_tgt = g->rlev_tgt;
  o.rz_tgt = g->rz_tgt;
  o.infl = g->infl;
  o.infl_mul = g->infl_mul;
  o.ri = w;
  o.rj = w + nd;
  o.rlev = w + 2 * nd;
  o.rz = w + 3 * nd;
  o.infl_ws = w + 4 * nd;
  o.gues = w + 6 * nd;
  o.anal = w + 6 * nd + ps;
  o.flags = reinterpret_cast<unsigned*>(c->obsanal_ws.p + o_flag);
  o.ya = g->ya;
  o.ya_mean = g->ya_mean;
  o.ya_table = g->ya_table;
  o.dep_a = g->dep_a;
  // ---- targets, count pass, prefix sum; the offsets and the argument flags back to the host (the one synchronisation)
  ScanWs sw;
  unsigned flags = 0;
  if (int rc = scan_ws(c, &c->scratch, nd, 0, &sw)) return rc;
  HIP_TRY(hipMemsetAsync(o.flags, 0, 4, c->stream));
  HIP_TRY(letkf::launch_obsanal_targets(o, c->stream));
  HIP_TRY(zero_total(c, sw));
  if (int rc = letkf_obs_search_dev(c, &tab, n, o.ri, o.rj, o.rlev, o.rz, 0, sw.counts, nullptr, nullptr, nullptr, nullptr)) return rc;
  HIP_TRY(scan_offsets(c, sw));
  if (int rc = offsets_to_host(c, sw, 1, &flags, o.flags, 4)) return rc;
  if (flags & letkf::kObsAnalBadRow) return fail(LETKF_E_INVALID, "a tgt_row entry outside [0, nobs)");
  if (flags & letkf::kObsAnalNoCtype) return fail(LETKF_E_INVALID, "a target row lies in no ctype block of the tables");
  if (flags & letkf::kObsAnalNoCoord)
    return fail(LETKF_E_INVALID, "the tables need a vertical coordinate of the targets that rlev_tgt / rz_tgt does not give");
  if (int rc = report_counts(c, sw.counts, n, g->beta, g->nobs_out)) return rc;
  // ---- chunks of targets whose lists fit the workspace (20 B per entry): fill pass, loop body
  const int64_t list_bytes = g->list_bytes > 0 ? g->list_bytes : ((int64_t)8 << 30);
  letkf_das_args a;
  std::memset(&a, 0, sizeof(a));
  a.k = k;
  a.nv = 2;
  a.det_run = det;
  a.relax_to_inflated_prior = g->relax_to_inflated_prior;
  a.iv_p = 1;
  a.iv_q_first = qvar ? 0 : 2;   // (an empty range beyond the two variables where tvar is no moisture variable)
  a.iv_q_last = qvar ? 0 : 1;
  a.relax_alpha = g->relax_alpha;
  a.relax_alpha_spread = g->relax_alpha_spread;
  a.q_update_top = qtop ? g->q_update_top : 0.0;
  a.q_sprd_max = qsprd ? g->q_sprd_max : 0.0;
  a.ensval = g->ensval;
  a.kld = g->kld;
  a.dep = g->dep;
  a.sp = 1;
  a.sm = n;
  a.sv = n * (int64_t)(k + 2);
  a.warm_run = 1;
  a.var_mask = 1u;
  a.infl_sv = n;
  std::string path;
  for (int64_t p0 = 0; p0 < n;) {
    const int64_t p1 = chunk_end(sw.hoff, p0, n, 1, 20, list_bytes);
    ListSlab ls;
    if (int rc = list_slab(c, sw.hoff[p0], sw.hoff[p1], &ls)) return rc;
    if (int rc = letkf_obs_search_dev(c, &tab, p1 - p0, o.ri + p0, o.rj + p0, o.rlev + p0, o.rz + p0, 1, nullptr, sw.off + p0, ls.idx, ls.rd,
                                      ls.rl))
      return rc;
    a.npts = p1 - p0;
    a.obs_off = sw.off + p0;
    a.obs_idx = ls.idx;
    a.rdiag_l = ls.rd;
    a.rloc_l = ls.rl;
    a.beta = g->beta ? g->beta + p0 : nullptr;
    a.infl = o.infl_ws + p0;
    a.gues = o.gues + p0;
    a.anal = o.anal + p0;
    a.status = g->status ? g->status + p0 : nullptr;
    if (int rc = das_points_impl(c, &a, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr)) return rc;
    path = c->last_path;
    p0 = p1;
  }
  HIP_TRY(letkf::launch_obsanal_finish(o, c->stream));
  c->last_path = "obs_search + " + path + " + obsanal_finish_kernel";
  return LETKF_OK;
} LETKF_ENTRY_END(letkf_das_obs_dev)

int letkf_obs_target_var(int32_t elm) try {
  switch (elm) {
    case 2819: return 0;              // id_u_obs -> iv3d_u
    case 2820: return 1;              // id_v_obs -> iv3d_v
    case 3073: case 3074: return 3;   // id_t_obs, id_tv_obs -> iv3d_t
    case 3330: case 3331: return 5;   // id_q_obs, id_rh_obs -> iv3d_q
    default: return -1;               // ps (nv2d = 0), rain, radar, H08, TC: n = 0
  }
} LETKF_ENTRY_END(letkf_obs_target_var)

}  // extern "C"
