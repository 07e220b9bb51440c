// letkf_api_search.hip -- C ABI, obs_local: the point search and the column search (with the rings of the dense limited case).

#include "letkf_api_internal.h"

using namespace letkf::api;

namespace letkf::api {

// does any combined type carry a MAX_NOBS_PER_GRID limit?  From the host's hint when given, else read back (one sync)
int tables_limited(letkf_ctx* c, const letkf_search_tables* t, bool* limited) {
  if (t->limit_hint == 1 || t->limit_hint == 2) {
    *limited = t->limit_hint == 2;
    return LETKF_OK;
  }
  std::vector<int32_t> mx(t->nctype);
  HIP_TRY(hipMemcpyAsync(mx.data(), t->max_nobs, sizeof(int32_t) * t->nctype, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  *limited = false;
  for (int ic = 0; ic < t->nctype; ++ic) *limited |= mx[ic] > 0;
  return LETKF_OK;
}

// the tables with what the host now knows of the limits: the fill passes of an entry's chunks read nothing back
int tables_hinted(letkf_ctx* c, const letkf_search_tables* t, letkf_search_tables* tab) {
  *tab = *t;
  if (tab->limit_hint != 1 && tab->limit_hint != 2) {
    bool limited = false;
    if (int rc = tables_limited(c, t, &limited)) return rc;
    tab->limit_hint = limited ? 2 : 1;
  }
  return LETKF_OK;
}

}  // namespace letkf::api

extern "C" {

int letkf_obs_search_dev(letkf_ctx* c, const letkf_search_tables* t, int64_t npts, const double* ri, const double* rj,
                         const double* rlev, const double* rz, int32_t fill, int32_t* counts, const int64_t* obs_off,
                         int32_t* obs_idx, double* rdiag_l, double* rloc_l) try {
  if (int rc = check_ctx(c)) return rc;
  if (!t || npts < 0) return fail(LETKF_E_INVALID, "tables is NULL or npts < 0");
  if (npts == 0) return LETKF_OK;
  if (!ri || !rj || !rlev || !rz) return fail(LETKF_E_INVALID, "a point coordinate array is NULL");
  if (t->nctype < 1 || t->ngroup < 1 || t->criterion < 1 || t->criterion > 3)
    return fail(LETKF_E_INVALID, "bad nctype / ngroup / criterion");
  if (fill ? (!obs_off || !obs_idx || !rdiag_l || !rloc_l) : !counts)
    return fail(LETKF_E_INVALID, "missing output array for this phase");
  letkf::SearchArgs a;
  a.t = *t;
  a.npts = npts;
  a.ri = ri;
  a.rj = rj;
  a.rlev = rlev;
  a.rz = rz;
  a.fill = fill;
  a.counts = counts;
  a.obs_off = reinterpret_cast<const long*>(obs_off);
  a.obs_idx = obs_idx;
  a.rdiag_l = rdiag_l;
  a.rloc_l = rloc_l;
  {   // MAX_NOBS_PER_GRID anywhere?  (the fill phase then gets its LDS candidate cache)
    bool limited = false;
    if (int rc = tables_limited(c, t, &limited)) return rc;
    a.limited = limited ? 1 : 0;
  }
  HIP_TRY(letkf::launch_search(a, c->num_cu, c->stream));
  return LETKF_OK;
} LETKF_ENTRY_END(letkf_obs_search_dev)

namespace {
// The limited column search on DENSE observations (letkf_search.hip, rings).  *taken = false: not eligible / not dense -- the
// caller goes on with the LDS-buffered column kernel.
int search_columns_rings(letkf_ctx* c, const letkf_search_tables* t, int64_t nij1, int32_t nlev, const double* rig,
                         const double* rjg, const double* rlev, const double* rz, int32_t fill, int32_t* counts,
                         const int64_t* obs_off, int32_t* obs_idx, double* rdiag_l, double* rloc_l, int32_t* nobs_ctype,
                         double* cutd_ctype, bool* taken) {
  *taken = false;
  if (c->limited_rings == 0 || t->criterion > 3 || t->nctype > 64 || nij1 * (int64_t)t->ngroup >= 0x7fffffff) return LETKF_OK;
  const void* key[5] = {t->ob_ri, t->ac_ext, t->max_nobs, rig, rjg};
  if (c->limited_rings == 2 && c->ring_no_n == nij1 && c->ring_no_crit == t->criterion && std::equal(key, key + 5, c->ring_no)) {
    if (!c->ring_keep) c->ring_no_n = -1;   // (a count -> fill pair: used once)
    return LETKF_OK;
  }
  c->ring_no_n = -1;
  std::vector<int32_t> mx(t->nctype), gstart(t->ngroup + 1);
  HIP_TRY(hipMemcpyAsync(gstart.data(), t->group_start, sizeof(int32_t) * (t->ngroup + 1), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipMemcpyAsync(mx.data(), t->max_nobs, sizeof(int32_t) * t->nctype, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  std::vector<int32_t> gmem(gstart[t->ngroup]);
  HIP_TRY(hipMemcpy(gmem.data(), t->group_member, sizeof(int32_t) * gmem.size(), hipMemcpyDeviceToHost));
  int nlim = 0;
  std::vector<double> vl;
  // The weight criterion orders like the distance where a group has ONE variable-localisation factor: the plain rings serve.
  // Several factors in a group, and the error criterion (3), take the GENERAL ring key (r4, letkf_search.hip ring_offset): an
  // offset per entry, the group's smallest one as its reference.
  bool gen = t->criterion == 3;
  if (t->criterion >= 2) {
    vl.resize(t->nctype);
    HIP_TRY(hipMemcpy(vl.data(), t->varloc, sizeof(double) * t->nctype, hipMemcpyDeviceToHost));
  }
  for (int g = 0; g < t->ngroup; ++g) {
    const int nm = mx[gmem[gstart[g]]];
    if (nm > letkf::search_rings_max_nobs()) return LETKF_OK;
    nlim += nm > 0;
    if (nm > 0 && t->criterion == 2)
      for (int m = gstart[g] + 1; m < gstart[g + 1]; ++m)
        if (vl[gmem[m]] != vl[gmem[gstart[g]]]) gen = true;
  }
  if (nlim == 0) return LETKF_OK;
  const int ng = t->ngroup;
  const size_t ncg = (size_t)nij1 * ng;
  // aux: survivor counts and offsets per (column, group), and behind them roff | kref [ngroup] | min err [nctype] (general ring key)
  const size_t nring1 = (size_t)letkf::search_rings_count() + 1;   // ring starts per (column, group)
  const size_t roff_b = align256(ncg * nring1 * 4);
  ScanWs sw;
  if (int rc = scan_ws(c, &c->ring_aux, ncg, roff_b + ((size_t)ng + (size_t)t->nctype) * 8, &sw)) return rc;
  int32_t* roff = reinterpret_cast<int32_t*>(sw.tail);
  double* kref = nullptr;
  if (gen) {
    // reference offsets: the smallest offset an entry of the group can have -- criterion 2: -2 ln(largest factor); criterion 3:
    // 2 ln(smallest error^2 / factor) over the group's types (the smallest error of a type: one small kernel + a read-back)
    kref = reinterpret_cast<double*>(sw.tail + roff_b);
    std::vector<double> emin(t->nctype, 1.0), kr(ng);
    if (t->criterion == 3) {
      HIP_TRY(letkf::launch_ctype_min_err(*t, kref + ng, c->stream));
      HIP_TRY(hipMemcpyAsync(emin.data(), kref + ng, sizeof(double) * t->nctype, hipMemcpyDeviceToHost, c->stream));
      HIP_TRY(hipStreamSynchronize(c->stream));
    }
    for (int g = 0; g < ng; ++g) {
      double lo = 1e300;
      for (int m = gstart[g]; m < gstart[g + 1]; ++m) {
        const int ic = gmem[m];
        if (!(vl[ic] > 0.0)) continue;
        const double off = t->criterion == 2 ? -2.0 * std::log(vl[ic]) : 2.0 * std::log(emin[ic] * emin[ic] / vl[ic]);
        if (off == off && off < lo) lo = off;
      }
      kr[g] = lo < 1e299 ? lo : 0.0;
    }
    HIP_TRY(hipMemcpyAsync(kref, kr.data(), sizeof(double) * ng, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));   // (kr goes out of scope)
  }
  if (c->ring_keep && c->ring_ready) {
    // (a later call of the same letkf_das_columns_dev: same tables, same columns -- the ring-ordered survivors are still there)
    *taken = true;
    HIP_TRY(letkf::launch_search_rings(*t, 0, nij1, nij1, nlev, rlev, rz, fill, counts, reinterpret_cast<const long*>(obs_off), obs_idx,
                                       rdiag_l, rloc_l, nobs_ctype, cutd_ctype, reinterpret_cast<const long*>(sw.off),
                                       reinterpret_cast<double*>(c->ring_ws.p), roff, kref, c->num_cu, c->stream));
    return LETKF_OK;
  }
  HIP_TRY(zero_total(c, sw));
  HIP_TRY(letkf::launch_ring_survivors(*t, 0, nij1, rig, rjg, 0, sw.counts, nullptr, nullptr, nullptr, nullptr, c->num_cu, c->stream));
  HIP_TRY(scan_offsets(c, sw));
  if (int rc = offsets_to_host(c, sw)) return rc;
  if (c->limited_rings == 2) {
    // dense = more than one in twenty (column, limited group) pairs overflow the column kernel's LDS buffer and would take its
    // multi-sweep fall-back (20 x the cost of a pair that fits); while they fit, that kernel -- everything of a column resident,
    // all levels against it -- is the faster one (C2's grid under a limit of 100: ~450 survivors per pair, 34 against 68 ms)
    size_t n_over = 0, n_lim = 0;
    for (size_t i = 0; i < ncg; ++i)
      if (mx[gmem[gstart[i % ng]]] > 0) {
        ++n_lim;
        n_over += (sw.hoff[i + 1] - sw.hoff[i]) > (int64_t)letkf::search_rings_lds_survivors();
      }
    if (n_over * 20 <= n_lim) {
      if (c->ring_keep || !fill) {   // (remembered for the fill call of this pair / the later calls of this letkf_das_columns_dev)
        std::copy(key, key + 5, c->ring_no);
        c->ring_no_n = nij1;
        c->ring_no_crit = t->criterion;
      }
      return LETKF_OK;
    }
  }
  *taken = true;
  // LETKF_OPT_RING_BATCH_MB (8 GiB) of survivors per batch of columns; inside letkf_das_columns_dev ONE batch, kept for the calls that follow, where
  // that takes no more than half of the device memory still free (configs[3] with two limited types: 128 GiB)
  bool keep = false;
  if (c->ring_keep) {
    size_t fr = 0, tot = 0;
    HIP_TRY(hipMemGetInfo(&fr, &tot));
    const size_t want = (size_t)sw.hoff[ncg] * 32 + 256;
    keep = want <= c->ring_ws.cap + fr / 2;
    if (keep && want > c->ring_ws.cap) {
      // the exact size (grow would ask for a quarter more), and a failure is no error: the batches below need 8 GiB
      if (int rc = drop(c, &c->ring_ws)) return rc;
      if (alloc(&c->ring_ws, want) != hipSuccess) {
        (void)hipGetLastError();
        keep = false;
      }
    }
  }
  const int64_t budget = keep ? sw.hoff[ncg] * 32 + 256 : ((int64_t)c->ring_batch_mb << 20);
  int64_t c0 = 0;
  while (c0 < nij1) {
    const int64_t c1 = chunk_end(sw.hoff, c0, nij1, ng, 32, budget);
    double* sv = nullptr;
    if (int rc = survivor_slab(c, &c->ring_ws, sw.hoff[(size_t)c0 * ng], sw.hoff[(size_t)c1 * ng], &sv)) return rc;
    const long* gq = reinterpret_cast<const long*>(sw.off + (size_t)c0 * ng);
    int32_t* rq = roff + (size_t)c0 * ng * nring1;
    HIP_TRY(letkf::launch_ring_survivors(*t, c0, c1 - c0, rig, rjg, 1, nullptr, gq, sv, rq, kref, c->num_cu, c->stream));
    HIP_TRY(letkf::launch_search_rings(*t, c0, c1 - c0, nij1, nlev, rlev, rz, fill, counts, reinterpret_cast<const long*>(obs_off),
                                       obs_idx, rdiag_l, rloc_l, nobs_ctype, cutd_ctype, gq, sv, rq, kref, c->num_cu, c->stream));
    c0 = c1;
  }
  c->ring_ready = keep;
  return LETKF_OK;
}
}  // namespace

int letkf_obs_search_columns_dev(letkf_ctx* c, const letkf_search_tables* t, int64_t nij1, int32_t nlev,
                                 const double* rig, const double* rjg, const double* rlev, const double* rz,
                                 int32_t fill, int32_t* counts, const int64_t* obs_off, int32_t* obs_idx,
                                 double* rdiag_l, double* rloc_l, int32_t* nobs_ctype, double* cutd_ctype) try {
  if (int rc = check_ctx(c)) return rc;
  if (!t || nij1 < 0 || nlev < 1) return fail(LETKF_E_INVALID, "tables is NULL or bad nij1 / nlev");
  if (nij1 == 0) return LETKF_OK;
  if (!rig || !rjg || !rlev || !rz) return fail(LETKF_E_INVALID, "a point coordinate array is NULL");
  if (t->nctype < 1 || t->ngroup < 1 || t->criterion < 1 || t->criterion > 3)
    return fail(LETKF_E_INVALID, "bad nctype / ngroup / criterion");
  if (fill ? (!obs_off || !obs_idx || !rdiag_l || !rloc_l) : !counts)
    return fail(LETKF_E_INVALID, "missing output array for this phase");
  if ((size_t)4 * (4 * 512 + 2 * ((nlev + 1) & ~1)) * sizeof(double) > c->lds_max ||
      (size_t)4 * (4 * 576 + ((nlev + 1) & ~1)) * sizeof(double) + 4608 > c->lds_max)
    return fail(LETKF_E_INVALID, "too many levels for the column kernel's LDS counters");
  bool limited = false;
  if (int rc = tables_limited(c, t, &limited)) return rc;
  if (limited) {
    bool taken = false;
    if (int rc = search_columns_rings(c, t, nij1, nlev, rig, rjg, rlev, rz, fill, counts, obs_off, obs_idx, rdiag_l, rloc_l,
                                      nobs_ctype, cutd_ctype, &taken))
      return rc;
    if (taken) return LETKF_OK;
  }
  if (limited || cutd_ctype)
    HIP_TRY(letkf::launch_search_columns_limited(*t, nij1, nlev, rig, rjg, rlev, rz, fill, counts,
                                                 reinterpret_cast<const long*>(obs_off), obs_idx, rdiag_l, rloc_l,
                                                 nobs_ctype, cutd_ctype, c->num_cu, c->stream));
  else
    HIP_TRY(letkf::launch_search_columns(*t, nij1, nlev, rig, rjg, rlev, rz, fill, counts,
                                         reinterpret_cast<const long*>(obs_off), obs_idx, rdiag_l, rloc_l, nobs_ctype,
                                         c->num_cu, c->stream));
  return LETKF_OK;
} LETKF_ENTRY_END(letkf_obs_search_columns_dev)

}  // extern "C"
