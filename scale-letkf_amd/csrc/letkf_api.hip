// letkf_api.hip -- host side of the C ABI declared in include/letkf_amd.h.
//
// This unit: the context (life cycle, options, stream, timing, last_path), the buffer and scan plumbing that the other
// units of the ABI (letkf_api_*.hip, by area; shared declarations in letkf_api_internal.h) build on, the choice of kernels
// (pick_route) with the launch of a loop-body / letkf_core call, letkf_core_batch_dev, and the host-pointer compatibility
// entry letkf_core_c that the Fortran shim (scale-letkf_amd/fortran) calls.
// Thin by design, and no CPU fallback anywhere: without a device every compute entry returns LETKF_E_NO_DEVICE.

#include <rocprim/device/device_scan.hpp>
#include <rocprim/iterator/transform_iterator.hpp>

#include "letkf_api_internal.h"
#include "letkf_sched_dev.h"

using namespace letkf::api;

namespace letkf {

// int32 counts -> int64 exclusive offsets (rocprim) with the scan's storage at temp; temp == nullptr: *temp_bytes = its size
hipError_t count_scan(void* temp, size_t* temp_bytes, const int32_t* counts, int64_t* off, size_t n, hipStream_t st) {
  auto in = rocprim::make_transform_iterator(counts, [] __device__(int32_t v) { return (int64_t)v; });
  return rocprim::exclusive_scan(temp, *temp_bytes, in, off, (int64_t)0, n, rocprim::plus<int64_t>(), st);
}

}  // namespace letkf

namespace letkf::api {

// Frees one of the context's device buffers.  It may still be read by work on the stream: that work is waited for first.
int drop(letkf_ctx* c, DevBuf* b) {
  HIP_TRY(hipStreamSynchronize(c->stream));
  if (b->p) HIP_TRY(hipFree(b->p));
  b->p = nullptr;
  b->cap = 0;
  return LETKF_OK;
}

hipError_t alloc(DevBuf* b, size_t cap) {   // (of a buffer that holds nothing)
  const hipError_t e = hipMalloc(reinterpret_cast<void**>(&b->p), cap);
  if (e == hipSuccess) b->cap = cap;
  else b->p = nullptr;
  return e;
}

// Grows a buffer to at least `need` bytes: a quarter more than that (+ 4 KiB), or exactly `need` without slack.
int grow(letkf_ctx* c, DevBuf* b, size_t need, bool slack) {
  if (need <= b->cap) return LETKF_OK;
  if (b->p)
    if (int rc = drop(c, b)) return rc;
  HIP_TRY(alloc(b, slack ? need + need / 4 + 4096 : need));
  return LETKF_OK;
}

// lays a ScanWs out in buffer b, grown to hold it
int scan_ws(letkf_ctx* c, DevBuf* b, size_t n, size_t tail_bytes, ScanWs* s) {
  s->n = n;
  HIP_TRY(count_scan(nullptr, &s->temp_bytes, nullptr, nullptr, n + 1, c->stream));
  const size_t o_off = align256((n + 1) * 4), o_scan = o_off + align256((n + 1) * 8);
  const size_t o_tail = o_scan + align256(s->temp_bytes);
  if (int rc = grow(c, b, (tail_bytes ? o_tail + tail_bytes : o_scan + s->temp_bytes) + 256)) return rc;
  s->counts = reinterpret_cast<int32_t*>(b->p);
  s->off = reinterpret_cast<int64_t*>(b->p + o_off);
  s->temp = b->p + o_scan;
  s->tail = b->p + o_tail;
  return LETKF_OK;
}

// in front of the count pass, which writes counts [0, n): the scan runs over n + 1 entries, and the last one is the total
hipError_t zero_total(letkf_ctx* c, const ScanWs& s) { return hipMemsetAsync(s.counts + s.n, 0, 4, c->stream); }
// behind the count pass: the prefix sum ...
hipError_t scan_offsets(letkf_ctx* c, const ScanWs& s) {
  size_t temp_bytes = s.temp_bytes;
  return count_scan(s.temp, &temp_bytes, s.counts, s.off, s.n + 1, c->stream);
}
// ... and offsets 0, stride, 2 stride, .. n back to the host -- with them, behind the same synchronisation (the entry's one),
// `also_bytes` of the caller's own
int offsets_to_host(letkf_ctx* c, ScanWs& s, size_t stride, void* also_dst, const void* also_src, size_t also_bytes) {
  s.hoff.resize(s.n / stride + 1);
  if (stride == 1)
    HIP_TRY(hipMemcpyAsync(s.hoff.data(), s.off, s.hoff.size() * 8, hipMemcpyDeviceToHost, c->stream));
  else
    HIP_TRY(hipMemcpy2DAsync(s.hoff.data(), 8, s.off, stride * 8, 8, s.hoff.size(), hipMemcpyDeviceToHost, c->stream));
  if (also_bytes) HIP_TRY(hipMemcpyAsync(also_dst, also_src, also_bytes, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return LETKF_OK;
}

// The end of the chunk of items that starts at `first`.  Item i has entries off[i * stride] to off[(i + 1) * stride]: at least one
// item, however long its list (the workspace grows to hold it), then as many more, below `end`, as keep the chunk's entries within
// `budget` bytes at entry_bytes each and within max_entries.
int64_t chunk_end(const std::vector<int64_t>& off, int64_t first, int64_t end, int64_t stride, int64_t entry_bytes,
                  int64_t budget, int64_t max_entries) {
  auto ne = [&](int64_t i) { return off[(size_t)(i * stride)] - off[(size_t)(first * stride)]; };   // entries of items [first, i)
  int64_t last = first + 1;
  while (last < end && ne(last + 1) * entry_bytes <= budget && ne(last + 1) <= max_entries) ++last;
  return last;
}

int list_slab(letkf_ctx* c, int64_t e0, int64_t e1, ListSlab* l) {
  const size_t n1 = (size_t)std::max<int64_t>(e1 - e0, 1);
  const size_t o_rd = align256(n1 * 4), o_rl = o_rd + align256(n1 * 8);
  if (int rc = grow(c, &c->list_ws, o_rl + n1 * 8 + 256)) return rc;
  l->idx = reinterpret_cast<int32_t*>(c->list_ws.p) - e0;
  l->rd = reinterpret_cast<double*>(c->list_ws.p + o_rd) - e0;
  l->rl = reinterpret_cast<double*>(c->list_ws.p + o_rl) - e0;
  return LETKF_OK;
}
// ... the horizontal survivors of a batch of columns in buffer b (4 doubles each)
int survivor_slab(letkf_ctx* c, DevBuf* b, int64_t e0, int64_t e1, double** sv) {
  if (int rc = grow(c, b, (size_t)std::max<int64_t>(e1 - e0, 1) * 32 + 256)) return rc;
  *sv = reinterpret_cast<double*>(b->p) - 4 * e0;
  return LETKF_OK;
}

// The column entries' count pass over all nlev levels of ncol columns, in the context's scratch buffer, and its prefix sum ...
int count_columns(letkf_ctx* c, const letkf_search_tables* t, int64_t ncol, int32_t nlev, const double* rig, const double* rjg,
                  const double* rlev, const double* rz, ScanWs* sw) {
  if (int rc = scan_ws(c, &c->scratch, (size_t)(ncol * nlev), 0, sw)) return rc;
  HIP_TRY(zero_total(c, *sw));
  if (int rc = letkf_obs_search_columns_dev(c, t, ncol, nlev, rig, rjg, rlev, rz, 0, sw->counts, nullptr, nullptr, nullptr, nullptr,
                                            nullptr, nullptr))
    return rc;
  HIP_TRY(scan_offsets(c, *sw));
  return LETKF_OK;
}
// ... and the fill pass of levels [l0, l1), whose boundaries offsets_to_host brought back (stride ncol), into a slab of list_ws
int fill_columns(letkf_ctx* c, const letkf_search_tables* t, int64_t ncol, int l0, int l1, const double* rig, const double* rjg,
                 const double* rlev, const double* rz, const ScanWs& sw, ListSlab* ls) {
  const int64_t p0 = (int64_t)l0 * ncol;
  if (int rc = list_slab(c, sw.hoff[(size_t)l0], sw.hoff[(size_t)l1], ls)) return rc;
  return letkf_obs_search_columns_dev(c, t, ncol, l1 - l0, rig, rjg, rlev + p0, rz + p0, 1, nullptr, sw.off + p0, ls->idx, ls->rd,
                                      ls->rl, nullptr, nullptr);
}

int check_ctx(letkf_ctx* c) {
  if (!c || c->device < 0) return fail(LETKF_E_NO_DEVICE, "context is not bound to a device");
  HIP_TRY(hipSetDevice(c->device));
  return LETKF_OK;
}

}  // namespace letkf::api

namespace {

// Measurement-only knobs exist in the PROF twin of the library (make PROF=1) and nowhere else: the production build
// reads no environment variable that could change a result.
#ifdef LETKF_WAVE_PROF
#define LETKF_KNOB(name) std::getenv(name)
#else
#define LETKF_KNOB(name) static_cast<const char*>(nullptr)
#endif

struct EventPair {   // timing events that do not outlive a failed launch
  hipEvent_t e0 = nullptr, e1 = nullptr;
  ~EventPair() {
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
  }
};

// The route of a loop-body / letkf_core call.  pick_route decides it, and nothing else does:
//
//   family  serves                                                       kernels
//   trio    mode 0, nv = 11, k <= 20, no per-point outputs (T, Pa,        letkf_trio_kernel (letkf_trio.hip): three points per wave
//           w-bar), the trivial pre-pass ran; LETKF_OPT_SMALL_K_TRIO
//   wave    k <= 100 and nv = 11 (modes 0, 2, 3) or nv = 0 (mode 1),      letkf_wave_kernel (letkf_wave_dev.h): one wave per point to
//           but not the staged path's eigen-free calls below               k = 62, two from 63
//   staged  every other call with nv + 2 <= 16 right-hand sides;          Gram (matrix cores for mode 0, letkf_stage_gram_kernel for
//           from k = 63 also mode 0 without T / Pa where                  the other modes and beyond k = 512) -> eigen-free stage
//           LETKF_OPT_STAGED_POLY (eigen-free: 1.07 M solves/s against    (mode 0 without T / Pa, LETKF_OPT_STAGED_POLY) -> eigen
//           0.64 M on the two-wave kernel at k = 100)                     stage (workgroup Jacobi to order 208, block Jacobi beyond)
//                                                                          -> apply (letkf_gram / krylov / eig / staged.hip)
//   point   nv + 2 > 16                                                   letkf_point_kernel (letkf_kernels.hip): LDS, or BIG with its
//                                                                          matrices in an HBM workspace where they do not fit
//
// The streaming pre-pass (letkf_trivial.hip: points without observations or with beta = 0) runs in front of the trio, wave and
// staged families wherever trivial_pass_supports.
enum class Family { trio, wave, staged, point };
struct Route {
  Family family = Family::wave;
  bool trivial = false;       // the pre-pass runs first, and the solve skips its points
  letkf::GramKernels gram{};  // staged: the Gram kernel(s) ...
  bool krylov = false;        // ... the eigen-free stage ...
  int eig_wg_order = 0;       // ... the order cap of the workgroup Jacobi ...
  bool eig_block = false;     // ... and the block Jacobi behind it
  letkf::PointPlan plan{};    // point: LDS or BIG, and its launch shape
};

int pick_route(const letkf_ctx* c, const letkf::PointArgs& a, Route* r) {
  *r = Route{};
  const bool kkout = a.trans_out || a.pa_out;
  const bool staged_ok = a.mode != 2 && a.nv + 2 <= 16;
  bool wave = letkf::wave_kernel_supports(a.k, a.nv, a.mode);
  if (wave && a.k >= 63 && a.mode == 0 && !kkout && c->staged_poly && staged_ok) wave = false;
  if (wave || staged_ok) r->trivial = letkf::trivial_pass_supports(a) && !LETKF_KNOB("LETKF_AMD_NO_TRIVIAL_PASS");
  if (wave) {
    r->family = c->trio && r->trivial && letkf::trio_kernel_supports(a) ? Family::trio : Family::wave;
  } else if (staged_ok) {
    r->family = Family::staged;
    r->gram = letkf::stage_gram_kernels(a.k, a.mode);
    r->krylov = a.mode == 0 && !kkout && c->staged_poly;
    r->eig_wg_order = std::min(a.k, letkf::eig_wg_max_order());
    r->eig_block = a.k > letkf::eig_wg_max_order();
  } else {
    r->family = Family::point;
    if (!letkf::point_kernel_plan(a.k, a.nv, a.npts, c->num_cu, c->lds_max, &r->plan))
      return fail(LETKF_E_INVALID, "ensemble size too large for the LDS vectors");
  }
  return LETKF_OK;
}

std::string route_path(const letkf::PointArgs& a, const Route& r) {
  switch (r.family) {
    case Family::trio:
      return "letkf_trio_kernel<KR=" + std::to_string(letkf::trio_kernel_kr(a.k)) + ",P=" + std::to_string(letkf::trio_points_per_wave(a.k)) + ">";
    case Family::wave:
      return "letkf_wave_kernel<KR=" + std::to_string(letkf::wave_kernel_kr(a.k)) + ",NV=" + std::to_string(a.nv) +
             ",NW=" + std::to_string(letkf::wave_kernel_nw(a.k)) + (a.mode == 2 ? ",FUSED" : a.mode == 3 ? ",FUSED: column survivors" : "") + ">";
    case Family::point: return r.plan.big ? "letkf_point_kernel<BIG>" : "letkf_point_kernel<LDS>";
    case Family::staged: break;
  }
  std::string eig = letkf::eig_wg_kernel_name(r.eig_wg_order) + (r.eig_block ? " / letkf_eig_block_kernel" : "");
  if (r.krylov) eig = "letkf_stage_krylov_kernel (CG + Lanczos; points it gives up: " + eig + ")";
  return std::string("staged: ") + (r.gram.mfma ? "letkf_stage_gram_mfma_kernel + " : "") + (r.gram.plain ? "letkf_stage_gram_kernel + " : "") +
         eig + " + letkf_stage_apply_kernel";
}

// Register kernels (trio, wave): run length, grid, the warm-start, local-list slot and scheduling workspaces
int prepare_wave(letkf_ctx* c, letkf::PointArgs& a, const Route& r, int warm_run, long warm_stride) {
  int run_req = warm_run;
  if (const char* e = LETKF_KNOB("LETKF_AMD_RUN_LEN")) run_req = std::atoi(e);   // PROF knob: 1 = all cold
  a.warm_stride = warm_stride > 1 ? warm_stride : 1;
  if (a.npts % a.warm_stride != 0) return fail(LETKF_E_INVALID, "warm_stride does not divide npts");
  // (occupancy 0: the launcher asks again with its kernel's; what is taken here does not depend on it)
  const letkf::LaunchShape s = letkf::launch_shape(r.family == Family::trio, a.k, a.mode, a.npts, a.warm_stride, run_req, c->num_cu,
                                                   0, true, letkf::wave_grid_per_cu());
  a.run_len = s.run_len;
  a.wave_grid = s.grid_ws;
  if (r.family == Family::wave) {   // (the trio kernel parks its eigenvectors in LDS)
    if (int rc = grow(c, &c->warm_ws, s.warm_bytes)) return rc;
    a.warm_ws = reinterpret_cast<double*>(c->warm_ws.p);
  }
  if (a.mode == 3) {   // one local-list slot per wave of the grid (4 waves per workgroup): idx | rdiag | rloc
    const size_t nslot = (size_t)a.wave_grid * 4, cap = 2 * (size_t)(a.sl_cap > 0 ? a.sl_cap : 4);   // (two lists per wave: this level's and the next one's)
    const size_t o_rd = align256(nslot * cap * 4), o_rl = o_rd + nslot * cap * 8;
    if (int rc = grow(c, &c->slot_ws, o_rl + nslot * cap * 8 + 256)) return rc;
    a.sl_idx = reinterpret_cast<int*>(c->slot_ws.p);
    a.sl_rd = reinterpret_cast<double*>(c->slot_ws.p + o_rd);
    a.sl_rl = reinterpret_cast<double*>(c->slot_ws.p + o_rl);
    a.obs_idx = a.sl_idx;
    a.rdiag_l = a.sl_rd;
    a.rloc_l = a.sl_rl;
  }
  if (!c->sched) {
    HIP_TRY(hipMalloc(reinterpret_cast<void**>(&c->sched), 512));
    HIP_TRY(hipMemsetAsync(c->sched, 0, 512, c->stream));   // (later launches reset it themselves when they draw)
  }
  a.sched = LETKF_KNOB("LETKF_AMD_STATIC_SCHED") ? nullptr : c->sched;   // PROF knob: the static dealing, for A/B runs
  a.warm_dbg = 0;
  if (const char* e = LETKF_KNOB("LETKF_AMD_WARM_DBG")) a.warm_dbg = std::atoi(e);
  a.prof = nullptr;
#ifdef LETKF_CHECKED
  {   // the violation record of the checked build (letkf_wave_dev.h LETKF_CHECK): code | workgroup | value | bound
    static unsigned long long* rec = nullptr;
    if (!rec) HIP_TRY(hipMalloc(reinterpret_cast<void**>(&rec), 4 * sizeof(unsigned long long)));
    HIP_TRY(hipMemsetAsync(rec, 0, 4 * sizeof(unsigned long long), c->stream));
    a.prof = rec;
  }
#endif
  return LETKF_OK;
}

// Staged path: the points go in batches whose slabs fit a fixed workspace budget; grows that workspace
int prepare_staged(letkf_ctx* c, const letkf::PointArgs& a, const Route& r, long* nb_out, long* wpp_out) {
  const int kkout = (a.trans_out || a.pa_out) ? 1 : 0;
  const long hist = r.krylov ? letkf::stage_krylov_hist_doubles(a.k) : 0;
  const long wpp = letkf::staged_ws_per_point(a.k, a.nv, kkout, hist);
  // slabs of one batch: at most 6 GiB (+ as much again per 2 MB of residual history per point, up to 24 GiB)
  size_t budget = (size_t)6 << 30;
  if (hist) budget += std::min<size_t>((size_t)18 << 30, (size_t)hist * sizeof(double) * 3072);
  long nb = (long)(budget / ((size_t)wpp * sizeof(double)));
  const long want = (long)c->num_cu * 16;
  if (nb > want) nb = want;
  if (nb < 1) nb = 1;
  if (nb > a.npts) nb = a.npts;
  {   // equal batches (a last batch of a few points would leave the chip idle for a whole eigen-solve) ...
    const long nbat = (a.npts + nb - 1) / nb;
    const long cap = nb;
    nb = (a.npts + nbat - 1) / nbat;
    // ... of whole rounds of workgroups: the stages run 2 (Gram, eigen-free stage at small orders) to 4 (apply) workgroups per CU,
    // and a batch that is no multiple of 2 x #CU ends every one of its kernels on a partly filled round (27648 points in 7
    // batches of 3950 = 7.7 rounds of 512: r4, MEMBER = 100)
    const long q = 2L * c->num_cu;
    const long up = (nb + q - 1) / q * q;
    if (up <= cap) nb = up;
  }
  const size_t need = (size_t)nb * (size_t)wpp * sizeof(double) + (size_t)nb * 4 * sizeof(int) + 256;
  if (int rc = grow(c, &c->staged_ws, need)) return rc;
  *nb_out = nb;
  *wpp_out = wpp;
  return LETKF_OK;
}

// ... and per batch: Gram stage, eigen-free stage, eigen stage, apply stage -- all on the context's stream, no host
// synchronisation in between
int launch_staged(letkf_ctx* c, const letkf::PointArgs& a, const Route& r, long nb, long wpp) {
  const size_t slab_bytes = (size_t)nb * (size_t)wpp * sizeof(double);
  letkf::StagedArgs s;
  s.A = a;
  s.A.ws = reinterpret_cast<double*>(c->staged_ws.p);
  s.A.ws_per_block = wpp;
  s.A.max_sweep = 60;
  s.meta = reinterpret_cast<int*>(c->staged_ws.p + slab_bytes);
  s.info = s.meta + 2 * nb;
  s.kkout = (a.trans_out || a.pa_out) ? 1 : 0;
  s.wg_max_order = letkf::eig_wg_max_order();
  s.poly_max_n = r.krylov ? letkf::stage_krylov_max_n(a.k) : 0;
  s.gram_mfma = r.gram.mfma ? 1 : 0;
  for (long p0 = 0; p0 < a.npts; p0 += nb) {
    s.pt0 = p0;
    s.nbatch = (a.npts - p0 < nb) ? a.npts - p0 : nb;
    if (r.gram.mfma) HIP_TRY(letkf::launch_stage_gram_mfma(s, c->stream));
    if (r.gram.plain) HIP_TRY(letkf::launch_stage_gram(s, c->lds_max, c->stream));
    if (r.krylov) HIP_TRY(letkf::launch_stage_krylov(s, c->lds_max, c->stream));   // (points it gives up: eigen stage, next)
    letkf::EigArgs e;
    e.ws = s.A.ws;
    e.ws_per_point = wpp;
    e.npts = s.nbatch;
    e.pt0 = p0;
    e.meta = s.meta;
    e.info = s.info;
    e.max_sweep = 60;
    HIP_TRY(letkf::launch_eig_wg(e, r.eig_wg_order, c->num_cu, c->stream));
    if (r.eig_block) HIP_TRY(letkf::launch_eig_block(e, a.k, c->num_cu, c->stream));
    HIP_TRY(letkf::launch_stage_apply(s, c->stream));
  }
  return LETKF_OK;
}

}  // namespace

namespace letkf::api {

int launch(letkf_ctx* c, letkf::PointArgs& a, int warm_run, long warm_stride) {
  if (a.k < 2) return fail(LETKF_E_INVALID, "ensemble size must be >= 2");
  if (a.nv < 0 || a.npts < 0) return fail(LETKF_E_INVALID, "negative size");
  a.max_sweep = 60;
  if (const char* e = LETKF_KNOB("LETKF_AMD_MAX_SWEEP")) {   // PROF knob: time the non-eigensolve phases
    int v = std::atoi(e);
    if (v >= 0 && v < 60) a.max_sweep = v;   // 0: skip the eigensolve entirely (timing only, results invalid)
  }
  Route r;
  if (int rc = pick_route(c, a, &r)) return rc;
  const bool reg = r.family == Family::trio || r.family == Family::wave;
  long nb = 0, wpp = 0;
  if (reg) {
    if (int rc = prepare_wave(c, a, r, warm_run, warm_stride)) return rc;
  } else if (r.family == Family::staged) {
    if (int rc = prepare_staged(c, a, r, &nb, &wpp)) return rc;
  } else {
    if (int rc = grow(c, &c->ws, r.plan.ws_bytes(), false)) return rc;
    a.ldg = r.plan.ldg;
    a.ldy = r.plan.ldy;
    a.tn = r.plan.tn;
    a.ws = reinterpret_cast<double*>(c->ws.p);
    a.ws_per_block = r.plan.ws_per_block;
    a.big_block = (r.plan.big && !LETKF_KNOB("LETKF_AMD_BIG_STREAM")) ? 1 : 0;   // PROF knob: the older streaming Jacobi
  }
  // every argument check is behind us: only now create the timing events (destroyed again if the launch fails)
  EventPair ev;
  if (c->timing) {
    HIP_TRY(hipEventCreate(&ev.e0));
    HIP_TRY(hipEventCreate(&ev.e1));
    HIP_TRY(hipEventRecord(ev.e0, c->stream));
  }
#ifdef LETKF_WAVE_PROF
  static unsigned long long* prof_dev = nullptr;
  if (reg) {
    if (!prof_dev) HIP_TRY(hipMalloc(reinterpret_cast<void**>(&prof_dev), 26 * sizeof(unsigned long long)));
    HIP_TRY(hipMemsetAsync(prof_dev, 0, 26 * sizeof(unsigned long long), c->stream));
    a.prof = prof_dev;
  }
#endif
  if (r.trivial) {
    HIP_TRY(letkf::launch_trivial_points(a, c->stream));
    a.skip_trivial = 1;
  }
  switch (r.family) {
    case Family::trio: HIP_TRY(letkf::launch_trio_kernel(a, c->num_cu, c->stream)); break;
    case Family::wave: HIP_TRY(letkf::launch_wave_kernel(a, c->num_cu, c->stream)); break;
    case Family::staged:
      if (int rc = launch_staged(c, a, r, nb, wpp)) return rc;
      break;
    case Family::point: HIP_TRY(letkf::launch_point_kernel(a, r.plan, c->stream)); break;
  }
#ifdef LETKF_WAVE_PROF
  if (reg) {
    unsigned long long h[26];
    HIP_TRY(hipMemcpyAsync(h, prof_dev, sizeof(h), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    unsigned long long tot = 0;
    for (int i = 0; i < 10; ++i) tot += h[i];
    std::fprintf(stderr, "[letkf prof] wave-time share by phase (s_memtime ticks, all waves):");
    for (int i = 0; i < 10; ++i) std::fprintf(stderr, " p%d=%.1f%%", i, tot ? 100.0 * (double)h[i] / (double)tot : 0.0);
    std::fprintf(stderr, " total=%llu\n", tot);
    std::fprintf(stderr, "[letkf prof] first wave start .. last wave end: %llu ticks; waves by units done (0..11+):", h[11] - ~h[10]);
    for (int i = 12; i < 24; ++i) std::fprintf(stderr, " %llu", h[i]);
    std::fprintf(stderr, "; units done in all: %llu\n", h[24]);
  }
#endif
  if (c->timing) {
    HIP_TRY(hipEventRecord(ev.e1, c->stream));
    c->events.emplace_back(ev.e0, ev.e1);
    ev.e0 = ev.e1 = nullptr;   // owned by the context from here
  }
  c->last_path = route_path(a, r);
#ifdef LETKF_CHECKED
  if (reg && a.prof) {
    unsigned long long h[4];
    HIP_TRY(hipMemcpyAsync(h, a.prof, sizeof(h), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (h[0])
      return fail(LETKF_E_HIP, "checked build: bound " + std::to_string(h[0]) + " violated in workgroup " + std::to_string(h[1]) + ": value " +
                                   std::to_string((long long)h[2]) + " against " + std::to_string((long long)h[3]));
  }
#endif
  return LETKF_OK;
}

}  // namespace letkf::api

extern "C" {

int letkf_ctx_create(int device_id, letkf_ctx** out) try {
  if (!out) return fail(LETKF_E_INVALID, "ctx out pointer is NULL");
  *out = nullptr;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return fail(LETKF_E_NO_DEVICE, "no HIP device visible: this library has no CPU path");
  int dev = device_id;
  if (dev < 0) HIP_TRY(hipGetDevice(&dev));
  if (dev >= ndev) return fail(LETKF_E_INVALID, "device id out of range");
  HIP_TRY(hipSetDevice(dev));
  hipDeviceProp_t prop;
  HIP_TRY(hipGetDeviceProperties(&prop, dev));
  if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
    return fail(LETKF_E_NO_DEVICE, std::string("device is ") + prop.gcnArchName + ", this build targets gfx950 only");
  letkf_ctx* c = new letkf_ctx();
  c->device = dev;
  c->num_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
  c->lds_max = prop.sharedMemPerBlock >= 64 * 1024 ? (size_t)prop.sharedMemPerBlock : 64 * 1024;
  {
    int v = 0;
    if (hipDeviceGetAttribute(&v, hipDeviceAttributeMaxSharedMemoryPerBlock, dev) == hipSuccess && v > 0)
      c->lds_max = (size_t)v;
  }
  hipError_t e = hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking);
  if (e != hipSuccess) {
    delete c;
    return fail(LETKF_E_HIP, std::string("hipStreamCreate: ") + hipGetErrorString(e));
  }
  c->stream = c->own_stream;
  *out = c;
  return LETKF_OK;
} LETKF_ENTRY_END(letkf_ctx_create)

int letkf_ctx_destroy(letkf_ctx* c) try {
  if (!c) return LETKF_OK;
  if (c->device >= 0) {
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    for (auto& ev : c->events) {
      (void)hipEventDestroy(ev.first);
      (void)hipEventDestroy(ev.second);
    }
    if (c->sched) (void)hipFree(c->sched);
    if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
  }
  delete c;   // (its device buffers free themselves)
  return LETKF_OK;
} LETKF_ENTRY_END(letkf_ctx_destroy)

int letkf_ctx_set_option(letkf_ctx* c, int option, int value) try {
  if (int rc = check_ctx(c)) return rc;
  c->ring_no_n = -1;   // (no verdict of the limited column search outlives a change of options)
  switch (option) {
    case LETKF_OPT_STAGED_POLY: c->staged_poly = value != 0; return LETKF_OK;
    case LETKF_OPT_RING_BATCH_MB:
      if (value < 1) return fail(LETKF_E_INVALID, "LETKF_OPT_RING_BATCH_MB: >= 1");
      c->ring_batch_mb = value;
      return LETKF_OK;
    case LETKF_OPT_RING_RELEASE: c->ring_release = value != 0; return LETKF_OK;
    case LETKF_OPT_SMALL_K_TRIO: c->trio = value != 0; return LETKF_OK;
    case LETKF_OPT_LIMITED_RINGS:
      if (value < 0 || value > 2) return fail(LETKF_E_INVALID, "LETKF_OPT_LIMITED_RINGS: 0, 1 or 2");
      c->limited_rings = value;
      return LETKF_OK;
    case LETKF_OPT_COLUMN_SURVIVORS:
      if (value < 0 || value > 2) return fail(LETKF_E_INVALID, "LETKF_OPT_COLUMN_SURVIVORS: 0, 1 or 2");
      c->col_survivors = value;
      return LETKF_OK;
    default: return fail(LETKF_E_INVALID, "unknown option");
  }
} LETKF_ENTRY_END(letkf_ctx_set_option)

int letkf_ctx_set_stream(letkf_ctx* c, void* hip_stream) try {
  if (int rc = check_ctx(c)) return rc;
  // the handle is used as is: NULL is HIP's default (null) stream, which is also what torch.cuda.current_stream()
  // hands out unless the caller switched streams -- work then orders with the caller's other work on that stream
  c->stream = static_cast<hipStream_t>(hip_stream);
  return LETKF_OK;
} LETKF_ENTRY_END(letkf_ctx_set_stream)

int letkf_ctx_synchronize(letkf_ctx* c) try {
  if (int rc = check_ctx(c)) return rc;
  HIP_TRY(hipStreamSynchronize(c->stream));
  return LETKF_OK;
} LETKF_ENTRY_END(letkf_ctx_synchronize)

int letkf_sched_plan_check(int64_t npts, int64_t stride, int32_t run_len, int32_t grid, int32_t ppw, int32_t resident_per_xcd) try {
  return letkf::sched_plan_check((long)npts, (long)stride, run_len, grid, ppw, resident_per_xcd, 1);
} LETKF_ENTRY_END(letkf_sched_plan_check)
int letkf_sched_plan_check_units(int64_t npts, int64_t stride, int32_t run_len, int32_t grid, int32_t ppw, int32_t resident_per_xcd, int32_t ub_of) try {
  return letkf::sched_plan_check((long)npts, (long)stride, run_len, grid, ppw, resident_per_xcd, ub_of);
} LETKF_ENTRY_END(letkf_sched_plan_check_units)

int letkf_ctx_last_path(letkf_ctx* c, char* buf, int32_t len) try {
  if (!c || !buf || len < 1) return fail(LETKF_E_INVALID, "bad argument");
  std::snprintf(buf, (size_t)len, "%s", c->last_path.c_str());
  return LETKF_OK;
} LETKF_ENTRY_END(letkf_ctx_last_path)

int letkf_ctx_timing_enable(letkf_ctx* c, int enable) try {
  if (int rc = check_ctx(c)) return rc;
  c->timing = enable != 0;
  return LETKF_OK;
} LETKF_ENTRY_END(letkf_ctx_timing_enable)

int letkf_ctx_timing_read(letkf_ctx* c, double* avg_ms, int64_t* nlaunch, int reset) try {
  if (int rc = check_ctx(c)) return rc;
  HIP_TRY(hipStreamSynchronize(c->stream));
  double tot = 0.0;
  for (auto& ev : c->events) {
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, ev.first, ev.second));
    tot += ms;
  }
  if (nlaunch) *nlaunch = (int64_t)c->events.size();
  if (avg_ms) *avg_ms = c->events.empty() ? 0.0 : tot / (double)c->events.size();
  if (reset) {
    for (auto& ev : c->events) {
      (void)hipEventDestroy(ev.first);
      (void)hipEventDestroy(ev.second);
    }
    c->events.clear();
  }
  return LETKF_OK;
} LETKF_ENTRY_END(letkf_ctx_timing_read)

int letkf_core_batch_dev(letkf_ctx* c, const letkf_core_batch_args* g) try {
  if (int rc = check_ctx(c)) return rc;
  if (!g) return fail(LETKF_E_INVALID, "args is NULL");
  if (g->nbatch == 0) return LETKF_OK;
  if (g->ne < 2 || g->nobs < 1 || g->nbatch < 0) return fail(LETKF_E_INVALID, "bad ne/nobs/nbatch");
  if (!g->nobsl || !g->hdxb || !g->rdiag || !g->rloc || !g->dep || !g->parm_infl || !g->trans)
    return fail(LETKF_E_INVALID, "a required device pointer is NULL");
  letkf::PointArgs a;
  std::memset(&a, 0, sizeof(a));
  a.k = g->ne;
  a.nv = 0;
  a.var_mask = ~0u;
  a.mode = 1;
  a.npts = g->nbatch;
  a.nobsl = g->nobsl;
  a.hdxb = g->hdxb;
  a.rdiag = g->rdiag;
  a.rloc = g->rloc;
  a.depv = g->dep;
  a.depd = (g->depd && g->transmd) ? g->depd : nullptr;       // common_letkf.f90:188
  a.nobs = g->nobs;
  a.rdiag_wloc = g->rdiag_wloc;
  a.infl_adaptive = g->infl_update;
  a.det_run = 0;
  a.infl = g->parm_infl;
  a.trans_out = g->trans;
  a.transm_out = g->transm;
  a.transmd_out = (g->depd && g->transmd) ? g->transmd : nullptr;
  a.pa_out = g->pao;
  a.add_wbar_to_trans = g->transm ? 0 : 1;                    // common_letkf.f90:218-226
  a.status = g->status;
  a.nsweep = g->nsweep;
  if (int rc = launch(c, a)) return rc;
  if (g->transmd && !g->depd) {
    // transmd without depd: the reference zeroes a present transmd at nobsl == 0 whatever depd is (common_letkf.f90:97-99) and
    // leaves it untouched at nobsl > 0 (:188)
    HIP_TRY(letkf::launch_zero_transmd_unobserved(g->nbatch, g->ne, g->nobsl, g->transmd, c->stream));
  }
  return LETKF_OK;
} LETKF_ENTRY_END(letkf_core_batch_dev)

// ---------------------------------------------------------------------------------------------
// Fine boundary on host pointers: the drop-in for common/common_letkf.f90:52 used by the Fortran shim.
// One context per calling thread (the reference calls letkf_core from inside !$OMP PARALLEL).
// ---------------------------------------------------------------------------------------------
namespace {
struct TlsCtx {
  letkf_ctx* c = nullptr;
  ~TlsCtx() {
    if (c) letkf_ctx_destroy(c);
  }
};
thread_local TlsCtx g_tls;

int core_host(int ne, int nobs, int nobsl, const double* hdxb, const double* rdiag, const double* rloc,
              const double* dep, double* parm_infl, double* trans, double* transm, double* pao,
              const int* rdiag_wloc, const int* infl_update, const double* depd, double* transmd, int* st_out) {
  if (ne < 2 || nobs < 0 || nobsl < 0 || nobsl > nobs) return fail(LETKF_E_INVALID, "bad ne/nobs/nobsl");
  if (!parm_infl || !trans) return fail(LETKF_E_INVALID, "parm_infl/trans is NULL");
  if (nobsl > 0 && (!hdxb || !rdiag || !rloc || !dep)) return fail(LETKF_E_INVALID, "an input array is NULL");
  if (!g_tls.c) {
    if (int rc = letkf_ctx_create(-1, &g_tls.c)) return rc;
  }
  letkf_ctx* c = g_tls.c;
  if (int rc = check_ctx(c)) return rc;
  const size_t k = (size_t)ne, n = (size_t)(nobsl > 0 ? nobsl : 1);
  const bool det = depd && transmd;
  // scratch layout (doubles): hdxb[n*k] rdiag[n] rloc[n] dep[n] depd[n] infl[1] trans[k*k] pao[k*k] transm[k] transmd[k] | ints: nobsl, status
  const size_t nd = n * k + 4 * n + 1 + 2 * k * k + 2 * k;
  const size_t bytes = nd * sizeof(double) + 4 * sizeof(int);
  if (int rc = grow(c, &c->scratch, bytes)) return rc;
  double* d = reinterpret_cast<double*>(c->scratch.p);
  double* d_h = d;
  double* d_rdiag = d_h + n * k;
  double* d_rloc = d_rdiag + n;
  double* d_dep = d_rloc + n;
  double* d_depd = d_dep + n;
  double* d_infl = d_depd + n;
  double* d_trans = d_infl + 1;
  double* d_pao = d_trans + k * k;
  double* d_transm = d_pao + k * k;
  double* d_transmd = d_transm + k;
  int* d_i = reinterpret_cast<int*>(d_transmd + k);
  hipStream_t s = c->stream;
  if (nobsl > 0) {
    // only rows 1..nobsl of hdxb(nobs, ne) are meaningful (common_letkf.f90:35-37): compact while copying
    HIP_TRY(hipMemcpy2DAsync(d_h, (size_t)nobsl * sizeof(double), hdxb, (size_t)nobs * sizeof(double),
                             (size_t)nobsl * sizeof(double), k, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(d_rdiag, rdiag, (size_t)nobsl * sizeof(double), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(d_rloc, rloc, (size_t)nobsl * sizeof(double), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(d_dep, dep, (size_t)nobsl * sizeof(double), hipMemcpyHostToDevice, s));
    if (det) HIP_TRY(hipMemcpyAsync(d_depd, depd, (size_t)nobsl * sizeof(double), hipMemcpyHostToDevice, s));
  }
  int hi[2] = {nobsl, 0};
  HIP_TRY(hipMemcpyAsync(d_i, hi, sizeof(hi), hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(d_infl, parm_infl, sizeof(double), hipMemcpyHostToDevice, s));
  letkf_core_batch_args g;
  std::memset(&g, 0, sizeof(g));
  g.ne = ne;
  g.nobs = (int)n;
  g.nbatch = 1;
  g.nobsl = d_i;
  g.hdxb = d_h;
  g.rdiag = d_rdiag;
  g.rloc = d_rloc;
  g.dep = d_dep;
  g.depd = det ? d_depd : nullptr;
  g.parm_infl = d_infl;
  g.trans = d_trans;
  g.transm = transm ? d_transm : nullptr;
  g.pao = pao ? d_pao : nullptr;
  g.transmd = transmd ? d_transmd : nullptr;                // (without depd: zeroed at nobsl == 0 only, :97-99)
  g.rdiag_wloc = rdiag_wloc ? (*rdiag_wloc != 0) : 0;      // common_letkf.f90:84-85
  g.infl_update = infl_update ? (*infl_update != 0) : 0;   // :86-87
  g.status = d_i + 1;
  if (int rc = letkf_core_batch_dev(c, &g)) return rc;
  HIP_TRY(hipMemcpyAsync(trans, d_trans, k * k * sizeof(double), hipMemcpyDeviceToHost, s));
  if (transm) HIP_TRY(hipMemcpyAsync(transm, d_transm, k * sizeof(double), hipMemcpyDeviceToHost, s));
  if (pao) HIP_TRY(hipMemcpyAsync(pao, d_pao, k * k * sizeof(double), hipMemcpyDeviceToHost, s));
  if (transmd && (depd || nobsl == 0)) HIP_TRY(hipMemcpyAsync(transmd, d_transmd, k * sizeof(double), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipMemcpyAsync(parm_infl, d_infl, sizeof(double), hipMemcpyDeviceToHost, s));
  int hst = 0;
  HIP_TRY(hipMemcpyAsync(&hst, d_i + 1, sizeof(int), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  *st_out = hst;
  return LETKF_OK;
}
}  // namespace

void letkf_core_c(int ne, int nobs, int nobsl, const double* hdxb, const double* rdiag, const double* rloc,
                  const double* dep, double* parm_infl, double* trans, double* transm, double* pao,
                  const int* rdiag_wloc, const int* infl_update, const double* depd, double* transmd, int* status) try {
  int st = 0;
  int rc = core_host(ne, nobs, nobsl, hdxb, rdiag, rloc, dep, parm_infl, trans, transm, pao, rdiag_wloc,
                     infl_update, depd, transmd, &st);
  if (rc != LETKF_OK) {
    std::fprintf(stderr, "!!! ERROR (letkf_core_c): %s\n", letkf_amd_last_error());
    st = rc;
  }
  if (status) *status = st;
} LETKF_ENTRY_END_TO(letkf_core_c, if (status) *status =)

}  // extern "C"
