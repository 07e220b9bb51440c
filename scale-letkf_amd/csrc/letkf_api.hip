// letkf_api.hip -- host side of the C ABI declared in include/letkf_amd.h.
//
// Thin by design: argument checking, the choice of kernels (pick_route), the workspaces,
// optional HIP-event timing for bench.py, and the host-pointer compatibility entry
// letkf_core_c that the Fortran shim (scale-letkf_amd/fortran) calls.
// There is no CPU fallback anywhere in this file: without a device every compute entry
// returns LETKF_E_NO_DEVICE.

#include <hip/hip_runtime.h>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/iterator/transform_iterator.hpp>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/letkf_amd.h"
#include "../../include/letkf_amd_interp_window.h"
#include "letkf_device.h"
#include "letkf_interp_dev.h"
#include "letkf_obsope_dev.h"

namespace letkf {

// int32 counts -> int64 exclusive offsets (rocprim) with the scan's storage at temp; temp == nullptr: *temp_bytes = its size
hipError_t count_scan(void* temp, size_t* temp_bytes, const int32_t* counts, int64_t* off, size_t n, hipStream_t st) {
  auto in = rocprim::make_transform_iterator(counts, [] __device__(int32_t v) { return (int64_t)v; });
  return rocprim::exclusive_scan(temp, *temp_bytes, in, off, (int64_t)0, n, rocprim::plus<int64_t>(), st);
}

}  // namespace letkf

namespace {

thread_local std::string g_last_error;

int fail(int code, const std::string& msg) {
  g_last_error = msg;
  return code;
}

#define HIP_TRY(expr)                                                                              \
  do {                                                                                             \
    hipError_t _e = (expr);                                                                        \
    if (_e != hipSuccess)                                                                          \
      return fail(LETKF_E_HIP, std::string(#expr) + ": " + hipGetErrorString(_e));                 \
  } while (0)

}  // namespace

// One of the context's device buffers; grow() below sizes it.
struct DevBuf {
  char* p = nullptr;
  size_t cap = 0;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() { release(); }
  void release() {   // (hipFree waits for the work that still reads the buffer)
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
  }
};

struct letkf_ctx {
  int device = -1;
  int num_cu = 256;
  size_t lds_max = 160 * 1024;
  hipStream_t own_stream = nullptr;
  hipStream_t stream = nullptr;
  DevBuf ws;                  // letkf_point_kernel<BIG>: its per-workgroup matrices
  DevBuf warm_ws;             // wave kernel: eigenvectors handed from point to point inside a run
  unsigned* sched = nullptr;  // wave kernel: the 8 run counters of the dynamic scheduling (512 bytes)
  DevBuf scratch;             // staging for the host-pointer entry; counts | offsets | scan scratch of the list-driven entries
  DevBuf list_ws;             // letkf_das_columns_dev: the local-observation lists of one slab of levels / the survivors of a batch of columns
  DevBuf slot_ws;             // ... its list-free route: one local list per resident wave
  DevBuf ring_ws;             // limited column search on dense observations: ring-ordered survivors of a batch of columns
  DevBuf ring_aux;            // ... their counts / offsets / ring starts
  // (the last "not dense" verdict, by the identity of the tables and columns it was given for: the weighing costs a survivor count
  // and two read-backs -- 17 ms on C2's grid.  Pointer identity says nothing about the CONTENT -- a host that frees and reallocates
  // its tables every analysis gets the same addresses with other observations -- so the verdict only serves (a) the fill call that
  // directly follows the count call it was made in and (b) the calls of one letkf_das_columns_dev; it is dropped after that use, at
  // the end of that entry and by letkf_ctx_set_option.)
  const void* ring_no[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
  int64_t ring_no_n = -1;
  int ring_no_crit = 0;
  bool ring_keep = false;     // inside letkf_das_columns_dev: the survivors of the first search call serve the later ones
  bool ring_ready = false;
  int ring_batch_mb = 8192;   // LETKF_OPT_RING_BATCH_MB
  bool ring_release = false;  // LETKF_OPT_RING_RELEASE
  int limited_rings = 2;      // LETKF_OPT_LIMITED_RINGS: 0 never, 1 wherever eligible, 2 where a group's survivors overflow the column kernel's buffer
  DevBuf efso_ws;             // EFSO: the pair contributions of a slab, their sort by observation row and the row offsets
  DevBuf obsanal_ws;          // das_letkf_obs: the targets' coordinates, pseudo-state, inflation and flag word
  DevBuf staged_ws;           // staged path: per-point slabs of a batch + meta / info words
  DevBuf interp_fix;          // letkf_das_interp_dev: the coarse indices and the coarse points' coordinates
  DevBuf interp_ws;           // ... the kept T / w-bar and the gathered observation rows of a slab of levels
  std::string last_path;      // kernels the last loop-body / letkf_core launch went through (bench.py reports it)
  bool timing = false;
  bool staged_poly = true;    // LETKF_OPT_STAGED_POLY
  bool trio = true;           // LETKF_OPT_SMALL_K_TRIO
  int col_survivors = 2;      // LETKF_OPT_COLUMN_SURVIVORS: 0 never, 1 wherever the one-wave kernel serves the call, 2 where the lists would not fit
  std::vector<std::pair<hipEvent_t, hipEvent_t>> events;
};

namespace {

size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

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
int grow(letkf_ctx* c, DevBuf* b, size_t need, bool slack = true) {
  if (need <= b->cap) return LETKF_OK;
  if (b->p)
    if (int rc = drop(c, b)) return rc;
  HIP_TRY(alloc(b, slack ? need + need / 4 + 4096 : need));
  return LETKF_OK;
}

using letkf::count_scan;

// ---- The plumbing of the list-driven entries: count pass -> offsets -> chunks that fit a budget -> fill pass per chunk.
//
// counts [n + 1] int32 | offsets [n + 1] int64 | rocprim's scan scratch | tail: bytes of the caller's own, where it asks for any
// (every part 256-byte aligned)
struct ScanWs {
  size_t n = 0, temp_bytes = 0;
  int32_t* counts = nullptr;
  int64_t* off = nullptr;
  char *temp = nullptr, *tail = nullptr;
  std::vector<int64_t> hoff;   // the offsets that offsets_to_host brought back
};
// lays it out in buffer b, grown to hold it
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
int offsets_to_host(letkf_ctx* c, ScanWs& s, size_t stride = 1, void* also_dst = nullptr, const void* also_src = nullptr,
                    size_t also_bytes = 0) {
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
                  int64_t budget, int64_t max_entries = INT64_MAX) {
  auto ne = [&](int64_t i) { return off[(size_t)(i * stride)] - off[(size_t)(first * stride)]; };   // entries of items [first, i)
  int64_t last = first + 1;
  while (last < end && ne(last + 1) * entry_bytes <= budget && ne(last + 1) <= max_entries) ++last;
  return last;
}

// A chunk's entries [e0, e1) in a workspace of their own.  The kernels address entry j of item p as base[off[p] + j] with the
// GLOBAL offsets: shift the bases.  A chunk without entries still has a base: room for one.
//
// ... local-observation lists idx | rdiag | rloc in list_ws (20 B per entry)
struct ListSlab {
  int32_t* idx = nullptr;
  double *rd = nullptr, *rl = nullptr;
};
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
  size_t wbytes = 0;
  a.warm_stride = warm_stride > 1 ? warm_stride : 1;
  if (a.npts % a.warm_stride != 0) return fail(LETKF_E_INVALID, "warm_stride does not divide npts");
  letkf::wave_launch_shape(a.k, a.mode, a.npts, c->num_cu, run_req, a.warm_stride, &a.run_len, &a.wave_grid, &wbytes);
  if (r.family == Family::wave) {   // (the trio kernel parks its eigenvectors in LDS)
    if (int rc = grow(c, &c->warm_ws, wbytes)) return rc;
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

int launch(letkf_ctx* c, letkf::PointArgs& a, int warm_run = 0, long warm_stride = 1) {
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

// Inside letkf_das_columns_dev / letkf_efso_columns_dev: the column searches of one entry (a count pass, a fill pass per
// slab) share the ring-ordered survivors of the dense limited case; the guard drops them when the entry returns.
struct RingKeep {
  letkf_ctx* c;
  explicit RingKeep(letkf_ctx* c_) : c(c_) { c->ring_keep = true; c->ring_ready = false; c->ring_no_n = -1; }
  ~RingKeep() {
    c->ring_keep = false;
    c->ring_ready = false;
    c->ring_no_n = -1;
    // the kept survivors can be a large part of the device (configs[3] with two limited types: 128 GiB).  By default the buffer
    // stays with the context for the next analysis (allocating and freeing 64 GB per call cost the MEMBER = 100 tile 1.7 s of a
    // 4 s analysis); LETKF_OPT_RING_RELEASE = 1 hands back whatever exceeds the batch budget when the entry returns, for a host
    // model that needs the memory between analyses (hipFree waits for the work that still reads the buffer)
    if (c->ring_release && c->ring_ws.cap > ((size_t)c->ring_batch_mb << 20) + ((size_t)c->ring_batch_mb << 18) + 8192) c->ring_ws.release();
  }
};

int check_ctx(letkf_ctx* c) {
  if (!c || c->device < 0) return fail(LETKF_E_NO_DEVICE, "context is not bound to a device");
  HIP_TRY(hipSetDevice(c->device));
  return LETKF_OK;
}


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

// One slab: points [0, npts) of a, entries [e0, e1) of its lists
int efso_run_slab(letkf_ctx* c, const letkf::EfsoArgs& a, int64_t npts, int64_t e0, int64_t e1) {
  if (npts <= 0 || e1 <= e0 || a.nobs == 0) return LETKF_OK;
  letkf::EfsoWs ws;
  HIP_TRY(letkf::efso_ws_layout(e1 - e0, a.nobs, a.nterm, c->stream, &ws));
  if (int rc = grow(c, &c->efso_ws, ws.total)) return rc;
  HIP_TRY(letkf::efso_slab(a, npts, e0, e1, c->efso_ws.p, ws, c->num_cu, c->stream));
  return LETKF_OK;
}
}  // namespace

extern "C" {

int letkf_amd_abi_version(void) { return LETKF_AMD_ABI_VERSION; }

const char* letkf_amd_last_error(void) { return g_last_error.c_str(); }

int letkf_ctx_create(int device_id, letkf_ctx** out) {
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
}

int letkf_ctx_destroy(letkf_ctx* c) {
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
}

int letkf_ctx_set_option(letkf_ctx* c, int option, int value) {
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
}

int letkf_ctx_set_stream(letkf_ctx* c, void* hip_stream) {
  if (int rc = check_ctx(c)) return rc;
  // the handle is used as is: NULL is HIP's default (null) stream, which is also what torch.cuda.current_stream()
  // hands out unless the caller switched streams -- work then orders with the caller's other work on that stream
  c->stream = static_cast<hipStream_t>(hip_stream);
  return LETKF_OK;
}

int letkf_ctx_synchronize(letkf_ctx* c) {
  if (int rc = check_ctx(c)) return rc;
  HIP_TRY(hipStreamSynchronize(c->stream));
  return LETKF_OK;
}

int letkf_sched_plan_check(int64_t npts, int64_t stride, int32_t run_len, int32_t grid, int32_t ppw, int32_t resident_per_xcd) {
  return letkf::sched_plan_check((long)npts, (long)stride, run_len, grid, ppw, resident_per_xcd, 1);
}
int letkf_sched_plan_check_units(int64_t npts, int64_t stride, int32_t run_len, int32_t grid, int32_t ppw, int32_t resident_per_xcd, int32_t ub_of) {
  return letkf::sched_plan_check((long)npts, (long)stride, run_len, grid, ppw, resident_per_xcd, ub_of);
}

int letkf_ctx_last_path(letkf_ctx* c, char* buf, int32_t len) {
  if (!c || !buf || len < 1) return fail(LETKF_E_INVALID, "bad argument");
  std::snprintf(buf, (size_t)len, "%s", c->last_path.c_str());
  return LETKF_OK;
}

int letkf_ctx_timing_enable(letkf_ctx* c, int enable) {
  if (int rc = check_ctx(c)) return rc;
  c->timing = enable != 0;
  return LETKF_OK;
}

int letkf_ctx_timing_read(letkf_ctx* c, double* avg_ms, int64_t* nlaunch, int reset) {
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
}

namespace {
// transmd without depd: the reference zeroes a present transmd at nobsl == 0 whatever depd is (common_letkf.f90:97-99) and
// leaves it untouched at nobsl > 0 (:188)
__global__ void zero_transmd_where_nobsl_is_zero(int64_t nbatch, int ne, const int32_t* __restrict__ nobsl,
                                                 double* __restrict__ transmd) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < nbatch * ne && nobsl[i / ne] == 0) transmd[i] = 0.0;
}
}  // namespace

int letkf_core_batch_dev(letkf_ctx* c, const letkf_core_batch_args* g) {
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
    const int64_t n = g->nbatch * (int64_t)g->ne;
    hipLaunchKernelGGL(zero_transmd_where_nobsl_is_zero, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, g->nbatch,
                       g->ne, g->nobsl, g->transmd);
    HIP_TRY(hipGetLastError());
  }
  return LETKF_OK;
}

namespace {

__global__ void zero_where_beta_is_zero(int64_t n, const double* __restrict__ beta, int32_t* __restrict__ cnt) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n && beta[i] == 0.0) cnt[i] = 0;
}

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

// the counts of a count pass to the caller's nobs_out, if it has one: as the list-free route of letkf_das_columns_dev reports
// them, zero where beta = 0 (the reference does not run obs_local there, letkf_tools.f90:333-359)
int report_counts(letkf_ctx* c, const int32_t* counts, int64_t n, const double* beta, int32_t* nobs_out) {
  if (!nobs_out) return LETKF_OK;
  HIP_TRY(hipMemcpyAsync(nobs_out, counts, (size_t)n * 4, hipMemcpyDeviceToDevice, c->stream));
  if (beta) {
    hipLaunchKernelGGL(zero_where_beta_is_zero, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, n, beta, nobs_out);
    HIP_TRY(hipGetLastError());
  }
  return LETKF_OK;
}

// shared by the list-driven and the fused-search entry
// (mode 3, letkf_das_columns_dev's list-free route: the points are pt0 + a * pt_stride + b, b < g->warm_stride columns whose
// horizontal survivors are sv[4 * sv_off[b] ..]; every per-point array of g is indexed by that GLOBAL point number)
struct SurvivorView {
  const int64_t* sv_off;
  const double* sv;
  int64_t pt_stride, pt0;
  int64_t cap;               // most survivors of a column of the batch (bounds a point's local list)
};
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

int das_points_impl(letkf_ctx* c, const letkf_das_args* g, const letkf_search_tables* t, const double* ri,
                    const double* rj, const double* rlev, const double* rz, int32_t* nobs_out,
                    const SurvivorView* sview = nullptr) {
  if (int rc = check_ctx(c)) return rc;
  if (!g) return fail(LETKF_E_INVALID, "args is NULL");
  if (g->npts == 0) return LETKF_OK;
  if (int rc = das_args_check(g, !t)) return rc;
  letkf::PointArgs a;
  std::memset(&a, 0, sizeof(a));
  a.k = g->k;
  a.nv = g->nv;
  a.mode = 0;
  a.npts = g->npts;
  a.obs_off = reinterpret_cast<const long*>(g->obs_off);
  a.obs_idx = g->obs_idx;
  a.rdiag_l = g->rdiag_l;
  a.rloc_l = g->rloc_l;
  a.ensval = g->ensval;
  a.kld = g->kld;
  a.dep = g->dep;
  a.det_run = g->det_run;
  a.infl_adaptive = g->infl_adaptive;
  a.relax_to_inflated_prior = g->relax_to_inflated_prior;
  a.iv_p = g->iv_p;
  a.iv_q_first = g->iv_q_first;
  a.iv_q_last = g->iv_q_last;
  a.relax_alpha = g->relax_alpha;
  a.relax_alpha_spread = g->relax_alpha_spread;
  a.q_update_top = g->q_update_top;
  a.q_sprd_max = g->q_sprd_max;
  a.beta = g->beta;
  a.infl = g->infl;
  a.infl_sv = g->infl_sv > 0 ? g->infl_sv : g->npts;
  a.gues = g->gues;
  a.anal = g->anal;
  a.sp = g->sp;
  a.sm = g->sm;
  a.sv = g->sv;
  a.trans_out = g->trans_out;
  a.transm_out = g->transm_out;
  a.pa_out = g->pa_out;
  a.status = g->status;
  a.nsweep = g->nsweep;
  a.rtps_out = g->rtps_infl_out;
  a.var_mask = g->var_mask ? g->var_mask : ~0u;
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

}  // namespace

int letkf_das_points_dev(letkf_ctx* c, const letkf_das_args* g) {
  return das_points_impl(c, g, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
}

int letkf_das_points_fused_dev(letkf_ctx* c, const letkf_das_args* g, const letkf_search_tables* t, const double* ri,
                               const double* rj, const double* rlev, const double* rz, int32_t* nobs_out) {
  if (!t) return fail(LETKF_E_INVALID, "tables is NULL");
  return das_points_impl(c, g, t, ri, rj, rlev, rz, nobs_out);
}

// (3c) das_letkf's main loop for a whole subdomain: column search + loop body by slabs of levels whose lists fit a
// workspace of the library (scale/letkf/letkf_tools.f90:313, the level loop)
int letkf_das_columns_dev(letkf_ctx* c, const letkf_das_args* g, const letkf_search_tables* t, int64_t nij1, int32_t nlev,
                          const double* rig, const double* rjg, const double* rlev, const double* rz, int64_t list_bytes,
                          int32_t* nobs_out) {
  if (int rc = check_ctx(c)) return rc;
  if (!g || !t) return fail(LETKF_E_INVALID, "args / tables is NULL");
  if (nij1 < 1 || nlev < 1 || g->npts != nij1 * (int64_t)nlev) return fail(LETKF_E_INVALID, "npts must be nij1 * nlev");
  if (!rig || !rjg || !rlev || !rz) return fail(LETKF_E_INVALID, "a point coordinate array is NULL");
  if (g->trans_out || g->transm_out || g->pa_out) return fail(LETKF_E_INVALID, "per-point k x k / w-bar outputs: use letkf_das_points_dev");
  // (the loop body's checks, before the count pass of the list route copies its counts to nobs_out: a refused call writes nothing)
  if (int rc = das_args_check(g, false)) return rc;
  const int64_t npts = g->npts;
  if (list_bytes <= 0) list_bytes = (int64_t)8 << 30;
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
      if (take) return LETKF_OK;
    }
  }
  // (the searches below -- one count pass, a fill pass per slab -- share the ring-ordered survivors of the dense limited case)
  RingKeep ring_keep_guard(c);
  // ---- count pass over all levels, prefix sum, level boundaries back to the host
  ScanWs sw;
  if (int rc = scan_ws(c, &c->scratch, (size_t)npts, 0, &sw)) return rc;
  HIP_TRY(zero_total(c, sw));
  if (int rc = letkf_obs_search_columns_dev(c, t, nij1, nlev, rig, rjg, rlev, rz, 0, sw.counts, nullptr, nullptr, nullptr, nullptr,
                                            nullptr, nullptr))
    return rc;
  HIP_TRY(scan_offsets(c, sw));
  if (int rc = report_counts(c, sw.counts, npts, g->beta, nobs_out)) return rc;
  if (int rc = offsets_to_host(c, sw, (size_t)nij1)) return rc;
  const std::vector<int64_t>& lev_off = sw.hoff;
  // ---- slabs of levels: as many as fit the list workspace (20 B per entry)
  int l0 = 0;
  while (l0 < nlev) {
    const int l1 = (int)chunk_end(lev_off, l0, nlev, 1, 20, list_bytes);
    const int64_t p0 = (int64_t)l0 * nij1, np = (int64_t)(l1 - l0) * nij1;
    ListSlab ls;
    if (int rc = list_slab(c, lev_off[l0], lev_off[l1], &ls)) return rc;
    if (int rc = letkf_obs_search_columns_dev(c, t, nij1, l1 - l0, rig, rjg, rlev + p0, rz + p0, 1, nullptr, sw.off + p0, ls.idx, ls.rd,
                                              ls.rl, nullptr, nullptr))
      return rc;
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

// (3d) weight interpolation (include/letkf_amd_interp.h): letkf_core at the coarse points of a tile by slabs of levels -- the
// column search on the coarse columns, the lists gathered into the batch form of letkf_core_batch_dev, every solver route with
// T, w-bar (and w-bar_det) kept -- then the blend and the apply at every fine point of the slab (letkf_interp.hip)
int letkf_das_interp_dev(letkf_ctx* c, const letkf_das_args* g, const letkf_search_tables* t, const letkf_interp_args* ia) {
  return letkf_das_interp_window_dev(c, g, t, ia, nullptr);
}

// ... on the coarse lattice of a whole domain, for the window of it that the call owns (include/letkf_amd_interp_window.h);
// without a window the arrays are the domain
int letkf_das_interp_window_dev(letkf_ctx* c, const letkf_das_args* g, const letkf_search_tables* t, const letkf_interp_args* ia,
                                const letkf_interp_window* win) {
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
  const int64_t npts = g->npts;
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
  if (int rc = scan_ws(c, &c->scratch, (size_t)npc, 0, &sw)) return rc;
  HIP_TRY(zero_total(c, sw));
  if (int rc = letkf_obs_search_columns_dev(c, t, ncc, nlev, ca.crig, ca.crjg, ca.crlev, ca.crz, 0, sw.counts, nullptr, nullptr, nullptr,
                                            nullptr, nullptr, nullptr))
    return rc;
  HIP_TRY(scan_offsets(c, sw));
  if (ia->nobs_coarse) HIP_TRY(hipMemcpyAsync(ia->nobs_coarse, sw.counts, (size_t)npc * 4, hipMemcpyDeviceToDevice, c->stream));
  std::vector<int32_t> hcount((size_t)npc);
  if (int rc = offsets_to_host(c, sw, (size_t)ncc, hcount.data(), sw.counts, (size_t)npc * 4)) return rc;
  const std::vector<int64_t>& lev_off = sw.hoff;
  std::vector<int32_t> lev_max((size_t)nlev, 0);
  for (int l = 0; l < nlev; ++l)
    for (int64_t cc = 0; cc < ncc; ++cc) lev_max[(size_t)l] = std::max(lev_max[(size_t)l], hcount[(size_t)(l * ncc + cc)]);

  // the rules' switches and the state of the call, as the kernels of this route read them
  letkf::PointArgs P;
  std::memset(&P, 0, sizeof(P));
  P.k = k;
  P.nv = g->nv;
  P.npts = npts;
  P.ensval = g->ensval;
  P.kld = g->kld;
  P.dep = g->dep;
  P.det_run = g->det_run;
  P.relax_to_inflated_prior = g->relax_to_inflated_prior;
  P.iv_p = g->iv_p;
  P.iv_q_first = g->iv_q_first;
  P.iv_q_last = g->iv_q_last;
  P.relax_alpha = g->relax_alpha;
  P.relax_alpha_spread = g->relax_alpha_spread;
  P.q_update_top = g->q_update_top;
  P.q_sprd_max = g->q_sprd_max;
  P.beta = g->beta;
  P.infl = g->infl;
  P.infl_sv = g->infl_sv > 0 ? g->infl_sv : npts;
  P.gues = g->gues;
  P.anal = g->anal;
  P.sp = g->sp;
  P.sm = g->sm;
  P.sv = g->sv;
  P.status = g->status;
  P.rtps_out = g->rtps_infl_out;
  P.var_mask = g->var_mask ? g->var_mask : ~0u;

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
    const int64_t p0c = (int64_t)l0 * ncc, nb = (int64_t)nl * ncc;
    ListSlab ls;
    if (int rc = list_slab(c, lev_off[(size_t)l0], lev_off[(size_t)l1], &ls)) return rc;
    if (int rc = letkf_obs_search_columns_dev(c, t, ncc, nl, ca.crig, ca.crjg, ca.crlev + p0c, ca.crz + p0c, 1, nullptr, sw.off + p0c, ls.idx,
                                              ls.rd, ls.rl, nullptr, nullptr))
      return rc;
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
}

// EFSO, das_efso's loop (scale/letkf/letkf_tools.f90:1158-1302) on caller-built lists: points in chunks whose pair
// workspace fits pair_bytes (the offsets are read back only when the lists do not fit at once)
int letkf_efso_points_dev(letkf_ctx* c, const letkf_efso_args* g) {
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
  if (ends[1] - ends[0] <= cap) return efso_run_slab(c, a, g->npts, ends[0], ends[1]);
  std::vector<int64_t> off((size_t)g->npts + 1);
  HIP_TRY(hipMemcpyAsync(off.data(), g->obs_off, off.size() * 8, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  for (int64_t p0 = 0; p0 < g->npts;) {
    const int64_t p1 = chunk_end(off, p0, g->npts, 1, 1, cap);   // (the budget in entries: cap of them, 1 B each)
    if (off[p1] - off[p0] > kEfsoMaxSlab) return fail(LETKF_E_INVALID, "a point with more than 2^31 local observations");
    letkf::EfsoArgs s = a;
    s.obs_off = a.obs_off + p0;
    s.fcst = a.fcst + p0 * a.sp;
    s.fcer = a.fcer + p0 * a.fsp;
    if (int rc = efso_run_slab(c, s, p1 - p0, off[p0], off[p1])) return rc;
    p0 = p1;
  }
  return LETKF_OK;
}

// EFSO for a whole subdomain: the column search (3a) by slabs of levels whose lists and pair workspace fit list_bytes,
// then the EFSO passes on each slab -- the list route of letkf_das_columns_dev
int letkf_efso_columns_dev(letkf_ctx* c, const letkf_efso_args* g, const letkf_search_tables* t, int64_t nij1, int32_t nlev,
                           const double* rig, const double* rjg, const double* rlev, const double* rz, int64_t list_bytes) {
  letkf::EfsoArgs a;
  if (int rc = efso_check(c, g, false, &a)) return rc;
  if (!t) return fail(LETKF_E_INVALID, "tables is NULL");
  if (nij1 < 1 || nlev < 1 || g->npts != nij1 * (int64_t)nlev) return fail(LETKF_E_INVALID, "npts must be nij1 * nlev");
  if (!rig || !rjg || !rlev || !rz) return fail(LETKF_E_INVALID, "a point coordinate array is NULL");
  c->last_path = std::string("search_columns + ") + letkf::efso_path_name(g->nterm);
  if (list_bytes <= 0) list_bytes = (int64_t)8 << 30;
  const int64_t npts = g->npts, per_entry = 20 + efso_entry_bytes(g->nterm);
  RingKeep ring_keep_guard(c);
  // ---- count pass over all levels, prefix sum, level boundaries back to the host
  ScanWs sw;
  if (int rc = scan_ws(c, &c->scratch, (size_t)npts, 0, &sw)) return rc;
  HIP_TRY(zero_total(c, sw));
  if (int rc = letkf_obs_search_columns_dev(c, t, nij1, nlev, rig, rjg, rlev, rz, 0, sw.counts, nullptr, nullptr, nullptr, nullptr,
                                            nullptr, nullptr))
    return rc;
  HIP_TRY(scan_offsets(c, sw));
  if (int rc = offsets_to_host(c, sw, (size_t)nij1)) return rc;
  const std::vector<int64_t>& lev_off = sw.hoff;
  // ---- slabs of levels whose lists and pair workspace fit: fill pass, EFSO passes
  int l0 = 0;
  while (l0 < nlev) {
    const int l1 = (int)chunk_end(lev_off, l0, nlev, 1, per_entry, list_bytes, kEfsoMaxSlab);
    const int64_t p0 = (int64_t)l0 * nij1, np = (int64_t)(l1 - l0) * nij1;
    if (lev_off[l1] - lev_off[l0] > kEfsoMaxSlab) return fail(LETKF_E_INVALID, "a level with more than 2^31 local observations");
    ListSlab ls;
    if (int rc = list_slab(c, lev_off[l0], lev_off[l1], &ls)) return rc;
    if (int rc = letkf_obs_search_columns_dev(c, t, nij1, l1 - l0, rig, rjg, rlev + p0, rz + p0, 1, nullptr, sw.off + p0, ls.idx, ls.rd,
                                              ls.rl, nullptr, nullptr))
      return rc;
    letkf::EfsoArgs s = a;
    s.obs_off = reinterpret_cast<const long*>(sw.off + p0);
    s.obs_idx = ls.idx;
    s.rdiag_l = ls.rd;
    s.rloc_l = ls.rl;
    s.fcst = a.fcst + p0 * a.sp;
    s.fcer = a.fcer + p0 * a.fsp;
    if (int rc = efso_run_slab(c, s, np, lev_off[l0], lev_off[l1])) return rc;
    l0 = l1;
  }
  return LETKF_OK;
}

// obsense(t, j) = djdy(t, j) * dep(j), das_efso :1283-1290
int letkf_efso_obsense_dev(letkf_ctx* c, int32_t nterm, int64_t nobs, const double* djdy, const double* dep, double* obsense) {
  if (int rc = check_ctx(c)) return rc;
  if (nterm < 1 || nterm > 4) return fail(LETKF_E_INVALID, "nterm must be 1..4");
  if (nobs < 0) return fail(LETKF_E_INVALID, "negative nobs");
  if (nobs > 0 && (!djdy || !dep || !obsense)) return fail(LETKF_E_INVALID, "a required pointer is NULL (djdy, dep, obsense)");
  HIP_TRY(letkf::launch_efso_obsense(nterm, nobs, djdy, dep, obsense, c->stream));
  return LETKF_OK;
}

// (12) das_efso's advection branch (letkf_tools.f90:1225-1229): loc_advection (efso_tools.f90:158-195) on SCALE's grid
int letkf_efso_locadv_dev(letkf_ctx* c, int64_t nij1, int32_t nlev, const double* rig, const double* rjg, const double* u0,
                          const double* v0, const double* u1, const double* v1, double locadv_rate, double eft, double dx,
                          double dy, double* ri, double* rj) {
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
}

// (12) EFSO at per-point positions: the point search (3) and the EFSO passes in runs of consecutive points whose lists and
// pair workspace fit list_bytes -- the chunking of letkf_das_obs_dev
int letkf_efso_search_dev(letkf_ctx* c, const letkf_efso_args* g, const letkf_search_tables* t, int64_t npts, const double* ri,
                          const double* rj, const double* rlev, const double* rz, int64_t list_bytes) {
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
      letkf::EfsoArgs s = a;
      s.obs_off = reinterpret_cast<const long*>(sw.off + p0);
      s.obs_idx = ls.idx;
      s.rdiag_l = ls.rd;
      s.rloc_l = ls.rl;
      s.fcst = a.fcst + p0 * a.sp;
      s.fcer = a.fcer + p0 * a.fsp;
      if (int rc = efso_run_slab(c, s, p1 - p0, sw.hoff[p0], sw.hoff[p1])) return rc;
    }
    p0 = p1;
  }
  return LETKF_OK;
}

// (13) EFSO's front end: the fcer assembly (efso.f90:100-117) and lnorm (efso_tools.f90:52-156) in SCALE's frame
int letkf_efso_norm_dev(letkf_ctx* c, const letkf_efso_norm_params* prm, int64_t nij1, int32_t nlev, double* fcst, int64_t sp,
                        int64_t sm, int64_t sv, double* fmean, double* fcer, int64_t fsp, int64_t fsv, const double* xf,
                        const double* xg, const double* xa, const double* wlev, const double* wg1, const double* lon,
                        const double* lat) {
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
}

// (13) EFSO's back end: print_obsense's table (efso_tools.f90:232-253) for every term
int letkf_efso_summary_dev(letkf_ctx* c, int32_t nterm, int64_t nobs, const double* obsense, const int32_t* elm,
                           const int32_t* typ, const double* lat, const int32_t* qc, int32_t nid, const int32_t* elem_uid,
                           int32_t nobtype, double latbound, int32_t* count, double* sum, int32_t* nneg) {
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
}

// (11) das_letkf_obs (scale/letkf/letkf_tools.f90:933-1156): the loop body at every target observation's own location, on
// the two-variable pseudo-state of letkf_obsanal.hip (variable 0 the target, variable 1 its pressure for Q_UPDATE_TOP), in
// chunks of targets whose lists fit list_bytes
int letkf_das_obs_dev(letkf_ctx* c, const letkf_das_obs_args* g, const letkf_search_tables* t) {
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
}

int letkf_obs_target_var(int32_t elm) {
  switch (elm) {
    case 2819: return 0;              // id_u_obs -> iv3d_u
    case 2820: return 1;              // id_v_obs -> iv3d_v
    case 3073: case 3074: return 3;   // id_t_obs, id_tv_obs -> iv3d_t
    case 3330: case 3331: return 5;   // id_q_obs, id_rh_obs -> iv3d_q
    default: return -1;               // ps (nv2d = 0), rain, radar, H08, TC: n = 0
  }
}

int letkf_ens_to_perturbations_dev(letkf_ctx* c, int32_t k, int32_t nv, int64_t npts, double* x, int64_t sp,
                                   int64_t sm, int64_t sv) {
  if (int rc = check_ctx(c)) return rc;
  if (!x || k < 1 || nv < 1 || npts < 0) return fail(LETKF_E_INVALID, "bad argument");
  if (npts == 0) return LETKF_OK;
  HIP_TRY(letkf::launch_ens_to_pert(k, nv, npts, x, sp, sm, sv, c->stream));
  return LETKF_OK;
}

int letkf_ens_mean_dev(letkf_ctx* c, int32_t k, int32_t nv, int64_t npts, double* x, int64_t sp, int64_t sm,
                       int64_t sv) {
  if (int rc = check_ctx(c)) return rc;
  if (!x || k < 1 || nv < 1 || npts < 0) return fail(LETKF_E_INVALID, "bad argument");
  if (npts == 0) return LETKF_OK;
  HIP_TRY(letkf::launch_ens_mean(k, nv, npts, x, sp, sm, sv, c->stream));
  return LETKF_OK;
}

int letkf_obs_search_dev(letkf_ctx* c, const letkf_search_tables* t, int64_t npts, const double* ri, const double* rj,
                         const double* rlev, const double* rz, int32_t fill, int32_t* counts, const int64_t* obs_off,
                         int32_t* obs_idx, double* rdiag_l, double* rloc_l) {
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
}

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
                                 double* rdiag_l, double* rloc_l, int32_t* nobs_ctype, double* cutd_ctype) {
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
}

int letkf_obs_departure_dev(letkf_ctx* c, const letkf_qc_params* p, int64_t nobs, const int32_t* elm, const double* dat,
                            const double* err, double* ensval, int64_t kld, double* val, int32_t* qc) {
  if (int rc = check_ctx(c)) return rc;
  if (!p || nobs < 0) return fail(LETKF_E_INVALID, "params is NULL or nobs < 0");
  if (nobs == 0) return LETKF_OK;
  if (!elm || !dat || !err || !ensval || !val || !qc) return fail(LETKF_E_INVALID, "an observation array is NULL");
  if (p->member < 1 || kld < p->member + (p->det_run ? 1 : 0))
    return fail(LETKF_E_INVALID, "kld must hold MEMBER (+1 with DET_RUN) columns");
  if ((size_t)64 * (size_t)(kld | 1) * sizeof(double) > c->lds_max) return fail(LETKF_E_INVALID, "kld too large");
  HIP_TRY(letkf::launch_obs_departure(*p, nobs, elm, dat, err, ensval, kld, val, qc, c->num_cu, c->stream));
  return LETKF_OK;
}

int letkf_obs_mesh_sort_dev(letkf_ctx* c, const letkf_mesh* m, int64_t nobs, const int32_t* ctype, const double* ri,
                            const double* rj, const int32_t* qc, int32_t* n_cell, int32_t* key, int64_t* nsorted) {
  if (int rc = check_ctx(c)) return rc;
  if (!m || nobs < 0 || !nsorted) return fail(LETKF_E_INVALID, "mesh / nsorted is NULL or nobs < 0");
  if (m->nctype < 1 || !m->ngrd_i || !m->ngrd_j || m->nlon < 1 || m->nlat < 1)
    return fail(LETKF_E_INVALID, "bad mesh description");
  if (nobs > 0 && (!ctype || !ri || !rj || !qc || !key)) return fail(LETKF_E_INVALID, "an observation array is NULL");
  if (!n_cell) return fail(LETKF_E_INVALID, "n_cell is NULL");
  if (nobs >= (1LL << 31)) return fail(LETKF_E_INVALID, "more than 2^31 local observations");
  size_t need = 0;
  long ns = 0;
  HIP_TRY(letkf::obs_mesh_sort(*m, nobs, ctype, ri, rj, qc, n_cell, key, &ns, nullptr, &need, c->num_cu, c->stream));
  if (int rc = grow(c, &c->scratch, need)) return rc;
  size_t have = c->scratch.cap;
  HIP_TRY(letkf::obs_mesh_sort(*m, nobs, ctype, ri, rj, qc, n_cell, key, &ns, c->scratch.p, &have, c->num_cu, c->stream));
  *nsorted = ns;
  return LETKF_OK;
}

int letkf_obs_halo_plan_dev(letkf_ctx* c, const letkf_halo_layout* l, const int32_t* n_all, int32_t* ac_ext,
                            int32_t* src_row, int64_t cap, int64_t* nobstotal) {
  if (int rc = check_ctx(c)) return rc;
  if (!l || !nobstotal || !n_all || !ac_ext) return fail(LETKF_E_INVALID, "a required pointer is NULL");
  if (l->nctype < 1 || l->nprocs < 1 || l->prc_num_x < 1 || l->myrank < 0 || l->myrank >= l->nprocs ||
      l->nprocs % l->prc_num_x != 0 || !l->ngrd_i || !l->ngrd_j || !l->ngrdsch_i || !l->ngrdsch_j)
    return fail(LETKF_E_INVALID, "bad rank layout / mesh description");
  if (cap > 0 && !src_row) return fail(LETKF_E_INVALID, "src_row is NULL");
  long nt = 0;
  hipError_t e = letkf::obs_halo_plan(*l, n_all, ac_ext, src_row, cap, &nt, c->num_cu, c->stream);
  *nobstotal = nt;
  if (e == hipErrorInvalidValue && nt > cap) return fail(LETKF_E_INVALID, "src_row capacity is smaller than nobstotal");
  HIP_TRY(e);
  return LETKF_OK;
}

int letkf_obs_gather_rows_dev(letkf_ctx* c, int64_t nrows, const int32_t* src_row, int32_t ncols, const double* src,
                              int64_t ld_src, double* dst, int64_t ld_dst) {
  if (int rc = check_ctx(c)) return rc;
  if (nrows < 0 || ncols < 0) return fail(LETKF_E_INVALID, "negative size");
  if (nrows == 0 || ncols == 0) return LETKF_OK;
  if (!src_row || !src || !dst || ld_src < ncols || ld_dst < ncols) return fail(LETKF_E_INVALID, "bad argument");
  HIP_TRY(letkf::launch_gather_rows(nrows, src_row, ncols, src, ld_src, dst, ld_dst, c->num_cu, c->stream));
  return LETKF_OK;
}

int letkf_obs_gather_i32_dev(letkf_ctx* c, int64_t nrows, const int32_t* src_row, const int32_t* src, int32_t* dst) {
  if (int rc = check_ctx(c)) return rc;
  if (nrows < 0) return fail(LETKF_E_INVALID, "negative size");
  if (nrows == 0) return LETKF_OK;
  if (!src_row || !src || !dst) return fail(LETKF_E_INVALID, "bad argument");
  HIP_TRY(letkf::launch_gather_i32(nrows, src_row, src, dst, c->num_cu, c->stream));
  return LETKF_OK;
}

int letkf_obs_mesh_dims(int32_t nctype, const int32_t* typ_ctype, const double* hori_loc_ctype, int32_t nobtype,
                        const double* obs_sort_grid_spacing, const int32_t* max_nobs_per_grid, const double* obs_min_spacing,
                        double dx, double dy, int32_t nlon, int32_t nlat, int32_t* ngrd_i, int32_t* ngrd_j, double* grdspc_i,
                        double* grdspc_j, int32_t* ngrdsch_i, int32_t* ngrdsch_j, int32_t* ngrdext_i, int32_t* ngrdext_j) {
  if (nctype < 0 || nobtype < 1 || nlon < 1 || nlat < 1) return fail(LETKF_E_INVALID, "bad sizes");
  if (nctype > 0 && (!typ_ctype || !hori_loc_ctype || !obs_sort_grid_spacing || !max_nobs_per_grid || !obs_min_spacing ||
                     !ngrd_i || !ngrd_j || !grdspc_i || !grdspc_j || !ngrdsch_i || !ngrdsch_j || !ngrdext_i || !ngrdext_j))
    return fail(LETKF_E_INVALID, "an array is NULL");
  if (letkf::obs_mesh_dims(nctype, typ_ctype, hori_loc_ctype, nobtype, obs_sort_grid_spacing, max_nobs_per_grid,
                           obs_min_spacing, dx, dy, nlon, nlat, ngrd_i, ngrd_j, grdspc_i, grdspc_j, ngrdsch_i, ngrdsch_j,
                           ngrdext_i, ngrdext_j))
    return fail(LETKF_E_INVALID, "a report type outside 1..nobtype or an empty mesh");
  return LETKF_OK;
}

int letkf_set_obs_local_dev(letkf_ctx* c, const letkf_setobs_params* p, const letkf_qc_params* qcp, const letkf_obs_file_rows* files,
                            int64_t nobs, const int32_t* set, const int32_t* idx, int32_t* qc, double* ensval, int64_t kld,
                            letkf_obs_table** tab) {
  if (int rc = check_ctx(c)) return rc;
  std::string msg;
  if (int rc = letkf::set_obs_local(c->device, c->stream, c->num_cu, p, qcp, files, nobs, set, idx, qc, ensval, kld, tab, &msg))
    return fail(rc, msg);
  return LETKF_OK;
}

int letkf_set_obs_finish_dev(letkf_ctx* c, letkf_obs_table* tab, const int32_t* n_all, const int32_t* tot_g, int64_t nrecv,
                             const double* recv) {
  if (int rc = check_ctx(c)) return rc;
  std::string msg;
  if (int rc = letkf::set_obs_finish(c->stream, c->num_cu, tab, n_all, tot_g, nrecv, recv, &msg)) return fail(rc, msg);
  return LETKF_OK;
}

int letkf_set_obs_dev(letkf_ctx* c, const letkf_setobs_params* p, const letkf_qc_params* qcp, const letkf_obs_file_rows* files,
                      int64_t nobs, const int32_t* set, const int32_t* idx, int32_t* qc, double* ensval, int64_t kld,
                      letkf_obs_table** tab) {
  if (!p || p->nprocs != 1) return fail(LETKF_E_INVALID, "letkf_set_obs_dev is the one-rank call: nprocs must be 1");
  if (int rc = letkf_set_obs_local_dev(c, p, qcp, files, nobs, set, idx, qc, ensval, kld, tab)) return rc;
  letkf_obs_table_info i;
  letkf::obs_table_info(*tab, &i);
  if (int rc = letkf_set_obs_finish_dev(c, *tab, i.n_cell, nullptr, i.nsorted, i.sendbuf)) {
    letkf_obs_table_destroy(*tab);
    *tab = nullptr;
    return rc;
  }
  return LETKF_OK;
}

int letkf_obs_table_info_get(const letkf_obs_table* tab, letkf_obs_table_info* info) {
  if (letkf::obs_table_info(tab, info)) return fail(LETKF_E_INVALID, "tab / info is NULL");
  return LETKF_OK;
}

int letkf_obs_table_search(const letkf_obs_table* tab, letkf_search_tables* tables) {
  if (letkf::obs_table_search(tab, tables)) return fail(LETKF_E_INVALID, "tab / tables is NULL or the finish half has not run");
  return LETKF_OK;
}

int letkf_obs_table_set_varloc(letkf_ctx* c, letkf_obs_table* tab, const double* varloc) {
  if (int rc = check_ctx(c)) return rc;
  std::string msg;
  if (int rc = letkf::obs_table_set_varloc(c->stream, tab, varloc, &msg)) return fail(rc, msg);
  return LETKF_OK;
}

int letkf_obs_table_download(letkf_ctx* c, const letkf_obs_table* tab, double* ensval, double* val, int32_t* qc, double* ob_ri,
                             double* ob_rj, double* ob_lev, double* ob_dat, double* ob_err, int32_t* ac_ext) {
  if (int rc = check_ctx(c)) return rc;
  std::string msg;
  double* ob[5] = {ob_ri, ob_rj, ob_lev, ob_dat, ob_err};
  if (int rc = letkf::obs_table_download(c->stream, tab, ensval, val, qc, ob, ac_ext, &msg)) return fail(rc, msg);
  return LETKF_OK;
}

int letkf_obs_table_destroy(letkf_obs_table* tab) {
  letkf::obs_table_destroy(tab);
  return LETKF_OK;
}

int letkf_monit_dep_dev(letkf_ctx* c, int32_t nid, const int32_t* elem_uid, int64_t nn, const int32_t* elm,
                        const double* dep, const int32_t* qc, int32_t* nobs, double* bias, double* rmse) {
  if (int rc = check_ctx(c)) return rc;
  if (nid < 1 || nid > 32 || !elem_uid || nn < 0 || !nobs || !bias || !rmse)
    return fail(LETKF_E_INVALID, "bad element table / outputs");
  if (nn > 0 && (!elm || !dep || !qc)) return fail(LETKF_E_INVALID, "an observation array is NULL");
  const size_t need = letkf::monit_scratch_bytes(nid, c->num_cu);
  if (int rc = grow(c, &c->scratch, need)) return rc;
  HIP_TRY(letkf::launch_monit_dep(nid, elem_uid, nn, elm, dep, qc, nobs, bias, rmse, c->scratch.p, c->num_cu, c->stream));
  return LETKF_OK;
}

int letkf_additive_inflation_dev(letkf_ctx* c, int32_t k, int32_t nv, int64_t npts, int64_t nij1, double* anal,
                                 const double* add, int64_t sp, int64_t sm, int64_t sv, double infl_add,
                                 const double* weight, const double* qmean, int64_t q_sp, int64_t q_sv,
                                 int32_t iv_q_first, int32_t iv_q_last, const int32_t* ishuf) {
  if (int rc = check_ctx(c)) return rc;
  if (k < 1 || nv < 1 || npts < 0 || nij1 < 1 || !anal || !add) return fail(LETKF_E_INVALID, "bad argument");
  if (npts % nij1 != 0) return fail(LETKF_E_INVALID, "npts must be nij1 * nlev");
  HIP_TRY(letkf::launch_additive(k, nv, npts, nij1, anal, add, sp, sm, sv, infl_add, weight, qmean, q_sp, q_sv,
                                 iv_q_first, iv_q_last, ishuf, c->num_cu, c->stream));
  return LETKF_OK;
}

int letkf_addinfl_weight_dev(letkf_ctx* c, int64_t nij1, const double* rig, const double* rjg, int64_t nob,
                             const double* ob_ri, const double* ob_rj, double dx, double dy, double hori_loc,
                             double* weight) {
  if (int rc = check_ctx(c)) return rc;
  if (nij1 < 0 || nob < 0 || !(hori_loc > 0.0)) return fail(LETKF_E_INVALID, "bad argument");
  if (nij1 == 0) return LETKF_OK;
  if (!rig || !rjg || !weight || (nob > 0 && (!ob_ri || !ob_rj))) return fail(LETKF_E_INVALID, "a pointer is NULL");
  const double cut2 = (double)13.33333333f;   // dist_zero_fac_square, a single-precision literal (letkf_obs.f90:28)
  HIP_TRY(letkf::launch_addinfl_weight(nij1, rig, rjg, nob, ob_ri, ob_rj, dx, dy, hori_loc, cut2, weight, c->num_cu,
                                       c->stream));
  return LETKF_OK;
}

int letkf_obs_allgatherv_dev(letkf_ctx* c, void* nccl_comm, int32_t nranks, int32_t myrank, const int64_t* counts,
                             int64_t row_bytes, const void* send, void* recv) {
  if (int rc = check_ctx(c)) return rc;
  if (!nccl_comm || nranks < 1 || myrank < 0 || myrank >= nranks || !counts || row_bytes < 1)
    return fail(LETKF_E_INVALID, "bad communicator / rank layout / counts");
  int64_t total = 0;
  for (int r = 0; r < nranks; ++r) {
    if (counts[r] < 0) return fail(LETKF_E_INVALID, "negative row count");
    total += counts[r];
  }
  if ((counts[myrank] > 0 && !send) || (total > 0 && !recv)) return fail(LETKF_E_INVALID, "a buffer is NULL");
  const char* what = "";
  const int rc = letkf::rccl_allgatherv(nccl_comm, nranks, myrank, counts, row_bytes, send, recv, c->stream, &what);
  if (rc == -1) return fail(LETKF_E_INVALID, "RCCL (librccl.so.1) is not available in this process");
  if (rc != 0) return fail(LETKF_E_HIP, std::string("RCCL: ") + what);
  return LETKF_OK;
}

namespace {
int rccl_result(int rc, const char* what) {
  if (rc == 0) return LETKF_OK;
  if (rc == -1) return fail(LETKF_E_INVALID, "RCCL (librccl.so.1) is not available in this process");
  if (rc == -2) return fail(LETKF_E_INVALID, what);
  return fail(LETKF_E_HIP, std::string("RCCL: ") + what);
}
}  // namespace

int letkf_alltoallv_dev(letkf_ctx* c, void* nccl_comm, int32_t nranks, int32_t myrank, const int64_t* send_counts,
                        const int64_t* send_offs, const int64_t* recv_counts, const int64_t* recv_offs, int64_t row_bytes,
                        const void* send, void* recv) {
  if (int rc = check_ctx(c)) return rc;
  if ((nranks > 1 && !nccl_comm) || nranks < 1 || myrank < 0 || myrank >= nranks || !send_counts || !send_offs || !recv_counts ||
      !recv_offs || row_bytes < 1)
    return fail(LETKF_E_INVALID, "bad communicator / rank layout / counts");
  int64_t ns = 0, nr = 0;
  for (int r = 0; r < nranks; ++r) {
    if (send_counts[r] < 0 || recv_counts[r] < 0 || send_offs[r] < 0 || recv_offs[r] < 0) return fail(LETKF_E_INVALID, "negative count / offset");
    ns += send_counts[r];
    nr += recv_counts[r];
  }
  if ((ns > 0 && !send) || (nr > 0 && !recv)) return fail(LETKF_E_INVALID, "a buffer is NULL");
  const char* what = "";
  return rccl_result(letkf::rccl_alltoallv(nccl_comm, nranks, myrank, send_counts, send_offs, recv_counts, recv_offs, row_bytes, send,
                                           recv, c->stream, &what), what);
}

int letkf_allreduce_sum_i32_dev(letkf_ctx* c, void* nccl_comm, int32_t nranks, int64_t count, int32_t* buf) {
  if (int rc = check_ctx(c)) return rc;
  if ((nranks > 1 && !nccl_comm) || nranks < 1 || count < 0 || (count > 0 && !buf)) return fail(LETKF_E_INVALID, "bad argument");
  const char* what = "";
  return rccl_result(letkf::rccl_allreduce_sum_i32(nccl_comm, nranks, count, buf, c->stream, &what), what);
}

// scatter_grd_mpi_alltoall / gather_grd_mpi_alltoall (scale/common/common_mpi_scale.f90:1279-1396) with the exchange inside the
// library: per-destination blocks [nv3d][nlev * nij1(d)] dealt out of / assembled into the member field by the kernel of
// letkf_member_points_dev (grd_to_buf / buf_to_grd), ONE grouped exchange with true counts, the blocks filed into / taken from
// the member slots of the state.  Workspace: the context's scratch buffer (send blocks | receive blocks).
int letkf_members_alltoall_dev(letkf_ctx* c, void* nccl_comm, int32_t nranks, int32_t myrank, int32_t dir, int32_t nlev,
                               int32_t nlon, int32_t nlat, int32_t nv3d, int32_t mstart, int32_t mcount, double* v3dg, double* x,
                               int64_t sp, int64_t sm, int64_t sv) {
  if (int rc = check_ctx(c)) return rc;
  if ((nranks > 1 && !nccl_comm) || nranks < 1 || myrank < 0 || myrank >= nranks || nlev < 1 || nlon < 1 || nlat < 1 || nv3d < 1 ||
      mstart < 0 || mcount < 0 || mcount > nranks || (dir != 0 && dir != 1))
    return fail(LETKF_E_INVALID, "bad argument");
  const bool holder = myrank < mcount;                    // this rank holds / receives the whole field of member mstart + myrank
  if (holder && !v3dg) return fail(LETKF_E_INVALID, "v3dg is NULL on a rank that holds a member");
  const long nxy = (long)nlon * nlat;
  auto share = [&](int r) { return (nxy - r + nranks - 1) / nranks; };   // points r, r + nranks, ... (grd_to_buf)
  const long nij1 = share(myrank), npl = (long)nlev * nij1;
  // a rank beyond the last point (nranks > nlon * nlat: nij1 = 0, common_mpi_scale.f90:267-273) has an empty state and still
  // takes part: it may hold a member, and its peers' groups count on it
  if (!x && nij1 > 0) return fail(LETKF_E_INVALID, "x is NULL on a rank that owns points");
  if (mcount == 0) return LETKF_OK;                       // an empty batch: nothing to move, nothing posted
  std::vector<int64_t> fc(nranks), fo(nranks), pc(nranks), po(nranks);   // field side (all points of my member), point side (my points of every member)
  int64_t ftot = 0, ptot = 0;
  for (int r = 0; r < nranks; ++r) {
    fc[r] = holder ? (int64_t)nv3d * nlev * share(r) : 0;
    fo[r] = ftot;
    ftot += fc[r];
    pc[r] = r < mcount ? (int64_t)nv3d * npl : 0;
    po[r] = ptot;
    ptot += pc[r];
  }
  const size_t need = (size_t)(ftot + ptot) * sizeof(double) + 256;
  if (int rc = grow(c, &c->scratch, need)) return rc;
  double* fbuf = reinterpret_cast<double*>(c->scratch.p);
  double* pbuf = fbuf + ftot;
  const char* what = "";
  if (dir == 0) {   // member fields -> point-major state
    if (holder)
      for (int d = 0; d < nranks; ++d) {
        const long nd = share(d);
        if (nd > 0) HIP_TRY(letkf::launch_member_points(0, nlev, nlon, nxy, nv3d, nranks, d, nd, v3dg, fbuf + fo[d], 1, 0, nd * nlev, c->stream));
      }
    if (int rc = rccl_result(letkf::rccl_alltoallv(nccl_comm, nranks, myrank, fc.data(), fo.data(), pc.data(), po.data(), 8, fbuf, pbuf,
                                                   c->stream, &what), what))
      return rc;
    for (int s_ = 0; s_ < mcount; ++s_)
      HIP_TRY(letkf::launch_block_slot(0, npl, nv3d, pbuf + po[s_], x, sp, (long)(mstart + s_) * sm, sv, c->stream));
  } else {          // point-major state -> member fields
    for (int d = 0; d < mcount; ++d)
      HIP_TRY(letkf::launch_block_slot(1, npl, nv3d, pbuf + po[d], x, sp, (long)(mstart + d) * sm, sv, c->stream));
    if (int rc = rccl_result(letkf::rccl_alltoallv(nccl_comm, nranks, myrank, pc.data(), po.data(), fc.data(), fo.data(), 8, pbuf, fbuf,
                                                   c->stream, &what), what))
      return rc;
    if (holder)
      for (int s_ = 0; s_ < nranks; ++s_) {
        const long ns = share(s_);
        if (ns > 0) HIP_TRY(letkf::launch_member_points(1, nlev, nlon, nxy, nv3d, nranks, s_, ns, v3dg, fbuf + fo[s_], 1, 0, ns * nlev, c->stream));
      }
  }
  return LETKF_OK;
}

int letkf_relax_beta_dev(letkf_ctx* c, const letkf_beta_params* p, int64_t nij1, int32_t nlev, const double* rig,
                         const double* rjg, const double* hgt, double* beta) {
  if (int rc = check_ctx(c)) return rc;
  if (!p || nij1 < 0 || nlev < 1) return fail(LETKF_E_INVALID, "params is NULL or bad nij1 / nlev");
  if (nij1 == 0) return LETKF_OK;
  if (!rig || !rjg || !hgt || !beta) return fail(LETKF_E_INVALID, "a point array is NULL");
  HIP_TRY(letkf::launch_relax_beta(*p, nij1, nlev, rig, rjg, hgt, beta, c->num_cu, c->stream));
  return LETKF_OK;
}

int letkf_infl_init_dev(letkf_ctx* c, int64_t n, double* work3d, double infl_mul, double infl_mul_min) {
  if (int rc = check_ctx(c)) return rc;
  if (n < 0) return fail(LETKF_E_INVALID, "negative size");
  if (n == 0) return LETKF_OK;
  if (!work3d) return fail(LETKF_E_INVALID, "work3d is NULL");
  HIP_TRY(letkf::launch_infl_init(n, work3d, infl_mul, infl_mul_min, c->num_cu, c->stream));
  return LETKF_OK;
}

int letkf_state_trans_dev(letkf_ctx* c, const letkf_state_consts* k, int32_t nlev, int32_t nlon, int32_t nlat,
                          int32_t nv3d, double* v3dg, int32_t inverse) {
  if (int rc = check_ctx(c)) return rc;
  if (!k || !v3dg || nlev < 1 || nlon < 1 || nlat < 1) return fail(LETKF_E_INVALID, "bad argument");
  if (k->iv_q < 0 || k->iv_q >= nv3d || nv3d - k->iv_q > 8) return fail(LETKF_E_INVALID, "moisture range must be 1..8 variables");
  HIP_TRY(letkf::launch_state_trans(*k, nlev, (long)nlon * nlat, nv3d, v3dg, inverse, c->stream));
  return LETKF_OK;
}

int letkf_member_points_dev(letkf_ctx* c, int32_t dir, int32_t nlev, int32_t nlon, int32_t nlat, int32_t nv3d,
                            int32_t np, int32_t rank, int32_t m, double* v3dg, double* x, int64_t nij1, int64_t sp,
                            int64_t sm, int64_t sv) {
  if (int rc = check_ctx(c)) return rc;
  if (!v3dg || !x || np < 1 || rank < 0 || rank >= np || m < 0 || nij1 < 0) return fail(LETKF_E_INVALID, "bad argument");
  const long nxy = (long)nlon * nlat;
  const long expect = (nxy - rank + np - 1) / np;               // points r, r+np, ... below nlon*nlat
  if (nij1 != expect) return fail(LETKF_E_INVALID, "nij1 does not match the cyclic share of this rank");
  if (nij1 == 0) return LETKF_OK;
  HIP_TRY(letkf::launch_member_points(dir, nlev, nlon, nxy, nv3d, np, rank, nij1, v3dg, x, sp, (long)m * sm, sv, c->stream));
  return LETKF_OK;
}

int letkf_ens_spread_dev(letkf_ctx* c, int32_t k, int32_t nv, int64_t npts, const double* x, int64_t sp, int64_t sm,
                         int64_t sv, double* sprd) {
  if (int rc = check_ctx(c)) return rc;
  if (!x || !sprd || k < 2 || nv < 1 || npts < 0) return fail(LETKF_E_INVALID, "bad argument");
  if (npts == 0) return LETKF_OK;
  HIP_TRY(letkf::launch_ens_spread(k, nv, npts, x, sp, sm, sv, sprd, c->stream));
  return LETKF_OK;
}

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
                  const int* rdiag_wloc, const int* infl_update, const double* depd, double* transmd, int* status) {
  int st = 0;
  int rc = core_host(ne, nobs, nobsl, hdxb, rdiag, rloc, dep, parm_infl, trans, transm, pao, rdiag_wloc,
                     infl_update, depd, transmd, &st);
  if (rc != LETKF_OK) {
    std::fprintf(stderr, "!!! ERROR (letkf_core_c): %s\n", g_last_error.c_str());
    st = rc;
  }
  if (status) *status = st;
}

// The observation operator (include/letkf_amd_obsope.h, letkf_obsope.hip): argument checks, the row flag's word, the launch.
int letkf_obsope_dev(letkf_ctx* c, const letkf_obsope_params* p, const letkf_obs_file_rows* files, const letkf_obsope_fields* f,
                     int64_t row0, int64_t nrows, const int32_t* set, const int32_t* idx, int32_t* qc, double* ensval,
                     int64_t kld) try {
  if (int rc = check_ctx(c)) return rc;
  std::string msg;
  if (int rc = letkf::obsope_check(p, files, f, row0, nrows, set, idx, qc, ensval, kld, &msg)) return fail(rc, msg);
  if (int rc = grow(c, &c->scratch, 256)) return rc;
  if (int rc = letkf::obsope_run(c->stream, p, files, f, row0, nrows, set, idx, qc, ensval, kld,
                                 reinterpret_cast<int32_t*>(c->scratch.p), &msg))
    return fail(rc, msg);
  return LETKF_OK;
} catch (const std::exception& e) {
  return fail(LETKF_E_INVALID, std::string("letkf_obsope_dev: ") + e.what());
} catch (...) {
  return fail(LETKF_E_INVALID, "letkf_obsope_dev: unknown exception");
}

}  // extern "C"
