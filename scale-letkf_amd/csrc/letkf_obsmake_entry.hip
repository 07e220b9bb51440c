// letkf_obsmake_entry.hip -- C ABI of the fifth companion header include/letkf_amd_obsmake.h: the random stream of com_rand /
// com_randn and the two halves of obsmake_cal.  Host side only, in the library of the OSSE tools (libletkf_amd_osse.so): the
// kernels are letkf_obsmake.hip's, the operator's letkf_obsope.hip's, the generator letkf_sfmt.cpp's; the context, its scratch
// buffer, the scan plumbing and the error text are the main library's (letkf_api_internal.h).

#include "letkf_api_internal.h"
#include "letkf_obsmake_dev.h"
#include "letkf_sfmt.h"

using namespace letkf::api;

// The generator and its staging: two pinned host buffers and their device twins of `cap` pairs, an event per pair of buffers.
// Chunk c + 1 is generated on the host while the copy and the kernel of chunk c run; a buffer is refilled once its event has passed.
struct letkf_rand {
  letkf::Sfmt gen;
  int64_t chunk = 262144, cap = 0;
  double* host[2] = {nullptr, nullptr};
  double* dev[2] = {nullptr, nullptr};
  hipEvent_t ev[2] = {nullptr, nullptr};
  bool pending[2] = {false, false};
  int next = 0;

  void release() {
    for (int b = 0; b < 2; ++b) {
      if (pending[b]) (void)hipEventSynchronize(ev[b]);
      pending[b] = false;
      if (host[b]) (void)hipHostFree(host[b]);
      if (dev[b]) (void)hipFree(dev[b]);
      if (ev[b]) (void)hipEventDestroy(ev[b]);
      host[b] = dev[b] = nullptr, ev[b] = nullptr;
    }
    cap = 0;
  }
};

namespace {

int staging(letkf_rand* r) {
  if (r->cap == r->chunk) return LETKF_OK;
  r->release();
  for (int b = 0; b < 2; ++b) {
    HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&r->host[b]), (size_t)r->chunk * 16, hipHostMallocDefault));
    HIP_TRY(hipMalloc(reinterpret_cast<void**>(&r->dev[b]), (size_t)r->chunk * 16));
    HIP_TRY(hipEventCreateWithFlags(&r->ev[b], hipEventDisableTiming));
  }
  r->cap = r->chunk;
  return LETKF_OK;
}

// com_randn(n, out) on the context's stream
int randn(letkf_ctx* c, letkf_rand* r, int64_t n, double* out) {
  if (n == 0) return LETKF_OK;
  if (int rc = staging(r)) return rc;
  const int64_t npairs = (n + 1) / 2;
  for (int64_t p0 = 0; p0 < npairs; p0 += r->cap) {
    const int64_t cp = std::min(r->cap, npairs - p0);
    const int b = r->next;
    r->next ^= 1;
    if (r->pending[b]) {
      HIP_TRY(hipEventSynchronize(r->ev[b]));
      r->pending[b] = false;
    }
    r->gen.res53(2 * cp, r->host[b]);
    HIP_TRY(hipMemcpyAsync(r->dev[b], r->host[b], (size_t)cp * 16, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(letkf::randn_pairs(c->stream, cp, r->dev[b], out + 2 * p0, n - 2 * p0));
    HIP_TRY(hipEventRecord(r->ev[b], c->stream));
    r->pending[b] = true;
  }
  return LETKF_OK;
}

}  // namespace

extern "C" {

int letkf_rand_create(int32_t seed, letkf_rand** r) try {
  if (!r) return fail(LETKF_E_INVALID, "r is NULL");
  *r = new letkf_rand();
  (*r)->gen.seed((uint32_t)seed);
  return LETKF_OK;
} LETKF_ENTRY_END(letkf_rand_create)

int letkf_rand_destroy(letkf_rand* r) try {
  if (r) r->release();
  delete r;
  return LETKF_OK;
} LETKF_ENTRY_END(letkf_rand_destroy)

int letkf_rand_set_chunk(letkf_rand* r, int64_t pairs) try {
  if (!r) return fail(LETKF_E_INVALID, "r is NULL");
  if (pairs < 1 || pairs > ((int64_t)1 << 30)) return fail(LETKF_E_INVALID, "pairs must be 1 .. 2^30");
  r->chunk = pairs;
  return LETKF_OK;
} LETKF_ENTRY_END(letkf_rand_set_chunk)

int letkf_rand_res53(letkf_rand* r, int64_t n, double* out) try {
  if (!r) return fail(LETKF_E_INVALID, "r is NULL");
  if (n < 0) return fail(LETKF_E_INVALID, "n is negative");
  if (n > 0 && !out) return fail(LETKF_E_INVALID, "out is NULL");
  r->gen.res53(n, out);
  return LETKF_OK;
} LETKF_ENTRY_END(letkf_rand_res53)

int letkf_randn_dev(letkf_ctx* c, letkf_rand* r, int64_t n, double* out) try {
  if (int rc = check_ctx(c)) return rc;
  if (!r) return fail(LETKF_E_INVALID, "r is NULL");
  if (n < 0) return fail(LETKF_E_INVALID, "n is negative");
  if (n > 0 && !out) return fail(LETKF_E_INVALID, "out is NULL");
  return randn(c, r, n, out);
} LETKF_ENTRY_END(letkf_randn_dev)

// Count -> scan -> fill: the slot's rows of this subdomain as set / idx / rotc lists -> the operator on them in obsmake_cal's
// mode, the row count taken from the scan's total on the device (its row check is the call's one read-back) -> scatter.
// Nothing of the caller's is written before the read-back has passed.
int letkf_obsmake_slot_dev(letkf_ctx* c, const letkf_obsmake_slot* s, const letkf_obsope_params* op, const letkf_obs_file_rows* files,
                           const letkf_obsope_fields* f, int64_t* counts) try {
  if (int rc = check_ctx(c)) return rc;
  if (!s || !s->dif) return fail(LETKF_E_INVALID, "slot / dif is NULL");
  if (!std::isfinite(s->slot_lb) || !std::isfinite(s->slot_ub) || !(s->slot_lb < s->slot_ub))
    return fail(LETKF_E_INVALID, "slot_lb and slot_ub must be finite and slot_lb < slot_ub");
  if (f && f->nmem != 1) return fail(LETKF_E_INVALID, "obsmake takes one state per slot: nmem must be 1");
  static int32_t some_i = 0;                                        // (obsope_check tests its arrays for NULL only; the real ones follow)
  static double some_d = 0.0;
  std::string msg;
  if (int rc = letkf::obsope_check(op, files, f, 0, 0, &some_i, &some_i, &some_i, &some_d, 1, &msg)) return fail(rc, msg);
  if (files->off[0] != 0) return fail(LETKF_E_INVALID, "files->off[0] must be 0");
  const int64_t n = files->off[files->nfile];
  if (n > 0 && !files->dat) return fail(LETKF_E_INVALID, "files->dat is NULL");
  if (n > 0x7fffffff) return fail(LETKF_E_INVALID, "more than 2^31 - 1 file rows");

  ScanWs sw;
  if (int rc = scan_ws(c, &c->scratch, (size_t)n, letkf::obsmake_ws_bytes(n), &sw)) return rc;
  letkf::ObsmakeWs w;
  letkf::obsmake_ws_layout(sw.tail, n, &w);
  letkf::ObsmakeRows R = {};
  R.nfile = files->nfile;
  for (int i = 0; i <= files->nfile; ++i) R.off[i] = files->off[i];
  R.n = n, R.dif = s->dif, R.own = s->own, R.lb = s->slot_lb, R.ub = s->slot_ub, R.outside_undef = s->outside_undef != 0;
  HIP_TRY(zero_total(c, sw));
  HIP_TRY(letkf::obsmake_count(c->stream, R, sw.counts, w));
  HIP_TRY(scan_offsets(c, sw));
  HIP_TRY(letkf::obsmake_fill(c->stream, R, sw.counts, sw.off, op->rotc, w));
  letkf_obsope_params gop = *op;                                    // the operator on the compacted rows: rotc follows them
  if (op->rotc) gop.rotc = w.rotc;
  if (int rc = letkf::obsope_run(c->stream, &gop, files, f, 0, n, w.set, w.idx, w.qc, w.val, 1, w.flag, &msg, true, sw.off + n))
    return fail(rc, msg);
  HIP_TRY(letkf::obsmake_scatter(c->stream, R, sw.counts, sw.off, w, files->dat, counts));
  return LETKF_OK;
} LETKF_ENTRY_END(letkf_obsmake_slot_dev)

int letkf_obsmake_noise_dev(letkf_ctx* c, const letkf_obsmake_err* e, const letkf_obs_file_rows* files, letkf_rand* r) try {
  if (int rc = check_ctx(c)) return rc;
  if (!e || !files || !r) return fail(LETKF_E_INVALID, "err / files / r is NULL");
  if (files->nfile < 1 || files->nfile > LETKF_OBSOPE_MAX_FILES || !files->off) return fail(LETKF_E_INVALID, "nfile must be 1..16 and off given");
  if (files->off[0] != 0) return fail(LETKF_E_INVALID, "files->off[0] must be 0");
  for (int i = 0; i < files->nfile; ++i)
    if (files->off[i + 1] < files->off[i]) return fail(LETKF_E_INVALID, "file offsets must ascend");
  const int64_t n = files->off[files->nfile];
  if (n > 0 && (!files->elm || !files->dat || !files->err)) return fail(LETKF_E_INVALID, "files->elm / dat / err is NULL");
  if (n == 0) return LETKF_OK;
  if (int rc = grow(c, &c->scratch, (size_t)(n + 1) * sizeof(double))) return rc;
  double* error = reinterpret_cast<double*>(c->scratch.p);
  if (int rc = randn(c, r, n, error)) return rc;
  HIP_TRY(letkf::obsmake_noise(c->stream, e, n, files->elm, error, files->dat, files->err));
  return LETKF_OK;
} LETKF_ENTRY_END(letkf_obsmake_noise_dev)

}  // extern "C"
