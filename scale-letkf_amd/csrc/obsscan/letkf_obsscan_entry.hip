// letkf_obsscan_entry.hip -- C ABI of the eighth companion header include/letkf_amd_obsscan.h: obsope_cal's first scan on the
// device and the operator on one (subdomain, slot) of its lists.  Host side only, in the library of the scan
// (libletkf_amd_obsscan.so): the kernels are letkf_obsscan.hip's; the context, its stream and scratch buffer, the error text and
// the operator (letkf_obsope_dev.h, reached as the library of the OSSE tools reaches it) are the main library's.

#include "letkf_api_internal.h"
#include "letkf_obsscan_dev.h"

#include <climits>

using namespace letkf::api;

namespace {

struct Range {
  const char* p;
  size_t bytes;
};

bool overlap(const Range& a, const Range& b) {
  return a.p && b.p && a.bytes && b.bytes && a.p < b.p + b.bytes && b.p < a.p + a.bytes;
}

// the slots and the subdomains of a scan, as all four entries check them
int check_slots(int32_t slot_start, int32_t slot_end) {
  if (slot_start < 1) return fail(LETKF_E_INVALID, "slot_start must be >= 1");
  if (slot_end < slot_start) return fail(LETKF_E_INVALID, "slot_end must be >= slot_start");
  if (slot_end > INT_MAX - 3) return fail(LETKF_E_INVALID, "slot_end must be <= 2^31 - 4");
  return LETKF_OK;
}

int check_buckets(int64_t nprocs_d, int32_t slot_start, int32_t slot_end) {
  if (nprocs_d < 1) return fail(LETKF_E_INVALID, "nprocs_d must be >= 1");
  const int64_t nb = (int64_t)slot_end - slot_start + 3;
  if (nprocs_d > LETKF_OBSSCAN_MAX_BUCKETS / nb) return fail(LETKF_E_INVALID, "nprocs_d * (nslots + 2) must be <= 4194304 buckets");
  return LETKF_OK;
}

// letkf_obsscan_rows without the checks
void rows_of(const int32_t* bsna, int32_t slot_start, int32_t slot_end, int32_t ip, int32_t islot, int64_t* first, int64_t* count) {
  const int64_t ld = (int64_t)slot_end - slot_start + 4;
  const int32_t* row = bsna + ip * ld;
  const int64_t lo = islot == 0 ? 0 : islot - slot_start, hi = islot == 0 ? ld - 1 : lo + 1;
  *first = row[lo];
  *count = (int64_t)row[hi] - row[lo];
}

}  // namespace

extern "C" {

int letkf_obsscan_dev(letkf_ctx* c, const letkf_obsscan_params* p, const letkf_obs_file_rows* files, const letkf_obsscan_out* o) try {
  if (int rc = check_ctx(c)) return rc;
  if (!p || !files || !o) return fail(LETKF_E_INVALID, "params / files / out is NULL");
  if (files->nfile < 1 || files->nfile > LETKF_OBSOPE_MAX_FILES) return fail(LETKF_E_INVALID, "nfile must be 1 .. 16");
  if (!files->off) return fail(LETKF_E_INVALID, "files->off is NULL");
  if (!o->bsn || !o->bsna) return fail(LETKF_E_INVALID, "bsn / bsna is NULL");
  if (p->nlon < 1 || p->nlat < 1) return fail(LETKF_E_INVALID, "nlon and nlat must be >= 1");
  if (p->prc_num_x < 1 || p->prc_num_y < 1) return fail(LETKF_E_INVALID, "prc_num_x and prc_num_y must be >= 1");
  if (p->ihalo < 0 || p->jhalo < 0) return fail(LETKF_E_INVALID, "ihalo and jhalo must be >= 0");
  if ((int64_t)p->nlon * p->prc_num_x + p->ihalo > INT_MAX || (int64_t)p->nlat * p->prc_num_y + p->jhalo > INT_MAX)
    return fail(LETKF_E_INVALID, "nlon * prc_num_x + ihalo and nlat * prc_num_y + jhalo must be < 2^31");
  if (int rc = check_slots(p->slot_start, p->slot_end)) return rc;
  if (!std::isfinite(p->slot_tinterval) || !(p->slot_tinterval > 0.0)) return fail(LETKF_E_INVALID, "slot_tinterval must be finite and > 0");
  const int64_t nprocs_d = (int64_t)p->prc_num_x * p->prc_num_y;
  if (int rc = check_buckets(nprocs_d, p->slot_start, p->slot_end)) return rc;
  if (files->off[0] != 0) return fail(LETKF_E_INVALID, "files->off must start at 0");
  int64_t nlist = 0;
  uint32_t run_mask = 0;
  for (int f = 0; f < files->nfile; ++f) {
    if (files->off[f + 1] < files->off[f]) return fail(LETKF_E_INVALID, "files->off decreases");
    if (!p->obsda_run || p->obsda_run[f]) run_mask |= 1u << f, nlist += files->off[f + 1] - files->off[f];
  }
  const int64_t n = files->off[files->nfile];
  if (n > 0x7fffffffLL) return fail(LETKF_E_INVALID, "files->off: 2^31 file rows or more");
  if (n > 0 && (!files->ri || !files->rj || !p->dif)) return fail(LETKF_E_INVALID, "ri / rj / dif is NULL");
  if (nlist > 0 && (!o->set || !o->idx || !o->qc)) return fail(LETKF_E_INVALID, "set / idx / qc is NULL");
  if (o->own && (p->myrank_d < 0 || p->myrank_d >= nprocs_d)) return fail(LETKF_E_INVALID, "myrank_d must be 0 .. nprocs_d - 1");
  {
    const Range in[3] = {{reinterpret_cast<const char*>(files->ri), (size_t)n * 8}, {reinterpret_cast<const char*>(files->rj), (size_t)n * 8},
                         {reinterpret_cast<const char*>(p->dif), (size_t)n * 8}};
    const Range out[6] = {{reinterpret_cast<const char*>(o->set), (size_t)nlist * 4}, {reinterpret_cast<const char*>(o->idx), (size_t)nlist * 4},
                          {reinterpret_cast<const char*>(o->qc), (size_t)nlist * 4}, {reinterpret_cast<const char*>(o->rank), (size_t)n * 4},
                          {reinterpret_cast<const char*>(o->slot), (size_t)n * 4}, {reinterpret_cast<const char*>(o->own), (size_t)n * 4}};
    for (const Range& x : out)
      for (const Range& y : in)
        if (overlap(x, y)) return fail(LETKF_E_INVALID, "an output overlaps an input");
  }

  letkf::ObsscanArgs a = {};
  a.n = n, a.nlist = nlist, a.ri = files->ri, a.rj = files->rj, a.dif = p->dif;
  for (int q = 0; q <= LETKF_OBSOPE_MAX_FILES; ++q) a.off[q] = q <= files->nfile ? files->off[q] : INT64_MAX;
  a.run_mask = run_mask;
  a.nlon = p->nlon, a.nlat = p->nlat, a.ihalo = p->ihalo, a.jhalo = p->jhalo, a.px = p->prc_num_x, a.py = p->prc_num_y;
  a.slot_start = p->slot_start, a.slot_end = p->slot_end, a.slot_base = p->slot_base, a.myrank_d = p->myrank_d;
  a.nb = p->slot_end - p->slot_start + 3, a.nbucket = (int32_t)(nprocs_d * a.nb), a.tint = p->slot_tinterval;
  a.set = o->set, a.idx = o->idx, a.qc = o->qc, a.rank = o->rank, a.slot = o->slot, a.own = o->own;

  std::vector<int32_t> ub((size_t)a.nbucket, 0);        // the upper bound of every bucket in the lists
  if (n > 0) {
    const size_t ws_bytes = letkf::obsscan_ws_bytes(a, c->stream);
    if (!ws_bytes) return fail(LETKF_E_HIP, "rocprim workspace query failed");
    if (int rc = grow(c, &c->scratch, ws_bytes)) return rc;
    HIP_TRY(letkf::obsscan_run(c->stream, a, c->scratch.p, ub.data()));
    if (nlist > 0) HIP_TRY(hipStreamSynchronize(c->stream));
  }
  const int nb = a.nb;
  for (int64_t ip = 0; ip < nprocs_d; ++ip) {           // :269-277
    int32_t* acc = o->bsna + ip * (nb + 1);
    acc[0] = ip > 0 ? ub[ip * nb - 1] : 0;
    for (int s = 0; s < nb; ++s) {
      acc[s + 1] = ub[ip * nb + s];
      o->bsn[ip * nb + s] = acc[s + 1] - acc[s];
    }
  }
  return LETKF_OK;
} LETKF_ENTRY_END(letkf_obsscan_dev)

int letkf_obsscan_rows(const int32_t* bsna, int32_t nprocs_d, int32_t slot_start, int32_t slot_end, int32_t ip, int32_t islot,
                       int64_t* first, int64_t* count) try {
  if (!bsna || !first || !count) return fail(LETKF_E_INVALID, "bsna / first / count is NULL");
  if (int rc = check_slots(slot_start, slot_end)) return rc;
  if (int rc = check_buckets(nprocs_d, slot_start, slot_end)) return rc;
  if (ip < 0 || ip >= nprocs_d) return fail(LETKF_E_INVALID, "ip must be 0 .. nprocs_d - 1");
  if (islot != 0 && (islot < slot_start || islot > slot_end + 2)) return fail(LETKF_E_INVALID, "islot must be 0 or slot_start .. slot_end + 2");
  rows_of(bsna, slot_start, slot_end, ip, islot, first, count);
  return LETKF_OK;
} LETKF_ENTRY_END(letkf_obsscan_rows)

int letkf_obsscan_slot_bounds(int32_t slot_start, int32_t slot_end, int32_t slot_base, double slot_tinterval, double* slot_lb,
                              double* slot_ub) try {
  if (!slot_lb || !slot_ub) return fail(LETKF_E_INVALID, "slot_lb / slot_ub is NULL");
  if (int rc = check_slots(slot_start, slot_end)) return rc;
  if (!std::isfinite(slot_tinterval) || !(slot_tinterval > 0.0)) return fail(LETKF_E_INVALID, "slot_tinterval must be finite and > 0");
  for (int64_t s = slot_start; s <= slot_end; ++s) {     // :315-319
    const double d = (double)(int32_t)(s - slot_base);
    slot_lb[s - slot_start] = (d - 0.5) * slot_tinterval;
    slot_ub[s - slot_start] = (d + 0.5) * slot_tinterval;
  }
  return LETKF_OK;
} LETKF_ENTRY_END(letkf_obsscan_slot_bounds)

int letkf_obsope_slot_dev(letkf_ctx* c, const letkf_obsscan_lists* l, int32_t ip, int32_t islot, const letkf_obsope_params* p,
                          const letkf_obs_file_rows* files, const letkf_obsope_fields* f, double* ensval, int64_t kld) try {
  if (int rc = check_ctx(c)) return rc;
  if (!l || !l->bsna) return fail(LETKF_E_INVALID, "lists / bsna is NULL");
  if (int rc = check_slots(l->slot_start, l->slot_end)) return rc;
  if (int rc = check_buckets(l->nprocs_d, l->slot_start, l->slot_end)) return rc;
  if (ip < 0 || ip >= l->nprocs_d) return fail(LETKF_E_INVALID, "ip must be 0 .. nprocs_d - 1");
  if (islot < l->slot_start || islot > l->slot_end) return fail(LETKF_E_INVALID, "islot must be slot_start .. slot_end");
  int64_t first = 0, count = 0;
  rows_of(l->bsna, l->slot_start, l->slot_end, ip, islot, &first, &count);
  if (first < 0 || count < 0) return fail(LETKF_E_INVALID, "bsna is not a running sum");
  std::string msg;
  if (int rc = letkf::obsope_check(p, files, f, first, count, l->set, l->idx, l->qc, ensval, kld, &msg)) return fail(rc, msg);
  if (count == 0) return LETKF_OK;
  if (int rc = grow(c, &c->scratch, 256)) return rc;
  if (int rc = letkf::obsope_run(c->stream, p, files, f, first, count, l->set, l->idx, l->qc, ensval, kld,
                                 reinterpret_cast<int32_t*>(c->scratch.p), &msg))
    return fail(rc, msg);
  return LETKF_OK;
} LETKF_ENTRY_END(letkf_obsope_slot_dev)

}  // extern "C"
