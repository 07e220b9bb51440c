// letkf_h08_entry.hip -- C ABI of the thirteenth companion header include/letkf_amd_h08.h: the records of the Himawari-8
// observation file, the selection of the profiles a call serves, the profile arrays the host's radiative transfer takes and the
// obsda rows from what it returns.  Host side only, in the library of the Himawari-8 radiances (libletkf_amd_h08.so): the kernels
// are letkf_h08.hip's; the context, its stream, its scratch buffer, the scan plumbing and the error text are the main library's.

#include "letkf_api_internal.h"
#include "letkf_h08_dev.h"

#include <climits>

using namespace letkf::api;
namespace h8 = letkf::h08;

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

bool aligned4(const void* p) { return reinterpret_cast<uintptr_t>(p) % 4 == 0; }

int check_count(int64_t n, const char* name) {
  if (n < 0) return fail(LETKF_E_INVALID, std::string(name) + " must be >= 0");
  if (n > INT_MAX) return fail(LETKF_E_INVALID, std::string(name) + " must be < 2^31");
  return LETKF_OK;
}

int check_set(int32_t h08_set) {
  if (h08_set < 1 || h08_set > LETKF_OBSOPE_MAX_FILES) return fail(LETKF_E_INVALID, "h08_set must be in 1 .. 16");
  return LETKF_OK;
}

bool positive(double x) { return std::isfinite(x) && x > 0.0; }

// p + n, NULL staying NULL
template <class T>
T* at(T* p, int64_t n) { return p ? p + n : nullptr; }

// bytes from the base to the last element of an array of the given sizes and element strides; 0 where a stride is negative
// (the base is then not the lowest address: such an array is not checked)
size_t extent(std::initializer_list<std::pair<int64_t, int64_t>> dims) {
  size_t last = 0;
  for (const auto& [n, s] : dims) {
    if (s < 0) return 0;
    last += (size_t)(n - 1) * (size_t)s;
  }
  return (last + 1) * 8;
}

constexpr int64_t kRecBytes = 4 * h8::kRecWords;

}  // namespace

extern "C" {

int letkf_h08_count(int64_t nbytes, int64_t* nprof) try {
  if (!nprof) return fail(LETKF_E_INVALID, "nprof is NULL");
  if (nbytes < 0 || nbytes % kRecBytes) return fail(LETKF_E_INVALID, "nbytes is not a whole number of 64-byte records");   // (:3019)
  *nprof = nbytes / kRecBytes;
  return LETKF_OK;
} LETKF_ENTRY_END(letkf_h08_count)

int letkf_h08_bytes(int64_t nprof, int64_t* nbytes) try {
  if (!nbytes) return fail(LETKF_E_INVALID, "nbytes is NULL");
  if (nprof < 0 || nprof > INT64_MAX / kRecBytes) return fail(LETKF_E_INVALID, "nprof must be >= 0 and <= 2^57");
  *nbytes = nprof * kRecBytes;
  return LETKF_OK;
} LETKF_ENTRY_END(letkf_h08_bytes)

int letkf_h08_decode_dev(letkf_ctx* c, int32_t big_endian, const uint32_t* image, int64_t nprof, const double* obserr,
                         const letkf_obsfile_cols* o, int64_t* nbad) try {
  if (int rc = check_ctx(c)) return rc;
  if (!o) return fail(LETKF_E_INVALID, "cols is NULL");
  if (!obserr) return fail(LETKF_E_INVALID, "obserr is NULL");
  if (int rc = check_count(nprof, "nprof")) return rc;
  if (nprof * h8::kNch > INT_MAX) return fail(LETKF_E_INVALID, "nprof * nch must be < 2^31");
  if (!image && nprof > 0) return fail(LETKF_E_INVALID, "image is NULL");
  if (!aligned4(image)) return fail(LETKF_E_INVALID, "image must be 4-byte aligned");
  const size_t n = (size_t)nprof * h8::kNch, b4 = n * 4, b8 = n * 8;
  const Range in[1] = {{"image", image, (size_t)nprof * kRecBytes}};
  const Range out[8] = {{"elm", o->elm, b4}, {"typ", o->typ, b4}, {"lon", o->lon, b8}, {"lat", o->lat, b8},
                        {"lev", o->lev, b8}, {"dat", o->dat, b8}, {"err", o->err, b8}, {"dif", o->dif, b8}};
  if (int rc = check_ranges(in, 1, out, 8)) return rc;
  if (nprof == 0) {
    if (nbad) *nbad = 0;
    return LETKF_OK;
  }
  double e[h8::kNch];
  for (int k = 0; k < h8::kNch; ++k) e[k] = obserr[k];
  int32_t* cnt = nullptr;
  int64_t* total = nullptr;
  const int64_t nblock = h8::blocks_of(nprof);
  if (nbad) {
    if (int rc = grow(c, &c->scratch, align256((size_t)nblock * 4) + 256)) return rc;
    cnt = reinterpret_cast<int32_t*>(c->scratch.p);
    total = reinterpret_cast<int64_t*>(c->scratch.p + align256((size_t)nblock * 4));
  }
  HIP_TRY(h8::launch_decode(big_endian != 0, image, nprof, e, *o, cnt, c->stream));
  if (nbad) {
    HIP_TRY(h8::launch_count_total(cnt, nblock, total, c->stream));
    HIP_TRY(hipMemcpyAsync(nbad, total, 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
  }
  return LETKF_OK;
} LETKF_ENTRY_END(letkf_h08_decode_dev)

int letkf_h08_encode_dev(letkf_ctx* c, int32_t big_endian, int64_t nprof, const letkf_obsfile_cols* in, uint32_t* image) try {
  if (int rc = check_ctx(c)) return rc;
  if (!in) return fail(LETKF_E_INVALID, "cols is NULL");
  if (int rc = check_count(nprof, "nprof")) return rc;
  if (nprof * h8::kNch > INT_MAX) return fail(LETKF_E_INVALID, "nprof * nch must be < 2^31");
  if (!image && nprof > 0) return fail(LETKF_E_INVALID, "image is NULL");
  if (!aligned4(image)) return fail(LETKF_E_INVALID, "image must be 4-byte aligned");
  if (nprof > 0 && (!in->elm || !in->typ || !in->lon || !in->lat || !in->dat))
    return fail(LETKF_E_INVALID, "elm, typ, lon, lat and dat of cols must not be NULL");
  const size_t n = (size_t)nprof * h8::kNch, b4 = n * 4, b8 = n * 8;
  const Range ins[5] = {{"elm", in->elm, b4}, {"typ", in->typ, b4}, {"lon", in->lon, b8}, {"lat", in->lat, b8}, {"dat", in->dat, b8}};
  const Range out[1] = {{"image", image, (size_t)nprof * kRecBytes}};
  if (int rc = check_ranges(ins, 5, out, 1)) return rc;
  if (nprof > 0) HIP_TRY(h8::launch_encode(big_endian != 0, nprof, *in, image, c->stream));
  return LETKF_OK;
} LETKF_ENTRY_END(letkf_h08_encode_dev)

int letkf_h08_select_dev(letkf_ctx* c, const int32_t* set, const int32_t* idx, int64_t row0, int64_t nrows, int32_t h08_set,
                         int64_t nprof_file, int32_t* prof_list, int32_t* slot_of_prof, int64_t* nsel) try {
  if (int rc = check_ctx(c)) return rc;
  if (!nsel) return fail(LETKF_E_INVALID, "nsel is NULL");
  if (row0 < 0) return fail(LETKF_E_INVALID, "row0 must be >= 0");
  if (int rc = check_count(nrows, "nrows")) return rc;
  if (int rc = check_count(nprof_file, "nprof_file")) return rc;
  if (nprof_file * h8::kNch > INT_MAX) return fail(LETKF_E_INVALID, "nprof_file * nch must be < 2^31");
  if (int rc = check_set(h08_set)) return rc;
  if (nrows > 0 && (!set || !idx)) return fail(LETKF_E_INVALID, "set / idx is NULL");
  if (nprof_file > 0 && (!prof_list || !slot_of_prof)) return fail(LETKF_E_INVALID, "prof_list / slot_of_prof is NULL");
  const Range in[2] = {{"set", set ? set + row0 : nullptr, (size_t)nrows * 4}, {"idx", idx ? idx + row0 : nullptr, (size_t)nrows * 4}};
  const Range out[2] = {{"prof_list", prof_list, (size_t)nprof_file * 4}, {"slot_of_prof", slot_of_prof, (size_t)nprof_file * 4}};
  if (int rc = check_ranges(in, 2, out, 2)) return rc;
  *nsel = 0;
  if (nprof_file == 0) return LETKF_OK;
  // the stable compaction: a flag per profile, the scan, then every selected profile at its offset
  ScanWs sw;
  if (int rc = scan_ws(c, &c->scratch, (size_t)nprof_file, 0, &sw)) return rc;
  HIP_TRY(hipMemsetAsync(sw.counts, 0, ((size_t)nprof_file + 1) * 4, c->stream));
  if (nrows > 0) HIP_TRY(h8::launch_select_mark(set, idx, row0, nrows, h08_set, nprof_file, sw.counts, c->stream));
  HIP_TRY(scan_offsets(c, sw));
  HIP_TRY(h8::launch_select_fill(nprof_file, sw.counts, sw.off, prof_list, slot_of_prof, c->stream));
  HIP_TRY(hipMemcpyAsync(nsel, sw.off + nprof_file, 8, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return LETKF_OK;
} LETKF_ENTRY_END(letkf_h08_select_dev)

int letkf_h08_profiles_dev(letkf_ctx* c, const letkf_h08_params* p, const letkf_obsope_fields* f, int64_t nsel, const int32_t* prof_list,
                           const double* ri, const double* rj, const double* lon, const double* lat, const double* rotc,
                           const letkf_h08_profiles* out) try {
  if (int rc = check_ctx(c)) return rc;
  if (!p || !f || !out) return fail(LETKF_E_INVALID, "params / fields / out is NULL");
  if (int rc = check_count(nsel, "nsel")) return rc;
  if (int rc = check_count(p->nprof_file, "params->nprof_file")) return rc;
  if (!f->v3d || !f->v2d) return fail(LETKF_E_INVALID, "fields->v3d / v2d is NULL");
  if (f->nmem < 1) return fail(LETKF_E_INVALID, "nmem < 1");
  if (f->nlev < 2) return fail(LETKF_E_INVALID, "nlev < 2");
  if (p->nlev != f->nlev) return fail(LETKF_E_INVALID, "params->nlev differs from fields->nlev");
  if (f->nlon < 1 || f->nlat < 1 || f->khalo < 0 || f->ihalo < 0 || f->jhalo < 0)
    return fail(LETKF_E_INVALID, "nlon / nlat < 1 or a negative halo");
  if (f->nv3dd < 13 || f->nv2dd < 9) return fail(LETKF_E_INVALID, "nv3dd < 13 or nv2dd < 9");
  if (!f->s3k || !f->s3i || !f->s3j || !f->s3v || !f->s3m || !f->s2i || !f->s2j || !f->s2v || !f->s2m)
    return fail(LETKF_E_INVALID, "a zero stride");
  if (!positive(p->rd) || !positive(p->rv) || !positive(p->q_ppmv) || !positive(p->qmin))
    return fail(LETKF_E_INVALID, "rd / rv / q_ppmv / qmin must be finite and positive");
  if (nsel > 0 && (!out->lev3 || !out->sfc || !out->pflag)) return fail(LETKF_E_INVALID, "out->lev3 / sfc / pflag is NULL");
  if (nsel > 0 && p->rttov_units && !out->cloud) return fail(LETKF_E_INVALID, "out->cloud is NULL with rttov_units");
  if (nsel > 0 && (!prof_list || !ri || !rj || !lon || !lat)) return fail(LETKF_E_INVALID, "prof_list / ri / rj / lon / lat is NULL");
  const int64_t tasks = nsel * (int64_t)f->nmem;
  if (tasks > INT_MAX) return fail(LETKF_E_INVALID, "nsel * nmem must be < 2^31");
  const size_t t = (size_t)tasks, nlev = (size_t)f->nlev;
  const size_t np8 = (size_t)p->nprof_file * 8;
  const int64_t nlevh = f->nlev + 2 * (int64_t)f->khalo, nlonh = f->nlon + 2 * (int64_t)f->ihalo, nlath = f->nlat + 2 * (int64_t)f->jhalo;
  const Range in[8] = {{"prof_list", prof_list, (size_t)nsel * 4}, {"ri", ri, np8}, {"rj", rj, np8}, {"lon", lon, np8}, {"lat", lat, np8},
                       {"rotc", rotc, 2 * np8},
                       {"fields->v3d", f->v3d, extent({{nlevh, f->s3k}, {nlonh, f->s3i}, {nlath, f->s3j}, {f->nv3dd, f->s3v}, {f->nmem, f->s3m}})},
                       {"fields->v2d", f->v2d, extent({{nlonh, f->s2i}, {nlath, f->s2j}, {f->nv2dd, f->s2v}, {f->nmem, f->s2m}})}};
  const Range outs[4] = {{"lev3", out->lev3, t * 5 * nlev * 8}, {"sfc", out->sfc, t * 8 * 8},
                         {"cloud", p->rttov_units ? out->cloud : nullptr, t * 3 * (nlev - 1) * 8}, {"pflag", out->pflag, (size_t)nsel * 4}};
  if (int rc = check_ranges(in, 8, outs, 4)) return rc;
  if (nsel == 0) return LETKF_OK;
  h8::ProfileArgs a = {};
  a.v3d = f->v3d, a.v2d = f->v2d;
  a.s3k = f->s3k, a.s3i = f->s3i, a.s3j = f->s3j, a.s3v = f->s3v, a.s3m = f->s3m;
  a.s2i = f->s2i, a.s2j = f->s2j, a.s2v = f->s2v, a.s2m = f->s2m;
  a.nlev = f->nlev, a.nlonh = f->nlon + 2 * f->ihalo, a.nlath = f->nlat + 2 * f->jhalo, a.khalo = f->khalo, a.nmem = f->nmem;
  a.nsel = (int32_t)nsel, a.nprof_file = p->nprof_file;
  a.top_down = p->top_down != 0, a.stggrd = p->stggrd, a.rttov_units = p->rttov_units != 0;
  a.ri_off = p->ri_off, a.rj_off = p->rj_off, a.rd = p->rd;
  const double epsb = p->rd / p->rv;                                // (scale_H08_fwd.F90:257-258)
  a.repsb = 1.0 / epsb;
  a.q_ppmv = p->q_ppmv, a.qmin = p->qmin, a.minq = p->minq, a.cfrac_cnst = p->cfrac_cnst;
  a.sub_lon = p->sub_lon, a.r_pol = p->r_pol, a.r_sat = p->r_sat, a.ell_tan = p->ell_tan, a.ell_ecc = p->ell_ecc;
  a.prof_list = prof_list, a.ri = ri, a.rj = rj, a.lon = lon, a.lat = lat, a.rotc = rotc;
  a.lev3 = out->lev3, a.sfc = out->sfc, a.cloud = out->cloud, a.pflag = out->pflag;
  HIP_TRY(h8::launch_profiles(a, c->stream));
  return LETKF_OK;
} LETKF_ENTRY_END(letkf_h08_profiles_dev)

int letkf_h08_rows_dev(letkf_ctx* c, const letkf_h08_params* p, int64_t row0, int64_t nrows, const int32_t* set, const int32_t* idx,
                       int32_t h08_set, const int32_t* slot_of_prof, int64_t nsel, int32_t nmem, int32_t m0, const double* lev3,
                       const double* sfc, const int32_t* pflag, const double* btall, const double* btclr, const double* trans,
                       const double* rig, const double* rjg, int32_t qc_replace, int32_t* qc, double* ensval, int64_t kld, double* lev,
                       double* val2) try {
  if (int rc = check_ctx(c)) return rc;
  if (!p) return fail(LETKF_E_INVALID, "params is NULL");
  if (row0 < 0) return fail(LETKF_E_INVALID, "row0 must be >= 0");
  if (int rc = check_count(nrows, "nrows")) return rc;
  if (int rc = check_count(nsel, "nsel")) return rc;
  if (int rc = check_count(p->nprof_file, "params->nprof_file")) return rc;
  if (int rc = check_set(h08_set)) return rc;
  if (nmem < 1) return fail(LETKF_E_INVALID, "nmem < 1");
  if (m0 < 0 || (int64_t)m0 + nmem > kld) return fail(LETKF_E_INVALID, "m0 < 0 or m0 + nmem > kld");
  if (p->nlev < 2) return fail(LETKF_E_INVALID, "nlev < 2");
  if (p->finish && p->member < 1) return fail(LETKF_E_INVALID, "member must be >= 1 with finish");
  if (!set || !idx || !slot_of_prof || !qc) return fail(LETKF_E_INVALID, "set / idx / slot_of_prof / qc is NULL");
  if (p->use_obs23) {                                               // (without report type 23 only qc is written: the rest is not read)
    if (!lev3 || !sfc || !pflag || !btall || !btclr || !trans || !rig || !rjg)
      return fail(LETKF_E_INVALID, "lev3 / sfc / pflag / btall / btclr / trans / rig / rjg is NULL");
    if (!ensval || !lev || !val2) return fail(LETKF_E_INVALID, "ensval / lev / val2 is NULL");
  }
  const size_t t = (size_t)nsel * (size_t)nmem, nlev = (size_t)p->nlev, nr = (size_t)nrows, nch = h8::kNch;
  const size_t np8 = (size_t)p->nprof_file * 8;
  const Range in[11] = {{"rig", rig, np8}, {"rjg", rjg, np8}, {"set", set + row0, nr * 4}, {"idx", idx + row0, nr * 4}, {"slot_of_prof", slot_of_prof, (size_t)p->nprof_file * 4},
                        {"lev3", lev3, t * 5 * nlev * 8}, {"sfc", sfc, t * 8 * 8}, {"pflag", pflag, (size_t)nsel * 4},
                        {"btall", btall, t * nch * 8}, {"btclr", btclr, t * nch * 8}, {"trans", trans, t * nch * nlev * 8}};
  const Range out[4] = {{"qc", qc + row0, nr * 4}, {"ensval", at(ensval, row0 * kld), nr * (size_t)kld * 8}, {"lev", at(lev, row0), nr * 8},
                        {"val2", at(val2, row0), nr * 8}};
  if (int rc = check_ranges(in, 11, out, 4)) return rc;
  if (nrows == 0 || nsel == 0) return LETKF_OK;
  h8::RowArgs a = {};
  a.row0 = row0, a.nrows = nrows, a.nsel = nsel, a.kld = kld, a.nprof_file = p->nprof_file;
  a.set = set, a.idx = idx, a.slot_of_prof = slot_of_prof, a.pflag = pflag;
  a.h08_set = h08_set, a.nmem = nmem, a.m0 = m0, a.nlev = p->nlev, a.top_down = p->top_down != 0, a.rttov_units = p->rttov_units != 0;
  a.reject_land = p->reject_land != 0, a.use_obs23 = p->use_obs23 != 0, a.finish = p->finish != 0, a.member = p->member;
  a.qc_replace = qc_replace != 0;
  for (int k = 0; k < h8::kNch; ++k)
    if (p->ch_use[k] == 1) a.ch_mask |= 1u << k;
  a.cldsky_thrs = p->cldsky_thrs, a.bris = p->bris, a.brie = p->brie, a.brjs = p->brjs, a.brje = p->brje;
  a.lev3 = lev3, a.sfc = sfc, a.btall = btall, a.btclr = btclr, a.trans = trans, a.rig = rig, a.rjg = rjg;
  a.qc = qc, a.ensval = ensval, a.lev = lev, a.val2 = val2;
  HIP_TRY(h8::launch_rows(a, c->stream));
  return LETKF_OK;
} LETKF_ENTRY_END(letkf_h08_rows_dev)

}  // extern "C"
