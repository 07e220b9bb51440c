// letkf_obsfile_entry.hip -- C ABI of the tenth companion header include/letkf_amd_obsfile.h: the record codec of the observation,
// obsda and departure files.  Host side only, in the library of the codec (libletkf_amd_obsfile.so): the kernels are
// letkf_obsfile.hip's, the context, its stream, its scratch buffer, the scan plumbing and the error text the main library's.

#include "letkf_api_internal.h"
#include "letkf_obsfile_dev.h"

#include <climits>

using namespace letkf::api;
namespace of = letkf::obsfile;

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

// dwords of a record and of the head; 0 where the format does not take that nrec
int record_words(int32_t format, int32_t nrec) {
  const bool ok = format == LETKF_OBSFILE_CONV    ? nrec == 8
                  : format == LETKF_OBSFILE_RADAR ? nrec == 7 || nrec == 8
                  : format == LETKF_OBSFILE_OBSDA ? nrec == 4 || nrec == 6
                  : format == LETKF_OBSFILE_DEP   ? nrec == 11
                                                  : false;
  return ok ? nrec + 2 : 0;
}
int head_words(int32_t format) { return format == LETKF_OBSFILE_RADAR ? of::kRadarHeadWords : 0; }

int check_format(int32_t format, int32_t nrec) {
  if (format < LETKF_OBSFILE_CONV || format > LETKF_OBSFILE_DEP) return fail(LETKF_E_INVALID, "format must be 1 (conventional), 2 (radar), 3 (obsda) or 4 (departure)");
  if (!record_words(format, nrec)) return fail(LETKF_E_INVALID, "nrec must be 8 (conventional), 7 or 8 (radar), 4 or 6 (obsda), 11 (departure)");
  return LETKF_OK;
}

int check_rows_count(int64_t n, const char* name) {
  if (n < 0) return fail(LETKF_E_INVALID, std::string(name) + " must be >= 0");
  if (n > INT_MAX) return fail(LETKF_E_INVALID, std::string(name) + " must be < 2^31");
  return LETKF_OK;
}

// a conventional or radar params
int check_obs_params(const letkf_obsfile_params* p) {
  if (!p) return fail(LETKF_E_INVALID, "params is NULL");
  if (p->format != LETKF_OBSFILE_CONV && p->format != LETKF_OBSFILE_RADAR) return fail(LETKF_E_INVALID, "format must be 1 (conventional) or 2 (radar)");
  return check_format(p->format, p->nrec);
}

// the sum of the per-block counts behind the launches, read back: the entry's synchronisation
int totals_to_host(letkf_ctx* c, const int32_t* cnt, int64_t nblock, int ncnt, int64_t* dev_total, int64_t* host_total) {
  HIP_TRY(of::count_total_run(c->stream, cnt, nblock, ncnt, dev_total));
  HIP_TRY(hipMemcpyAsync(host_total, dev_total, (size_t)ncnt * 8, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return LETKF_OK;
}

}  // namespace

extern "C" {

int letkf_obsfile_count(int32_t format, int32_t nrec, int64_t nbytes, int64_t* nrows) try {
  if (!nrows) return fail(LETKF_E_INVALID, "nrows is NULL");
  if (int rc = check_format(format, nrec)) return rc;
  if (nbytes < 0) return fail(LETKF_E_INVALID, "nbytes must be >= 0");
  const int64_t body = nbytes - 4 * head_words(format), rec = 4 * record_words(format, nrec);
  if (body < 0 || body % rec) return fail(LETKF_E_INVALID, "nbytes is not a whole number of records");   // (:2124, :2479-2481)
  *nrows = body / rec;
  return LETKF_OK;
} LETKF_ENTRY_END(letkf_obsfile_count)

int letkf_obsfile_bytes(int32_t format, int32_t nrec, int64_t nrows, int64_t* nbytes) try {
  if (!nbytes) return fail(LETKF_E_INVALID, "nbytes is NULL");
  if (int rc = check_format(format, nrec)) return rc;
  if (nrows < 0 || nrows > INT64_MAX / 64) return fail(LETKF_E_INVALID, "nrows must be >= 0 and <= 2^57");
  *nbytes = 4 * (head_words(format) + nrows * record_words(format, nrec));
  return LETKF_OK;
} LETKF_ENTRY_END(letkf_obsfile_bytes)

int letkf_obs_decode_dev(letkf_ctx* c, const letkf_obsfile_params* p, const letkf_mapproj* proj, const uint32_t* image, int64_t nrows,
                         const letkf_obsfile_cols* o, double* meta, int64_t* nbad) try {
  if (!c) return fail(LETKF_E_INVALID, "ctx is NULL");
  if (int rc = check_ctx(c)) return rc;
  if (int rc = check_obs_params(p)) return rc;
  if (!o) return fail(LETKF_E_INVALID, "o is NULL");
  if (int rc = check_rows_count(nrows, "nrows")) return rc;
  const bool radar = p->format == LETKF_OBSFILE_RADAR;
  if (p->proj_given) {
    if (!proj) return fail(LETKF_E_INVALID, "proj is NULL with proj_given");
    if (proj->type != LETKF_MAPPROJ_LC) return fail(LETKF_E_INVALID, "proj->type must be 1 (LC)");
  }
  if (!image && (nrows > 0 || (radar && meta))) return fail(LETKF_E_INVALID, "image is NULL");
  if (!aligned4(image)) return fail(LETKF_E_INVALID, "image must be 4-byte aligned");
  const int W = record_words(p->format, p->nrec), H = head_words(p->format);
  const size_t b4 = (size_t)nrows * 4, b8 = (size_t)nrows * 8;
  const Range in[1] = {{"image", image, 4 * ((size_t)H + (size_t)nrows * W)}};
  const Range out[8] = {{"elm", o->elm, b4}, {"typ", o->typ, b4}, {"lon", o->lon, b8}, {"lat", o->lat, b8},
                        {"lev", o->lev, b8}, {"dat", o->dat, b8}, {"err", o->err, b8}, {"dif", o->dif, b8}};
  if (int rc = check_ranges(in, 1, out, 8)) return rc;

  int32_t* cnt = nullptr;
  int64_t* total = nullptr;
  const int64_t nblock = of::row_blocks(nrows);
  if (nbad && nrows > 0) {
    if (int rc = grow(c, &c->scratch, align256((size_t)nblock * 4) + 256)) return rc;
    cnt = reinterpret_cast<int32_t*>(c->scratch.p);
    total = reinterpret_cast<int64_t*>(c->scratch.p + align256((size_t)nblock * 4));
  }
  if (nrows > 0) HIP_TRY(of::decode_run(c->stream, *p, proj, image + H, nrows, *o, cnt));
  uint32_t head[of::kRadarHeadWords] = {};
  const bool want_meta = radar && meta;
  if (want_meta) HIP_TRY(hipMemcpyAsync(head, image, sizeof head, hipMemcpyDeviceToHost, c->stream));
  if (cnt) {
    if (int rc = totals_to_host(c, cnt, nblock, 1, total, nbad)) return rc;
  } else {
    if (want_meta) HIP_TRY(hipStreamSynchronize(c->stream));
    if (nbad) *nbad = 0;
  }
  if (want_meta)
    for (int k = 0; k < 3; ++k) {
      const uint32_t w = p->big_endian ? __builtin_bswap32(head[3 * k + 1]) : head[3 * k + 1];
      float f;
      std::memcpy(&f, &w, 4);
      meta[k] = (double)f;
    }
  return LETKF_OK;
} LETKF_ENTRY_END(letkf_obs_decode_dev)

int letkf_obs_encode_dev(letkf_ctx* c, const letkf_obsfile_params* p, int64_t nrows, const letkf_obsfile_cols* in, const double* meta,
                         uint32_t* image, int64_t* nwritten) try {
  if (!c) return fail(LETKF_E_INVALID, "ctx is NULL");
  if (int rc = check_ctx(c)) return rc;
  if (int rc = check_obs_params(p)) return rc;
  if (!in) return fail(LETKF_E_INVALID, "in is NULL");
  if (int rc = check_rows_count(nrows, "nrows")) return rc;
  const bool radar = p->format == LETKF_OBSFILE_RADAR;
  if (radar && !meta) return fail(LETKF_E_INVALID, "meta is NULL");
  if (!p->missing && !nwritten) return fail(LETKF_E_INVALID, "nwritten is NULL without missing");
  if (!image && (nrows > 0 || radar)) return fail(LETKF_E_INVALID, "image is NULL");
  if (!aligned4(image)) return fail(LETKF_E_INVALID, "image must be 4-byte aligned");
  if (nrows > 0) {
    if (!in->elm || !in->typ || !in->lon || !in->lat || !in->lev || !in->dat || !in->err)
      return fail(LETKF_E_INVALID, "elm, typ, lon, lat, lev, dat and err of in must not be NULL");
    if (p->nrec == 8 && !in->dif) return fail(LETKF_E_INVALID, "dif of in is NULL with nrec = 8");
  }
  const int W = record_words(p->format, p->nrec), H = head_words(p->format);
  const size_t b4 = (size_t)nrows * 4, b8 = (size_t)nrows * 8;
  const Range ins[8] = {{"elm", in->elm, b4}, {"typ", in->typ, b4}, {"lon", in->lon, b8}, {"lat", in->lat, b8},
                        {"lev", in->lev, b8}, {"dat", in->dat, b8}, {"err", in->err, b8}, {"dif", p->nrec == 8 ? in->dif : nullptr, b8}};
  const Range out[1] = {{"image", image, 4 * ((size_t)H + (size_t)nrows * W)}};
  if (int rc = check_ranges(ins, 8, out, 1)) return rc;

  if (radar) {
    uint32_t bits[3];
    for (int k = 0; k < 3; ++k) {
      const float f = (float)meta[k];                                      // (:2573-2575)
      std::memcpy(&bits[k], &f, 4);
    }
    HIP_TRY(of::radar_head_run(c->stream, image, bits[0], bits[1], bits[2], p->big_endian));
  }
  if (p->missing || nrows == 0) {
    if (nrows > 0) HIP_TRY(of::encode_run(c->stream, *p, nrows, *in, nullptr, image + H));
    if (nwritten) *nwritten = nrows;
    return LETKF_OK;
  }
  // the stable compaction: survivors per block, the scan, then the records at block offset + rank in the block
  ScanWs sw;
  const int64_t nblock = of::row_blocks(nrows);
  if (int rc = scan_ws(c, &c->scratch, (size_t)nblock, 0, &sw)) return rc;
  HIP_TRY(zero_total(c, sw));
  HIP_TRY(of::encode_count_run(c->stream, nrows, in->dat, sw.counts));
  HIP_TRY(scan_offsets(c, sw));
  HIP_TRY(of::encode_run(c->stream, *p, nrows, *in, sw.off, image + H));
  HIP_TRY(hipMemcpyAsync(nwritten, sw.off + nblock, 8, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return LETKF_OK;
} LETKF_ENTRY_END(letkf_obs_encode_dev)

int letkf_obsda_assemble_dev(letkf_ctx* c, const letkf_obsda_params* p, const uint32_t* const* images, const int32_t* col,
                             const int32_t* is_member, const letkf_obsda_cols* o, int64_t* ninconsistent, int64_t* nbad) try {
  if (!c) return fail(LETKF_E_INVALID, "ctx is NULL");
  if (int rc = check_ctx(c)) return rc;
  if (!p) return fail(LETKF_E_INVALID, "params is NULL");
  if (int rc = check_format(LETKF_OBSFILE_OBSDA, p->nrec)) return rc;
  if (p->nmem < 1 || p->nmem > LETKF_OBSFILE_MAX_MEMBERS) return fail(LETKF_E_INVALID, "nmem must be in 1 .. 65536");
  if (int rc = check_rows_count(p->nobs, "nobs")) return rc;
  if (p->kld < 1 || p->kld >= (1 << 20)) return fail(LETKF_E_INVALID, "kld must be in 1 .. 2^20 - 1");
  if (p->nrec == 6 && p->finish && p->member < 1) return fail(LETKF_E_INVALID, "member must be >= 1 with finish");
  if (!images || !col || !o) return fail(LETKF_E_INVALID, "images / col / o is NULL");
  const int nmem = p->nmem;
  const int64_t nobs = p->nobs;
  std::vector<char> seen((size_t)p->kld, 0);
  for (int m = 0; m < nmem; ++m) {
    if (col[m] < 0 || col[m] >= p->kld) return fail(LETKF_E_INVALID, "col[" + std::to_string(m) + "] must be in 0 .. kld - 1");
    if (seen[(size_t)col[m]]++) return fail(LETKF_E_INVALID, "col[" + std::to_string(m) + "] repeats a column");
  }
  const int W = p->nrec + 2;
  const size_t img_bytes = (size_t)nobs * W * 4;
  for (int m = 0; m < nmem; ++m) {
    if (!images[m] && nobs > 0) return fail(LETKF_E_INVALID, "images[" + std::to_string(m) + "] is NULL");
    if (!aligned4(images[m])) return fail(LETKF_E_INVALID, "images[" + std::to_string(m) + "] must be 4-byte aligned");
  }
  if (nobs > 0 && (!o->set || !o->idx || !o->qc || !o->ensval)) return fail(LETKF_E_INVALID, "set, idx, qc and ensval of o must not be NULL");
  const bool h08 = p->nrec == 6;
  const Range out[6] = {{"set", o->set, (size_t)nobs * 4},          {"idx", o->idx, (size_t)nobs * 4},
                        {"qc", o->qc, (size_t)nobs * 4},            {"ensval", o->ensval, (size_t)nobs * (size_t)p->kld * 8},
                        {"lev", h08 ? o->lev : nullptr, (size_t)nobs * 8}, {"val2", h08 ? o->val2 : nullptr, (size_t)nobs * 8}};
  if (int rc = check_ranges(nullptr, 0, out, 6)) return rc;
  for (int m = 0; m < nmem; ++m) {
    const Range in = {"images", images[m], img_bytes};
    for (const Range& r : out)
      if (overlap(r, in)) return fail(LETKF_E_INVALID, std::string(r.name) + " overlaps images[" + std::to_string(m) + "]");
  }
  if (nobs == 0) {
    if (ninconsistent) *ninconsistent = 0;
    if (nbad) *nbad = 0;
    return LETKF_OK;
  }

  // scratch: the image table | per-tile counts [tiles][2] | totals [2]
  const bool counting = ninconsistent || nbad;
  const int64_t ntile = of::row_tiles(nobs);
  const size_t o_cnt = align256((size_t)nmem * sizeof(of::ImageRef)), o_tot = o_cnt + (counting ? align256((size_t)ntile * 8) : 0);
  if (int rc = grow(c, &c->scratch, o_tot + 256)) return rc;
  std::vector<of::ImageRef> tab((size_t)nmem);
  for (int m = 0; m < nmem; ++m) tab[(size_t)m] = {images[m], col[m], is_member ? (is_member[m] != 0) : 1};
  HIP_TRY(hipMemcpyAsync(c->scratch.p, tab.data(), (size_t)nmem * sizeof(of::ImageRef), hipMemcpyHostToDevice, c->stream));
  int32_t* cnt = counting ? reinterpret_cast<int32_t*>(c->scratch.p + o_cnt) : nullptr;
  letkf_obsda_cols oc = *o;
  if (!h08) oc.lev = oc.val2 = nullptr;
  HIP_TRY(of::assemble_run(c->stream, *p, reinterpret_cast<const of::ImageRef*>(c->scratch.p), oc, cnt));
  if (counting) {
    int64_t tot[2] = {0, 0};
    if (int rc = totals_to_host(c, cnt, ntile, 2, reinterpret_cast<int64_t*>(c->scratch.p + o_tot), tot)) return rc;
    if (nbad) *nbad = tot[0];
    if (ninconsistent) *ninconsistent = tot[1];
  } else {
    HIP_TRY(hipStreamSynchronize(c->stream));   // (the table left pageable host memory: it must not be freed under the copy)
  }
  return LETKF_OK;
} LETKF_ENTRY_END(letkf_obsda_assemble_dev)

int letkf_obsda_encode_dev(letkf_ctx* c, int32_t nrec, int32_t big_endian, int64_t nobs, const int32_t* set, const int32_t* idx,
                           const int32_t* qc, const double* ensval, int64_t kld, int32_t col, const double* val, const double* lev,
                           const double* val2, uint32_t* image) try {
  if (!c) return fail(LETKF_E_INVALID, "ctx is NULL");
  if (int rc = check_ctx(c)) return rc;
  if (int rc = check_format(LETKF_OBSFILE_OBSDA, nrec)) return rc;
  if (int rc = check_rows_count(nobs, "nobs")) return rc;
  if (col >= 0 && (kld < 1 || kld >= (1 << 20))) return fail(LETKF_E_INVALID, "kld must be in 1 .. 2^20 - 1");
  if (col >= 0 && col >= kld) return fail(LETKF_E_INVALID, "col must be < kld (or negative: val)");
  if (!aligned4(image)) return fail(LETKF_E_INVALID, "image must be 4-byte aligned");
  if (nobs == 0) return LETKF_OK;
  if (!set || !idx || !qc || !image) return fail(LETKF_E_INVALID, "set / idx / qc / image is NULL");
  if (col >= 0 ? !ensval : !val) return fail(LETKF_E_INVALID, col >= 0 ? "ensval is NULL" : "val is NULL with col < 0");
  if (nrec == 6 && (!lev || !val2)) return fail(LETKF_E_INVALID, "lev / val2 is NULL with nrec = 6");
  const size_t b4 = (size_t)nobs * 4, b8 = (size_t)nobs * 8;
  const Range in[7] = {{"set", set, b4}, {"idx", idx, b4}, {"qc", qc, b4}, {"ensval", col >= 0 ? ensval : nullptr, b8 * (size_t)kld},
                       {"val", col < 0 ? val : nullptr, b8}, {"lev", nrec == 6 ? lev : nullptr, b8}, {"val2", nrec == 6 ? val2 : nullptr, b8}};
  const Range out[1] = {{"image", image, (size_t)nobs * (nrec + 2) * 4}};
  if (int rc = check_ranges(in, 7, out, 1)) return rc;
  HIP_TRY(of::obsda_encode_run(c->stream, nrec, big_endian, nobs, set, idx, qc, col >= 0 ? ensval + col : val, col >= 0 ? kld : 1, lev, val2, image));
  return LETKF_OK;
} LETKF_ENTRY_END(letkf_obsda_encode_dev)

int letkf_obsdep_encode_dev(letkf_ctx* c, int32_t big_endian, int64_t nobs, const int32_t* set, const int32_t* idx, const int32_t* qc,
                            const double* omb, const double* oma, const letkf_obsfile_rows* f, uint32_t* image) try {
  if (!c) return fail(LETKF_E_INVALID, "ctx is NULL");
  if (int rc = check_ctx(c)) return rc;
  if (int rc = check_rows_count(nobs, "nobs")) return rc;
  if (!f) return fail(LETKF_E_INVALID, "files is NULL");
  if (f->nfile < 0) return fail(LETKF_E_INVALID, "files->nfile must be >= 0");
  if (!f->off) return fail(LETKF_E_INVALID, "files->off is NULL");
  for (int k = 0; k < f->nfile; ++k)
    if (f->off[k + 1] < f->off[k] || f->off[k] < 0) return fail(LETKF_E_INVALID, "files->off must start at >= 0 and not decrease");
  if (!aligned4(image)) return fail(LETKF_E_INVALID, "image must be 4-byte aligned");
  if (nobs == 0) return LETKF_OK;
  if (!set || !idx || !qc || !omb || !oma || !image) return fail(LETKF_E_INVALID, "set / idx / qc / omb / oma / image is NULL");
  const int64_t nrow = f->off[f->nfile];
  if (nrow > 0 && (!f->elm || !f->typ || !f->lon || !f->lat || !f->lev || !f->dat || !f->err || !f->dif))
    return fail(LETKF_E_INVALID, "a column of files is NULL");
  const size_t b4 = (size_t)nobs * 4, b8 = (size_t)nobs * 8, f4 = (size_t)nrow * 4, f8 = (size_t)nrow * 8;
  const Range in[13] = {{"set", set, b4},      {"idx", idx, b4},      {"qc", qc, b4},        {"omb", omb, b8},      {"oma", oma, b8},
                        {"files->elm", f->elm, f4}, {"files->typ", f->typ, f4}, {"files->lon", f->lon, f8}, {"files->lat", f->lat, f8},
                        {"files->lev", f->lev, f8}, {"files->dat", f->dat, f8}, {"files->err", f->err, f8}, {"files->dif", f->dif, f8}};
  const Range out[1] = {{"image", image, (size_t)nobs * 13 * 4}};
  if (int rc = check_ranges(in, 13, out, 1)) return rc;

  // scratch: off [nfile + 1] | per-block counts | total
  const int64_t nblock = of::row_blocks(nobs);
  const size_t o_cnt = align256(((size_t)f->nfile + 1) * 8), o_tot = o_cnt + align256((size_t)nblock * 4);
  if (int rc = grow(c, &c->scratch, o_tot + 256)) return rc;
  int64_t* off = reinterpret_cast<int64_t*>(c->scratch.p);
  int32_t* cnt = reinterpret_cast<int32_t*>(c->scratch.p + o_cnt);
  HIP_TRY(hipMemcpyAsync(off, f->off, ((size_t)f->nfile + 1) * 8, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(of::obsdep_check_run(c->stream, nobs, set, idx, f->nfile, off, cnt));
  int64_t outside = 0;
  if (int rc = totals_to_host(c, cnt, nblock, 1, reinterpret_cast<int64_t*>(c->scratch.p + o_tot), &outside)) return rc;
  if (outside) return fail(LETKF_E_INVALID, std::to_string(outside) + " rows have a set / idx outside the files");
  HIP_TRY(of::obsdep_encode_run(c->stream, big_endian, nobs, set, idx, qc, omb, oma, *f, off, image));
  return LETKF_OK;
} LETKF_ENTRY_END(letkf_obsdep_encode_dev)

}  // extern "C"
