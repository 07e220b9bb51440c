// letkf_superob_entry.hip -- C ABI of the seventh companion header include/letkf_amd_superob.h: superob on the device.  Host side
// only, in the library of superob (libletkf_amd_superob.so): the kernels are letkf_superob.hip's; the context, its stream and
// scratch buffer and the error text are the main library's (letkf_api_internal.h).

#include "letkf_api_internal.h"
#include "letkf_superob_dev.h"

using namespace letkf::api;

namespace {

struct Range {
  const char* p;
  size_t bytes;
};

bool overlap(const Range& a, const Range& b) {
  return a.p && b.p && a.bytes && b.bytes && a.p < b.p + b.bytes && b.p < a.p + a.bytes;
}

// slot_priority (scale/obs/superob.f90:164-175), 1-based slots
void slot_priority(int nslots, int nbslot, int32_t* out) {
  std::vector<char> used(nslots + 1, 0);
  for (int n = 0; n < nslots; ++n) {
    int best = 0, tmin = 99999999;
    for (int is = 1; is <= nslots; ++is) {
      const int t = std::abs(is - nbslot);
      if (!used[is] && t < tmin) best = is, tmin = t;
    }
    out[n] = best, used[best] = 1;
  }
}

}  // namespace

extern "C" {

int letkf_superob_dev(letkf_ctx* c, const letkf_superob_params* p, const letkf_superob_out* o) try {
  if (int rc = check_ctx(c)) return rc;
  if (!p || !o) return fail(LETKF_E_INVALID, "params / out is NULL");
  if (p->nobs < 0 || p->nobs > 0x7fffffffLL) return fail(LETKF_E_INVALID, "nobs must be 0 .. 2^31 - 1");
  if (p->nlon < 1 || p->nlat < 1 || p->nlevx < 1) return fail(LETKF_E_INVALID, "nlon, nlat and nlevx must be >= 1");
  if (p->nslots < 1 || p->nslots > LETKF_SUPEROB_MAX_SLOTS) return fail(LETKF_E_INVALID, "nslots must be 1 .. 64");
  if (p->nbslot < 1 || p->nbslot > p->nslots) return fail(LETKF_E_INVALID, "nbslot must be 1 .. nslots");
  if (p->nobtype < 1 || p->nobtype > LETKF_SUPEROB_MAX_TYPES || p->nid < 1 || p->nid > LETKF_SUPEROB_MAX_TYPES)
    return fail(LETKF_E_INVALID, "nobtype and nid must be 1 .. 32");
  if (!p->slot_off || !p->elem_uid || !p->method_g || !p->method_v || !p->method_t || !p->method_h)
    return fail(LETKF_E_INVALID, "slot_off / elem_uid / a method table is NULL");
  const size_t n = (size_t)p->nobs;
  const void* in_ptr[10] = {p->elm, p->typ, p->lon, p->lat, p->lev, p->dat, p->err, p->ri, p->rj, p->rk};
  const void* out_ptr[14] = {o->elm, o->typ, o->slot, o->lon, o->lat, o->lev, o->dat, o->err, o->ri, o->rj, o->rk, o->i, o->j, o->k};
  if (n > 0) {
    for (const void* q : in_ptr)
      if (!q) return fail(LETKF_E_INVALID, "an input array is NULL");
    for (const void* q : out_ptr)
      if (!q) return fail(LETKF_E_INVALID, "an output array is NULL");
  }
  if (!o->nout) return fail(LETKF_E_INVALID, "nout is NULL");
  if (p->slot_off[0] != 0 || p->slot_off[p->nslots] != p->nobs) return fail(LETKF_E_INVALID, "slot_off must start at 0 and end at nobs");
  for (int s = 0; s < p->nslots; ++s)
    if (p->slot_off[s + 1] < p->slot_off[s]) return fail(LETKF_E_INVALID, "slot_off decreases");
  const int nm = p->nid * p->nobtype;
  letkf::SuperobArgs a = {};
  for (int m = 0; m < nm; ++m) {
    const int g = p->method_g[m], v = p->method_v[m], t = p->method_t[m], h = p->method_h[m];
    if (g < 0 || g > 1 || v < 0 || v > 3 || t < 0 || t > 2 || h < 0 || h > 3)
      return fail(LETKF_E_INVALID, "a method is outside its range (g 0..1, v and h 0..3, t 0..2)");
    a.meth[m] = (uint8_t)(g | v << 1 | t << 3 | h << 5);
    a.any_v |= v > 0, a.any_t |= t > 0;
  }
  {
    unsigned __int128 cells = (unsigned __int128)p->nslots * p->nobtype * p->nid;
    cells *= (unsigned __int128)((int64_t)p->nlevx + 1);
    cells *= (unsigned __int128)p->nlat;
    cells *= (unsigned __int128)p->nlon;
    if (cells >= ((unsigned __int128)1 << 62)) return fail(LETKF_E_INVALID, "the grid has 2^62 cells or more");
  }
  {
    std::vector<Range> in, out;
    for (int q = 0; q < 10; ++q) in.push_back({static_cast<const char*>(in_ptr[q]), n * (q < 2 ? 4 : 8)});
    for (int q = 0; q < 14; ++q) out.push_back({static_cast<const char*>(out_ptr[q]), n * (q >= 3 && q < 11 ? 8 : 4)});
    out.push_back({reinterpret_cast<const char*>(o->nout), 8});
    out.push_back({reinterpret_cast<const char*>(o->slot_off_out), (size_t)(p->nslots + 1) * 8});
    out.push_back({reinterpret_cast<const char*>(o->qc1), n * 4});
    out.push_back({reinterpret_cast<const char*>(o->counts), 7 * 8});
    out.push_back({reinterpret_cast<const char*>(o->obsnum), (size_t)4 * nm * 8});
    for (const Range& x : out)
      for (const Range& y : in)
        if (overlap(x, y)) return fail(LETKF_E_INVALID, "an output overlaps an input");
  }

  a.n = p->nobs, a.elm = p->elm, a.typ = p->typ;
  a.in = letkf::SuperobRows{const_cast<double*>(p->lon), const_cast<double*>(p->lat), const_cast<double*>(p->lev),
                            const_cast<double*>(p->dat), const_cast<double*>(p->err), const_cast<double*>(p->ri),
                            const_cast<double*>(p->rj), const_cast<double*>(p->rk)};
  a.nlon = p->nlon, a.nlat = p->nlat, a.nlevx = p->nlevx, a.nslots = p->nslots, a.nobtype = p->nobtype, a.nid = p->nid;
  a.surf_mask = (uint32_t)p->surface_typ_mask;
  for (int s = 0; s <= p->nslots; ++s) a.slot_off[s] = p->slot_off[s];
  for (int s = p->nslots + 1; s <= LETKF_SUPEROB_MAX_SLOTS; ++s) a.slot_off[s] = p->nobs;
  for (int u = 0; u < p->nid; ++u) a.elem_uid[u] = p->elem_uid[u];
  int32_t pr[LETKF_SUPEROB_MAX_SLOTS];
  slot_priority(p->nslots, p->nbslot, pr);
  for (int r = 0; r < p->nslots; ++r) a.prio[pr[r] - 1] = (uint8_t)r;
  a.out = *o;

  const size_t ws_bytes = letkf::superob_ws_bytes(a, c->stream);
  if (!ws_bytes) return fail(LETKF_E_HIP, "rocprim workspace query failed");
  if (int rc = grow(c, &c->scratch, ws_bytes)) return rc;
  HIP_TRY(letkf::superob_run(c->stream, a, c->scratch.p));
  return LETKF_OK;
} LETKF_ENTRY_END(letkf_superob_dev)

int letkf_superob_default_methods(int32_t nobtype, int32_t nid, int32_t* method_g, int32_t* method_v, int32_t* method_t, int32_t* method_h) try {
  if (!method_g || !method_v || !method_t || !method_h) return fail(LETKF_E_INVALID, "a method table is NULL");
  if (nobtype < 1 || nobtype > LETKF_SUPEROB_MAX_TYPES || nid < 1 || nid > LETKF_SUPEROB_MAX_TYPES)
    return fail(LETKF_E_INVALID, "nobtype and nid must be 1 .. 32");
  for (int u = 0; u < nid; ++u)
    for (int t = 1; t <= nobtype; ++t) {
      const int m = u * nobtype + t - 1;
      method_g[m] = 0;                                                          // scale/obs/superob.f90:120
      method_v[m] = t == 1 || t == 5 || t == 6 ? 2 : 0;                         // :127-130
      method_t[m] = t == 5 || t == 6 || t == 8 ? 1 : t == 9 || t == 10 ? 2 : 0; // :136-141
      method_h[m] = t == 1 || t == 5 || t == 6 ? 0 : 3;                         // :148-151
    }
  return LETKF_OK;
} LETKF_ENTRY_END(letkf_superob_default_methods)

int letkf_superob_slot_priority(int32_t nslots, int32_t nbslot, int32_t* out) try {
  if (!out) return fail(LETKF_E_INVALID, "slot_priority is NULL");
  if (nslots < 1 || nslots > LETKF_SUPEROB_MAX_SLOTS) return fail(LETKF_E_INVALID, "nslots must be 1 .. 64");
  if (nbslot < 1 || nbslot > nslots) return fail(LETKF_E_INVALID, "nbslot must be 1 .. nslots");
  slot_priority(nslots, nbslot, out);
  return LETKF_OK;
} LETKF_ENTRY_END(letkf_superob_slot_priority)

}  // extern "C"
