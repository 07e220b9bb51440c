// letkf_obssim_entry.hip -- C ABI of the sixth companion header include/letkf_amd_obssim.h: obssim_cal on the device.  Host side
// only, in the library of the simulator (libletkf_amd_obssim.so): the kernels are letkf_obssim.hip's; the context, its stream and
// scratch buffer, the operator's field checks and the error text are the main library's (letkf_api_internal.h).

#include "letkf_api_internal.h"
#include "letkf_obssim_dev.h"

using namespace letkf::api;

extern "C" {

int letkf_obssim_dev(letkf_ctx* c, const letkf_obssim_params* p, const letkf_obsope_fields* f, const letkf_obssim_out* o) try {
  if (int rc = check_ctx(c)) return rc;
  if (!p || !f || !o) return fail(LETKF_E_INVALID, "params / fields / out is NULL");
  if (!p->lon || !p->lat) return fail(LETKF_E_INVALID, "lon / lat is NULL");
  if (!o->v3 && !o->v2 && !o->rec) return fail(LETKF_E_INVALID, "v3, v2 and rec are all NULL");
  if (p->nvar3 < 0 || p->nvar3 > LETKF_OBSSIM_MAX_VARS || p->nvar2 < 0 || p->nvar2 > LETKF_OBSSIM_MAX_VARS)
    return fail(LETKF_E_INVALID, "nvar3 and nvar2 must be 0..16");
  if (p->nvar3 == 0 && p->nvar2 == 0) return fail(LETKF_E_INVALID, "nvar3 and nvar2 are both 0");
  if (o->v3 && p->nvar3 == 0) return fail(LETKF_E_INVALID, "v3 is given but nvar3 is 0");
  if (o->v2 && p->nvar2 == 0) return fail(LETKF_E_INVALID, "v2 is given but nvar2 is 0");
  if (f->m0 != 0) return fail(LETKF_E_INVALID, "m0 must be 0");
  if (p->stggrd < 0 || p->stggrd > 1) return fail(LETKF_E_INVALID, "stggrd must be 0 or 1");
  if (p->round_single < 0 || p->round_single > 1) return fail(LETKF_E_INVALID, "round_single must be 0 or 1");
  if (!std::isfinite(p->radar_lon) || !std::isfinite(p->radar_lat) || !std::isfinite(p->radar_z))
    return fail(LETKF_E_INVALID, "radar_lon / radar_lat / radar_z must be finite");
  {
    // the operator's own checks of the fields and of method_ref_calc (letkf_obsope_dev's), behind one conventional file without rows
    static const int64_t off[2] = {0, 0};
    static const int32_t conventional = -1, use = 1;
    static int32_t some_i = 0;
    static double some_d = 0.0;
    letkf_obs_file_rows files = {};
    files.nfile = 1, files.off = off;
    letkf_obsope_params op = {};
    op.file_radar = &conventional, op.use_obs = &use, op.nobtype = 1, op.method_ref_calc = p->method_ref_calc;
    std::string msg;
    if (int rc = letkf::obsope_check(&op, &files, f, 0, 0, &some_i, &some_i, &some_i, &some_d, f->nmem, &msg)) return fail(rc, msg);
  }
  if (f->nlat > 65535 || f->nmem > 65535) return fail(LETKF_E_INVALID, "nlat and nmem must be <= 65535");
  if ((int64_t)f->nlev * f->nlon > 0x7fffffff - 256) return fail(LETKF_E_INVALID, "nlev * nlon must be below 2^31 - 256");

  const size_t ws_bytes = letkf::obssim_ws_bytes(p, f);
  if (ws_bytes)
    if (int rc = grow(c, &c->scratch, ws_bytes)) return rc;
  HIP_TRY(letkf::obssim_run(c->stream, p, f, o, ws_bytes ? c->scratch.p : nullptr));
  return LETKF_OK;
} LETKF_ENTRY_END(letkf_obssim_dev)

}  // extern "C"
