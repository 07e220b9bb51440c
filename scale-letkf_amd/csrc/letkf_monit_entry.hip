// letkf_monit_entry.hip -- C ABI of the fourth companion header include/letkf_amd_monit.h: state_to_history, monit_obs and the
// list of monitored elements.  Host side only (the kernels are letkf_monit.hip's, the operator's letkf_obsope.hip's and
// launch_monit_dep's); the context, its buffers and the error text are the ones of letkf_api_internal.h.

#include "letkf_api_internal.h"
#include "letkf_monit_dev.h"

using namespace letkf::api;

extern "C" {

int letkf_state_to_history_dev(letkf_ctx* c, const letkf_hist_state* s, const letkf_obsope_fields* layout, double* v3d,
                               double* v2d) try {
  if (int rc = check_ctx(c)) return rc;
  std::string msg;
  if (int rc = letkf::hist_check(s, layout, v3d, v2d, &msg)) return fail(rc, msg);
  if (int rc = grow(c, &c->scratch, letkf::hist_ws_bytes(layout))) return rc;
  HIP_TRY(letkf::hist_run(c->stream, s, layout, v3d, v2d, c->scratch.p));
  return LETKF_OK;
} LETKF_ENTRY_END(letkf_state_to_history_dev)

// Gather by key -> the operator on the gathered rows (its row check is the call's one read-back) -> the rules of monit_obs and
// the records -> monit_dep.  Nothing of the caller's is written before the read-back has passed.
int letkf_monit_obs_dev(letkf_ctx* c, const letkf_monit_params* mp, const letkf_obsope_params* op, const letkf_obs_file_rows* files,
                        const letkf_obsope_fields* f, int64_t nn, const int32_t* key, const int32_t* set, const int32_t* idx,
                        const letkf_obsdep* rec, int32_t* nobs, double* bias, double* rmse) try {
  if (int rc = check_ctx(c)) return rc;
  if (!mp || !mp->elem_uid) return fail(LETKF_E_INVALID, "monit params / elem_uid is NULL");
  if (mp->step < 1 || mp->step > 2) return fail(LETKF_E_INVALID, "step must be 1 (guess) or 2 (analysis)");
  if (mp->nid < 1 || mp->nid > 32) return fail(LETKF_E_INVALID, "nid must be 1..32");
  if (!rec || !rec->set || !rec->idx || !rec->qc || !rec->omb || !rec->oma) return fail(LETKF_E_INVALID, "rec or one of its arrays is NULL");
  if (!nobs || !bias || !rmse) return fail(LETKF_E_INVALID, "nobs / bias / rmse is NULL");
  if (mp->t_range > 0.0 && !mp->dif) return fail(LETKF_E_INVALID, "t_range > 0 needs dif");
  if (nn < 0) return fail(LETKF_E_INVALID, "nn is negative");
  if (f && f->nmem != 1) return fail(LETKF_E_INVALID, "monit_obs takes one state: nmem must be 1");
  const size_t stat_bytes = letkf::monit_scratch_bytes(mp->nid, c->num_cu);
  if (int rc = grow(c, &c->scratch, letkf::monit_ws_bytes(nn, stat_bytes))) return rc;
  letkf::MonitWs w;
  letkf::monit_ws_layout(c->scratch.p, nn, stat_bytes, &w);
  std::string msg;
  if (int rc = letkf::obsope_check(op, files, f, 0, nn, set, idx, w.oqc, w.val, 1, &msg)) return fail(rc, msg);
  if (files->off[files->nfile] > 0 && !files->dat) return fail(LETKF_E_INVALID, "files->dat is NULL");
  HIP_TRY(letkf::monit_gather(c->stream, nn, key, set, idx, op->rotc, w));
  letkf_obsope_params gop = *op;                                    // the operator on the gathered rows: rotc is per obsda row
  if (op->rotc) gop.rotc = w.rotc;
  if (int rc = letkf::obsope_run(c->stream, &gop, files, f, 0, nn, w.set, w.idx, w.oqc, w.val, 1, w.flag, &msg))
    return fail(rc, rc == LETKF_E_INVALID && key ? "a key entry is negative, or " + msg : msg);
  HIP_TRY(letkf::monit_finish(c->stream, mp, op, files, nn, rec, w));
  HIP_TRY(letkf::launch_monit_dep(mp->nid, mp->elem_uid, nn, w.elm, w.dep, w.qc, nobs, bias, rmse, w.stat, c->num_cu, c->stream));
  return LETKF_OK;
} LETKF_ENTRY_END(letkf_monit_obs_dev)

int letkf_monit_type(int32_t nid, const int32_t* elem_uid, int32_t departure_stat_radar, int32_t departure_stat_h08,
                     int32_t* monit_type) try {
  if (nid < 1 || nid > 32 || !elem_uid || !monit_type) return fail(LETKF_E_INVALID, "nid must be 1..32, elem_uid and monit_type given");
  for (int i = 0; i < nid; ++i) {
    const int e = elem_uid[i];
    const bool conv = e == 2819 || e == 2820 || e == 3073 || e == 3074 || e == 3330 || e == 14593;   // U V T Tv Q PS (:1822-1828)
    const bool radar = e == 4001 || e == 4004 || e == 4002;                                           // REF RE0 Vr (:1830-1832)
    monit_type[i] = (conv || (radar && departure_stat_radar) || (e == 8800 && departure_stat_h08)) ? 1 : 0;
  }
  return LETKF_OK;
} LETKF_ENTRY_END(letkf_monit_type)

}  // extern "C"
