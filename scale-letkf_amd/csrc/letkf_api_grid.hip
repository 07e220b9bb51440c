// letkf_api_grid.hip -- C ABI, the state on the grid: what das_letkf derives before its loop, ensemble mean / perturbations /
// spread, the state transforms, relaxation weights, inflation fields and the departure monitor.

#include <cfloat>

#include "letkf_api_internal.h"

using namespace letkf::api;

extern "C" {

// ---- what das_letkf derives before its loop, on the host: tens of integers, once per analysis

// letkf_tools.f90:139-157
int letkf_var_local_classes(int32_t nvar, int32_t nlt, const double* var_local, int32_t* n2nc, int32_t* n2n,
                            int32_t* nclass) try {
  if (nvar < 1 || nlt < 1 || !var_local || !n2nc || !n2n || !nclass) return LETKF_E_INVALID;
  int nc = 1;
  n2nc[0] = 0;
  n2n[0] = 0;
  for (int n = 1; n < nvar; ++n) {
    bool found = false;
    for (int i = 0; i < nc && !found; ++i) {
      // the reference compares against row var_local_n2nc(i) -- the class NUMBER used as a variable index (:143);
      // restated as written: class i is looked up through the class id of variable i
      const int rep = n2nc[i];
      double mx = 0.0;
      for (int t = 0; t < nlt; ++t) mx = fmax(mx, fabs(var_local[rep + (long)nvar * t] - var_local[n + (long)nvar * t]));
      if (mx < DBL_MIN) {                          // tiny(var_local)
        n2nc[n] = n2nc[i];
        n2n[n] = n2n[n2nc[n]];
        found = true;
      }
    }
    if (!found) {
      n2nc[n] = nc++;
      n2n[n] = n;
    }
  }
  *nclass = nc;
  return LETKF_OK;
} LETKF_ENTRY_END(letkf_var_local_classes)

// letkf_tools.f90:167-192
int letkf_ctype_merge_groups(int32_t nctype, const int32_t* elm_u_ctype, const int32_t* typ_ctype, int32_t nid_obs,
                             int32_t nobtype, const int32_t* ctype_merge, int32_t* group_start, int32_t* group_member,
                             int32_t* ngroup) try {
  if (nctype < 0 || nid_obs < 1 || nobtype < 1 || !ngroup || !group_start) return LETKF_E_INVALID;
  if (nctype > 0 && (!elm_u_ctype || !typ_ctype || !ctype_merge || !group_member)) return LETKF_E_INVALID;
  for (int ic = 0; ic < nctype; ++ic)
    if (elm_u_ctype[ic] < 1 || elm_u_ctype[ic] > nid_obs || typ_ctype[ic] < 1 || typ_ctype[ic] > nobtype)
      return LETKF_E_INVALID;
  auto merge_of = [&](int ic) { return ctype_merge[(elm_u_ctype[ic] - 1) + (long)nid_obs * (typ_ctype[ic] - 1)]; };
  int ng = 0, pos = 0;
  // n_merge(ic) == 0 marks a ctype that an earlier master took (:176-181); kept in group_start's tail as scratch
  // would alias the output, so a small bitmap on the stack / heap it is
  bool* taken = new bool[nctype > 0 ? nctype : 1]();
  group_start[0] = 0;
  for (int ic = 0; ic < nctype; ++ic) {
    if (taken[ic]) continue;
    group_member[pos++] = ic;
    if (merge_of(ic) > 0)
      for (int ic2 = ic + 1; ic2 < nctype; ++ic2)
        if (merge_of(ic2) == merge_of(ic)) {
          group_member[pos++] = ic2;
          taken[ic2] = true;
        }
    group_start[++ng] = pos;
  }
  delete[] taken;
  *ngroup = ng;
  return LETKF_OK;
} LETKF_ENTRY_END(letkf_ctype_merge_groups)

// letkf_tools.f90:197-203
int letkf_radar_only(int32_t nctype, const int32_t* typ_ctype, int32_t typ_radar) try {
  for (int ic = 0; ic < nctype; ++ic)
    if (typ_ctype[ic] != typ_radar) return 0;
  return 1;
} LETKF_ENTRY_END(letkf_radar_only)

int letkf_ens_to_perturbations_dev(letkf_ctx* c, int32_t k, int32_t nv, int64_t npts, double* x, int64_t sp,
                                   int64_t sm, int64_t sv) try {
  if (int rc = check_ctx(c)) return rc;
  if (!x || k < 1 || nv < 1 || npts < 0) return fail(LETKF_E_INVALID, "bad argument");
  if (npts == 0) return LETKF_OK;
  HIP_TRY(letkf::launch_ens_to_pert(k, nv, npts, x, sp, sm, sv, c->stream));
  return LETKF_OK;
} LETKF_ENTRY_END(letkf_ens_to_perturbations_dev)

int letkf_ens_mean_dev(letkf_ctx* c, int32_t k, int32_t nv, int64_t npts, double* x, int64_t sp, int64_t sm,
                       int64_t sv) try {
  if (int rc = check_ctx(c)) return rc;
  if (!x || k < 1 || nv < 1 || npts < 0) return fail(LETKF_E_INVALID, "bad argument");
  if (npts == 0) return LETKF_OK;
  HIP_TRY(letkf::launch_ens_mean(k, nv, npts, x, sp, sm, sv, c->stream));
  return LETKF_OK;
} LETKF_ENTRY_END(letkf_ens_mean_dev)

int letkf_relax_beta_dev(letkf_ctx* c, const letkf_beta_params* p, int64_t nij1, int32_t nlev, const double* rig,
                         const double* rjg, const double* hgt, double* beta) try {
  if (int rc = check_ctx(c)) return rc;
  if (!p || nij1 < 0 || nlev < 1) return fail(LETKF_E_INVALID, "params is NULL or bad nij1 / nlev");
  if (nij1 == 0) return LETKF_OK;
  if (!rig || !rjg || !hgt || !beta) return fail(LETKF_E_INVALID, "a point array is NULL");
  HIP_TRY(letkf::launch_relax_beta(*p, nij1, nlev, rig, rjg, hgt, beta, c->num_cu, c->stream));
  return LETKF_OK;
} LETKF_ENTRY_END(letkf_relax_beta_dev)

int letkf_infl_init_dev(letkf_ctx* c, int64_t n, double* work3d, double infl_mul, double infl_mul_min) try {
  if (int rc = check_ctx(c)) return rc;
  if (n < 0) return fail(LETKF_E_INVALID, "negative size");
  if (n == 0) return LETKF_OK;
  if (!work3d) return fail(LETKF_E_INVALID, "work3d is NULL");
  HIP_TRY(letkf::launch_infl_init(n, work3d, infl_mul, infl_mul_min, c->num_cu, c->stream));
  return LETKF_OK;
} LETKF_ENTRY_END(letkf_infl_init_dev)

int letkf_state_trans_dev(letkf_ctx* c, const letkf_state_consts* k, int32_t nlev, int32_t nlon, int32_t nlat,
                          int32_t nv3d, double* v3dg, int32_t inverse) try {
  if (int rc = check_ctx(c)) return rc;
  if (!k || !v3dg || nlev < 1 || nlon < 1 || nlat < 1 || nv3d < 1) return fail(LETKF_E_INVALID, "bad argument");
  if (k->iv_q < 0 || k->iv_q >= nv3d || nv3d - k->iv_q > 8) return fail(LETKF_E_INVALID, "moisture range must be 1..8 variables");
  for (const int32_t iv : {k->iv_rho, k->iv_rhou, k->iv_rhov, k->iv_rhow, k->iv_rhot, k->iv_u, k->iv_v, k->iv_w, k->iv_t, k->iv_p})
    if (iv < 0 || iv >= nv3d) return fail(LETKF_E_INVALID, "a variable slot lies outside [0, nv3d)");
  HIP_TRY(letkf::launch_state_trans(*k, nlev, (long)nlon * nlat, nv3d, v3dg, inverse, c->stream));
  return LETKF_OK;
} LETKF_ENTRY_END(letkf_state_trans_dev)

int letkf_member_points_dev(letkf_ctx* c, int32_t dir, int32_t nlev, int32_t nlon, int32_t nlat, int32_t nv3d,
                            int32_t np, int32_t rank, int32_t m, double* v3dg, double* x, int64_t nij1, int64_t sp,
                            int64_t sm, int64_t sv) try {
  if (int rc = check_ctx(c)) return rc;
  if (!v3dg || !x || np < 1 || rank < 0 || rank >= np || m < 0 || nij1 < 0) return fail(LETKF_E_INVALID, "bad argument");
  if (nlev < 1 || nlon < 1 || nlat < 1 || nv3d < 1) return fail(LETKF_E_INVALID, "nlev, nlon, nlat and nv3d must be at least 1");
  const long nxy = (long)nlon * nlat;
  const long expect = (nxy - rank + np - 1) / np;               // points r, r+np, ... below nlon*nlat
  if (nij1 != expect) return fail(LETKF_E_INVALID, "nij1 does not match the cyclic share of this rank");
  if (nij1 == 0) return LETKF_OK;
  HIP_TRY(letkf::launch_member_points(dir, nlev, nlon, nxy, nv3d, np, rank, nij1, v3dg, x, sp, (long)m * sm, sv, c->stream));
  return LETKF_OK;
} LETKF_ENTRY_END(letkf_member_points_dev)

int letkf_ens_spread_dev(letkf_ctx* c, int32_t k, int32_t nv, int64_t npts, const double* x, int64_t sp, int64_t sm,
                         int64_t sv, double* sprd) try {
  if (int rc = check_ctx(c)) return rc;
  if (!x || !sprd || k < 2 || nv < 1 || npts < 0) return fail(LETKF_E_INVALID, "bad argument");
  if (npts == 0) return LETKF_OK;
  HIP_TRY(letkf::launch_ens_spread(k, nv, npts, x, sp, sm, sv, sprd, c->stream));
  return LETKF_OK;
} LETKF_ENTRY_END(letkf_ens_spread_dev)

int letkf_monit_dep_dev(letkf_ctx* c, int32_t nid, const int32_t* elem_uid, int64_t nn, const int32_t* elm,
                        const double* dep, const int32_t* qc, int32_t* nobs, double* bias, double* rmse) try {
  if (int rc = check_ctx(c)) return rc;
  if (nid < 1 || nid > 32 || !elem_uid || nn < 0 || !nobs || !bias || !rmse)
    return fail(LETKF_E_INVALID, "bad element table / outputs");
  if (nn > 0 && (!elm || !dep || !qc)) return fail(LETKF_E_INVALID, "an observation array is NULL");
  const size_t need = letkf::monit_scratch_bytes(nid, c->num_cu);
  if (int rc = grow(c, &c->scratch, need)) return rc;
  HIP_TRY(letkf::launch_monit_dep(nid, elem_uid, nn, elm, dep, qc, nobs, bias, rmse, c->scratch.p, c->num_cu, c->stream));
  return LETKF_OK;
} LETKF_ENTRY_END(letkf_monit_dep_dev)

int letkf_additive_inflation_dev(letkf_ctx* c, int32_t k, int32_t nv, int64_t npts, int64_t nij1, double* anal,
                                 const double* add, int64_t sp, int64_t sm, int64_t sv, double infl_add,
                                 const double* weight, const double* qmean, int64_t q_sp, int64_t q_sv,
                                 int32_t iv_q_first, int32_t iv_q_last, const int32_t* ishuf) try {
  if (int rc = check_ctx(c)) return rc;
  if (k < 1 || nv < 1 || npts < 0 || nij1 < 1 || !anal || !add) return fail(LETKF_E_INVALID, "bad argument");
  if (npts % nij1 != 0) return fail(LETKF_E_INVALID, "npts must be nij1 * nlev");
  HIP_TRY(letkf::launch_additive(k, nv, npts, nij1, anal, add, sp, sm, sv, infl_add, weight, qmean, q_sp, q_sv,
                                 iv_q_first, iv_q_last, ishuf, c->num_cu, c->stream));
  return LETKF_OK;
} LETKF_ENTRY_END(letkf_additive_inflation_dev)

int letkf_addinfl_weight_dev(letkf_ctx* c, int64_t nij1, const double* rig, const double* rjg, int64_t nob,
                             const double* ob_ri, const double* ob_rj, double dx, double dy, double hori_loc,
                             double* weight) try {
  if (int rc = check_ctx(c)) return rc;
  if (nij1 < 0 || nob < 0 || !(hori_loc > 0.0)) return fail(LETKF_E_INVALID, "bad argument");
  if (nij1 == 0) return LETKF_OK;
  if (!rig || !rjg || !weight || (nob > 0 && (!ob_ri || !ob_rj))) return fail(LETKF_E_INVALID, "a pointer is NULL");
  const double cut2 = (double)13.33333333f;   // dist_zero_fac_square, a single-precision literal (letkf_obs.f90:28)
  HIP_TRY(letkf::launch_addinfl_weight(nij1, rig, rjg, nob, ob_ri, ob_rj, dx, dy, hori_loc, cut2, weight, c->num_cu,
                                       c->stream));
  return LETKF_OK;
} LETKF_ENTRY_END(letkf_addinfl_weight_dev)

}  // extern "C"
