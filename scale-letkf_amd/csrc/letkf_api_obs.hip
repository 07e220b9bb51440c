// letkf_api_obs.hip -- C ABI, the observation side: departures, mesh sort, halo plan, gathers, set_letkf_obs and its table,
// the observation operator, and the exchanges between ranks.

#include "letkf_api_internal.h"

using namespace letkf::api;

namespace {
struct NamedPtr {
  const void* p;
  const char* name;
};
// LETKF_E_INVALID naming the first NULL pointer of the list, or 0
int first_null(std::initializer_list<NamedPtr> l) {
  for (const NamedPtr& a : l)
    if (!a.p) return fail(LETKF_E_INVALID, std::string(a.name) + " is NULL");
  return 0;
}
}  // namespace

extern "C" {

int letkf_obs_departure_dev(letkf_ctx* c, const letkf_qc_params* p, int64_t nobs, const int32_t* elm, const double* dat,
                            const double* err, double* ensval, int64_t kld, double* val, int32_t* qc) try {
  if (int rc = check_ctx(c)) return rc;
  if (!p) return fail(LETKF_E_INVALID, "p is NULL");
  if (nobs < 0) return fail(LETKF_E_INVALID, "nobs is negative");
  if (nobs == 0) return LETKF_OK;
  if (int rc = first_null({{elm, "elm"}, {dat, "dat"}, {err, "err"}, {ensval, "ensval"}, {val, "val"}, {qc, "qc"}})) return rc;
  if (p->member < 1) return fail(LETKF_E_INVALID, "p->member must be positive");
  if (kld < p->member + (p->det_run ? 1 : 0)) return fail(LETKF_E_INVALID, "kld must hold MEMBER (+1 with DET_RUN) columns");
  HIP_TRY(letkf::launch_obs_departure(*p, nobs, elm, dat, err, ensval, kld, val, qc, c->num_cu, c->lds_max, c->stream));
  return LETKF_OK;
} LETKF_ENTRY_END(letkf_obs_departure_dev)

int letkf_obs_mesh_sort_dev(letkf_ctx* c, const letkf_mesh* m, int64_t nobs, const int32_t* ctype, const double* ri,
                            const double* rj, const int32_t* qc, int32_t* n_cell, int32_t* key, int64_t* nsorted) try {
  if (int rc = check_ctx(c)) return rc;
  if (int rc = first_null({{m, "mesh"}, {nsorted, "nsorted"}, {n_cell, "n_cell"}})) return rc;
  if (nobs < 0 || nobs >= (1LL << 31)) return fail(LETKF_E_INVALID, "nobs outside 0..2^31-1");
  if (m->nctype < 1) return fail(LETKF_E_INVALID, "mesh->nctype must be positive");
  if (int rc = first_null({{m->ngrd_i, "mesh->ngrd_i"}, {m->ngrd_j, "mesh->ngrd_j"}})) return rc;
  if (m->nlon < 1) return fail(LETKF_E_INVALID, "mesh->nlon must be positive");
  if (m->nlat < 1) return fail(LETKF_E_INVALID, "mesh->nlat must be positive");
  for (int ic = 0; ic < m->nctype; ++ic)
    if (m->ngrd_i[ic] < 1 || m->ngrd_j[ic] < 1) return fail(LETKF_E_INVALID, "mesh->ngrd_i / ngrd_j: an empty mesh");
  if (nobs > 0)
    if (int rc = first_null({{ctype, "ctype"}, {ri, "ri"}, {rj, "rj"}, {qc, "qc"}, {key, "key"}})) return rc;
  size_t need = 0;
  long ns = 0;
  bool bad = false;
  HIP_TRY(letkf::obs_mesh_sort(*m, nobs, ctype, ri, rj, qc, n_cell, key, &ns, &bad, nullptr, &need, c->num_cu, c->stream));
  if (int rc = grow(c, &c->scratch, need)) return rc;
  size_t have = c->scratch.cap;
  HIP_TRY(letkf::obs_mesh_sort(*m, nobs, ctype, ri, rj, qc, n_cell, key, &ns, &bad, c->scratch.p, &have, c->num_cu, c->stream));
  if (bad) return fail(LETKF_E_INVALID, "ctype: a row with qc = 0 has a value outside 0..nctype-1");
  *nsorted = ns;
  return LETKF_OK;
} LETKF_ENTRY_END(letkf_obs_mesh_sort_dev)

int letkf_obs_halo_plan_dev(letkf_ctx* c, const letkf_halo_layout* l, const int32_t* n_all, int32_t* ac_ext,
                            int32_t* src_row, int64_t cap, int64_t* nobstotal) try {
  if (int rc = check_ctx(c)) return rc;
  if (int rc = first_null({{l, "layout"}, {nobstotal, "nobstotal"}, {n_all, "n_all"}, {ac_ext, "ac_ext"}})) return rc;
  if (l->nctype < 1) return fail(LETKF_E_INVALID, "layout->nctype must be positive");
  if (l->nprocs < 1) return fail(LETKF_E_INVALID, "layout->nprocs must be positive");
  if (l->prc_num_x < 1 || l->nprocs % l->prc_num_x != 0)
    return fail(LETKF_E_INVALID, "layout->prc_num_x must be positive and divide nprocs");
  if (l->myrank < 0 || l->myrank >= l->nprocs) return fail(LETKF_E_INVALID, "layout->myrank outside 0..nprocs-1");
  if (int rc = first_null({{l->ngrd_i, "layout->ngrd_i"}, {l->ngrd_j, "layout->ngrd_j"}, {l->ngrdsch_i, "layout->ngrdsch_i"},
                           {l->ngrdsch_j, "layout->ngrdsch_j"}}))
    return rc;
  for (int ic = 0; ic < l->nctype; ++ic) {
    if (l->ngrd_i[ic] < 1 || l->ngrd_j[ic] < 1) return fail(LETKF_E_INVALID, "layout->ngrd_i / ngrd_j: an empty mesh");
    if (l->ngrdsch_i[ic] < 0 || l->ngrdsch_j[ic] < 0) return fail(LETKF_E_INVALID, "layout->ngrdsch_i / ngrdsch_j is negative");
  }
  if (cap < 0) return fail(LETKF_E_INVALID, "cap is negative");
  if (cap > 0 && !src_row) return fail(LETKF_E_INVALID, "src_row is NULL");
  long nt = -1;                                          // stays so when a count of n_all is refused: nothing is written then
  const char* refused = nullptr;
  hipError_t e = letkf::obs_halo_plan(*l, n_all, ac_ext, src_row, cap, &nt, &refused, c->num_cu, c->stream);
  if (nt >= 0) *nobstotal = nt;
  if (refused) return fail(LETKF_E_INVALID, refused);
  HIP_TRY(e);
  return LETKF_OK;
} LETKF_ENTRY_END(letkf_obs_halo_plan_dev)

int letkf_obs_gather_rows_dev(letkf_ctx* c, int64_t nrows, const int32_t* src_row, int32_t ncols, const double* src,
                              int64_t ld_src, double* dst, int64_t ld_dst) try {
  if (int rc = check_ctx(c)) return rc;
  if (nrows < 0) return fail(LETKF_E_INVALID, "nrows is negative");
  if (ncols < 0) return fail(LETKF_E_INVALID, "ncols is negative");
  if (nrows == 0 || ncols == 0) return LETKF_OK;
  if (int rc = first_null({{src_row, "src_row"}, {src, "src"}, {dst, "dst"}})) return rc;
  if (ld_src < ncols) return fail(LETKF_E_INVALID, "ld_src is smaller than ncols");
  if (ld_dst < ncols) return fail(LETKF_E_INVALID, "ld_dst is smaller than ncols");
  HIP_TRY(letkf::launch_gather_rows(nrows, src_row, ncols, src, ld_src, dst, ld_dst, c->num_cu, c->stream));
  return LETKF_OK;
} LETKF_ENTRY_END(letkf_obs_gather_rows_dev)

int letkf_obs_gather_i32_dev(letkf_ctx* c, int64_t nrows, const int32_t* src_row, const int32_t* src, int32_t* dst) try {
  if (int rc = check_ctx(c)) return rc;
  if (nrows < 0) return fail(LETKF_E_INVALID, "nrows is negative");
  if (nrows == 0) return LETKF_OK;
  if (int rc = first_null({{src_row, "src_row"}, {src, "src"}, {dst, "dst"}})) return rc;
  HIP_TRY(letkf::launch_gather_i32(nrows, src_row, src, dst, c->num_cu, c->stream));
  return LETKF_OK;
} LETKF_ENTRY_END(letkf_obs_gather_i32_dev)

int letkf_obs_mesh_dims(int32_t nctype, const int32_t* typ_ctype, const double* hori_loc_ctype, int32_t nobtype,
                        const double* obs_sort_grid_spacing, const int32_t* max_nobs_per_grid, const double* obs_min_spacing,
                        double dx, double dy, int32_t nlon, int32_t nlat, int32_t* ngrd_i, int32_t* ngrd_j, double* grdspc_i,
                        double* grdspc_j, int32_t* ngrdsch_i, int32_t* ngrdsch_j, int32_t* ngrdext_i, int32_t* ngrdext_j) try {
  if (nctype < 0) return fail(LETKF_E_INVALID, "nctype is negative");
  if (nobtype < 1) return fail(LETKF_E_INVALID, "nobtype must be positive");
  if (nlon < 1) return fail(LETKF_E_INVALID, "nlon must be positive");
  if (nlat < 1) return fail(LETKF_E_INVALID, "nlat must be positive");
  if (nctype == 0) return LETKF_OK;
  if (int rc = first_null({{typ_ctype, "typ_ctype"}, {hori_loc_ctype, "hori_loc_ctype"},
                           {obs_sort_grid_spacing, "obs_sort_grid_spacing"}, {max_nobs_per_grid, "max_nobs_per_grid"},
                           {obs_min_spacing, "obs_min_spacing"}, {ngrd_i, "ngrd_i"}, {ngrd_j, "ngrd_j"}, {grdspc_i, "grdspc_i"},
                           {grdspc_j, "grdspc_j"}, {ngrdsch_i, "ngrdsch_i"}, {ngrdsch_j, "ngrdsch_j"}, {ngrdext_i, "ngrdext_i"},
                           {ngrdext_j, "ngrdext_j"}}))
    return rc;
  // the types first, so that a refusal leaves every output as it was
  for (int ic = 0; ic < nctype; ++ic)
    if (typ_ctype[ic] < 1 || typ_ctype[ic] > nobtype) return fail(LETKF_E_INVALID, "typ_ctype: a report type outside 1..nobtype");
  if (letkf::obs_mesh_dims(nctype, typ_ctype, hori_loc_ctype, nobtype, obs_sort_grid_spacing, max_nobs_per_grid,
                           obs_min_spacing, dx, dy, nlon, nlat, ngrd_i, ngrd_j, grdspc_i, grdspc_j, ngrdsch_i, ngrdsch_j,
                           ngrdext_i, ngrdext_j))
    return fail(LETKF_E_INVALID, "a sorting mesh came out empty (check hori_loc_ctype / obs_sort_grid_spacing / dx / dy)");
  return LETKF_OK;
} LETKF_ENTRY_END(letkf_obs_mesh_dims)

int letkf_set_obs_local_dev(letkf_ctx* c, const letkf_setobs_params* p, const letkf_qc_params* qcp, const letkf_obs_file_rows* files,
                            int64_t nobs, const int32_t* set, const int32_t* idx, int32_t* qc, double* ensval, int64_t kld,
                            letkf_obs_table** tab) try {
  if (int rc = check_ctx(c)) return rc;
  std::string msg;
  if (int rc = letkf::set_obs_local(c->device, c->stream, c->num_cu, c->lds_max, p, qcp, files, nobs, set, idx, qc, ensval, kld, tab,
                                    &msg))
    return fail(rc, msg);
  return LETKF_OK;
} LETKF_ENTRY_END(letkf_set_obs_local_dev)

int letkf_set_obs_finish_dev(letkf_ctx* c, letkf_obs_table* tab, const int32_t* n_all, const int32_t* tot_g, int64_t nrecv,
                             const double* recv) try {
  if (int rc = check_ctx(c)) return rc;
  std::string msg;
  if (int rc = letkf::set_obs_finish(c->stream, c->num_cu, tab, n_all, tot_g, nrecv, recv, &msg)) return fail(rc, msg);
  return LETKF_OK;
} LETKF_ENTRY_END(letkf_set_obs_finish_dev)

int letkf_set_obs_dev(letkf_ctx* c, const letkf_setobs_params* p, const letkf_qc_params* qcp, const letkf_obs_file_rows* files,
                      int64_t nobs, const int32_t* set, const int32_t* idx, int32_t* qc, double* ensval, int64_t kld,
                      letkf_obs_table** tab) try {
  if (!tab) return fail(LETKF_E_INVALID, "tab is NULL");
  *tab = nullptr;
  if (!p) return fail(LETKF_E_INVALID, "p is NULL");
  if (p->nprocs != 1) return fail(LETKF_E_INVALID, "letkf_set_obs_dev is the one-rank call: nprocs must be 1");
  if (int rc = letkf_set_obs_local_dev(c, p, qcp, files, nobs, set, idx, qc, ensval, kld, tab)) return rc;
  letkf_obs_table_info i;
  letkf::obs_table_info(*tab, &i);
  if (int rc = letkf_set_obs_finish_dev(c, *tab, i.n_cell, nullptr, i.nsorted, i.sendbuf)) {
    letkf_obs_table_destroy(*tab);
    *tab = nullptr;
    return rc;
  }
  return LETKF_OK;
} LETKF_ENTRY_END(letkf_set_obs_dev)

int letkf_obs_table_info_get(const letkf_obs_table* tab, letkf_obs_table_info* info) try {
  if (int rc = first_null({{tab, "tab"}, {info, "info"}})) return rc;
  letkf::obs_table_info(tab, info);
  return LETKF_OK;
} LETKF_ENTRY_END(letkf_obs_table_info_get)

int letkf_obs_table_search(const letkf_obs_table* tab, letkf_search_tables* tables) try {
  if (int rc = first_null({{tab, "tab"}, {tables, "tables"}})) return rc;
  if (letkf::obs_table_search(tab, tables)) return fail(LETKF_E_INVALID, "tab: the finish half has not run");
  return LETKF_OK;
} LETKF_ENTRY_END(letkf_obs_table_search)

int letkf_obs_table_set_varloc(letkf_ctx* c, letkf_obs_table* tab, const double* varloc) try {
  if (int rc = check_ctx(c)) return rc;
  std::string msg;
  if (int rc = letkf::obs_table_set_varloc(c->stream, tab, varloc, &msg)) return fail(rc, msg);
  return LETKF_OK;
} LETKF_ENTRY_END(letkf_obs_table_set_varloc)

int letkf_obs_table_download(letkf_ctx* c, const letkf_obs_table* tab, double* ensval, double* val, int32_t* qc, double* ob_ri,
                             double* ob_rj, double* ob_lev, double* ob_dat, double* ob_err, int32_t* ac_ext) try {
  if (int rc = check_ctx(c)) return rc;
  std::string msg;
  double* ob[5] = {ob_ri, ob_rj, ob_lev, ob_dat, ob_err};
  if (int rc = letkf::obs_table_download(c->stream, tab, ensval, val, qc, ob, ac_ext, &msg)) return fail(rc, msg);
  return LETKF_OK;
} LETKF_ENTRY_END(letkf_obs_table_download)

int letkf_obs_table_destroy(letkf_obs_table* tab) try {
  letkf::obs_table_destroy(tab);
  return LETKF_OK;
} LETKF_ENTRY_END(letkf_obs_table_destroy)

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
} LETKF_ENTRY_END(letkf_obsope_dev)

int letkf_obs_allgatherv_dev(letkf_ctx* c, void* nccl_comm, int32_t nranks, int32_t myrank, const int64_t* counts,
                             int64_t row_bytes, const void* send, void* recv) try {
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
} LETKF_ENTRY_END(letkf_obs_allgatherv_dev)

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
                        const void* send, void* recv) try {
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
} LETKF_ENTRY_END(letkf_alltoallv_dev)

int letkf_allreduce_sum_i32_dev(letkf_ctx* c, void* nccl_comm, int32_t nranks, int64_t count, int32_t* buf) try {
  if (int rc = check_ctx(c)) return rc;
  if ((nranks > 1 && !nccl_comm) || nranks < 1 || count < 0 || (count > 0 && !buf)) return fail(LETKF_E_INVALID, "bad argument");
  const char* what = "";
  return rccl_result(letkf::rccl_allreduce_sum_i32(nccl_comm, nranks, count, buf, c->stream, &what), what);
} LETKF_ENTRY_END(letkf_allreduce_sum_i32_dev)

// scatter_grd_mpi_alltoall / gather_grd_mpi_alltoall (scale/common/common_mpi_scale.f90:1279-1396) with the exchange inside the
// library: per-destination blocks [nv3d][nlev * nij1(d)] dealt out of / assembled into the member field by the kernel of
// letkf_member_points_dev (grd_to_buf / buf_to_grd), ONE grouped exchange with true counts, the blocks filed into / taken from
// the member slots of the state.  Workspace: the context's scratch buffer (send blocks | receive blocks).
int letkf_members_alltoall_dev(letkf_ctx* c, void* nccl_comm, int32_t nranks, int32_t myrank, int32_t dir, int32_t nlev,
                               int32_t nlon, int32_t nlat, int32_t nv3d, int32_t mstart, int32_t mcount, double* v3dg, double* x,
                               int64_t sp, int64_t sm, int64_t sv) try {
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
} LETKF_ENTRY_END(letkf_members_alltoall_dev)

}  // extern "C"
