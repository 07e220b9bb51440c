// letkf_api_internal.h -- what the units of the C ABI (letkf_api*.hip) share: the context, the error barrier, the device
// buffers, the plumbing of the list-driven entries and the launch of the loop body.  Host side, not installed; beside them only
// letkf_monit_entry.hip (the entries of include/letkf_amd_monit.h) and, from the libraries of the OSSE tools, of the simulator and
// of superob, letkf_obsmake_entry.hip (include/letkf_amd_obsmake.h), letkf_obssim_entry.hip (include/letkf_amd_obssim.h) and
// letkf_superob_entry.hip (include/letkf_amd_superob.h) include it, and obsscan/letkf_obsscan_entry.hip
// (include/letkf_amd_obsscan.h) from the library of the first scan and mapproj/letkf_mapproj_entry.hip
// (include/letkf_amd_mapproj.h) from the library of the map projection, and nobsout/letkf_nobsout_entry.hip
// (include/letkf_amd_nobsout.h) from the library of NOBS_OUT, and tcvital/letkf_tcvital_entry.hip (include/letkf_amd_tcvital.h)
// from the library of the TC vitals, and h08/letkf_h08_entry.hip (include/letkf_amd_h08.h) from the library of the Himawari-8
// radiances.  Every function is defined in the one unit named above its declaration.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/letkf_amd.h"
#include "../../include/letkf_amd_interp_window.h"
#include "letkf_api_error.h"
#include "letkf_device.h"
#include "letkf_interp_dev.h"
#include "letkf_obsope_dev.h"

#define HIP_TRY(expr)                                                                              \
  do {                                                                                             \
    hipError_t _e = (expr);                                                                        \
    if (_e != hipSuccess)                                                                          \
      return letkf::api::fail(LETKF_E_HIP, std::string(#expr) + ": " + hipGetErrorString(_e));     \
  } while (0)

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

namespace letkf::api {

inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

// ---- letkf_api.hip: the context and its buffers
int check_ctx(letkf_ctx* c);
int drop(letkf_ctx* c, DevBuf* b);
hipError_t alloc(DevBuf* b, size_t cap);
int grow(letkf_ctx* c, DevBuf* b, size_t need, bool slack = true);

// ---- letkf_api.hip: the plumbing of the list-driven entries: count pass -> offsets -> chunks that fit a budget -> fill pass
// per chunk.
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
int scan_ws(letkf_ctx* c, DevBuf* b, size_t n, size_t tail_bytes, ScanWs* s);
hipError_t zero_total(letkf_ctx* c, const ScanWs& s);
hipError_t scan_offsets(letkf_ctx* c, const ScanWs& s);
int offsets_to_host(letkf_ctx* c, ScanWs& s, size_t stride = 1, void* also_dst = nullptr, const void* also_src = nullptr,
                    size_t also_bytes = 0);
int64_t chunk_end(const std::vector<int64_t>& off, int64_t first, int64_t end, int64_t stride, int64_t entry_bytes,
                  int64_t budget, int64_t max_entries = INT64_MAX);

// A chunk's entries [e0, e1) in a workspace of their own.  The kernels address entry j of item p as base[off[p] + j] with the
// GLOBAL offsets: shift the bases.  A chunk without entries still has a base: room for one.
//
// ... local-observation lists idx | rdiag | rloc in list_ws (20 B per entry)
struct ListSlab {
  int32_t* idx = nullptr;
  double *rd = nullptr, *rl = nullptr;
};
int list_slab(letkf_ctx* c, int64_t e0, int64_t e1, ListSlab* l);
// ... the horizontal survivors of a batch of columns in buffer b (4 doubles each)
int survivor_slab(letkf_ctx* c, DevBuf* b, int64_t e0, int64_t e1, double** sv);

// the column entries' two passes over letkf_obs_search_columns_dev: all levels counted and scanned; the lists of levels [l0, l1)
int count_columns(letkf_ctx* c, const letkf_search_tables* t, int64_t ncol, int32_t nlev, const double* rig, const double* rjg,
                  const double* rlev, const double* rz, ScanWs* sw);
int fill_columns(letkf_ctx* c, const letkf_search_tables* t, int64_t ncol, int l0, int l1, const double* rig, const double* rjg,
                 const double* rlev, const double* rz, const ScanWs& sw, ListSlab* ls);

// Inside the column entries: the column searches of one entry (a count pass, a fill pass per slab) share the ring-ordered
// survivors of the dense limited case; the guard drops them when the entry returns.
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

// ---- letkf_api.hip: a loop-body / letkf_core call through the route that pick_route chooses
int launch(letkf_ctx* c, letkf::PointArgs& a, int warm_run = 0, long warm_stride = 1);

// ---- letkf_api_search.hip
int tables_limited(letkf_ctx* c, const letkf_search_tables* t, bool* limited);
int tables_hinted(letkf_ctx* c, const letkf_search_tables* t, letkf_search_tables* tab);

// ---- letkf_api_das.hip
int report_counts(letkf_ctx* c, const int32_t* counts, int64_t n, const double* beta, int32_t* nobs_out);
// (mode 3, letkf_das_columns_dev's list-free route: the points are pt0 + a * pt_stride + b, b < g->warm_stride columns whose
// horizontal survivors are sv[4 * sv_off[b] ..]; every per-point array of g is indexed by that GLOBAL point number)
struct SurvivorView {
  const int64_t* sv_off;
  const double* sv;
  int64_t pt_stride, pt0;
  int64_t cap;               // most survivors of a column of the batch (bounds a point's local list)
};
int das_args_check(const letkf_das_args* g, bool lists);
int das_points_impl(letkf_ctx* c, const letkf_das_args* g, const letkf_search_tables* t, const double* ri, const double* rj,
                    const double* rlev, const double* rz, int32_t* nobs_out, const SurvivorView* sview = nullptr);
// (letkf_das_columns_dev is das_columns_impl with d = NULL.  With d -- nobsout/letkf_nobsout_entry.hip, from the library of
// include/letkf_amd_nobsout.h -- the search passes of the call also write nobsl_t / cutd_t of its points, dev [npts][nctype], either
// may be NULL; at return cutd_from_tables says that no combined type has a limit and cutd_ctype is still to be filled with the
// criterion's default, which is the caller's kernel.  Points with beta = 0 are not zeroed here either.)
struct DasColumnsDiag {
  int32_t* nobs_ctype;
  double* cutd_ctype;
  bool cutd_from_tables;
};
int das_columns_impl(letkf_ctx* c, const letkf_das_args* g, const letkf_search_tables* t, int64_t nij1, int32_t nlev,
                     const double* rig, const double* rjg, const double* rlev, const double* rz, int64_t list_bytes,
                     int32_t* nobs_out, DasColumnsDiag* d);

// ---- letkf_api_efso.hip
int64_t efso_entry_bytes(int nterm);
int efso_check(letkf_ctx* c, const letkf_efso_args* g, bool lists, letkf::EfsoArgs* a);
int efso_run_slab(letkf_ctx* c, letkf::EfsoArgs a, int64_t p0, int64_t npts, const int64_t* off, const ListSlab* ls, int64_t e0,
                  int64_t e1);

}  // namespace letkf::api
