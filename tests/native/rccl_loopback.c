/* rccl_loopback.c -- a loop-back stand-in for RCCL (test infrastructure only; tests/_loopback.py builds and drives it).
 *
 * Loaded RTLD_GLOBAL into a fresh process before libletkf_amd.so makes its first exchange call, it is what the library's
 * run-time binding (csrc/letkf_exchange.hip bind_rccl: dlsym on the process image first) finds as ncclSend / ncclRecv /
 * ncclGroupStart / ncclGroupEnd / ncclAllReduce / ncclGetErrorString.  R simulated ranks live in ONE process and are
 * called one after the other; a "communicator" is a pointer to an lb_comm {magic, world, rank, nranks}.
 *
 *   ncclSend   copies the bytes device-to-device, ordered on the caller's stream, into the mailbox slot [rank][peer]
 *              (stand-in-owned device memory, grown on demand) and logs (src, dst, bytes, group depth, group, call)
 *   ncclRecv   slot [peer][rank] holds a message: its size must equal the posted size (else a non-zero result and the
 *              mismatch counter), and it is copied out on the stream; the slot is empty: the unmatched counter, nothing
 *              is written.  It never waits -- there is no waiting primitive of any kind in this file.
 *   groups     operations posted inside a group run at the outermost ncclGroupEnd, sends first, so that the order inside
 *              a group does not matter (as in RCCL) and a send to oneself is served within the group
 *   ncclAllReduce (int32, sum, in place)  deposit pass: stash the rank's input on the host, leave the buffer alone;
 *              deliver pass: write the sum of the stashes of all nranks ranks
 *
 * Two passes: the driver calls an entry for every rank in turn (deposit: receives from ranks that have not run yet are
 * unmatched, as expected), calls lb_deliver() -- counters and log restart, slots and stashes stay -- refills the outputs
 * and calls the entry for every rank again; that second pass is complete and is the one that is checked.
 *
 * The HIP runtime is the one the process already carries: found among the loaded objects (dl_iterate_phdr) and opened
 * with RTLD_NOLOAD; nothing is linked and no second runtime is brought in.  lb_bind_hip() != 0 says it was not found. */
#define _GNU_SOURCE
#include <dlfcn.h>
#include <link.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#define LB_MAGIC 0x4c42434f4d4d3031ull /* "LBCOMM01" */
#define LB_MAXR 16
#define LB_MAXQ 256
#define LB_MAXLOG 65536

typedef struct {
  uint64_t magic;
  int32_t world, rank, nranks, reserved;
} lb_comm;

typedef struct {
  void *dev;
  size_t cap, bytes;
  int full;
  long call; /* the entry call that wrote it last */
} lb_slot;

typedef struct {
  int kind; /* 0 send, 1 recv */
  int src, dst;
  void *p;
  size_t n;
  void *st;
} lb_op;

enum { C_SENDS, C_RECVS, C_SEND_BYTES, C_RECV_BYTES, C_GROUPS, C_UNMATCHED, C_MISMATCH, C_UNGROUPED, C_OVERWRITES,
       C_ALLREDUCES, C_BAD_COMM, C_HIP_ERRORS, C_LOG_DROPPED, C_N };

static lb_comm g_comm[LB_MAXR];
static lb_slot g_slot[LB_MAXR][LB_MAXR];
static int32_t *g_stash[LB_MAXR];
static size_t g_stash_n[LB_MAXR];
static int g_stash_full[LB_MAXR];
static int g_world = 0, g_nranks = 0, g_deliver = 0, g_depth = 0;
static long g_group = 0, g_call = 0;
static int64_t g_cnt[C_N];
static lb_op g_q[LB_MAXQ];
static int g_nq = 0;
static int64_t (*g_log)[7] = NULL; /* kind, src, dst, bytes, depth, group, call */
static long g_nlog = 0;
static char g_err[512] = "";

/* ---- the process's own HIP runtime */
typedef int (*hip_malloc_fn)(void **, size_t);
typedef int (*hip_free_fn)(void *);
typedef int (*hip_memcpy_async_fn)(void *, const void *, size_t, int, void *);
typedef int (*hip_stream_sync_fn)(void *);
static hip_malloc_fn p_malloc;
static hip_free_fn p_free;
static hip_memcpy_async_fn p_copy;
static hip_stream_sync_fn p_sync;
static int g_hip = 0; /* 0 not tried, 1 bound, -1 failed */
static char g_hip_path[4096] = "";
enum { H2D = 1, D2H = 2, D2D = 3 };

static int find_hip(struct dl_phdr_info *info, size_t size, void *data) {
  (void)size;
  (void)data;
  if (info->dlpi_name && strstr(info->dlpi_name, "libamdhip64")) {
    snprintf(g_hip_path, sizeof g_hip_path, "%s", info->dlpi_name);
    return 1;
  }
  return 0;
}

int lb_bind_hip(void) {
  if (g_hip) return g_hip > 0 ? 0 : -1;
  g_hip = -1;
  if (!dl_iterate_phdr(find_hip, NULL)) {
    snprintf(g_err, sizeof g_err, "no HIP runtime (libamdhip64) among the objects this process has loaded");
    return -1;
  }
  void *h = dlopen(g_hip_path, RTLD_NOW | RTLD_NOLOAD);
  if (!h) {
    snprintf(g_err, sizeof g_err, "%.300s is listed as loaded but RTLD_NOLOAD did not return it: %.100s", g_hip_path, dlerror());
    return -1;
  }
  p_malloc = (hip_malloc_fn)dlsym(h, "hipMalloc");
  p_free = (hip_free_fn)dlsym(h, "hipFree");
  p_copy = (hip_memcpy_async_fn)dlsym(h, "hipMemcpyAsync");
  p_sync = (hip_stream_sync_fn)dlsym(h, "hipStreamSynchronize");
  if (!p_malloc || !p_free || !p_copy || !p_sync) {
    snprintf(g_err, sizeof g_err, "%.300s lacks hipMalloc / hipFree / hipMemcpyAsync / hipStreamSynchronize", g_hip_path);
    return -1;
  }
  g_hip = 1;
  return 0;
}
const char *lb_hip_path(void) { return g_hip_path; }
const char *lb_last_error(void) { return g_err; }

static int hip_fail(const char *what, int e) {
  ++g_cnt[C_HIP_ERRORS];
  snprintf(g_err, sizeof g_err, "%s failed with hipError_t %d", what, e);
  return 2; /* ncclSystemError */
}

/* ---- control */
static void clear_world(void) {
  for (int s = 0; s < LB_MAXR; ++s) {
    for (int d = 0; d < LB_MAXR; ++d) {
      g_slot[s][d].bytes = 0;
      g_slot[s][d].full = 0;
      g_slot[s][d].call = -1;
    }
    g_stash_full[s] = 0;
  }
}

static void clear_records(void) {
  memset(g_cnt, 0, sizeof g_cnt);
  g_nlog = 0;
  g_nq = 0;
  g_depth = 0;
}

/* a new world of nranks ranks, in the deposit pass: empty mailbox, counters and log at zero.  Returns its id, or -1. */
int lb_world_begin(int nranks) {
  if (nranks < 1 || nranks > LB_MAXR) return -1;
  if (!g_log && !(g_log = malloc(sizeof(int64_t[7]) * LB_MAXLOG))) return -1;
  ++g_world;
  g_nranks = nranks;
  g_deliver = 0;
  clear_world();
  clear_records();
  for (int r = 0; r < LB_MAXR; ++r) {
    g_comm[r].magic = r < nranks ? LB_MAGIC : 0;
    g_comm[r].world = g_world;
    g_comm[r].rank = r;
    g_comm[r].nranks = nranks;
  }
  return g_world;
}
void *lb_comm_of(int world, int rank) {
  return (world == g_world && rank >= 0 && rank < g_nranks) ? (void *)&g_comm[rank] : NULL;
}
/* deposit -> deliver: what is counted and logged from here on is the pass that is checked */
void lb_deliver(void) {
  g_deliver = 1;
  clear_records();
}
/* the driver marks the start of every entry call, so that the log says which operations and groups belong to it */
long lb_call_begin(void) { return ++g_call; }
int lb_ncounters(void) { return C_N; }
void lb_counters(int64_t *out) { memcpy(out, g_cnt, sizeof g_cnt); }
long lb_log_size(void) { return g_nlog; }
void lb_log_get(long i, int64_t *out) {
  if (i >= 0 && i < g_nlog) memcpy(out, g_log[i], sizeof g_log[i]);
}

static void log_op(int kind, int src, int dst, size_t n) {
  if (g_nlog >= LB_MAXLOG) {
    ++g_cnt[C_LOG_DROPPED];
    return;
  }
  int64_t *e = g_log[g_nlog++];
  e[0] = kind, e[1] = src, e[2] = dst, e[3] = (int64_t)n, e[4] = g_depth, e[5] = g_group, e[6] = g_call;
}

static lb_comm *comm_of(void *c) {
  lb_comm *k = (lb_comm *)c;
  if (!k || k < g_comm || k >= g_comm + LB_MAXR || k->magic != LB_MAGIC || k->world != g_world) {
    ++g_cnt[C_BAD_COMM];
    snprintf(g_err, sizeof g_err, "a communicator that is not a live loop-back handle reached the stand-in");
    return NULL;
  }
  return k;
}

/* ---- the operations themselves */
static int do_send(const lb_op *o) {
  lb_slot *s = &g_slot[o->src][o->dst];
  if (s->call == g_call && s->full) ++g_cnt[C_OVERWRITES];
  if (s->cap < o->n) {
    int e;
    if (s->dev && (e = p_free(s->dev))) return hip_fail("hipFree", e);
    s->dev = NULL, s->cap = 0;
    if ((e = p_malloc(&s->dev, o->n))) return hip_fail("hipMalloc", e);
    s->cap = o->n;
  }
  if (o->n) {
    const int e = p_copy(s->dev, o->p, o->n, D2D, o->st);
    if (e) return hip_fail("hipMemcpyAsync (send)", e);
  }
  s->bytes = o->n, s->full = 1, s->call = g_call;
  return 0;
}

static int do_recv(const lb_op *o) {
  lb_slot *s = &g_slot[o->src][o->dst];
  if (!s->full) {
    ++g_cnt[C_UNMATCHED];
    return 0;
  }
  if (s->bytes != o->n) return 0; /* counted and reported when it was posted, or below */
  if (o->n) {
    const int e = p_copy(o->p, s->dev, o->n, D2D, o->st);
    if (e) return hip_fail("hipMemcpyAsync (recv)", e);
  }
  return 0;
}

static int post(int kind, int src, int dst, void *p, size_t n, void *st) {
  if (lb_bind_hip()) return 2;
  log_op(kind, src, dst, n);
  if (kind == 0) ++g_cnt[C_SENDS], g_cnt[C_SEND_BYTES] += (int64_t)n;
  else ++g_cnt[C_RECVS], g_cnt[C_RECV_BYTES] += (int64_t)n;
  if (kind == 1) { /* the size of the message this receive will meet: a send queued in this group, else the slot */
    long have = -1;
    for (int i = 0; i < g_nq; ++i)
      if (g_q[i].kind == 0 && g_q[i].src == src && g_q[i].dst == dst) have = (long)g_q[i].n;
    if (have < 0 && g_slot[src][dst].full) have = (long)g_slot[src][dst].bytes;
    if (have >= 0 && (size_t)have != n) {
      ++g_cnt[C_MISMATCH];
      snprintf(g_err, sizeof g_err, "rank %d posted a receive of %zu bytes from rank %d, which sent %ld", dst, n, src, have);
      return 4; /* ncclInvalidArgument */
    }
  }
  lb_op o = {kind, src, dst, p, n, st};
  if (g_depth == 0) {
    ++g_cnt[C_UNGROUPED];
    return kind == 0 ? do_send(&o) : do_recv(&o);
  }
  if (g_nq >= LB_MAXQ) {
    snprintf(g_err, sizeof g_err, "more than %d operations in one group", LB_MAXQ);
    return 3; /* ncclInternalError */
  }
  g_q[g_nq++] = o;
  return 0;
}

int ncclGroupStart(void) {
  if (g_depth++ == 0) {
    ++g_group;
    ++g_cnt[C_GROUPS];
    g_nq = 0;
  }
  return 0;
}

int ncclGroupEnd(void) {
  if (g_depth <= 0) return 4;
  if (--g_depth > 0) return 0;
  int rc = 0;
  for (int kind = 0; kind <= 1; ++kind)
    for (int i = 0; i < g_nq; ++i)
      if (g_q[i].kind == kind) {
        const int e = kind == 0 ? do_send(&g_q[i]) : do_recv(&g_q[i]);
        if (e && !rc) rc = e;
      }
  g_nq = 0;
  return rc;
}

int ncclSend(const void *p, size_t n, int dt, int peer, void *comm, void *st) {
  lb_comm *k = comm_of(comm);
  if (!k || dt != 0 || peer < 0 || peer >= k->nranks) return 4;
  return post(0, k->rank, peer, (void *)p, n, st);
}

int ncclRecv(void *p, size_t n, int dt, int peer, void *comm, void *st) {
  lb_comm *k = comm_of(comm);
  if (!k || dt != 0 || peer < 0 || peer >= k->nranks) return 4;
  return post(1, peer, k->rank, p, n, st);
}

int ncclAllReduce(const void *s, void *r, size_t n, int dt, int op, void *comm, void *st) {
  lb_comm *k = comm_of(comm);
  if (!k || dt != 2 || op != 0 || s != r) return 4; /* ncclInt32, ncclSum, in place: all the library asks for */
  if (lb_bind_hip()) return 2;
  ++g_cnt[C_ALLREDUCES];
  const int me = k->rank;
  int e;
  if (g_stash_n[me] < n || !g_stash[me]) {
    free(g_stash[me]);
    g_stash[me] = malloc((n ? n : 1) * sizeof(int32_t));
    g_stash_n[me] = n;
    if (!g_stash[me]) return 3;
  }
  g_stash_n[me] = n;
  if ((e = p_copy(g_stash[me], s, n * sizeof(int32_t), D2H, st))) return hip_fail("hipMemcpyAsync (all-reduce in)", e);
  if ((e = p_sync(st))) return hip_fail("hipStreamSynchronize", e);
  g_stash_full[me] = 1;
  if (!g_deliver) return 0;
  int32_t *sum = calloc(n ? n : 1, sizeof(int32_t));
  if (!sum) return 3;
  int rc = 0;
  for (int q = 0; q < k->nranks && !rc; ++q) {
    if (!g_stash_full[q]) {
      ++g_cnt[C_UNMATCHED];
      rc = 4;
    } else if (g_stash_n[q] != n) {
      ++g_cnt[C_MISMATCH];
      rc = 4;
    } else
      for (size_t i = 0; i < n; ++i) sum[i] = (int32_t)((uint32_t)sum[i] + (uint32_t)g_stash[q][i]);
  }
  if (!rc) {
    if ((e = p_copy(r, sum, n * sizeof(int32_t), H2D, st))) rc = hip_fail("hipMemcpyAsync (all-reduce out)", e);
    else if ((e = p_sync(st))) rc = hip_fail("hipStreamSynchronize", e);
  }
  free(sum);
  return rc;
}

const char *ncclGetErrorString(int rc) {
  (void)rc;
  return g_err[0] ? g_err : "loop-back stand-in error";
}
