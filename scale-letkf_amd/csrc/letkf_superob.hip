// letkf_superob.hip -- superob on the device (include/letkf_amd_superob.h; scale/obs/superob.f90 and superob_tools.f90 of the
// reference, restated for SCALE's regional grid).  Sort and segmented reduce over nobs-sized buffers; nothing is sized by the
// number of cells and nothing is read back.
//
//   stage 1   superob_row_kernel       one lane per row: qc, i / j / k, uid, slot, record heads by comparison with the row before
//   stage 2   rocprim max-scan of the head positions -> the record of every row; superob_reckey_kernel: key = record * (nlevx+1)
//             + k for the qc-0 rows of records of >= 2 rows; stable radix_sort_pairs (key, row); superob_select_kernel<true>
//   stage 3   five stable radix_sort_pairs passes order the candidate rows by (cell, lon, lat, lev, priority, row);
//             superob_tflag_kernel flags every row that is not the first of its class -- linear in the size of a cell
//   stage 4   superob_cellkey_kernel: key = (slot, typ, uid, k, j, i); stable radix_sort_pairs; superob_outcnt_kernel and a scan
//             give every output row its position; superob_select_kernel<false> writes the output; superob_finish_kernel
//
// superob_select_kernel is the one segmented select / average kernel of both stages: one lane per outer segment (a record, a
// cell) walks the segment's rows in sorted order, so every mean is the sequential sum of the reference, in list order.  A wave
// per segment would leave 63 lanes idle on the 2-3 rows of a typical radar cell and would still have to add in order; a lane
// per segment costs a long cell its length in one lane, linear and without a limit on it.
// Built with -ffp-contract=off: dx*dx + dy*dy + dz*dz and the sums are rounded term by term.

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include "letkf_device.h"
#include "letkf_superob_dev.h"

namespace letkf {
namespace {

constexpr int kBlock = 256;
enum { C_BD = 0, C_G, C_TP, C_V, C_T, C_H, C_QC6, C_N };
// The counters and print_obsnum's tables are kept in kReplicas copies, one per block modulo kReplicas, and summed at the end: a
// volume scan is one type and two elements, and 2^18 waves adding to the same two words took 3 ms of a kernel that reads for 0.3.
constexpr int kReplicas = 64;

struct Ws {
  SuperobRows w;                      // the rows after stage 2 (the caller's own where no method_v is > 0)
  int32_t *ii, *jj, *kk, *qc, *rs, *c32;
  uint8_t *uidx, *slt, *tfl;
  unsigned long long *kA, *kB;
  uint32_t *vA, *vB;
  int64_t *pos, *cnt;                 // cnt: kReplicas x (C_N + 1 counters | 4 x nid x nobtype of obsnum)
  int64_t cstride;
  char* temp;
  size_t temp_bytes, total;
};

// adds 1 to tab[bin] for every lane whose bin is >= 0: one atomic per distinct bin of the wave (the bench's 2^24 rows are one
// type and two elements).  Every lane of the wave calls it.
__device__ inline void hist_add(int64_t* tab, int bin) {
  unsigned long long todo = __ballot(bin >= 0);
  while (todo) {
    const int leader = __ffsll((long long)todo) - 1;
    const int b = __shfl(bin, leader);
    const unsigned long long same = __ballot(bin == b);
    if ((int)__lane_id() == leader) atomicAdd(reinterpret_cast<unsigned long long*>(tab + b), (unsigned long long)__popcll(same));
    todo &= ~same;
  }
}

__device__ inline int64_t* counters(const Ws& w) { return w.cnt + (blockIdx.x % kReplicas) * w.cstride; }
__device__ inline int64_t* obsnum_of(const Ws& w, int point, int nb) { return counters(w) + C_N + 1 + (int64_t)point * nb; }

__device__ inline int uid_of(const SuperobArgs& a, int elm) {
  for (int u = 0; u < a.nid; ++u)
    if (a.elem_uid[u] == elm) return u + 1;
  return 0;
}

__device__ inline bool coord_ok(double r) { return fabs(r) < 1073741824.0; }   // (false for NaN and inf)

__global__ void __launch_bounds__(kBlock) superob_row_kernel(const SuperobArgs a, const Ws w) {
  const int64_t n = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  const bool live = n < a.n;
  int cbin = -1, obin = -1;
  if (live) {
    int s = 0;
    while (a.slot_off[s + 1] <= n) ++s;
    const int elm = a.elm[n], typ = a.typ[n], uid = uid_of(a, elm);
    const bool valid = uid > 0 && typ >= 1 && typ <= a.nobtype;
    const int mb = valid ? a.meth[(uid - 1) * a.nobtype + typ - 1] : 0;
    const double ri = a.in.ri[n], rj = a.in.rj[n], rk = a.in.rk[n], lon = a.in.lon[n], lat = a.in.lat[n];
    int qc = 0, i = 0, j = 0, k = 0;
    if (!(coord_ok(ri) && coord_ok(rj) && coord_ok(rk))) {
      qc = 6;
    } else {
      i = (int)floor(ri + 0.5), j = (int)floor(rj + 0.5), k = (int)floor(rk + 0.5);
      const bool surface = typ >= 1 && typ <= 32 && ((a.surf_mask >> (typ - 1)) & 1u);
      if (surface || elm > 9999) {
        k = 0;
      } else {
        if (k < 1) k = 1;
        if (ceil(rk) > (double)a.nlevx) qc = 3;
      }
      if (qc == 0 && (ceil(rj) < 2.0 || ceil(rj) > (double)a.nlat)) qc = 2;
      if (qc == 0 && (ceil(ri) < 2.0 || ceil(ri) > (double)a.nlon)) qc = 2;
      if (qc == 0 && valid && (mb & 1)) qc = 4;
      if (qc == 0 && !valid) qc = 5;
    }
    w.ii[n] = i, w.jj[n] = j, w.kk[n] = k, w.qc[n] = qc;
    w.uidx[n] = (uint8_t)uid, w.slt[n] = (uint8_t)s;
    cbin = qc == 2 || qc == 3 ? C_BD : qc == 4 ? C_G : qc == 5 ? C_TP : qc == 6 ? C_QC6 : -1;
    if (valid) obin = (uid - 1) * a.nobtype + typ - 1;
    if (a.any_v) {
      bool head = n == a.slot_off[s] || ((mb >> 1) & 3) == 0;
      if (!head)
        head = !(lon == a.in.lon[n - 1] && lat == a.in.lat[n - 1] && typ == a.typ[n - 1] && uid == uid_of(a, a.elm[n - 1]));
      w.c32[n] = head ? (int32_t)n : -1;
      w.w.lon[n] = lon, w.w.lat[n] = lat, w.w.lev[n] = a.in.lev[n], w.w.dat[n] = a.in.dat[n], w.w.err[n] = a.in.err[n];
      w.w.ri[n] = ri, w.w.rj[n] = rj, w.w.rk[n] = rk;
    }
  }
  hist_add(counters(w), cbin);
  hist_add(obsnum_of(w, 0, a.nid * a.nobtype), obin);
}

// stage 2: rs[n] is the head of the record that row n is in.  The rows of a record of >= 2 rows get qc 9; those that were at 0
// go into the sort under (record, k).
__global__ void __launch_bounds__(kBlock) superob_reckey_kernel(const SuperobArgs a, const Ws w, unsigned long long sentinel) {
  const int64_t n = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  const bool live = n < a.n;
  int cbin = -1;
  if (live) {
    const int64_t rs = w.rs[n];
    const bool multi = rs != n || (n + 1 < a.n && w.c32[n + 1] < 0);
    unsigned long long key = sentinel;
    if (multi) {
      if (w.qc[n] == 0) key = (unsigned long long)rs * (unsigned long long)(a.nlevx + 1) + (unsigned long long)w.kk[n];
      w.qc[n] = 9;
      cbin = C_V;
    }
    w.kA[n] = key, w.vA[n] = (uint32_t)n;
  }
  hist_add(counters(w), cbin);
}

struct Sel {
  double lon, lat, lev, dat, err, ri, rj, rk;
};

__device__ inline Sel load_row(const SuperobRows& s, int64_t r) {
  return Sel{s.lon[r], s.lat[r], s.lev[r], s.dat[r], s.err[r], s.ri[r], s.rj[r], s.rk[r]};
}
__device__ inline void store_row(const SuperobRows& d, int64_t r, const Sel& v) {
  d.lon[r] = v.lon, d.lat[r] = v.lat, d.lev[r] = v.lev, d.dat[r] = v.dat, d.err[r] = v.err, d.ri[r] = v.ri, d.rj[r] = v.rj, d.rk[r] = v.rk;
}

// superob_select (superob_tools.f90:21-140) over the rows rows[q .. e) of s, in that order; method 1..3, e - q >= 1
__device__ inline Sel superob_select(const SuperobRows& s, const uint32_t* rows, int64_t q, int64_t e, int ci, int cj, int ck, int method) {
  if (e - q == 1) return load_row(s, rows[q]);
  const double big = (double)1.e20f;
  double err_min = big;
  for (int64_t p = q; p < e; ++p) {
    const double er = s.err[rows[p]];
    if (er < err_min) err_min = er;
  }
  if (method == 1) {
    double dist_min = big;
    int64_t best = -1;
    for (int64_t p = q; p < e; ++p) {
      const int64_t r = rows[p];
      if (!(s.err[r] == err_min)) continue;
      const double dx = s.ri[r] - (double)ci, dy = s.rj[r] - (double)cj;
      double d2 = dx * dx + dy * dy;
      if (ck != 0) {
        const double dz = s.rk[r] - (double)ck;
        d2 = d2 + dz * dz;
      }
      const double dist = sqrt(d2);
      if (dist < dist_min) best = r, dist_min = dist;
    }
    return load_row(s, best < 0 ? (int64_t)rows[q] : best);   // (n_use == 0: the group's first row)
  }
  double ai = 0.0, aj = 0.0, ak = 0.0, alon = 0.0, alat = 0.0, alev = 0.0, adat = 0.0;
  int64_t n_use = 0, last = rows[q];
  for (int64_t p = q; p < e; ++p) {
    const int64_t r = rows[p];
    if (method == 3 && !(s.err[r] == err_min)) continue;
    ai = ai + s.ri[r], aj = aj + s.rj[r], ak = ak + s.rk[r], alon = alon + s.lon[r], alat = alat + s.lat[r];
    alev = alev + s.lev[r], adat = adat + s.dat[r];
    ++n_use, last = r;
  }
  if (n_use <= 1) return load_row(s, last);                   // (1: that row itself; 0: the group's first row)
  const double d = (double)n_use;
  return Sel{alon / d, alat / d, alev / d, adat / d, err_min, ai / d, aj / d, ak / d};
}

// The segmented select / average of stage 2 (REC) and stage 4 (!REC) over the sorted (keys, rows).
//   REC:  outer segment = a record (key / nk), inner groups = its k (key % nk); group number g of the record goes to position
//         record + g of the stage-2 rows w.w, with k and qc 0.  Reads the caller's rows, which stage 2 does not touch.
//   !REC: outer = inner = a cell with method_h > 0, written at pos[p] of the output with the cell's i, j, k; a row with
//         method_h == 0 is copied by its own lane.
template <bool REC>
__global__ void __launch_bounds__(kBlock) superob_select_kernel(const SuperobArgs a, const Ws w, const unsigned long long* keys,
                                                                const uint32_t* rows, unsigned long long sentinel) {
  const int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  const unsigned long long nk = (unsigned long long)(a.nlevx + 1);
  int obin = -1;
  unsigned long long key = sentinel;
  if (p < a.n) key = keys[p];
  if (key != sentinel) {
    const int64_t r0 = rows[p];
    if (REC) {
      const unsigned long long rec = key / nk;
      if (p == 0 || keys[p - 1] / nk != rec) {
        const int method = (a.meth[(w.uidx[rec] - 1) * a.nobtype + a.typ[rec] - 1] >> 1) & 3;
        const int ci = w.ii[rec], cj = w.jj[rec];
        int64_t q = p, g = 0, outside = 0;
        while (q < a.n && keys[q] != sentinel && keys[q] / nk == rec) {
          const unsigned long long kq = keys[q];
          int64_t e = q + 1;
          while (e < a.n && keys[e] == kq) ++e;
          const int k = (int)(kq % nk);
          store_row(w.w, (int64_t)rec + g, superob_select(a.in, rows, q, e, ci, cj, k, method));
          // (the position keeps its own i, j: where they lie outside the grid the reference indexes nobsgrd out of bounds; qc 2)
          const int pi = w.ii[rec + g], pj = w.jj[rec + g];
          const bool inside = pi >= 1 && pi <= a.nlon && pj >= 1 && pj <= a.nlat;
          w.kk[rec + g] = k, w.qc[rec + g] = inside ? 0 : 2;
          outside += !inside;
          ++g, q = e;
        }
        atomicAdd(reinterpret_cast<unsigned long long*>(counters(w) + C_V), (unsigned long long)(-g));
        if (outside) atomicAdd(reinterpret_cast<unsigned long long*>(counters(w) + C_BD), (unsigned long long)outside);
      }
    } else {
      const int uid = w.uidx[r0], typ = a.typ[r0];
      const int method = (a.meth[(uid - 1) * a.nobtype + typ - 1] >> 5) & 3;
      if (method == 0 || p == 0 || keys[p - 1] != key) {
        int64_t e = p + 1;
        if (method != 0)
          while (e < a.n && keys[e] == key) ++e;
        const int ci = w.ii[r0], cj = w.jj[r0], ck = w.kk[r0];
        const Sel v = superob_select(w.w, rows, p, e, ci, cj, ck, method);
        const int64_t o = w.pos[p];
        const letkf_superob_out& out = a.out;
        out.elm[o] = a.elem_uid[uid - 1], out.typ[o] = typ, out.slot[o] = w.slt[r0] + 1;
        store_row(SuperobRows{out.lon, out.lat, out.lev, out.dat, out.err, out.ri, out.rj, out.rk}, o, v);
        out.i[o] = ci, out.j[o] = cj, out.k[o] = ck;
        obin = (uid - 1) * a.nobtype + typ - 1;
      }
    }
  }
  if (!REC) hist_add(obsnum_of(w, 3, a.nid * a.nobtype), obin);
}

__device__ inline unsigned long long canon_bits(double x) {
  if (x == 0.0) return 0ull;                                  // -0.0 == 0.0
  if (x != x) return 0x7ff8000000000000ull;                   // (one place for every NaN; the flag kernel never calls them equal)
  return (unsigned long long)__double_as_longlong(x);
}

__device__ inline unsigned long long cell3_key(const SuperobArgs& a, const Ws& w, int64_t r) {
  unsigned long long c = (unsigned long long)(a.typ[r] - 1) * a.nid + (w.uidx[r] - 1);
  c = c * (unsigned long long)(a.nlevx + 1) + (unsigned long long)w.kk[r];
  c = c * (unsigned long long)a.nlat + (unsigned long long)(w.jj[r] - 1);
  return c * (unsigned long long)a.nlon + (unsigned long long)(w.ii[r] - 1);
}

// stage 3's keys, one pass of the least-significant-first order at a time: 0 the slot's priority (from row order; sets the
// flag to 0, or to 2 under method 2 off the first-priority slot), 1 lev, 2 lat, 3 lon, 4 the cell (typ, uid, k, j, i) or, for a
// row that is no candidate, the sentinel
__global__ void __launch_bounds__(kBlock) superob_tkey_kernel(const SuperobArgs a, const Ws w, int pass, const uint32_t* rows,
                                                              unsigned long long* keys, uint32_t* rows0, unsigned long long sentinel) {
  const int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  int cbin = -1;
  if (p < a.n) {
    const int64_t r = pass == 0 ? p : (int64_t)rows[p];
    unsigned long long key = 0;
    if (pass == 1) key = canon_bits(w.w.lev[r]);
    else if (pass == 2) key = canon_bits(w.w.lat[r]);
    else if (pass == 3) key = canon_bits(w.w.lon[r]);
    else {
      const int uid = w.uidx[r], typ = a.typ[r];
      const int mt = w.qc[r] == 0 ? (a.meth[(uid - 1) * a.nobtype + typ - 1] >> 3) & 3 : 0;   // (qc 0: uid and typ are valid)
      const int pr = a.prio[w.slt[r]];
      const bool off = mt == 2 && pr > 0;
      if (pass == 0) {
        key = (unsigned long long)pr;
        rows0[p] = (uint32_t)p;
        w.tfl[p] = off ? 2 : 0;
        if (off) cbin = C_T;
      } else {
        key = mt > 0 && !off ? cell3_key(a, w, r) : sentinel;
      }
    }
    keys[p] = key;
  }
  if (pass == 0) hist_add(counters(w), cbin);
}

__global__ void __launch_bounds__(kBlock) superob_tflag_kernel(const SuperobArgs a, const Ws w, const unsigned long long* keys,
                                                               const uint32_t* rows, unsigned long long sentinel) {
  const int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  int cbin = -1;
  if (p > 0 && p < a.n && keys[p] != sentinel && keys[p - 1] == keys[p]) {
    const int64_t r = rows[p], b = rows[p - 1];
    if (w.w.lon[r] == w.w.lon[b] && w.w.lat[r] == w.w.lat[b] && w.w.lev[r] == w.w.lev[b]) w.tfl[r] = 1, cbin = C_T;
  }
  hist_add(counters(w), cbin);
}

__global__ void __launch_bounds__(kBlock) superob_cellkey_kernel(const SuperobArgs a, const Ws w, unsigned long long cells3,
                                                                 unsigned long long sentinel) {
  const int64_t n = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  int b1 = -1, b2 = -1;
  if (n < a.n) {
    unsigned long long key = sentinel;
    if (w.qc[n] == 0) {
      b1 = (w.uidx[n] - 1) * a.nobtype + a.typ[n] - 1;
      if (!a.any_t || w.tfl[n] == 0) {
        b2 = b1;
        key = (unsigned long long)w.slt[n] * cells3 + cell3_key(a, w, n);
      }
    }
    w.kA[n] = key, w.vA[n] = (uint32_t)n;
  }
  const int nb = a.nid * a.nobtype;
  hist_add(obsnum_of(w, 1, nb), b1);
  hist_add(obsnum_of(w, 2, nb), b2);
  hist_add(counters(w), b2 >= 0 ? C_H : -1);
}

// rows that position p of the sorted order puts out: a whole cell's one under method_h > 0, its own under method_h == 0
__global__ void __launch_bounds__(kBlock) superob_outcnt_kernel(const SuperobArgs a, const Ws w, const unsigned long long* keys,
                                                                const uint32_t* rows, unsigned long long sentinel) {
  const int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (p > a.n) return;
  int c = 0;
  if (p < a.n && keys[p] != sentinel) {
    const int64_t r = rows[p];
    const int method = (a.meth[(w.uidx[r] - 1) * a.nobtype + a.typ[r] - 1] >> 5) & 3;
    c = method == 0 || p == 0 || keys[p - 1] != keys[p];
  }
  w.c32[p] = c;
}

// nout, nobsrdc_h, the slots' offsets in the output (a binary search for each slot's first key) and the optional tables
__global__ void __launch_bounds__(kBlock) superob_finish_kernel(const SuperobArgs a, const Ws w, const unsigned long long* keys,
                                                                unsigned long long cells3) {
  const int t = threadIdx.x;
  const int64_t nout = a.n > 0 ? w.pos[a.n] : 0;
  if (t == 0) a.out.nout[0] = nout;
  if (a.out.slot_off_out && t <= a.nslots) {
    const unsigned long long first = (unsigned long long)t * cells3;
    int64_t lo = 0, hi = a.n;
    while (lo < hi) {
      const int64_t mid = lo + (hi - lo) / 2;
      if (keys[mid] < first) lo = mid + 1;
      else hi = mid;
    }
    a.out.slot_off_out[t] = a.n > 0 ? w.pos[lo] : 0;
  }
  auto total = [&](int b) {
    int64_t sum = 0;
    for (int r = 0; r < kReplicas; ++r) sum += w.cnt[r * w.cstride + b];
    return sum;
  };
  if (a.out.counts && t < C_N) a.out.counts[t] = total(t) - (t == C_H ? nout : 0);
  if (a.out.obsnum)
    for (int b = t; b < 4 * a.nid * a.nobtype; b += kBlock) a.out.obsnum[b] = total(C_N + 1 + b);
}

__global__ void __launch_bounds__(kBlock) superob_copy_qc_kernel(int64_t n, const int32_t* src, int32_t* dst) {
  const int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (p < n) dst[p] = src[p];
}

int bit_length(unsigned long long v) {
  int b = 0;
  while (v) ++b, v >>= 1;
  return b > 0 ? b : 1;
}

hipError_t sort_pairs(const Ws& w, const unsigned long long* kin, unsigned long long* kout, const uint32_t* vin, uint32_t* vout,
                      size_t n, int end_bit, hipStream_t st) {
  size_t bytes = w.temp_bytes;
  return rocprim::radix_sort_pairs(w.temp, bytes, kin, kout, vin, vout, n, 0u, (unsigned)end_bit, st);
}

// the workspace of a call, carved from base (nullptr: only the size)
hipError_t carve(const SuperobArgs& a, hipStream_t st, char* base, Ws* w) {
  const size_t n = (size_t)(a.n > 0 ? a.n : 1);
  size_t off = 0;
  auto take = [&](size_t bytes) {
    char* p = base + off;
    off += (bytes + 255) & ~(size_t)255;
    return p;
  };
  if (a.any_v) {
    double** d[8] = {&w->w.lon, &w->w.lat, &w->w.lev, &w->w.dat, &w->w.err, &w->w.ri, &w->w.rj, &w->w.rk};
    for (auto f : d) *f = reinterpret_cast<double*>(take(n * 8));
  } else {
    w->w = a.in;
  }
  int32_t** i4[6] = {&w->ii, &w->jj, &w->kk, &w->qc, &w->rs, &w->c32};
  for (auto f : i4) *f = reinterpret_cast<int32_t*>(take((n + 1) * 4));
  uint8_t** i1[3] = {&w->uidx, &w->slt, &w->tfl};
  for (auto f : i1) *f = reinterpret_cast<uint8_t*>(take(n));
  w->kA = reinterpret_cast<unsigned long long*>(take(n * 8));
  w->kB = reinterpret_cast<unsigned long long*>(take(n * 8));
  w->vA = reinterpret_cast<uint32_t*>(take(n * 4));
  w->vB = reinterpret_cast<uint32_t*>(take(n * 4));
  w->pos = reinterpret_cast<int64_t*>(take((n + 1) * 8));
  w->cstride = C_N + 1 + 4 * (int64_t)a.nid * a.nobtype;
  w->cnt = reinterpret_cast<int64_t*>(take((size_t)kReplicas * w->cstride * 8));
  size_t t_sort = 0, t_max = 0, t_sum = 0;
  hipError_t e = hipSuccess;
  for (unsigned bits : {6u, 32u, 64u}) {       // (every sort of superob_run: the scratch of none is larger than one of these)
    size_t t = 0;
    e = rocprim::radix_sort_pairs(nullptr, t, (const unsigned long long*)nullptr, (unsigned long long*)nullptr,
                                  (const uint32_t*)nullptr, (uint32_t*)nullptr, n, 0u, bits, st);
    if (e != hipSuccess) return e;
    if (t > t_sort) t_sort = t;
  }
  e = rocprim::inclusive_scan(nullptr, t_max, (const int32_t*)nullptr, (int32_t*)nullptr, n, rocprim::maximum<int32_t>(), st);
  if (e != hipSuccess) return e;
  if ((e = count_scan(nullptr, &t_sum, nullptr, nullptr, n + 1, st)) != hipSuccess) return e;
  w->temp_bytes = t_sort > t_max ? t_sort : t_max;
  if (t_sum > w->temp_bytes) w->temp_bytes = t_sum;
  w->temp = take(w->temp_bytes);
  w->total = off + 256;
  return hipSuccess;
}

}  // namespace

size_t superob_ws_bytes(const SuperobArgs& a, hipStream_t st) {
  Ws w = {};
  return carve(a, st, nullptr, &w) == hipSuccess ? w.total : 0;
}

hipError_t superob_run(hipStream_t st, const SuperobArgs& a, void* ws) {
  Ws w = {};
  hipError_t e = carve(a, st, static_cast<char*>(ws), &w);
  if (e != hipSuccess) return e;
  if ((e = hipMemsetAsync(w.cnt, 0, (size_t)kReplicas * w.cstride * 8, st)) != hipSuccess) return e;
  const size_t n = (size_t)a.n;
  const unsigned long long nk = (unsigned long long)(a.nlevx + 1);
  const unsigned long long cells3 = (unsigned long long)a.nobtype * a.nid * nk * (unsigned long long)a.nlat * (unsigned long long)a.nlon;
  const unsigned long long sent4 = cells3 * (unsigned long long)a.nslots;
  const dim3 grid((unsigned)((a.n + kBlock - 1) / kBlock)), grid1((unsigned)((a.n + kBlock) / kBlock)), block(kBlock);
#define LAUNCH(k, g, ...)                                 \
  hipLaunchKernelGGL(k, g, block, 0, st, __VA_ARGS__);    \
  if ((e = hipGetLastError()) != hipSuccess) return e
  if (a.n > 0) {
    LAUNCH(superob_row_kernel, grid, a, w);
    if (a.any_v) {
      size_t bytes = w.temp_bytes;
      if ((e = rocprim::inclusive_scan(w.temp, bytes, w.c32, w.rs, n, rocprim::maximum<int32_t>(), st)) != hipSuccess) return e;
      const unsigned long long sent2 = (unsigned long long)a.n * nk;
      LAUNCH(superob_reckey_kernel, grid, a, w, sent2);
      if ((e = sort_pairs(w, w.kA, w.kB, w.vA, w.vB, n, bit_length(sent2), st)) != hipSuccess) return e;
      LAUNCH(superob_select_kernel<true>, grid, a, w, w.kB, w.vB, sent2);
    }
    if (a.any_t) {
      unsigned long long *kin = w.kA, *kout = w.kB;
      uint32_t *vin = w.vA, *vout = w.vB;
      for (int pass = 0; pass < 5; ++pass) {
        LAUNCH(superob_tkey_kernel, grid, a, w, pass, vin, kin, vin, cells3);
        const int bits = pass == 0 ? 6 : pass == 4 ? bit_length(cells3) : 64;
        if ((e = sort_pairs(w, kin, kout, vin, vout, n, bits, st)) != hipSuccess) return e;
        std::swap(kin, kout), std::swap(vin, vout);
      }
      LAUNCH(superob_tflag_kernel, grid, a, w, kin, vin, cells3);
    }
    LAUNCH(superob_cellkey_kernel, grid, a, w, cells3, sent4);
    if ((e = sort_pairs(w, w.kA, w.kB, w.vA, w.vB, n, bit_length(sent4), st)) != hipSuccess) return e;
    LAUNCH(superob_outcnt_kernel, grid1, a, w, w.kB, w.vB, sent4);
    size_t bytes = w.temp_bytes;
    if ((e = count_scan(w.temp, &bytes, w.c32, w.pos, n + 1, st)) != hipSuccess) return e;
    LAUNCH(superob_select_kernel<false>, grid, a, w, w.kB, w.vB, sent4);
    if (a.out.qc1) { LAUNCH(superob_copy_qc_kernel, grid, a.n, w.qc, a.out.qc1); }
  }
  LAUNCH(superob_finish_kernel, dim3(1), a, w, w.kB, cells3);
#undef LAUNCH
  return hipSuccess;
}

}  // namespace letkf
