// letkf_wave_dev.h -- the wavefront-per-grid-point LETKF kernel for k <= 62, two wavefronts for 65 <= k <= 100 (gfx950):
// constants, slice sizing, warm-start products, the kernel template and its launcher.  Included by the two units that
// instantiate it: letkf_wave.hip (one wave per point) and letkf_wave2.hip (two waves per point, flags of its own).
//
// One 64-lane wavefront solves one grid point; the 4 waves of a workgroup are fully independent (no workgroup
// barrier anywhere), so a CU keeps 8 points in flight.  Each wave walks a run of consecutive points.
//
// Per point:
//   Gram         A = Ys^T Ys + (k-1)/rho I (common/common_letkf.f90:127-143) on the FP64 matrix cores, observation
//                rows straight from the obs table into MFMA operand layout; accumulator tiles -> lane j = column j
//   warm start   G0 = A Q, Q = eigenvectors of the previous point of the run (global workspace slot)
//   eigen-solve  (reference: common_mtx.f90:41 -> EISPACK rs, netlib.f:524) one-sided (Hestenes) Jacobi in registers,
//                row-split layout, odd-even transposition ordering, DPP exchanges only (jacobi_split).  Columns
//                converge to lambda_j v_j, so lambda_j = |g_j| and V needs no accumulation.
//   apply        (lane j holds v_j)
//                U[j][b] = v_j . B_b        B = [Ys^T d, Ys^T d_det, x'_1 .. x'_nv]  (LDS broadcast reads)
//                Out = V (D U)              through 8-column LDS transposition chunks, lane m gets row m
//                -> w-bar, w-bar_det, T x'_v;  RTPP/RTPS, beta, det member, q clamp as
//                   scale/letkf/letkf_tools.f90:457-513.  T / Pa themselves are only formed on request.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "letkf_device.h"
#include "letkf_search_dev.h"
#include "letkf_jacobi_dev.h"
#include "letkf_lane_dev.h"
#include "letkf_rules_dev.h"
#include "letkf_sched_dev.h"

namespace letkf {

using namespace jacobi_dev;
using namespace lane_dev;
using namespace rules_dev;

// sum / max / min over all lanes of the point.  With two waves the partials meet in a 4-double LDS scratch; `slot`
// alternates between consecutive calls (each call has its own barrier, so slot s is free again two calls later).
template <int NW, int OP>
__device__ __forceinline__ double preduce(double v, double* red, int& slot) {
  v = (OP == 0) ? wave_sum(v) : (OP == 1) ? wave_max(v) : wave_min(v);
  if constexpr (NW == 1) {
    return v;
  } else {
    if ((threadIdx.x & 63) == 0) red[2 * slot + (threadIdx.x >> 6)] = v;
    __syncthreads();
    const double a = red[2 * slot], b = red[2 * slot + 1];
    slot ^= 1;
    return (OP == 0) ? a + b : (OP == 1) ? fmax(a, b) : fmin(a, b);
  }
}

constexpr int kTnW = 8;               // obs rows per LDS tile (per wave)
constexpr int kChunk = 8;             // columns per LDS transposition chunk
constexpr int kVld = kChunk + 2;      // row stride of the transposition buffer (doubles, even)

// Out[b] (lane m: row m of V C) += sum over the wave's columns j of V[m][j] * C[j][b], b < NB.
// V[:, j] is lane j's register column vcol[], C[j][:] is lane j's crow[].  Done in chunks of
// kChunk columns through LDS:  vbuf[KR][kVld], cbuf[kChunk][NBP].
template <int KR, int NB, int NW>
__device__ __forceinline__ void rows_times_c(const double (&vcol)[KR], const double (&crow)[NB], double (&out)[NB],
                                             const int k, double* vbuf, double* cbuf) {
  constexpr int NBP = (NB + 1) & ~1;
  int lane = threadIdx.x & (64 * NW - 1);
  if constexpr (NW == 2) asm volatile("" : "+v"(lane));   // (two-wave points: see the point loop of letkf_wave_kernel)
#pragma unroll
  for (int b = 0; b < NB; ++b) out[b] = 0.0;
  const int ncol = (k + 1) & ~1;                 // columns live in lanes [0, ncol) (see jacobi_split)
  for (int j0 = 0; j0 < ncol; j0 += kChunk) {
    psync<NW>();
    if (lane >= j0 && lane < j0 + kChunk) {
      const int jj = lane - j0;
#pragma unroll
      for (int r = 0; r < KR; ++r) vbuf[r * kVld + jj] = vcol[r];
#pragma unroll
      for (int b = 0; b < NB; ++b) cbuf[jj * NBP + b] = crow[b];
      if (NBP > NB) cbuf[jj * NBP + NB] = 0.0;
    }
    psync<NW>();
    const int mrow = lane < KR ? lane : KR - 1;
    double vv[kChunk];
#pragma unroll
    for (int jj = 0; jj < kChunk; jj += 2) {
      const double2 t2 = *reinterpret_cast<const double2*>(&vbuf[mrow * kVld + jj]);
      vv[jj] = t2.x;
      vv[jj + 1] = t2.y;
    }
    const int nj = min(kChunk, ncol - j0);
#pragma unroll
    for (int jj = 0; jj < kChunk; ++jj) {
      if (jj < nj) {
#pragma unroll
        for (int b = 0; b < NBP; b += 2) {
          const double2 c2 = *reinterpret_cast<const double2*>(&cbuf[jj * NBP + b]);   // wave-uniform: broadcast
          out[b] = fma(vv[jj], c2.x, out[b]);
          if (b + 1 < NB) out[b + 1] = fma(vv[jj], c2.y, out[b + 1]);
        }
      }
      pin_acc<NB>(out);
    }
  }
  psync<NW>();
}

// ---------------------------------------------------------------------------------------------
// Warm start of the eigensolve: G0 = A Q with Q the eigenvector matrix of the PREVIOUS point of this wave's run.
// One-sided Jacobi on A Q (any orthogonal Q) still ends with columns lambda_j v_j of A -- the accumulated rotation
// is simply Q^T V -- but neighbouring grid points see almost the same observations, so Q nearly diagonalises A and
// the slow linear phase of the iteration (6 of the 9 sweeps at k = 50) is skipped: 9.1 -> 6.0 sweeps on the C2
// workload for x- or y-neighbours, no worse than the cold start for an unrelated Q.  Q's departure from
// orthogonality is the previous point's final residual (< 1e-10 measured BEFORE its last sweep rotated it away),
// so errors do not accumulate along a run.
//
// Lane j needs (A Q)[:, j] = sum_i A[:, i] Q[i][j]: its own Q column comes back from the wave's global workspace
// slot a chunk at a time (it cannot stay in registers: 256 VGPRs hold g, h and nothing else); the columns of A are
// written to LDS kWC at a time and read back as wave-uniform (broadcast) ds_read_b128.  2 k^2 FMAs + k^2/2 LDS reads
// per lane.  History: this LDS version was first measured at 1.6 sweeps' worth of time because the column-per-lane
// Jacobi's odd steps kept the LDS return path ~70 % busy; a v_readlane_b32 x2 + SGPR-operand FMA version
// (tools/ubench_readlane.hip: 5.6 ns per triple against 2.35 ns per bare v_fma_f64) cost one sweep; with the
// row-split Jacobi (no LDS in its steps) the LDS broadcast is the cheapest again.
// ---------------------------------------------------------------------------------------------
// early stop of the eigensolver (letkf_jacobi_dev.h, EARLY): on in every instantiation (two-wave points: both ballots ride one
// barrier, k = 64 1.00 M against 0.93 M solves/s).
#ifndef LETKF_INPLACE_NW
#define LETKF_INPLACE_NW(kr, nw) ((nw) == 2 && (kr) > 64)   // two half-column arrays instead of three (letkf_jacobi_dev.h)
#endif
// (launch bounds of two workgroups per CU were tried for the in-place instantiations: 256 registers in all, 2 KB/lane of
// scratch, k = 100 510 k -> 448 k; wave_occupancy asks for one)
#ifndef LETKF_GRAM_DEPTH
#define LETKF_GRAM_DEPTH 3
#endif
constexpr int kGramDepth = LETKF_GRAM_DEPTH;   // 4-obs Gram steps in flight (measured on C2: 3 -> 477 ms, 4 -> 487, 5 -> 492)
constexpr int kWC = 4;   // columns of A per LDS chunk (small: the unrolled chunk body is ~100 instructions per column)
// pins out[R0 .. R0+7] (those below KR): see pin_acc
template <int KR, int R0>
__device__ __forceinline__ void pin_rows8(double (&o)[KR]) {
  if constexpr (R0 + 8 <= KR) {
    asm volatile(""
                 : "+v"(o[R0]), "+v"(o[R0 + 1]), "+v"(o[R0 + 2]), "+v"(o[R0 + 3]), "+v"(o[R0 + 4]), "+v"(o[R0 + 5]),
                   "+v"(o[R0 + 6]), "+v"(o[R0 + 7])::"memory");
  } else if constexpr (R0 < KR) {
#pragma unroll
    for (int r = R0; r < KR; r += 2) asm volatile("" : "+v"(o[r]), "+v"(o[r + 1])::"memory");
  }
}
template <int KR, int NW>
__device__ __forceinline__ void warm_start_product(double (&g)[KR], const double* __restrict__ uws, const int k,
                                                   double* cb) {
  constexpr int NL = 64 * NW;
  constexpr int NG = (KR + 7) / 8;
  static_assert(NG <= 13, "pin_rows8 dispatch below");
  int lane = threadIdx.x & (NL - 1);
  if constexpr (NW == 2) asm volatile("" : "+v"(lane));   // (two-wave points: see the point loop of letkf_wave_kernel)
  const int ncol = (k + 1) & ~1;
  double out[KR];
#pragma unroll
  for (int r = 0; r < KR; ++r) out[r] = 0.0;
  double un[kWC];
#pragma unroll
  for (int q = 0; q < kWC; ++q) un[q] = (q < ncol) ? uws[(size_t)q * NL] : 0.0;
#pragma unroll 1
  for (int i0 = 0; i0 < ncol; i0 += kWC) {
    double u[kWC];
#pragma unroll
    for (int q = 0; q < kWC; ++q) u[q] = un[q];
    psync<NW>();
    if (lane >= i0 && lane < i0 + kWC) {
      double* mine = cb + (lane - i0) * KR;
#pragma unroll
      for (int r = 0; r < KR; r += 2) *reinterpret_cast<double2*>(&mine[r]) = double2{g[r], g[r + 1]};
    }
    psync<NW>();
#pragma unroll
    for (int q = 0; q < kWC; ++q) un[q] = (i0 + kWC + q < ncol) ? uws[(size_t)(i0 + kWC + q) * NL] : 0.0;
    // 8-row groups, the loads of group g+1 issued before the FMAs of group g
    double2 cur[4], nxt[4];
    auto ld = [&](const int q, const int gi, double2 (&d)[4]) {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (8 * gi + 2 * e < KR) d[e] = *reinterpret_cast<const double2*>(&cb[q * KR + 8 * gi + 2 * e]);   // broadcast
    };
    ld(0, 0, cur);
#pragma unroll
    for (int q = 0; q < kWC; ++q) {
#pragma unroll
      for (int gi = 0; gi < NG; ++gi) {
        const int nq = (gi + 1 < NG) ? q : q + 1, ng = (gi + 1 < NG) ? gi + 1 : 0;
        if (nq < kWC) ld(nq, ng, nxt);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int r = 8 * gi + 2 * e;
          if (r < KR) {
            out[r] = fma(cur[e].x, u[q], out[r]);
            out[r + 1] = fma(cur[e].y, u[q], out[r + 1]);
          }
        }
        if (gi == 0) pin_rows8<KR, 0>(out);
        if (gi == 1) pin_rows8<KR, 8>(out);
        if (gi == 2) pin_rows8<KR, 16>(out);
        if (gi == 3) pin_rows8<KR, 24>(out);
        if (gi == 4) pin_rows8<KR, 32>(out);
        if (gi == 5) pin_rows8<KR, 40>(out);
        if (gi == 6) pin_rows8<KR, 48>(out);
        if (gi == 7) pin_rows8<KR, 56>(out);
        if (gi == 8) pin_rows8<KR, 64>(out);
        if (gi == 9) pin_rows8<KR, 72>(out);
        if (gi == 10) pin_rows8<KR, 80>(out);
        if (gi == 11) pin_rows8<KR, 88>(out);
        if (gi == 12) pin_rows8<KR, 96>(out);
#pragma unroll
        for (int e = 0; e < 4; ++e) cur[e] = nxt[e];
      }
    }
  }
  psync<NW>();
#pragma unroll
  for (int r = 0; r < KR; ++r) g[r] = out[r];
}

// The same product on the FP64 matrix cores, for one-wave points with KR <= 50 (A fits the wave's LDS slice whole:
// 4 x 20 KB per workgroup, two workgroups still share a CU -- tools/ubench_lds_occ.hip).  The LDS-broadcast version
// above is latency-bound (4 ds_read_b128 in flight against 8 FMAs: 23 cycles per instruction, 15 % of the kernel's
// wave time on C2, measured with the PROF build) and it competes with the other wave's Jacobi for the vector ALU;
// here every lane first parks its column of A in LDS -- which frees the 2 KR registers of g for the accumulators --
// and the product runs as KS = KR/4 steps of 16 v_mfma_f64_16x16x4 with
//   A operand, row block I : A[4c + I][4s + q]   = 4 consecutive doubles of LDS column 4s+q (A is symmetric)
//   B operand, col block J : Q[4s + q][4c + J]   = 4 consecutive doubles of workspace row 4s+q (coalesced 32-B loads)
// (lane = 16 q + c; the blocks interleave rows / columns with stride 4 instead of covering 16 contiguous ones, so that
// both operands of a step are one 32-byte read per lane).  Accumulator (I, J), register `reg` of lane (q, c) is
// G0[16 reg + 4q + I][4c + J]; the tiles go back to "lane j owns column j" through the same LDS region.
typedef __attribute__((address_space(1))) double gdouble;
typedef double v2d_t __attribute__((ext_vector_type(2)));
typedef __attribute__((address_space(1))) v2d_t gdouble2;

template <int KR>
__device__ __forceinline__ void warm_start_product_mfma(double (&g)[KR], const double* __restrict__ qslot, double* cb) {
  static_assert(KR % 2 == 0 && KR <= 50, "A must fit the LDS slice");
  constexpr int KS = (KR + 3) / 4;             // contraction steps of 4
  constexpr int PD = (KS < 6) ? KS : 6;        // workspace row-quads in flight
  const int wlane = threadIdx.x & 63;
  const int q = wlane >> 4, c = wlane & 15;
  struct Quad {
    double2 lo, hi;
  };
  unsigned long long qaddr = reinterpret_cast<unsigned long long>(qslot + q * 64 + 4 * c);
  asm volatile("" : "+v"(qaddr));
  const gdouble2* qp = (const gdouble2*)qaddr;   // integer -> global pointer: no generic pointer in between
  auto ldq = [&](const int s) {
    Quad t{double2{0.0, 0.0}, double2{0.0, 0.0}};
    if (4 * s + 3 < KR || 4 * s + q < KR) {    // rows >= KR do not exist in the slot
      // (global address space spelled out: behind the laundering asm the pointer is generic, hipcc emits flat_load,
      // flat operations count in lgkmcnt as well and return out of order, so every LDS wait in this loop became
      // lgkmcnt(0) and drained the workspace loads in flight)
      const gdouble2* a = qp + (size_t)s * 128;
      const v2d_t lo = a[0], hi = a[1];
      t.lo = double2{lo.x, lo.y};
      t.hi = double2{hi.x, hi.y};
    }
    return t;
  };
  auto lda = [&](const int s) {
    Quad t{double2{0.0, 0.0}, double2{0.0, 0.0}};
    if (4 * s + 3 < KR || 4 * s + q < KR) {
      const double* a = cb + (4 * s + q) * KR + 4 * c;   // rows 4c+I >= KR read finite-or-not garbage: only output
      t.lo = *reinterpret_cast<const double2*>(a);        // rows >= KR see it, and those are dropped below
      t.hi = *reinterpret_cast<const double2*>(a + 2);
    }
    return t;
  };
  Quad qr[PD];
#pragma unroll
  for (int s = 0; s < PD; ++s) qr[s] = ldq(s);
  wave_lds_sync();
  if (wlane < KR) {
    double* mine = cb + wlane * KR;
#pragma unroll
    for (int r = 0; r < KR; r += 2) *reinterpret_cast<double2*>(&mine[r]) = double2{g[r], g[r + 1]};
  }
  wave_lds_sync();
  v4d acc[16];
#pragma unroll
  for (int t = 0; t < 16; ++t) acc[t] = v4d{0.0, 0.0, 0.0, 0.0};
  Quad ar[2];
  ar[0] = lda(0);
#pragma unroll
  for (int s = 0; s < KS; ++s) {
    if (s + 1 < KS) ar[(s + 1) & 1] = lda(s + 1);
    const Quad a4 = ar[s & 1], b4 = qr[s % PD];
    const double av[4] = {a4.lo.x, a4.lo.y, a4.hi.x, a4.hi.y};
    const double bv[4] = {b4.lo.x, b4.lo.y, b4.hi.x, b4.hi.y};
#pragma unroll
    for (int I = 0; I < 4; ++I)
#pragma unroll
      for (int J = 0; J < 4; ++J) acc[4 * I + J] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[I], bv[J], acc[4 * I + J], 0, 0, 0);
    if (s + PD < KS) qr[s % PD] = ldq(s + PD);
  }
  wave_lds_sync();
#pragma unroll
  for (int J = 0; J < 4; ++J) {
    const int col = 4 * c + J;
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const int row0 = 16 * reg + 4 * q;
      if (col < KR && row0 < KR) *reinterpret_cast<double2*>(&cb[col * KR + row0]) = double2{acc[J][reg], acc[4 + J][reg]};
      if (col < KR && row0 + 2 < KR) *reinterpret_cast<double2*>(&cb[col * KR + row0 + 2]) = double2{acc[8 + J][reg], acc[12 + J][reg]};
    }
  }
  wave_lds_sync();
  {
    const double* mine = cb + (wlane < KR ? wlane : 0) * KR;
#pragma unroll
    for (int r = 0; r < KR; r += 2) {
      const double2 v2 = *reinterpret_cast<const double2*>(&mine[r]);
      g[r] = wlane < KR ? v2.x : 0.0;
      g[r + 1] = wlane < KR ? v2.y : 0.0;
    }
  }
  wave_lds_sync();
}

// STRIP form of the product for KR = 50 (LETKF_WARM_STRIP, default on; -DLETKF_WARM_STRIP=0 gives the form above for an A/B).
// Above, rows and columns are dealt to four interleaved blocks (4c + I) of which every one is 13/16 full: 13 steps x 16 tiles
// = 208 matrix instructions for a 50 x 50 x 50 product.  Here the blocks are contiguous -- 0-15, 16-31, 32-47 -- and only their
// nine full tiles go to the matrix cores (117 instructions); rows and columns 48, 49 of G0 are accumulated on the vector ALU
// from the operands the tiles load anyway (the narrow block of the Gram, r4, applied to the product).  Per step, lane (q, c)
// with i = 4s + q holds a[I] = A[16 I + c][i], ae[e] = A[48 + e][i], b[J] = Q[i][16 J + c], be[e] = Q[i][48 + e] and adds
//   rs[e][J] += ae[e] b[J]   -> G0[48 + e][16 J + c]      cs[e][I] += a[I] be[e]   -> G0[16 I + c][48 + e]
//   cn[e][f] += ae[e] be[f]  -> G0[48 + e][48 + f]
// 16 FMAs against the 7 x 16 issue slots of the seven matrix instructions they replace; the partial sums over the four
// residues q are folded once per point.  The operands are single 8-byte reads at fixed offsets from one address per lane (the
// memory instructions are not what bounds the kernel: DESIGN 4.1); neither the layout of A in LDS nor that of Q in the
// workspace slot changes.  Accumulator (I, J), register `reg` of lane (q, c) is G0[16 I + 4 reg + q][16 J + c].
#ifndef LETKF_WARM_STRIP
#define LETKF_WARM_STRIP 1
#endif
template <int KR>
__device__ __forceinline__ void warm_start_product_strip(double (&g)[KR], const double* __restrict__ qslot, double* cb) {
  constexpr int NBF = KR / 16;                 // full blocks (3)
  constexpr int RS = KR - 16 * NBF;            // rows / columns of the narrow block (2)
  static_assert(KR % 2 == 0 && KR <= 50 && RS == 2 && NBF == 3, "A must fit the LDS slice; the narrow block is a pair (16-byte reads); the pin below");
  constexpr int KS = (KR + 3) / 4;             // contraction steps of 4
  constexpr int PD = (KS < 6) ? KS : 6;        // workspace rows in flight
  const int wlane = threadIdx.x & 63;
  const int q = wlane >> 4, c = wlane & 15;
  struct QOp {
    double b[NBF];
    double2 be;
  };
  struct AOp {
    double a[NBF];
    double2 ae;
  };
  unsigned long long qaddr = reinterpret_cast<unsigned long long>(qslot + q * 64 + c);
  asm volatile("" : "+v"(qaddr));
  const gdouble* qp = (const gdouble*)qaddr;   // integer -> global pointer: see warm_start_product_mfma
  auto ldq = [&](const int s) {
    QOp t;
#pragma unroll
    for (int J = 0; J < NBF; ++J) t.b[J] = 0.0;
    t.be = double2{0.0, 0.0};
    if (4 * s + 3 < KR || 4 * s + q < KR) {    // rows >= KR do not exist in the slot
      const gdouble* a = qp + (size_t)s * 256;
#pragma unroll
      for (int J = 0; J < NBF; ++J) t.b[J] = a[16 * J];
      const v2d_t e2 = *(const gdouble2*)(a + (16 * NBF - c));
      t.be = double2{e2.x, e2.y};
    }
    return t;
  };
  auto lda = [&](const int s) {
    AOp t;
#pragma unroll
    for (int I = 0; I < NBF; ++I) t.a[I] = 0.0;
    t.ae = double2{0.0, 0.0};
    if (4 * s + 3 < KR || 4 * s + q < KR) {
      const double* a = cb + (4 * s + q) * KR;
#pragma unroll
      for (int I = 0; I < NBF; ++I) t.a[I] = a[16 * I + c];
      t.ae = *reinterpret_cast<const double2*>(a + 16 * NBF);
    }
    return t;
  };
  QOp qr[PD];
#pragma unroll
  for (int s = 0; s < PD; ++s) qr[s] = ldq(s);
  wave_lds_sync();
  if (wlane < KR) {
    double* mine = cb + wlane * KR;
#pragma unroll
    for (int r = 0; r < KR; r += 2) *reinterpret_cast<double2*>(&mine[r]) = double2{g[r], g[r + 1]};
  }
  wave_lds_sync();
  v4d acc[NBF * NBF];
#pragma unroll
  for (int t = 0; t < NBF * NBF; ++t) acc[t] = v4d{0.0, 0.0, 0.0, 0.0};
  double rs[RS][NBF], cs[RS][NBF], cn[RS][RS];
#pragma unroll
  for (int e = 0; e < RS; ++e) {
#pragma unroll
    for (int I = 0; I < NBF; ++I) rs[e][I] = cs[e][I] = 0.0;
#pragma unroll
    for (int f = 0; f < RS; ++f) cn[e][f] = 0.0;
  }
  AOp ar[2];
  ar[0] = lda(0);
#pragma unroll
  for (int s = 0; s < KS; ++s) {
    if (s + 1 < KS) ar[(s + 1) & 1] = lda(s + 1);
    const AOp a4 = ar[s & 1];
    const QOp b4 = qr[s % PD];
    const double ae[RS] = {a4.ae.x, a4.ae.y}, be[RS] = {b4.be.x, b4.be.y};
#pragma unroll
    for (int I = 0; I < NBF; ++I)
#pragma unroll
      for (int J = 0; J < NBF; ++J) acc[NBF * I + J] = __builtin_amdgcn_mfma_f64_16x16x4f64(a4.a[I], b4.b[J], acc[NBF * I + J], 0, 0, 0);
#pragma unroll
    for (int e = 0; e < RS; ++e) {
#pragma unroll
      for (int I = 0; I < NBF; ++I) {
        rs[e][I] = fma(ae[e], b4.b[I], rs[e][I]);
        cs[e][I] = fma(a4.a[I], be[e], cs[e][I]);
      }
#pragma unroll
      for (int f = 0; f < RS; ++f) cn[e][f] = fma(ae[e], be[f], cn[e][f]);
    }
    if (s + PD < KS) qr[s % PD] = ldq(s + PD);
    // (keeps the strip's FMAs in the step whose operands they use: left alone, hipcc moves all of them behind the last matrix
    // instruction and carries the operands of thirteen steps there through scratch -- 100 scratch accesses inside the product)
    asm volatile(""
                 : "+v"(rs[0][0]), "+v"(rs[0][1]), "+v"(rs[0][2]), "+v"(rs[1][0]), "+v"(rs[1][1]), "+v"(rs[1][2]), "+v"(cs[0][0]),
                   "+v"(cs[0][1]), "+v"(cs[0][2]), "+v"(cs[1][0]), "+v"(cs[1][1]), "+v"(cs[1][2]), "+v"(cn[0][0]), "+v"(cn[0][1]),
                   "+v"(cn[1][0]), "+v"(cn[1][1])::"memory");
  }
  // fold the four residues q (lanes c, c + 16, c + 32, c + 48): every lane ends with the whole sums
  auto fold = [](double v) {
    v += __shfl_xor(v, 16);
    v += __shfl_xor(v, 32);
    return v;
  };
#pragma unroll
  for (int e = 0; e < RS; ++e) {
#pragma unroll
    for (int I = 0; I < NBF; ++I) {
      rs[e][I] = fold(rs[e][I]);
      cs[e][I] = fold(cs[e][I]);
    }
#pragma unroll
    for (int f = 0; f < RS; ++f) cn[e][f] = fold(cn[e][f]);
  }
  wave_lds_sync();
  // back to "column j at cb[j * KR]" (all rows and columns written are < KR)
#pragma unroll
  for (int J = 0; J < NBF; ++J) {
    double* col = cb + (16 * J + c) * KR;
#pragma unroll
    for (int I = 0; I < NBF; ++I)
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) col[16 * I + 4 * reg + q] = acc[NBF * I + J][reg];
    if (q == 0) *reinterpret_cast<double2*>(&col[16 * NBF]) = double2{rs[0][J], rs[1][J]};
  }
  if (q == 1) {
#pragma unroll
    for (int e = 0; e < RS; ++e)
#pragma unroll
      for (int I = 0; I < NBF; ++I) cb[(16 * NBF + e) * KR + 16 * I + c] = cs[e][I];
  }
  if (wlane == 32) {
#pragma unroll
    for (int f = 0; f < RS; ++f) *reinterpret_cast<double2*>(&cb[(16 * NBF + f) * KR + 16 * NBF]) = double2{cn[0][f], cn[1][f]};
  }
  wave_lds_sync();
  {
    const double* mine = cb + (wlane < KR ? wlane : 0) * KR;
#pragma unroll
    for (int r = 0; r < KR; r += 2) {
      const double2 v2 = *reinterpret_cast<const double2*>(&mine[r]);
      g[r] = wlane < KR ? v2.x : 0.0;
      g[r + 1] = wlane < KR ? v2.y : 0.0;
    }
  }
  wave_lds_sync();
}

// Hand-over order of the eigenvectors (LETKF_WARM_SORT, default on; -DLETKF_WARM_SORT=0 gives the lane-order store for an A/B;
// LETKF_AMD_WARM_DBG bit 4 selects it at run time).  Rotate-and-swap moves the columns along the line and a solve stops after a
// partial cycle, so the lane order in which a point leaves its eigenvectors is a permutation that drifts further from any
// order with every point of a run; cyclic Jacobi converges faster when neighbours on the line have the closest eigenvalues
// (the large rotation angles are met in the first two steps of a cycle).  One-wave points therefore store the column of lane j
// into workspace column warm_rank(j): eigenvalue descending, ties by lane, columns without an eigenvector (the inert zero
// column of an odd k, lanes >= k) last.  The key is the high dword of lam with its low 6 bits replaced by 63 - lane: unique
// per lane whatever the bits of lam are, so the rank is a bijection of the line's lanes for any input, NaN included, and
// lanes outside the line keep their own column (they hold zeros, and so do all columns sorted last: the products find
// their zero padding where it was).  Cost: readlane + compare + add-with-carry per line lane, 3 min(KR, 64) instructions
// per point.  (The switch itself is letkf_jacobi_dev.h's: the three-point kernel parks its eigenvectors the same way.)
template <int KR>
__device__ __forceinline__ int warm_rank(const double lam, const bool colvalid, const int lane) {
  constexpr int NLN = KR < 64 ? KR : 64;       // lanes of the line
  const unsigned tie = 63u - (unsigned)(lane & 63);
  unsigned key = colvalid ? (((unsigned)__double2hiint(lam) & ~63u) | tie) : tie;
  int rank = 0;
#pragma unroll
  for (int i = 0; i < NLN; ++i) {
    // (8 keys in scalar registers at a time: left alone hipcc reads all NLN lanes first, and the scalar registers that takes
    // are paid for in the apply phase, which then re-loads the kernel arguments 58 times per point instead of keeping them)
    if ((i & 7) == 0) asm volatile("" : "+v"(key), "+v"(rank));
    rank += ((unsigned)__builtin_amdgcn_readlane((int)key, i) > key) ? 1 : 0;
  }
  return lane < NLN ? rank : lane;
}

// Line position of rank r (LETKF_WARM_ORDER, default on; -DLETKF_WARM_ORDER=0 gives position = rank for an A/B; LETKF_AMD_WARM_DBG
// bit 5 selects that at run time).  The ordering is odd-even transposition with rotate-and-swap: a column that starts at an even
// position travels right, one that starts at an odd position left.  With rank r at position r the ranks (2m, 2m+1) meet in step 1,
// but (2m+1, 2m+2) move apart and meet at the very end of the cycle; with rank r at position r ^ 1 they meet in step 2, so every
// eigenvalue-adjacent pair is rotated in the first step pair -- and the reversal a full cycle applies keeps that pattern.  Only
// whole pairs of ranks with an eigenvector swap ((r | 1) < nvalid): the unpaired last rank of an odd count keeps its position and
// the columns sorted last (zeros) keep theirs, so the map is an involution of the line's lanes whatever nvalid is, and with the
// rank it stays a bijection in bounds for any input, NaN included.
__device__ __forceinline__ int warm_position(const int rank, const int nvalid) { return (rank | 1) < nvalid ? (rank ^ 1) : rank; }

// smallest k the instantiation <KR, NW> is dispatched for (launch_wave_kernel walks the instances in this order)
__host__ __device__ constexpr int wave_kmin(int KR, int NW) {
  return NW == 1 ? (KR == 16 ? 1 : KR == 20 ? 17 : KR == 32 ? 17 : KR == 48 ? 33 : KR == 50 ? 49 : KR == 64 ? 51 : 1)
                 : (KR == 64 ? 63 : KR == 80 ? 65 : KR == 100 ? 81 : 1);
}

// Small ensembles (KR <= 20: C1, the k = 20 workloads) are issue- and latency-bound with 20 of 64 lanes carrying a column (one wave
// per SIMD -> two: x 1.47 on C2-k20, measured with padded LDS), so their slice is cut to what such a point needs -- the Jacobi's
// conversion chunk is KR rows (not 24), the apply phase's output buffer 32 rows (not 64): 12.5 KB per wave, 50 KB per workgroup,
// room for THREE workgroups per CU.  Measured (r4, A/B in one gpurun call, -DLETKF_SMALL_OCC=3 against 2): the register budget
// of three waves per SIMD (168) costs this kernel 464 B/lane of scratch instead of 136 -- C2-k20 -6 %, C1 +4 %.  The default
// stays at two (letkf_launch_shape.h, which counts the wave-slots in flight with it); the slice stays small.
__host__ __device__ constexpr bool wave_small(int KR, int NW) { return NW == 1 && KR <= 20; }
__host__ __device__ constexpr int wave_base_doubles(int KR, int NW) { return wave_small(KR, NW) ? 1280 : 1536 * NW; }
__host__ __device__ constexpr int wave_jacobi_rc(int KR, int NW) { return wave_small(KR, NW) ? KR : 24; }   // rows per conversion chunk
__host__ __device__ constexpr int wave_ob_rows(int KR) { return KR <= 20 ? 32 : 64; }                        // rows of the MAPPLY output buffer
__host__ __device__ constexpr int wave_occupancy(int KR, int NW) { return NW == 1 ? (wave_small(KR, NW) ? LETKF_SMALL_OCC : 2) : 1; }

// per-wave LDS slice (doubles)
__host__ __device__ inline int wave_slice_doubles(int KR, int nv, int NW) {
  const int nb = nv + 2;
  int tile = kTnW * 64;                       // obs tile, also reused as vbuf (KR * kVld) and kk-output C chunk
  const int vb = KR * kVld;
  if (vb > tile) tile = vb;
  int bmat = ((nb + 1) & ~1) * KR;            // B vectors [KR][NBP]; reused as the T/Pa C chunk (kChunk * KR)
  if (kChunk * KR > bmat) bmat = kChunk * KR;
  const int cb = kChunk * ((nb + 1) & ~1);
  const int small = 3 * kTnW + 8 * nv + 16;
  if (tile + bmat < wave_base_doubles(KR, NW)) bmat = wave_base_doubles(KR, NW) - tile;   // Gram transposition buffer abuf[64 NW][18] and
                                                         // the Jacobi exchange slots (64 NW * RC doubles) span tile + bmat
  int tot = tile + bmat + cb + small + 8;                // + 4 doubles of reduction scratch (two-wave points)
  if (NW == 1 && KR <= 50 && tot < (KR - 1) * KR + 64) tot = (KR - 1) * KR + 64;   // A whole: warm_start_product_mfma
  if (NW == 1 && KR < 32 && tot < 32 * KR + 64 * ((KR + 3) / 4) + 128 + 16 * wave_ob_rows(KR)) tot = 32 * KR + 64 * ((KR + 3) / 4) + 128 + 16 * wave_ob_rows(KR);   // + [rows][16] output buffer
  if (NW == 1 && KR <= 50 && tot < 32 * KR + 64 * ((KR + 3) / 4) + 128)               // half of V + padded B + spectra: the apply phase on the matrix cores
    tot = 32 * KR + 64 * ((KR + 3) / 4) + 128;
  return (tot + 1) & ~1;
}

// KKOUT: also materialise T / Pa (fine boundary, parity, diagnostics) -- a separate instantiation so that the
// production kernel carries neither the code nor the registers for it.
// FUSED = 2: obs_local walked inside the kernel (mode 2); FUSED = 3: the vertical half of obs_local on the column's horizontal
// survivors (mode 3) -- instantiations of their own: carried by the list-driven kernel
// the extra code cost 15 % of its speed (registers / instruction cache), measured.
// Profiling build (make PROF=1): per-phase wave time from s_memtime, kept in SGPRs, summed over all waves.
#ifdef LETKF_WAVE_PROF
#define PROF_DECL unsigned long long prof_t[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0}; unsigned long long prof_last = __builtin_amdgcn_s_memtime(); const unsigned long long prof_t0 = prof_last; int prof_units = 0;
#define PROF_MARK(i) { const unsigned long long t_ = __builtin_amdgcn_s_memtime(); prof_t[i] += t_ - prof_last; prof_last = t_; }
// [10]: ~earliest wave start, [11]: latest wave end (s_memtime), [12 + u]: waves that did u units (u capped at 11),
// [24]: units done in all (= the plan's units if every one was drawn exactly once)
#define PROF_FLUSH if (A.prof && wlane == 0) { for (int i_ = 0; i_ < 10; ++i_) atomicAdd(&A.prof[i_], prof_t[i_]); \
    atomicMax(&A.prof[10], ~prof_t0); atomicMax(&A.prof[11], (unsigned long long)__builtin_amdgcn_s_memtime()); \
    atomicAdd(&A.prof[12 + (prof_units < 11 ? prof_units : 11)], 1ull); atomicAdd(&A.prof[24], (unsigned long long)prof_units); }
#define PROF_UNIT ++prof_units;
#else
#define PROF_DECL
#define PROF_MARK(i)
#define PROF_FLUSH
#define PROF_UNIT
#endif

// Checked build (make CHECKED=1 -> lib/libletkf_amd_checked.so, run by tests/test_gpu_checked.py): every index the column-survivor
// mode derives from device data -- the run's column, the column's survivor range, the wave's slot, each list entry -- is tested
// against the bound the HOST sized the buffers by before it is used; a violation is recorded (code, workgroup, value, bound) in
// PointArgs::prof and the access is left out, so that the entry returns an error instead of the process dying on a memory fault
// with nothing to tell which access it was.  Absent from the normal build.
#ifdef LETKF_CHECKED
#define LETKF_CHECK(ok, code, val, lim) letkf_check_fail(A.prof, (ok), (code), (long)(val), (long)(lim))
__device__ __forceinline__ bool letkf_check_fail(unsigned long long* rec, const bool ok, const int code, const long val, const long lim) {
  if (!ok && rec && atomicCAS(&rec[0], 0ull, (unsigned long long)code) == 0ull) {
    rec[1] = blockIdx.x;
    rec[2] = (unsigned long long)val;
    rec[3] = (unsigned long long)lim;
  }
  return ok;
}
#else
#define LETKF_CHECK(ok, code, val, lim) true
#endif

// the kernel's arguments as the argument segment holds them, and a copy of that pointer that hipcc cannot see through: what is
// read through it is read where it is used, by scalar loads, and nothing built from it can be hoisted out of the point loop
// (letkf_wave_kernel; one-wave instantiations only -- two-wave points get the pointer back as it is and do not use it)
using KernArgs = const __attribute__((address_space(4))) PointArgs;
template <int NW>
__device__ __forceinline__ KernArgs* fresh_args(KernArgs* p) {
  if constexpr (NW == 1) asm volatile("" : "+s"(p));
  return p;
}

template <int KR, int NV, bool KKOUT, int NW, int FUSED>
__global__ void __launch_bounds__(NW == 1 ? 256 : 128, wave_occupancy(KR, NW)) letkf_wave_kernel(const PointArgs A) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  constexpr int NB = NV + 2;
  constexpr int NBP = (NB + 1) & ~1;
  constexpr int NL = 64 * NW;                 // lanes per point
  int lane = threadIdx.x & (NL - 1);          // lane of the point: column index in the eigen phase, member index after
  int wlane = threadIdx.x & 63;               // lane inside the wavefront (MFMA operand layout)
  const int wvp = (NW == 1) ? 0 : (threadIdx.x >> 6);   // wave inside the point
  const int wv = (NW == 1) ? (threadIdx.x >> 6) : 0;    // point slot inside the workgroup
  const int k = A.k;
  // (r12) The arguments a second time, as the argument segment holds them.  hipcc reads PointArgs in the prologue with
  // s_load_dwordx8 / x16, cannot keep the tuples in SGPRs across the point loop, parks them in lanes of a spill VGPR and fetches
  // the WHOLE tuple back -- 8 or 16 v_readlane_b32, vector issue slots -- in front of every use of one field: 1074 of the
  // production instantiation's 2926 lane reads wrote a scalar nobody read (tools/isa_point_census.py), 16 per variable of the
  // analysis loop to get q_sprd_max.  Masks built from a field and the lane number (lane < k && in-class, per variable) were
  // hoisted and parked the same way, two lane reads per use.  Through a pointer laundered at the head of a phase (fresh_args)
  // the phase re-reads what it needs with scalar loads, which are not vector instructions, and nothing built from those values
  // can be hoisted out of the point loop.  One-wave instantiations only: two-wave points keep A (and their assembly).
  // (every phase takes its own laundered copy, fresh_args: one laundered value carried from phase to phase would meet itself
  // behind branches hipcc takes for divergent -- the point number comes from a vector value -- and an SGPR cannot be merged
  // there.)
  [[maybe_unused]] KernArgs* const Ak0 = (KernArgs*)__builtin_amdgcn_kernarg_segment_ptr();
  const int nv = A.nv;                        // == NV on the das path, 0 on the letkf_core batch path
  const double km1 = (double)(k - 1);

  double* slice = smem + (size_t)wv * wave_slice_doubles(KR, NV, NW);
  int tile_sz = kTnW * 64;
  if (KR * kVld > tile_sz) tile_sz = KR * kVld;
  int bmat_sz = NBP * KR;
  if (kChunk * KR > bmat_sz) bmat_sz = kChunk * KR;
  if (tile_sz + bmat_sz < wave_base_doubles(KR, NW)) bmat_sz = wave_base_doubles(KR, NW) - tile_sz;
  double* vbuf = slice;                       // [KR][kVld]          (after the Gram phase)
  double* bmat = slice + tile_sz;             // [KR][NBP]
  double* cbuf = bmat + bmat_sz;              // [kChunk][NBP]
  double* wrow = cbuf + kChunk * NBP;         // 3 * kTnW
  double* xsm = wrow + 3 * kTnW;              // 8 * NV + 16
  double* xmean = xsm;
  double* xdet = xsm + NV;
  double* red = xsm + 8 * NV + 16;            // 4 doubles (+ pad): partials of two-wave reductions
  int rslot = 0;

  // Each wave walks a RUN of run_len consecutive points (warm-started eigensolves, see warm_start_product); the 4
  // runs of a workgroup are consecutive too, and workgroups are dealt over the XCDs so that neighbouring points
  // (which gather almost the same obs rows) hit the same L2
  constexpr int PPW = (NW == 1) ? 4 : 1;      // points in flight per workgroup
  const int run_len = A.run_len;
  // the points as an array [nA][S], p = a S + b: a run walks a at fixed b (S = 1: consecutive points; S = nij1 with
  // gues3d's point order: up a column), run number = chunk * S + b -- neighbouring runs are neighbouring columns
  const long S = A.warm_stride, nA = A.npts / S;
  // this wave's slot of the warm-start workspace: [KR][NL] doubles, lane-fastest
  double* uws = (run_len > 1) ? A.warm_ws + ((size_t)blockIdx.x * PPW + wv) * ((size_t)KR * NL) + lane : nullptr;
  PROF_DECL
#ifdef LETKF_WAVE_PROF
  long Bstat = blockIdx.x;
#endif
  bool first_draw = true;
  int pend = 0;                                // runs of the drawn unit that are still to do
  long next_rid = 0;
  for (;;) {
   long rid;
   int ir0 = 0, ir1 = run_len;
#ifdef LETKF_WAVE_PROF
   if (!A.sched) {
     // static (PROF twin only, LETKF_AMD_STATIC_SCHED): blocks of PPW consecutive runs, dealt to the workgroups in the
     // order of their XCDs -- what the production kernel did before the dynamic scheduling
     const long nruns = S * ((nA + run_len - 1) / run_len);
     const long nB = (nruns + PPW - 1) / PPW;
     if (Bstat >= nB) break;
     rid = xcd_remap(Bstat, nB) * PPW + wv;
     Bstat += gridDim.x;
     if (rid >= nruns) continue;
   } else
#endif
   if (pend > 0) {
     rid = next_rid++;
     --pend;
   } else {
     int code;
     // (wv stays a vector value: made scalar here by v_readfirstlane, hipcc's allocation of the whole kernel changes -- scratch 388 -> 612 B/lane)
     const int slot0 = first_draw ? (int)(blockIdx.x >> 3) * PPW + wv : -1;
     if constexpr (NW == 1) {
       code = sched_next(A.plan, A.sched, (int)(blockIdx.x & 7), slot0);
     } else {
       int* slot_ = reinterpret_cast<int*>(red + 6);
       __syncthreads();
       if (threadIdx.x < 64) {                  // (wave 0 draws for the workgroup)
         const int g = sched_next(A.plan, A.sched, (int)(blockIdx.x & 7), slot0);
         if (threadIdx.x == 0) *slot_ = g;
       }
       __syncthreads();
       code = *slot_;
     }
     first_draw = false;
     PROF_MARK(9)                              // (PROF twin: the time spent drawing)
     if (code < 0) break;
     PROF_UNIT
     if (code & 4) {
       ir0 = (code & 3) * run_len >> 2;
       ir1 = ((code & 3) + 1) * run_len >> 2;
     }
     rid = (long)(code >> 3) * A.plan.ub;
     const long left = A.plan.nruns - rid;
     pend = (int)(left < A.plan.ub ? left : A.plan.ub) - 1;
     next_rid = rid + 1;
   }
   const long rchunk = rid / S, rb = rid - rchunk * S;
   const long ra0 = rchunk * run_len;
   bool have_u = false;
   [[maybe_unused]] int pre_n = -1;             // mode 3: the NEXT point's list was assembled with this one's (its length; second half of the slot)
   for (int ir = ir0; ir < ir1; ++ir) {
    if (ra0 + ir >= nA) break;
    long pt = (ra0 + ir) * S + rb;
    if constexpr (FUSED == 3) {
      if (A.pt_stride) pt = (ra0 + ir) * A.pt_stride + rb + A.pt0;   // mode 3: columns pt0 .. pt0 + S of a wider domain
    }
    // Everything built from the lane number is the same for every point of the run, so hipcc hoists it out of this
    // loop -- dozens of LDS addresses -- cannot keep it in registers across the eigensolve, and reloads it from scratch
    // one dword at a time, each reload a round trip in front of its use.  Laundering the lane numbers keeps the address
    // arithmetic (one or two integer instructions) where it is used.  Measured (A/B on one box): in the apply phase
    // -0.8 % of the C2 time, in the Gram / tile transposition -2.2 % and k = 100 197 k -> 280 k solves/s; everywhere, as
    // here, another +13 % at k = 100 (316 k) but -1 % on C2 -- so the blanket version is for two-wave points only.
    if constexpr (NW == 2) asm volatile("" : "+v"(lane), "+v"(wlane));
    long o0 = 0;
    int n = 0;
    double beta = 1.0;
    const bool das = A.mode != 1;              // the das_letkf loop body (lists given: 0, search fused in: 2, column survivors: 3)
    if (A.mode == 0) {
      o0 = A.obs_off[pt];
      n = (int)(A.obs_off[pt + 1] - o0);
      if (A.beta) beta = A.beta[pt];
    } else if (FUSED == 3 && A.mode == 3) {
      if (A.beta) beta = A.beta[pt];
      n = 0;
      if constexpr (NW == 1 && FUSED == 3) {
        // ---- column-survivor mode: the horizontal half of obs_local was done once per COLUMN (letkf_survivors_kernel: the
        // rows inside the horizontal cut-off, in the reference's list order, with nd_h and their vertical coordinate); this
        // point adds its vertical half (search_dev::column_vertical_cal -- the expressions of the column search, so the weights
        // equal the lists' to the last bit) and leaves the accepted rows as a local list in this WAVE's slot of a small
        // workspace (written, read back by the Gram phase below and overwritten by the next point: it lives in L2).  The
        // lists of letkf_obs_search_columns_dev -- 20 B per (point, observation): 1 TB written and 1 TB read per analysis at
        // BASELINE configs[3] -- never exist, nor does the count pass over the levels.  (First version: the accepted rows went
        // straight into the Gram's staging buffer, flush and matrix-core steps inside this loop -- the four buffers and the
        // evaluated chunks stayed live across them, 800 B/lane of scratch, slower than the lists.)
        // Two levels per pass: the survivors are read once for this point AND the next one of the run (one level up the same
        // column): the stream is what bounds the pre-pass (configs[3]: 1.1 MB per point and level), the arithmetic doubles per
        // entry and halves per point.  The next point finds its list in the other half of the wave's slot (2 sl_cap entries).
        if (pre_n >= 0) {
          o0 = ((long)blockIdx.x * PPW + wv) * (2 * A.sl_cap) + A.sl_cap;
          n = LETKF_CHECK(pre_n <= A.sl_cap, 7, pre_n, A.sl_cap) ? pre_n : 0;
          pre_n = -1;
        } else if (beta != 0.0) {
          using namespace search_dev;
          const letkf_search_tables& t = A.stab;
          o0 = ((long)blockIdx.x * PPW + wv) * (2 * A.sl_cap);
          const long o1 = o0 + A.sl_cap;
          const bool two = ir + 1 < ir1 && ra0 + ir + 1 < nA;            // (wave-uniform) a next point in this run
          const long ptn = two ? pt + (A.pt_stride ? A.pt_stride : S) : pt;
          const double v_z = A.prz[pt], v_p = log(A.prlev[pt]), l_rain = log(t.rain_base);
          const double v_z1 = A.prz[ptn], v_p1 = log(A.prlev[ptn]);
          const unsigned long long lt_mask = lanes_below(wlane);
          long s_lo = A.sv_off[rb], s_hi = A.sv_off[rb + 1];
#ifdef LETKF_CHECKED
          {   // the run's column is one of the launch's, its survivors fit the slot the host sized, the slot is one of the grid's
            bool ok = LETKF_CHECK(rb >= 0 && rb < S, 1, rb, S);
            ok = ok && LETKF_CHECK(s_hi >= s_lo && ((s_hi - s_lo) & 63) == 0, 2, s_hi - s_lo, 64);
            ok = ok && LETKF_CHECK(s_hi - s_lo <= A.sl_cap, 3, s_hi - s_lo, A.sl_cap);
            ok = ok && LETKF_CHECK((long)blockIdx.x < (long)A.wave_grid, 4, blockIdx.x, A.wave_grid);
            if (!ok) s_hi = s_lo;
          }
#endif
          int ntot = 0, ntot1 = 0;
          if (s_hi > s_lo) {
            // Four chunks of 64 entries in flight, in four buffers with STATIC names: the survivors stream from HBM (no wave
            // reads a column's list while it is still in a cache: 320 KB per column at configs[3], 2048 columns in flight).
            // Found in the ISA of the first versions: one chunk ahead = a full memory round trip per chunk; four ahead
            // through a rotation of register copies (a0 = a1; ...) copies the destination of the load issued last --
            // s_waitcnt vmcnt(0) in every iteration; and the 64-bit `entry + lane` offsets were hoisted out of the point
            // loop, spilled, and their scratch_load -- which counts in vmcnt with the prefetches -- waited for everything in
            // flight.  Hence: four evaluations written out, each refilling its own buffer right behind itself, 32-bit
            // offsets from a laundered lane number, every load unconditional from a clamped address.
            const int ns_col = (int)(s_hi - s_lo);                         // (a multiple of 64: the survivor kernel pads)
            const double* sbase = A.surv + 4 * s_lo;
            int wl = wlane;
            asm volatile("" : "+v"(wl));
            auto ld = [&](const int e0, double2& x, double2& y) {
              int e = e0 + wl;
              e = e < ns_col ? e : ns_col - 1;
              x = *reinterpret_cast<const double2*>(&sbase[4 * e]);
              y = *reinterpret_cast<const double2*>(&sbase[4 * e + 2]);
            };
            double2 a0, b0, a1, b1, a2, b2, a3, b3;
            ld(0, a0, b0);
            ld(64, a1, b1);
            ld(128, a2, b2);
            ld(192, a3, b3);
            // the ctype's three numbers through the scalar cache (a chunk is of ONE type: the survivor kernel pads every type's
            // entries to whole chunks with rows outside every cut-off)
            int ic_s = -1, vm_s = 0;
            double vloc_s = 0.0, varloc_s = 0.0;
            auto eval = [&](const double2& ca, const double2& cb, const bool live) {
              const long rw = survivor_bits(ca.x);
              const int ic0 = __builtin_amdgcn_readfirstlane(survivor_ctype(rw));
              if (ic0 != ic_s) {
                ic_s = ic0;
                vm_s = t.vmode[ic0];
                vloc_s = t.vert_loc[ic0];
                varloc_s = t.varloc[ic0];
              }
              {
                const ColVert vo = column_vertical_cal(vm_s, vloc_s, varloc_s, ca.y, cb.x, cb.y, v_z, v_p, l_rain);
                const bool acc_ = live && vo.rloc != 0.0;                    // :1460
                const unsigned long long mk = __ballot(acc_);
                if (acc_ && LETKF_CHECK(ntot + __popcll(mk) <= A.sl_cap, 5, ntot + __popcll(mk), A.sl_cap)) {
                  const long j = o0 + ntot + __popcll(mk & lt_mask);
                  A.sl_idx[j] = survivor_row(rw);
                  A.sl_rd[j] = vo.rdiag;
                  A.sl_rl[j] = vo.rloc;
                }
                ntot += __popcll(mk);
              }
              if (two) {                                                     // (wave-uniform)
                const ColVert vo = column_vertical_cal(vm_s, vloc_s, varloc_s, ca.y, cb.x, cb.y, v_z1, v_p1, l_rain);
                const bool acc_ = live && vo.rloc != 0.0;
                const unsigned long long mk = __ballot(acc_);
                if (acc_ && LETKF_CHECK(ntot1 + __popcll(mk) <= A.sl_cap, 6, ntot1 + __popcll(mk), A.sl_cap)) {
                  const long j = o1 + ntot1 + __popcll(mk & lt_mask);
                  A.sl_idx[j] = survivor_row(rw);
                  A.sl_rd[j] = vo.rdiag;
                  A.sl_rl[j] = vo.rloc;
                }
                ntot1 += __popcll(mk);
              }
            };
            for (int g0 = 0; g0 < ns_col; g0 += 256) {
              eval(a0, b0, true);
              ld(g0 + 256, a0, b0);
              eval(a1, b1, g0 + 64 < ns_col);
              ld(g0 + 320, a1, b1);
              eval(a2, b2, g0 + 128 < ns_col);
              ld(g0 + 384, a2, b2);
              eval(a3, b3, g0 + 192 < ns_col);
              ld(g0 + 448, a3, b3);
            }
          }
          if (two) pre_n = ntot1;
          n = ntot;
        }
      }
    } else if (FUSED == 2 && A.mode == 2) {
      n = -1;                                  // known after the kernel's own walk over the sorting mesh
      if (A.beta) beta = A.beta[pt];
    } else {
      n = A.nobsl[pt];
    }
    if (A.skip_trivial && (n == 0 || beta == 0.0)) {   // done by the streaming pass (letkf_trivial.hip)
      if (beta != 0.0) have_u = false;         // (as below: a point without observations leaves no eigenvectors behind,
      continue;                                //  a beta = 0 point does not touch the run's)
    }
    // per-lane member offset, laundered so that LICM does not park 2*NV hoisted 64-bit offsets in VGPRs
    long moff = (long)lane * A.sm;
    asm volatile("" : "+v"(moff));
    const double* g0 = A.gues ? A.gues + pt * A.sp : nullptr;
    double* a0 = A.anal ? A.anal + pt * A.sp : nullptr;

    if (das && beta == 0.0) {                  // letkf_tools.f90:333-359
      for (int v = 0; v < nv; ++v) {
        if (lane < k && ((A.var_mask >> v) & 1u)) a0[moff + v * A.sv] = g0[k * A.sm + v * A.sv] + g0[moff + v * A.sv];
      }
      const bool mine = lane < nv && ((A.var_mask >> lane) & 1u);
      if (A.det_run && mine) a0[(k + 1) * A.sm + lane * A.sv] = g0[(k + 1) * A.sm + lane * A.sv];
      if (A.rtps_out && mine) A.rtps_out[pt + A.infl_sv * (long)lane] = 1.0;
      if (lane == 0) {
        if (A.status) A.status[pt] = 0;
        if (A.nsweep) A.nsweep[pt] = 0;
        if (A.nobs_out) A.nobs_out[pt] = 0;
      }
      continue;
    }

    bool qskip = false;
    if (das && A.q_update_top > 0.0) qskip = g0[k * A.sm + A.iv_p * A.sv] < A.q_update_top;
    // (rules_dev::q_update_skipped and solve_inflation, restated: as calls they move this kernel's register allocation)
    int v0 = 0;
    while (v0 < nv && (!((A.var_mask >> v0) & 1u) || (qskip && v0 >= A.iv_q_first && v0 <= A.iv_q_last))) ++v0;
    double* infl_p = das ? ((v0 < nv) ? &A.infl[pt + A.infl_sv * (long)v0] : nullptr) : &A.infl[pt];
    const double infl_old = infl_p ? *infl_p : 1.0;

    PROF_MARK(0)
    // ------------------------------------------------------------ Gram on the FP64 matrix cores
    // A_aug = Ya^T Ya with Ya = sqrt(w) * [y_1 .. y_k | dep | dep_det]  (n x (k+2)), v_mfma_f64_16x16x4:
    // 4 obs per step.  Lane l supplies, for member block I, Ya[obs0 + (l>>4)][16 I + (l&15)] -- the SAME register
    // is the A operand of tile (I,*) and the B operand of tile (*,I), so the rows are loaded straight from the obs
    // table into MFMA operand layout (128-B coalesced segments), no LDS staging, no broadcast reads; only the
    // tiles I <= J are accumulated.  Column k of A_aug is r = Ys^T sqrt(w) dep, column k+1 the deterministic one,
    // entry (k,k) = sum w dep^2 (parm(1) of the adaptive inflation, common_letkf.f90:233-237).
    double g[KR];
    double racc = 0.0, rdacc = 0.0, p1 = 0.0, p3 = 0.0;
    int sweeps = 0, jconv = 1;
    double lam = km1 / infl_old;               // n == 0: T = sqrt(rho) I, Pa = rho/(k-1) I (common_letkf.f90:89-107)
    bool colvalid = lane < k;                  // does this lane hold an eigen-column?

    bool solved = false;
    if (n != 0) {
      constexpr int NBLK = (KR + 2 + 15) / 16;                 // member blocks incl. the 2 augmented columns
      constexpr int KMIN = (NW == 1) ? wave_kmin(KR, NW) : 1;  // launch_wave_kernel: this instantiation serves wave_kmin <= k <= KR
      // STRIP (r4): where the last block is narrow at compile time -- KR = 50: members 48, 49 and the two augmented columns, 4 of 16;
      // KR = 20: members 16 .. 19 + 2 -- its row / column of tiles does not go to the matrix cores (four 16 x 16 tiles of which
      // 3/4 are padding: 4 of the 10 instructions of a step at k = 50) but to RS x NBLK broadcast-FMAs per step: lane (q, c)
      // accumulates accS[a][I] += Ya[obs_q][16 S + a] * Ya[obs_q][16 I + c] over its own observations (summed over q at the end).
#ifndef LETKF_GRAM_STRIP
#define LETKF_GRAM_STRIP 1
#endif
      constexpr bool STRIP = LETKF_GRAM_STRIP && NW == 1 && (KR == 50 || KR == 20);
      constexpr int NBF = STRIP ? NBLK - 1 : NBLK;             // blocks whose tiles are on the matrix cores
      // The two departure columns do not ride in the narrow block either: sqrt(w) dep is the same number in every lane of an
      // observation's row, so r = Ya^T (sqrt(w) dep) is a plain FMA per block (accD, accDD; entry (k, k) = sum w dep^2 likewise:
      // accP) -- no per-step selects that put the departures into the block's lanes, two broadcast rows fewer.
      constexpr int RS = STRIP ? KR - 16 * (NBLK - 1) : 1;      // member columns of the narrow block (KR = 50: 2, KR = 20: 4)
      static_assert(!STRIP || (RS >= 1 && RS <= 6 && KMIN > 16 * (NBLK - 1)), "the narrow block must be the last one for every k of the instantiation");
      constexpr int NTILE = NBF * (NBF + 1) / 2;
      v4d acc[NTILE];
      [[maybe_unused]] double accS[RS][NBLK], accD[NBLK], accDD[NBLK], accP = 0.0;
#pragma unroll
      for (int I = 0; I < NBLK; ++I) accD[I] = accDD[I] = 0.0;
#pragma unroll
      for (int t = 0; t < NTILE; ++t) acc[t] = v4d{0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int a = 0; a < RS; ++a)
#pragma unroll
        for (int I = 0; I < NBLK; ++I) accS[a][I] = 0.0;
      int q = wlane >> 4, c16 = wlane & 15;
      asm volatile("" : "+v"(q), "+v"(c16));   // (not loop-invariant for hipcc: see the apply phase)

      // Two phases per batch of kSC observations, so that the per-observation scalars are computed ONCE (lane = obs,
      // coalesced reads of the CSR slice, all gathers of a batch in flight together) instead of 16 times over in
      // every 4-obs MFMA step -- the first version spent ~250 VALU instructions and a dozen s_waitcnt per 4 obs in
      // its load pipeline, as much SIMD time as a Jacobi sweep per point:
      //   stage: lane i -> obs i: row base, sqrt(w), sqrt(w) dep, sqrt(w) dep_det into LDS (4 doubles per obs)
      //   MFMA : per 4-obs step 2 ds_read_b128 + NBLK row loads (three steps in flight) + NBLK multiplies
      constexpr int kSC = 256;                                 // obs per batch (4 kSC doubles <= wave_base_doubles of the slice)
      double* stg = slice;
      // TRIM (r13, default on; -DLETKF_GRAM_TRIM=0 gives the loop as it was for an A/B; one-wave instantiations only): the tile
      // loop issues nothing per step that its result does not need.
      //  * A step past the end is fetched (the pipeline has no conditions around its loads) but never consumed, so its weights
      //    are not selected to zero, and its chunk index is not clamped: behind the nsp entries of a batch the stage phase
      //    leaves kPad entries with the row base of the batch's FIRST entry and zero weights (every batch that reaches
      //    run_steps has one: nsp > 0), which is all the fetches can reach -- chunk nch + 2 kGramDepth - 2 at most.  No row
      //    base that the stage of THIS batch did not write becomes a load address; the padding of the last step (entries
      //    ns .. nsp - 1, which ARE consumed, with weight zero) carries that row base too, not row 0 of the table.
      //  * STRIP: the narrow block is not masked per step.  Its lanes at and past member k hold member 0 of the row (the
      //    clamped offset below), times sqrt(w): finite.  No matrix instruction reads that operand; what those lanes and the
      //    broadcast members >= k add up is zeroed once per point behind the loop (accS, racc, rdacc) or lies in columns >= k
      //    of the matrix, which the eigenproblem's column mask (colzero) clears.
      //  * The das instantiations (NV > 0) read the obs table, always (launch_wave refuses the dense batch for them), and a
      //    block below the smallest k of the instantiation needs no clamp: the row offsets are constants.
#ifndef LETKF_GRAM_TRIM
#define LETKF_GRAM_TRIM 1
#endif
      constexpr bool TRIM = LETKF_GRAM_TRIM && NW == 1;
      constexpr int kPad = 4 * (2 * kGramDepth - 1);           // TRIM: staged entries behind nsp that a fetch can reach
      static_assert(!TRIM || 4 * (kSC + kPad) <= wave_base_doubles(KR, NW), "the padded staging area must fit the Gram's part of the slice");
      const bool mode0 = (TRIM && NV > 0) || A.mode != 1;      // rows come from the obs table (member-fastest)
      const double* ybase = mode0 ? A.ensval : A.hdxb;
      bool rowok[NBLK];
      long mo[NBLK];
#pragma unroll
      for (int I = 0; I < NBLK; ++I) {
        const int m = 16 * I + c16;
        rowok[I] = m < k;
        // (the last block's clamp stays: a row holds kld >= k doubles, and a lane must not read past the table's last row)
        const long mm = (TRIM && 16 * (I + 1) <= KMIN) ? m : rowok[I] ? m : 0;
        mo[I] = mode0 ? mm : mm * (long)A.nobs;
      }
      // TRIM: entries [from, upto) of the staging area <- (row base rb0, weights zero); upto - from <= 64
      [[maybe_unused]] auto stage_pad = [&](const int from, const int upto, const long rb0) {
        if (wlane < upto - from) {
          *reinterpret_cast<double2*>(&stg[4 * (from + wlane)]) = double2{__longlong_as_double(rb0), 0.0};
          *reinterpret_cast<double2*>(&stg[4 * (from + wlane) + 2]) = double2{0.0, 0.0};
        }
      };
      const bool is_d = c16 == (k & 15), is_dd = c16 == ((k + 1) & 15);   // lanes of the two augmented columns
      const int blk_d = k >> 4, blk_dd = (k + 1) >> 4;
      struct Step {
        double f[NBLK];
        double sw, dsw, ddsw;
      };

      // MFMA steps of 4 obs over the first nsp (multiple of 4) staged entries; with two waves each takes every other step
      auto run_steps = [&](const int nsp) {
        // (TRIM: the step count on the scalar unit -- the observation count comes from a vector value, the point number)
        const int nch = TRIM ? uniform(nsp >> 2) : nsp >> 2;
        auto fetch = [&](const int c, Step& t) {
          if constexpr (TRIM) {
            const int i = 4 * c + q;                            // unclamped: see stage_pad
            const double2 a2 = *reinterpret_cast<const double2*>(&stg[4 * i]);
            const double2 b2 = *reinterpret_cast<const double2*>(&stg[4 * i + 2]);
            const long rb = __double_as_longlong(a2.x);
            t.sw = a2.y;
            t.dsw = b2.x;
            t.ddsw = b2.y;
#pragma unroll
            for (int I = 0; I < NBLK; ++I) t.f[I] = ybase[rb + mo[I]];
          } else {
          const bool ok = c < nch;
          const int i = 4 * (ok ? c : 0) + q;
          const double2 a2 = *reinterpret_cast<const double2*>(&stg[4 * i]);
          const double2 b2 = *reinterpret_cast<const double2*>(&stg[4 * i + 2]);
          const long rb = __double_as_longlong(a2.x);
          t.sw = ok ? a2.y : 0.0;
          t.dsw = ok ? b2.x : 0.0;
          t.ddsw = ok ? b2.y : 0.0;
#pragma unroll
          for (int I = 0; I < NBLK; ++I) t.f[I] = ybase[rb + mo[I]];
          }
        };
        auto mma = [&](const Step& t) {
          double y[NBLK];
#pragma unroll
          for (int I = 0; I < NBLK; ++I) {
            double v = t.f[I] * t.sw;
            // (blocks that lie below the smallest k this instantiation is dispatched for are all members at compile
            // time: hipcc turns the wave-uniform test into 9 v_cndmask per block and step otherwise)
            if (16 * (I + 1) > KMIN && 16 * (I + 1) > k) {     // wave-uniform: block reaches past the members
              if constexpr (!(TRIM && STRIP)) v = rowok[I] ? v : 0.0;   // (TRIM: the narrow block is cleaned up behind the loop)
              if constexpr (!STRIP) {
                if (I == blk_d && is_d) v = t.dsw;
                if (I == blk_dd && is_dd) v = t.ddsw;
              }
            }
            y[I] = v;
          }
          if constexpr (STRIP) {
#pragma unroll
            for (int I = 0; I < NBLK; ++I) {
              accD[I] = fma(y[I], t.dsw, accD[I]);
              accDD[I] = fma(y[I], t.ddsw, accDD[I]);
            }
            accP = fma(t.dsw, t.dsw, accP);
          }
          int tt = 0;
#pragma unroll
          for (int I = 0; I < NBF; ++I)
#pragma unroll
            for (int J = I; J < NBF; ++J) {
              acc[tt] = __builtin_amdgcn_mfma_f64_16x16x4f64(y[I], y[J], acc[tt], 0, 0, 0);
              ++tt;
            }
          if constexpr (STRIP) {
            auto strip_row = [&](auto a_) {
              constexpr int a = decltype(a_)::value;
              if constexpr (a < RS) {
#pragma unroll
                for (int I = 0; I < NBLK; ++I) {
                  if (a == 0 && I == 0) fmac_row_bcast<a, true>(accS[a][I], y[NBLK - 1], y[I]);
                  else fmac_row_bcast<a, false>(accS[a][I], y[NBLK - 1], y[I]);
                }
              }
            };
            strip_row(std::integral_constant<int, 0>{});
            strip_row(std::integral_constant<int, 1>{});
            strip_row(std::integral_constant<int, 2>{});
            strip_row(std::integral_constant<int, 3>{});
            strip_row(std::integral_constant<int, 4>{});
            strip_row(std::integral_constant<int, 5>{});
          }
        };
        // PD steps in flight.  Three things keep the pipeline the way it is written (each found in the ISA):
        //  * no conditions around the fetches (a step past the end is fetched from a valid row and never given to mma: the
        //    wave-uniform test in front of each mma below, and the loop condition for u = 0, keep it out of every sum): with
        //    branches hipcc can no longer count the loads in flight and waits for ALL of them -- s_waitcnt vmcnt(0) --
        //    at the top of every iteration, one exposed L2 latency per iteration;
        //  * the empty asm statements keep each fetch where it is written: left alone, hipcc rotates the loop so that
        //    all loads sit at the top of the iteration that consumes them;
        //  * the loaded rows are routed through one just before their use: otherwise the multiplies of the LATER steps
        //    are hoisted to the top of the iteration and wait for the youngest loads there.
        if constexpr (NW == 1) {
          constexpr int PD = kGramDepth;
          Step ts[PD];
#pragma unroll
          for (int u = 0; u < PD; ++u) {
            fetch(wvp + u * NW, ts[u]);
            asm volatile("" ::: "memory");       // (same order as in the loop: the waits are counted statically)
          }
          auto pin = [&](Step& t) {
#pragma unroll
            for (int I = 0; I < NBLK; ++I) asm volatile("" : "+v"(t.f[I])::"memory");
          };
          for (int c = wvp; c < nch; c += PD * NW) {
#pragma unroll
            for (int u = 0; u < PD; ++u) {
              pin(ts[u]);
              if (u == 0 || c + u * NW < nch) mma(ts[u]);   // (wave-uniform; only the matrix instructions are skipped)
              fetch(c + (PD + u) * NW, ts[u]);
            }
          }
        } else {
          // two-wave points (up to 7 member blocks, part of the register file in AGPRs) keep the plain loop; their
          // register allocation is fragile -- the compile-time full blocks (KMIN) alone cost k = 100 a quarter of its
          // speed (162 k -> 116 k solves/s, A/B on one box), so none of the one-wave changes is applied to them
          Step t0, t1, t2;
          fetch(wvp, t0);
          fetch(wvp + NW, t1);
          fetch(wvp + 2 * NW, t2);
          for (int c = wvp; c < nch; c += 3 * NW) {
            mma(t0);
            fetch(c + 3 * NW, t0);
            if (c + NW < nch) {
              mma(t1);
              fetch(c + 4 * NW, t1);
            }
            if (c + 2 * NW < nch) {
              mma(t2);
              fetch(c + 5 * NW, t2);
            }
          }
        }
      };

      if (FUSED == 2 && A.mode == 2) {
        // ---- obs_local fused in (no-limit mode, scale/letkf/letkf_tools.f90:1438-1476): walk the rectangle of
        // sorting-mesh cells of every observation type exactly like letkf_search_kernel, evaluate obs_local_cal per
        // lane for 64 candidate rows at a time, and append the accepted ones (ballot + prefix popcount: the
        // reference's list order) straight to the staging buffer -- the local list never exists in memory.
        if constexpr (NW == 1 && FUSED == 2) {
          using namespace search_dev;
          const letkf_search_tables& t = A.stab;
          const double ri = A.pri[pt], rj = A.prj[pt], rlev = A.prlev[pt], rz = A.prz[pt];
          const unsigned long long lt_mask = lanes_below(wlane);
          int cnt = 0, ntot = 0, nconv = 0;                   // staged entries / accepted so far / entries at the front
                                                              // that are already in final form (wave-uniform)
          // stage buffer, phase A: (row, rdiag, rloc) as the candidates are accepted; phase B (convert): lane = entry,
          // all dep / dep_det gathers of the batch in flight together -> (row base, sqrt(w), sqrt(w) dep, sqrt(w) dep_det)
          auto convert = [&]() {
            for (int i = nconv + wlane; i < cnt; i += 64) {
              const double2 a2 = *reinterpret_cast<const double2*>(&stg[4 * i]);
              const double rloc_ = stg[4 * i + 2];
              const long row = __double_as_longlong(a2.x);
              const long rb = row * A.kld;
              const double d = A.dep[row];
              const double dd = A.det_run ? A.ensval[rb + k] : 0.0;
              const double sw = fast_rsqrt(a2.y);
              p3 += rloc_;
              *reinterpret_cast<double2*>(&stg[4 * i]) = double2{__longlong_as_double(rb), sw};
              *reinterpret_cast<double2*>(&stg[4 * i + 2]) = double2{d * sw, dd * sw};
            }
          };
          struct Meta {
            double lev, dat, ori, orj, err;
          };
          psync<NW>();
          for (int m = 0; m < t.group_start[t.ngroup]; ++m) {
            const int ic = t.group_member[m];
            const int vm = t.vmode[ic];
            // search_dev::cell_rect restated (as a call it moves this kernel's scratch: profiles/r10_README.md)
            const double dzi = t.hori_loc[ic] * kDistZeroFac / t.dx;
            const double dzj = t.hori_loc[ic] * kDistZeroFac / t.dy;
            int imin, imax, jmin, jmax;
            ij_obsgrd_ext(t, ic, ri - dzi, rj - dzj, imin, jmin);
            ij_obsgrd_ext(t, ic, ri + dzi, rj + dzj, imax, jmax);
            imin = max(imin, 1);
            jmin = max(jmin, 1);
            imax = min(imax, t.ngrdext_i[ic]);
            jmax = min(jmax, t.ngrdext_j[ic]);
            if (imin > imax || jmin > jmax) continue;
            const long acb = t.ac_off[ic];
            const int ld = t.ngrdext_i[ic] + 1;
            // metadata of the candidate rows [base, base + 64): loaded one chunk AHEAD of its evaluation (the first
            // version loaded and evaluated chunk by chunk and waited three dependent memory round trips per chunk --
            // 165 ms per C2 analysis against 59 ms for the stand-alone search kernel)
            auto load_meta = [&](const int base, const int hi) -> Meta {
              Meta q_{1.0, 1.0, 0.0, 0.0, 1.0};
              const int row = base + wlane;
              if (row < hi) {
                if (vm != 2 && vm != 3) q_.lev = t.ob_lev[row];
                if (vm == 2) q_.dat = t.ob_dat[row];
                q_.ori = t.ob_ri[row];
                q_.orj = t.ob_rj[row];
                q_.err = t.ob_err[row];
              }
              return q_;
            };
            for (int j0 = jmin; j0 <= jmax; j0 += 64) {                      // 64 mesh rows at a time: lane = row
              const int nr = min(64, jmax - j0 + 1);
              int lo_l = 0, hi_l = 0;
              if (wlane < nr) {                                              // search_dev::row_span restated, lane = mesh row
                lo_l = t.ac_ext[acb + (imin - 1) + (long)ld * (j0 + wlane - 1)];
                hi_l = t.ac_ext[acb + imax + (long)ld * (j0 + wlane - 1)];
              }
              int r = 0;
              int base = __shfl(lo_l, 0, 64), hi = __shfl(hi_l, 0, 64);
              auto skip_empty = [&]() {
                while (r < nr && base >= hi) {
                  ++r;
                  if (r < nr) {
                    base = __shfl(lo_l, r, 64);
                    hi = __shfl(hi_l, r, 64);
                  }
                }
              };
              skip_empty();
              Meta cur{1.0, 1.0, 0.0, 0.0, 1.0};
              if (r < nr) cur = load_meta(base, hi);
              while (r < nr) {
                const int cb = base, chi = hi;
                base += 64;
                skip_empty();
                Meta nxt{1.0, 1.0, 0.0, 0.0, 1.0};
                if (r < nr) nxt = load_meta(base, hi);
                const int row = cb + wlane;
                CalOut c{0.0, -1.0, -1.0};
                if (row < chi) c = local_cal_v(t, ic, ri, rj, rlev, rz, cur.lev, cur.dat, cur.ori, cur.orj, cur.err);
                const bool acc_ = c.rloc != 0.0;                             // :1460
                const unsigned long long mk = __ballot(acc_);
                if (acc_) {
                  const int i = cnt + __popcll(mk & lt_mask);
                  *reinterpret_cast<double2*>(&stg[4 * i]) = double2{__longlong_as_double((long)row), c.rdiag};
                  stg[4 * i + 2] = c.rloc;
                }
                const int na = __popcll(mk);
                cnt += na;
                ntot += na;
                if (cnt > kSC - 64) {                                        // room for one more chunk is gone
                  const int nuse = cnt & ~3;
                  psync<NW>();
                  convert();
                  psync<NW>();
                  if constexpr (TRIM) {                                      // behind the 0..3 left-over entries: stale candidates
                    stage_pad(cnt, nuse + kPad, __double_as_longlong(stg[0]));
                    psync<NW>();
                  }
                  run_steps(nuse);
                  psync<NW>();
                  // the 0..3 left-over entries (already converted) move to the front
                  double2 l0{0.0, 0.0}, l1{0.0, 0.0};
                  if (wlane < cnt - nuse) {
                    l0 = *reinterpret_cast<const double2*>(&stg[4 * (nuse + wlane)]);
                    l1 = *reinterpret_cast<const double2*>(&stg[4 * (nuse + wlane) + 2]);
                  }
                  psync<NW>();
                  if (wlane < cnt - nuse) {
                    *reinterpret_cast<double2*>(&stg[4 * wlane]) = l0;
                    *reinterpret_cast<double2*>(&stg[4 * wlane + 2]) = l1;
                  }
                  cnt -= nuse;
                  nconv = cnt;
                }
                cur = nxt;
              }
            }
          }
          psync<NW>();
          convert();
          const int nsp = (cnt + 3) & ~3;
          if constexpr (TRIM) {                                              // pad the last step and what the fetches reach behind it
            if (cnt > 0) {                                                   // (wave-uniform; entry 0 is in final form)
              psync<NW>();
              stage_pad(cnt, nsp + kPad, __double_as_longlong(stg[0]));
            }
          } else
          if (wlane < nsp - cnt) {                                           // pad the last step with weight-0 rows
            *reinterpret_cast<double2*>(&stg[4 * (cnt + wlane)]) = double2{0.0, 0.0};
            *reinterpret_cast<double2*>(&stg[4 * (cnt + wlane) + 2]) = double2{0.0, 0.0};
          }
          psync<NW>();
          if (nsp > 0) run_steps(nsp);                                       // (an empty buffer has no valid row to prefetch)
          n = ntot;
        }
      } else
      for (int s0 = 0; s0 < n; s0 += kSC) {
        const int ns = min(kSC, n - s0);
        const int nsp = (ns + 3) & ~3;
        psync<NW>();                                           // the previous batch has been consumed
        // ---- stage
        constexpr int NPASS = kSC / NL;
        int iob[NPASS];
        double rdv[NPASS], rlv[NPASS], dv[NPASS], ddv[NPASS];
#pragma unroll
        for (int ps = 0; ps < NPASS; ++ps) {
          const int i = ps * NL + lane;
          iob[ps] = 0;
          rdv[ps] = 1.0;
          rlv[ps] = 0.0;
          dv[ps] = 0.0;
          ddv[ps] = 0.0;
          if (i < ns) {
            if (mode0) {
              const long e = o0 + s0 + i;
              iob[ps] = A.obs_idx[e];
              rlv[ps] = A.rloc_l[e];
              rdv[ps] = A.rdiag_l[e];
            } else {
              const long e = pt * (long)A.nobs + s0 + i;
              rlv[ps] = A.rloc[e];
              rdv[ps] = A.rdiag[e];
              dv[ps] = A.depv[e];
              if (A.depd) ddv[ps] = A.depd[e];
            }
          }
        }
        if (mode0) {
#pragma unroll
          for (int ps = 0; ps < NPASS; ++ps) {
            const int i = ps * NL + lane;
            if (i < ns) {
              dv[ps] = A.dep[iob[ps]];
              if (A.det_run) ddv[ps] = A.ensval[(long)iob[ps] * A.kld + k];
            }
          }
        }
        // TRIM: the row base of the batch's first entry (lane 0 of pass 0; ns > 0) for every padding entry
        long rb0 = 0;
        if constexpr (TRIM) {
          rb0 = mode0 ? (long)uniform(iob[0]) * A.kld : pt * (long)A.nobs * (long)k + s0;
          stage_pad(nsp, nsp + kPad, rb0);
        }
#pragma unroll
        for (int ps = 0; ps < NPASS; ++ps) {
          const int i = ps * NL + lane;
          if (i < nsp) {
            // sqrt(w) with w = 1/rdiag (or rloc/rdiag): one rsqrt + Newton instead of an IEEE division and sqrt
            double sw = 0.0;
            long rb = rb0;
            if (i < ns) {
              sw = fast_rsqrt(rdv[ps]);
              if (!mode0 && !A.rdiag_wloc) sw *= sqrt(rlv[ps]);
              rb = mode0 ? (long)iob[ps] * A.kld : pt * (long)A.nobs * (long)k + (s0 + i);
              p3 += rlv[ps];
            }
            *reinterpret_cast<double2*>(&stg[4 * i]) = double2{__longlong_as_double(rb), sw};
            *reinterpret_cast<double2*>(&stg[4 * i + 2]) = double2{dv[ps] * sw, ddv[ps] * sw};
          }
        }
        psync<NW>();
        run_steps(nsp);
      }
      PROF_MARK(1)
      if (n > 0) {
      solved = true;
      // accumulator tiles -> "lane j owns column j": 16 rows at a time through LDS.  C/D layout of the f64 MFMA:
      // lane l holds rows (l>>4) + 4*reg, column l&15 of its 16x16 tile.
      constexpr int LDA = 18;
      double* abuf = slice;                                    // [64 NW][LDA], spans the tile + bmat regions
      // diagonal: trace for the adaptive inflation, then the shift (common_letkf.f90:140-143)
      [[maybe_unused]] const double shift = (NW == 1) ? km1 / infl_old : 0.0;   // (two-wave points: where it was, below)
      double diag = 0.0;
      [[maybe_unused]] int ln = lane;                          // (laundered: what is built from it is built per point, not fetched)
      if constexpr (NW == 1) asm volatile("" : "+v"(ln));
      if constexpr (STRIP) {                                   // the narrow block's sums over the four observation residues q
        if constexpr (TRIM) {
          // the block went into the sums unmasked: a broadcast member at or past k (wave-uniform; none below the smallest k of
          // the instantiation) leaves zeros, as its masked lane did
#pragma unroll
          for (int a = 0; a < RS; ++a)
            if (16 * (NBLK - 1) + a >= KMIN && 16 * (NBLK - 1) + a >= k) {
#pragma unroll
              for (int I = 0; I < NBLK; ++I) accS[a][I] = 0.0;
            }
        }
#pragma unroll
        for (int a = 0; a < RS; ++a)
#pragma unroll
          for (int I = 0; I < NBLK; ++I) {
            accS[a][I] += wshfl_xor(accS[a][I], 16);
            accS[a][I] += wshfl_xor(accS[a][I], 32);
          }
#pragma unroll
        for (int I = 0; I < NBLK; ++I) {
          accD[I] += wshfl_xor(accD[I], 16);
          accD[I] += wshfl_xor(accD[I], 32);
          accDD[I] += wshfl_xor(accDD[I], 16);
          accDD[I] += wshfl_xor(accDD[I], 32);
        }
        accP += wshfl_xor(accP, 16);
        accP += wshfl_xor(accP, 32);
        // lane j = 16 q + c owns column j: its r_j, r_det_j are block q's sums (every lane (., c) holds the sums of all blocks)
        racc = rdacc = 0.0;
#pragma unroll
        for (int I = 0; I < NBLK; ++I)
          if (q == I) {
            racc = accD[I];
            rdacc = accDD[I];
          }
        if constexpr (TRIM) {                                  // (the narrow block's lanes at and past k: member 0's sums)
          racc = ln < k ? racc : 0.0;
          rdacc = ln < k ? rdacc : 0.0;
        }
        p1 = accP;                                             // A_aug[k][k] = sum w dep^2
      }
#pragma unroll
      for (int I = 0; I < NBLK; ++I) {
        psync<NW>();
        // wave 0 stores its partial tiles, wave 1 (two-wave points) adds its own on top
#pragma unroll
        for (int pass = 0; pass < NW; ++pass) {
          if (pass == 1) __syncthreads();
          if (wvp == pass) {
            if constexpr (STRIP) {
              // rows of block I < S: the columns 16 S + a are accS[a][I] (lane c = the row); rows of block S (a < RS): every
              // column 16 J + c is accS[a][J] -- element (row, col) at abuf[col * LDA + row-in-block], as the tiles below.
              // (Every q row writes -- the same values, folded above: NOT `if (q == 0)`.  At the join of that branch hipcc put a
              // register spill in front of the exec restore in letkf_wave_kernel<20, 11, false> -- the defect of DESIGN.md section 8,
              // caught by tools/isa_exec_audit.py at build time when wave_sum changed the allocation.)
              {
                if (I < NBLK - 1) {
#pragma unroll
                  for (int a = 0; a < 16; ++a) abuf[(16 * (NBLK - 1) + a) * LDA + c16] = a < RS ? accS[a][I] : 0.0;   // (the padding columns: zeros, as the tiles left them)
                } else {
#pragma unroll
                  for (int J = 0; J < NBLK; ++J)
#pragma unroll
                    for (int a = 0; a < RS; ++a) abuf[(16 * J + c16) * LDA + a] = accS[a][J];
                }
              }
            }
#pragma unroll
            for (int J = 0; J < NBF; ++J) {
              if (STRIP && I == NBLK - 1) continue;            // (the narrow block's rows: written above)
              const int ti = I <= J ? I : J, tj = I <= J ? J : I;
              const int t = ti * NBF - ti * (ti - 1) / 2 + (tj - ti);
#pragma unroll
              for (int reg = 0; reg < 4; ++reg) {
                const int a = q + 4 * reg, b = c16;            // tile-local (row, col) of this element
                // rows of block I, columns of block J: element (I:a, J:b) directly, or the mirror of tile (J, I)
                double* dst = (I <= J) ? &abuf[(16 * J + b) * LDA + a] : &abuf[(16 * J + a) * LDA + b];
                if (pass == 0) *dst = acc[t][reg];
                else *dst += acc[t][reg];
              }
            }
          }
        }
        psync<NW>();
        if constexpr (NW == 1) {
          // Every lane reads (the lanes past the last block a copy of its last row; their g is zeroed below, racc / rdacc keep
          // their value through a select): NOT `if (lane < 16 * NBLK)`.  Behind the join of that branch hipcc (ROCm 7.2) put the
          // copies of a live-range split IN FRONT of the instruction that re-enables the lanes which skipped it -- found in
          // letkf_wave_kernel<16, 11, true> and <20, 0, true>: the run scheduler's `pend` saved for lanes 0..31 only and restored
          // for all 64, lanes 32..63 walked on into points that were not theirs with a stale slice (memory fault).  tools/
          // isa_exec_audit.py looks for that pattern in every unit's ISA; the Makefile runs it on every build.
          const int lrow = lane < 16 * NBLK ? lane : 16 * NBLK - 1;
          const bool mine = lane < 16 * NBLK;
          {
            // (r12) the diagonal, while the column is still in LDS: lane j < k owns A[j][j], element j & 15 of its row in the pass
            // of block j >> 4 -- the trace takes it as it is and the shift goes on top before the column is read.  (As 50 masked
            // adds in registers, `if (r == lane && lane < k)`, every row had a lane mask of its own, all hoisted out of the point
            // loop and fetched from a spill register by two v_readlane_b32 each.)  No branch: a lane that owns nothing in this
            // pass stores what it read into the padding of its row (elements 16, 17 of LDA = 18 are never read).
            const bool own = (ln >> 4) == I && ln < k;
            double* const dp = &abuf[lrow * LDA + (ln & 15)];
            const double d = *dp;
            diag = own ? d : diag;
            *(own ? dp : &abuf[lrow * LDA + 16]) = own ? d + shift : d;
            psync<NW>();
          }
#pragma unroll
          for (int e = 0; e < 16; e += 2) {
            if (16 * I + e < KR) {
              const double2 v2 = *reinterpret_cast<const double2*>(&abuf[lrow * LDA + e]);
              g[16 * I + e] = v2.x;
              g[16 * I + e + 1] = v2.y;
            }
          }
          if constexpr (!STRIP) {
            if ((k >> 4) == I) {
              const double t = abuf[lrow * LDA + (k & 15)];
              racc = mine ? t : racc;
            }
            if (((k + 1) >> 4) == I) {
              const double t = abuf[lrow * LDA + ((k + 1) & 15)];
              rdacc = mine ? t : rdacc;
            }
          }
        } else if (lane < 16 * NBLK) {
#pragma unroll
          for (int e = 0; e < 16; e += 2) {
            if (16 * I + e < KR) {
              const double2 v2 = *reinterpret_cast<const double2*>(&abuf[lane * LDA + e]);
              g[16 * I + e] = v2.x;
              g[16 * I + e + 1] = v2.y;
            }
          }
          if constexpr (!STRIP) {
            if ((k >> 4) == I) racc = abuf[lane * LDA + (k & 15)];
            if (((k + 1) >> 4) == I) rdacc = abuf[lane * LDA + ((k + 1) & 15)];
          }
        }
        if constexpr (!STRIP) {
          if ((k >> 4) == I) p1 = abuf[k * LDA + (k & 15)];    // A_aug[k][k] = sum w dep^2
        }
      }
      psync<NW>();
      // rows >= k of a column (the augmented rows) and whole columns >= k play no part in the eigenproblem
      if constexpr (NW == 1) {
        // (r12) one lane mask for the columns, made here from the laundered lane number, and a wave-uniform test for the rows --
        // only those at and above the smallest k the instantiation is launched for (launch_wave) can be augmented rows
        const bool colzero = ln >= k || ln >= 16 * NBLK;
        int ku = k;
        asm volatile("" : "+s"(ku));
#pragma unroll
        for (int r = 0; r < KR; ++r) {
          g[r] = colzero ? 0.0 : g[r];
          if (r >= KMIN && r >= ku) g[r] = 0.0;
        }
      } else {
#pragma unroll
        for (int r = 0; r < KR; ++r)
          if (r >= k || lane >= k || lane >= 16 * NBLK) g[r] = 0.0;
        // diagonal: trace for the adaptive inflation, then the shift (common_letkf.f90:140-143)
        const double shift2 = km1 / infl_old;
#pragma unroll
        for (int r = 0; r < KR; ++r) {
          if (r == lane && lane < k) {
            diag = g[r];
            g[r] += shift2;
          }
        }
      }
      double parm1 = 0.0, parm2 = 0.0, parm3 = 0.0;
      if (A.infl_adaptive) {
        parm1 = p1;
        parm3 = preduce<NW, 0>(p3, red, rslot);
        parm2 = preduce<NW, 0>(lane < k ? diag : 0.0, red, rslot) / km1;
      }

      PROF_MARK(2)
      // ------------------------------------------------------------ eigen-decomposition in registers
      if (have_u && !(A.warm_dbg & 1)) {
        if constexpr (LETKF_WARM_STRIP && NW == 1 && KR == 50) warm_start_product_strip<KR>(g, uws - lane, slice);
        else if constexpr (NW == 1 && KR <= 50) warm_start_product_mfma<KR>(g, uws - lane, slice);
        else warm_start_product<KR, NW>(g, uws, k, slice);
      }
      PROF_MARK(3)
      sweeps = jacobi_split<KR, NW, wave_jacobi_rc(KR, NW), true, LETKF_INPLACE_NW(KR, NW)>(g, k, A.max_sweep, slice, nullptr, &jconv);   // exchange buffer: 64*10 + 64*4 doubles of the tile+bmat region
      // per-lane values that were spilled around the eigensolve come back HERE, in one batch: reloaded lazily, each
      // scratch load sits behind the 50 workspace stores below and its s_waitcnt vmcnt(0) waits for all of them
      asm volatile("" : "+v"(racc), "+v"(rdacc), "+v"(moff));
      PROF_MARK(4)

      double ss = 0.0;
#pragma unroll
      for (int r = 0; r < KR; ++r) ss = fma(g[r], g[r], ss);
      lam = sqrt(ss);
      colvalid = ss > 0.0;     // after the rotate-and-swap sweeps the columns sit in permuted lanes; with an odd k the
                               // inert zero column that pads the line to even length can be anywhere among them
      const double il = colvalid ? 1.0 / lam : 0.0;
#pragma unroll
      for (int r = 0; r < KR; ++r) g[r] *= il;

      if (A.infl_adaptive) p1 = adaptive_inflation(infl_old, parm1, parm2, parm3);   // reuse p1 as infl_new
      }
    }
    // apply phase on the matrix cores (see below); these instantiations also give points without observations a
    // closed-form path that never touches g
    constexpr bool MAPPLY = !KKOUT && NW == 1 && KR <= 50 && NV > 0 && NB <= 14;
    constexpr int kBmRows = 4 * ((KR + 3) / 4), kBmOff = 32 * KR;   // MAPPLY: padded B [kBmRows][16] in the wave's LDS slice
    constexpr int kObOff = (32 * KR >= 1024) ? 0 : kBmOff + 16 * kBmRows + 128;   // MAPPLY: output transposition buffer [64][16], clear of B
    if constexpr (!MAPPLY) {
      if (!solved) {
        if constexpr (NW == 1) {
          int li = lane;                           // (the compares are made here, per point -- see `ln` above)
          asm volatile("" : "+v"(li));
#pragma unroll
          for (int r = 0; r < KR; ++r) g[r] = (r == li && li < k) ? 1.0 : 0.0;
        } else {
#pragma unroll
          for (int r = 0; r < KR; ++r) g[r] = (r == lane && lane < k) ? 1.0 : 0.0;
        }
      }
    }
    const double infl_new = (A.infl_adaptive && n > 0) ? p1 : infl_old;
    double xv[NV > 0 ? NV : 1];                 // MAPPLY: x'_v of member `lane`
    double xm_l = 0.0, xd_l = 0.0;             // MAPPLY: lane v < NV holds x-bar_v and the deterministic member of variable v
    if constexpr (MAPPLY) {
      // the state loads of the apply phase, issued here so that their latency (8-byte accesses npts*8 B apart) runs
      // under the normalisation, the workspace store and the status reductions
      KernArgs* const Ax = fresh_args<NW>(Ak0);
      const long sv_ = Ax->sv, sm_ = Ax->sm;
      const double* gp = g0 + moff;
#pragma unroll
      for (int v = 0; v < NV; ++v) {
        xv[v] = (lane < k) ? *gp : 0.0;
        gp += sv_;
      }
      if (lane < NV) {
        xm_l = g0[k * sm_ + lane * sv_];
        xd_l = Ax->det_run ? g0[(k + 1) * sm_ + lane * sv_] : 0.0;
      }
      asm volatile("" ::: "memory");
    }
    {
      // leave the eigenvectors behind for the next point of the run.  Here, while g is still entirely in registers:
      // further down part of it is spilled, and a store loop that alternates scratch reloads with global stores
      // pays one store-acknowledge latency per element (s_waitcnt vmcnt counts both) -- measured 41 us per point.
      if (uws && solved && !(A.warm_dbg & 2)) {
        // (the pointer is laundered every 8 rows: otherwise all KR row addresses are hoisted out of the point loop
        // as 64-bit values, spilled, and reloaded one by one in front of each store -- same serialisation)
        unsigned long long pa = reinterpret_cast<unsigned long long>(uws);
        if constexpr (LETKF_WARM_SORT && NW == 1) {
          // column `lane` goes to the workspace column of its rank by eigenvalue (warm_rank, warm_position); warm_dbg bit 4:
          // lane order, bit 5: position = rank
          int rk = warm_rank<KR>(lam, colvalid, lane);
          if constexpr (LETKF_WARM_ORDER) {
            const int nvalid = __popcll(__ballot(colvalid && lane < (KR < 64 ? KR : 64)));
            if (lane < (KR < 64 ? KR : 64) && !(A.warm_dbg & 32)) rk = warm_position(rk, nvalid);
          }
          pa += (long long)(((A.warm_dbg & 16) ? lane : rk) - lane) * (long long)sizeof(double);
        }
#pragma unroll
        for (int r = 0; r < KR; ++r) {
          if ((r & 7) == 0) asm volatile("" : "+v"(pa));
          ((gdouble*)pa)[(size_t)(r & 7) * NL] = g[r];   // global_store, not flat_store: see warm_start_product_mfma
          if ((r & 7) == 7) pa += 8 * NL * sizeof(double);
        }
      }
    }

    // ------------------------------------------------------------ status
    int st;
    {
      const double lmx = preduce<NW, 1>(colvalid ? lam : 0.0, red, rslot);
      const double lmn = preduce<NW, 2>(colvalid ? lam : 1e300, red, rslot);
      st = eig_status(jconv, A.max_sweep, lmx, lmn);
    }
    // (a point without observations hands nothing on: its V = I would be a cold start anyway)
    have_u = uws != nullptr && st == 0 && solved;
    const Spectra sc = spectra(lam, km1, colvalid);
    const double sc1 = sc.sc1, sc2 = sc.sc2;                  // T spectrum, Pa spectrum

    PROF_MARK(5)
    // ------------------------------------------------------------ apply phase
    // U = V^T B, C = D U, Out = V C.  One-wave points with KR <= 50 run both products on the FP64 matrix cores
    // (MAPPLY); the others (two-wave points, the T / Pa instantiations) keep the LDS-broadcast version below.
    const int mrow_l = lane < KR ? lane : KR - 1;
    double cf[NV > 0 ? NV : 1];
    double out[NB];
    if constexpr (MAPPLY) {
      // The broadcast version is LDS-latency-bound like the old warm-start product was (16 % of the wave time on C2,
      // PROF build).  Here V is parked in LDS 32 columns at a time ([col][row], like A in warm_start_product_mfma --
      // a whole V plus B does not fit the 20 KB slice), and per half h:
      //   U tile il (rows j = 32h + 16 il + i): A operand V[4s+q][j] (ds_read_b64), B operand B[4s+q][c] (c = b < 14)
      //   C = D U on the accumulators: register `reg` of lane (q, c) is U[32h + 16 il + 4 reg + q][c] -- which is
      //     exactly the B-operand layout of contraction step s = 8h + 4 il + reg of Out = V C (j = 4s + q): no exchange
      //   Out tile I (rows m = 4i + I): A operand V[4c + I][4s + q] = 4 consecutive doubles of LDS column 4s+q.
      // var_a of the RTPS factor is summed from the same accumulators, var_g from the B operands.
      if (!solved) {
        // No observations: V = I and every eigenvalue is (k-1)/rho (common_letkf.f90:89-107), so U = B, w-bar = 0 and
        // T x' = sqrt(rho) x' in closed form.  (Besides saving these points the matrix work, this keeps g out of the
        // merge of the two paths: as a 50-register phi it cost every SOLVED point ~15 serialised scratch-to-scratch
        // copies, found in the ISA.)
        out[0] = 0.0;
        out[1] = 0.0;
        wave_lds_sync();
        if (lane < kBmRows) {
#pragma unroll
          for (int v = 0; v < NV; ++v) slice[kBmOff + lane * 16 + 2 + v] = xv[v];
        }
        wave_lds_sync();
#pragma unroll
        for (int v = 0; v < NV; ++v) {
          out[2 + v] = sc1 * xv[v];
          double cfv = 1.0;
          if (A.relax_alpha != 0.0) {
            cfv = 1.0 - A.relax_alpha;
          } else if (A.relax_alpha_spread != 0.0) {   // (rules_dev::relax_factor, restated)
            const double parm = A.relax_to_inflated_prior ? A.infl[pt + A.infl_sv * (long)v] : 1.0;
            const double var_g = wave_sum(xv[v] * xv[v]);
            const double var_a = var_g * uniform(sc2);
            if (var_g > 0.0 && var_a > 0.0)
              cfv = A.relax_alpha_spread * sqrt(var_g * parm / (var_a * km1)) - A.relax_alpha_spread + 1.0;
          }
          cf[v] = uniform(cfv);
          if (A.rtps_out && lane == 0 && ((A.var_mask >> v) & 1u)) {   // (rules_dev::rtps_reported, restated)
            const bool skipv = qskip && v >= A.iv_q_first && v <= A.iv_q_last;
            A.rtps_out[pt + A.infl_sv * (long)v] = (A.relax_alpha == 0.0 && A.relax_alpha_spread != 0.0 && !skipv) ? cfv : 1.0;
          }
        }
      } else {
      // No predicates anywhere in the two products (hipcc wraps every predicated LDS read in its own exec-mask
      // branch: 29 branches, ~100 v_readlane of spilled masks in the first version): B is stored 16 columns wide and
      // 4 KS rows deep with zeros in the padding, so a contraction row >= KR or a column >= NB multiplies zero;
      // eigen-columns j >= k have spectra (sc1, sc2) = 0, so whatever finite numbers U holds in their rows never
      // reach C; rows m >= KR of Out are computed from stale LDS contents and dropped.
      constexpr int KS = (KR + 3) / 4;
      constexpr int BR = 4 * KS;               // rows of the padded B
      double* vh = slice;                      // [32][KR]
      double* bm = slice + 32 * KR;            // [BR][16]
      double* scl = bm + BR * 16;              // [64][2]: (1/lam, sqrt((k-1)/lam)) per eigen-column
      // (q and c are laundered: they are the same for every point of the wave's run, so hipcc hoists the ~40 LDS
      // addresses built from them out of the point loop, keeps them in scratch, and reloads one -- a scratch round
      // trip -- in front of every MFMA step; found in the ISA)
      int q = wlane >> 4, c = wlane & 15;
      asm volatile("" : "+v"(q), "+v"(c));
      wave_lds_sync();
      {
        if (lane < BR) {
          double brow[16];
          brow[0] = (lane < k) ? racc : 0.0;
          brow[1] = (lane < k) ? rdacc : 0.0;
#pragma unroll
          for (int b = 2; b < 16; ++b) brow[b] = (b - 2 < NV) ? xv[b - 2 < NV ? b - 2 : 0] : 0.0;
          double* row = bm + lane * 16;
#pragma unroll
          for (int b = 0; b < 16; b += 2) *reinterpret_cast<double2*>(&row[b]) = double2{brow[b], brow[b + 1]};
        }
        *reinterpret_cast<double2*>(&scl[2 * lane]) = double2{sc2, sc1};
      }
      v4d accO[4];
#pragma unroll
      for (int t = 0; t < 4; ++t) accO[t] = v4d{0.0, 0.0, 0.0, 0.0};
      double va = 0.0, vg = 0.0;
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        if (32 * h < KR) {
          wave_lds_sync();
          if ((lane >> 5) == h && lane < KR) {
            double* mine = vh + (lane - 32 * h) * KR;
#pragma unroll
            for (int r = 0; r < KR; r += 2) *reinterpret_cast<double2*>(&mine[r]) = double2{g[r], g[r + 1]};
          }
          wave_lds_sync();
          v4d accU[2];
          accU[0] = v4d{0.0, 0.0, 0.0, 0.0};
          accU[1] = v4d{0.0, 0.0, 0.0, 0.0};
#pragma unroll
          for (int s_ = 0; s_ < KS; ++s_) {
            const double bq = bm[(4 * s_ + q) * 16 + c];
            if (h == 0) vg = fma(bq, bq, vg);
#pragma unroll
            for (int il = 0; il < 2; ++il) {
              if (32 * h + 16 * il < KR) {
                const double a = vh[(16 * il + c) * KR + 4 * s_ + q];
                accU[il] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, bq, accU[il], 0, 0, 0);
              }
            }
          }
#pragma unroll
          for (int il = 0; il < 2; ++il) {
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
              const int s_ = 4 * (2 * h + il) + reg;       // contraction step of Out: eigen-columns j = 4 s_ + q
              if (4 * s_ < KR) {
                const int j = 4 * s_ + q;
                const double2 sc = *reinterpret_cast<const double2*>(&scl[2 * j]);
                const double u = accU[il][reg];
                va = fma(u * u, sc.x, va);
                const double cv = u * (c < 2 ? sc.x : sc.y);
                const double* a = vh + (j - 32 * h) * KR + 4 * c;
                const double2 lo = *reinterpret_cast<const double2*>(a);
                const double2 hi = *reinterpret_cast<const double2*>(a + 2);
                accO[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(lo.x, cv, accO[0], 0, 0, 0);
                accO[1] = __builtin_amdgcn_mfma_f64_16x16x4f64(lo.y, cv, accO[1], 0, 0, 0);
                accO[2] = __builtin_amdgcn_mfma_f64_16x16x4f64(hi.x, cv, accO[2], 0, 0, 0);
                accO[3] = __builtin_amdgcn_mfma_f64_16x16x4f64(hi.y, cv, accO[3], 0, 0, 0);
              }
            }
          }
        }
      }
      PROF_MARK(6)
      // RTPS factor per variable in the lanes of column c = 2 + v:
      // var_a = x'^T Pa x' = sum_j U_jv^2 / lam_j, var_g = sum_m x'_v[m]^2 (both still split over the 4 q groups)
      va += wshfl_xor(va, 16);
      va += wshfl_xor(va, 32);
      vg += wshfl_xor(vg, 16);
      vg += wshfl_xor(vg, 32);
      {
        KernArgs* const Ar = fresh_args<NW>(Ak0);
        const int v = c - 2;
        const bool isv = c >= 2 && c < NB;
        const double ra_ = Ar->relax_alpha, ras_ = Ar->relax_alpha_spread;
        double cfv = 1.0;
        if (ra_ != 0.0) {
          cfv = 1.0 - ra_;
        } else if (ras_ != 0.0) {                                        // (rules_dev::relax_parm and rtps_factor, restated)
          const double parm = (isv && Ar->relax_to_inflated_prior) ? Ar->infl[pt + Ar->infl_sv * (long)v] : 1.0;
          if (vg > 0.0 && va > 0.0) cfv = ras_ * sqrt(vg * parm / (va * km1)) - ras_ + 1.0;
        }
        double* const rtps_out_ = Ar->rtps_out;
        if (rtps_out_ && q == 0 && isv && ((Ar->var_mask >> v) & 1u)) {   // (rules_dev::rtps_reported, restated)
          const bool skipv = qskip && v >= Ar->iv_q_first && v <= Ar->iv_q_last;
          rtps_out_[pt + Ar->infl_sv * (long)v] = (ra_ == 0.0 && ras_ != 0.0 && !skipv) ? cfv : 1.0;
        }
#pragma unroll
        for (int vv = 0; vv < NV; ++vv) cf[vv] = readlane_d(cfv, 2 + vv);
      }
      // Out tiles -> lane m holds row m: register `reg` of tile I, lane (q, c) is Out[16 reg + 4 q + I][c]
      wave_lds_sync();
      double* ob = slice + kObOff;             // [64][16] ([32][16] for KR <= 20: rows >= KR are never read), on top of the V half (behind B and the spectra when the half is smaller)
      constexpr int OBR = wave_ob_rows(KR);
#pragma unroll
      for (int I = 0; I < 4; ++I)
#pragma unroll
        for (int reg = 0; reg < 4; ++reg)
          if (16 * reg < OBR) ob[(16 * reg + 4 * q + I) * 16 + c] = accO[I][reg];
      wave_lds_sync();
      {
        const double* row = ob + (OBR == 64 || lane < OBR ? lane : OBR - 1) * 16;
#pragma unroll
        for (int b = 0; b < NB; b += 2) {
          const double2 o2 = *reinterpret_cast<const double2*>(&row[b]);
          out[b] = o2.x;
          if (b + 1 < NB) out[b + 1] = o2.y;
        }
      }
      wave_lds_sync();
      }
    } else {
      // ------------------------------------------------------------ B = [r, r_det, x'_v] as bmat[m][NBP]; U = V^T B
      psync<NW>();
      if (lane < KR) {
        bmat[lane * NBP + 0] = (lane < k) ? racc : 0.0;
        bmat[lane * NBP + 1] = (lane < k) ? rdacc : 0.0;
        if (NBP > NB) bmat[lane * NBP + NB] = 0.0;
      }
      if (NV > 0) {
        const double* gp = g0 + moff;
  #pragma unroll
        for (int v = 0; v < NV; ++v) {
          const double x = (lane < k) ? *gp : 0.0;
          gp += A.sv;
          if (lane < KR) bmat[lane * NBP + 2 + v] = x;
        }
        if (lane < NV) {
          xmean[lane] = g0[k * A.sm + lane * A.sv];
          xdet[lane] = A.det_run ? g0[(k + 1) * A.sm + lane * A.sv] : 0.0;
        }
      }
      psync<NW>();
      double crow[NB];
  #pragma unroll
      for (int b = 0; b < NB; ++b) crow[b] = 0.0;
  #pragma unroll
      for (int r = 0; r < KR; ++r) {
  #pragma unroll
        for (int b = 0; b < NBP; b += 2) {
          const double2 b2 = *reinterpret_cast<const double2*>(&bmat[r * NBP + b]);   // broadcast
          crow[b] = fma(g[r], b2.x, crow[b]);
          if (b + 1 < NB) crow[b + 1] = fma(g[r], b2.y, crow[b + 1]);
        }
        if ((r & 1) == 1) pin_acc<NB>(crow);
      }
      PROF_MARK(6)
      // RTPS factor per variable, kept in SGPRs: var_a = x'^T Pa x' = sum_j U_jv^2 / lam_j
      if (NV > 0) {
  #pragma unroll
        for (int v = 0; v < NV; ++v) {
          double cfv = 1.0;
          if (A.relax_alpha != 0.0) {
            cfv = 1.0 - A.relax_alpha;
          } else if (A.relax_alpha_spread != 0.0) {   // (rules_dev::relax_factor, restated)
            const double parm = A.relax_to_inflated_prior ? A.infl[pt + A.infl_sv * (long)v] : 1.0;
            const double x = (lane < k) ? bmat[mrow_l * NBP + 2 + v] : 0.0;
            const double var_g = preduce<NW, 0>(x * x, red, rslot);
            const double var_a = preduce<NW, 0>(crow[2 + v] * crow[2 + v] * sc2, red, rslot);
            if (var_g > 0.0 && var_a > 0.0)
              cfv = A.relax_alpha_spread * sqrt(var_g * parm / (var_a * km1)) - A.relax_alpha_spread + 1.0;
          }
          cf[v] = uniform(cfv);
          if (A.rtps_out && lane == 0 && ((A.var_mask >> v) & 1u)) {   // (rules_dev::rtps_reported, restated)
            const bool skipv = qskip && v >= A.iv_q_first && v <= A.iv_q_last;
            A.rtps_out[pt + A.infl_sv * (long)v] = (A.relax_alpha == 0.0 && A.relax_alpha_spread != 0.0 && !skipv) ? cfv : 1.0;
          }
        }
      }
      // C = D U : w-bar spectrum 1/lam, T spectrum sqrt((k-1)/lam)
      crow[0] *= sc2;
      crow[1] *= sc2;
  #pragma unroll
      for (int v = 0; v < NV; ++v) crow[2 + v] *= sc1;

      rows_times_c<KR, NB, NW>(g, crow, out, k, vbuf, cbuf);   // lane m: out[0] = w-bar_m, out[1] = w-bar_det_m, out[2+v] = (T x'_v)_m

    }
    PROF_MARK(7)
    // ------------------------------------------------------------ analysis members
    // One-wave points read the arguments of this phase from the argument segment (fresh_args, above) and restate the rules of
    // letkf_rules_dev.h on them; two-wave points keep the phase as it was, statement for statement, in the branch below: their
    // register allocation moves with any restatement of shared code (tools/isa_compare.py holds letkf_wave2 to its assembly),
    // so A CHANGE TO ONE BRANCH BELONGS IN THE OTHER TOO.
    if constexpr (NW == 1) {
      if (NV > 0 && das) {
        double* ap = a0 + moff;
#pragma unroll
        for (int v = 0; v < NV; ++v) {
          KernArgs* const Av = fresh_args<NW>(Ak0);                                 // (per variable: what it reads lives for one iteration, in SGPRs)
          const int ivq0 = Av->iv_q_first, det_run_ = Av->det_run;
          const bool skip = qskip && v >= ivq0 && v <= Av->iv_q_last;   // (rules_dev::var_skipped, restated)
          double x, xm, xdt;
          if constexpr (MAPPLY) {
            // x' comes back from the LDS copy of B (it survives the output transposition): keeping the 22 registers of xv
            // alive through the matrix phase made hipcc spill LDS addresses there -- a scratch round trip in front of
            // every MFMA step of the U product (PROF build ISA)
            const double xl = slice[kBmOff + (lane < kBmRows ? lane : kBmRows - 1) * 16 + 2 + v];
            x = (lane < k) ? xl : 0.0;
            xm = readlane_d(xm_l, v);
            xdt = readlane_d(xd_l, v);
          } else {
            x = (lane < k) ? bmat[mrow_l * NBP + 2 + v] : 0.0;
            xm = xmean[v];
            xdt = xdet[v];
          }
          const double sdot = preduce<NW, 0>(x * out[0], red, rslot);
          const double sdotd = det_run_ ? preduce<NW, 0>(x * out[1], red, rslot) : 0.0;
          double val;
          if (skip) {
            val = xm + x;
          } else {
            double rd = 0.0;                         // (rules_dev::rtpp_diag and relax_parm, restated)
            if (const double ra_ = Av->relax_alpha; ra_ != 0.0)
              rd = ra_ * sqrt(Av->relax_to_inflated_prior ? Av->infl[pt + Av->infl_sv * (long)v] : 1.0);
            // (the contraction hipcc chose for `cf * out + rtpp_diag * x` before the restatement, written out: left to it, the
            // restated sum is contracted the other way round and RTPP results move in the last bit)
            const double pert = fma(cf[v], out[2 + v], rd * x);
            val = analysis_value(xm, x, beta, pert, sdot);
            const double qsm = Av->q_sprd_max;
            if (qsm > 0.0 && v == ivq0) {
              const double q_mean = preduce<NW, 0>(lane < k ? val : 0.0, red, rslot) / (double)k;
              const double dq = (lane < k) ? val - q_mean : 0.0;
              const double q_sprd = sqrt(preduce<NW, 0>(dq * dq, red, rslot) / km1) / q_mean;
              val = q_clamped(val, q_mean, dq, q_sprd, qsm);
            }
          }
          const bool inclass = (Av->var_mask >> v) & 1u;
          const long sv_ = Av->sv;
          if (lane < k && inclass) *ap = val;
          ap += sv_;
          if (det_run_ && lane == 0 && inclass)
            a0[(k + 1) * Av->sm + v * sv_] = skip ? xdt : xdt + sdotd * beta;     // :489-497
        }
        KernArgs* const Ai = fresh_args<NW>(Ak0);
        if (Ai->infl_adaptive) {                   // (rules_dev::var_updated, restated; also without obs: the class copies its first slot), after every parm read above
          const int ivq0 = Ai->iv_q_first, ivq1 = Ai->iv_q_last;
          const unsigned vmask = Ai->var_mask;
          double* const infl_ = Ai->infl;
          const long isv_ = Ai->infl_sv;
#pragma unroll
          for (int v = 0; v < NV; ++v) {
            const bool skip = qskip && v >= ivq0 && v <= ivq1;
            if (!skip && lane == 0 && ((vmask >> v) & 1u)) infl_[pt + isv_ * (long)v] = infl_new;
          }
        }
      } else if (A.infl_adaptive && n > 0 && lane == 0) {
        A.infl[pt] = infl_new;
      }
    } else {
      if (NV > 0 && das) {
        double* ap = a0 + moff;
#pragma unroll
        for (int v = 0; v < NV; ++v) {
          const bool skip = qskip && v >= A.iv_q_first && v <= A.iv_q_last;   // (rules_dev::var_skipped, restated)
          double x, xm, xdt;
          if constexpr (MAPPLY) {
            // x' comes back from the LDS copy of B (it survives the output transposition): keeping the 22 registers of xv
            // alive through the matrix phase made hipcc spill LDS addresses there -- a scratch round trip in front of
            // every MFMA step of the U product (PROF build ISA)
            const double xl = slice[kBmOff + (lane < kBmRows ? lane : kBmRows - 1) * 16 + 2 + v];
            x = (lane < k) ? xl : 0.0;
            xm = readlane_d(xm_l, v);
            xdt = readlane_d(xd_l, v);
          } else {
            x = (lane < k) ? bmat[mrow_l * NBP + 2 + v] : 0.0;
            xm = xmean[v];
            xdt = xdet[v];
          }
          const double sdot = preduce<NW, 0>(x * out[0], red, rslot);
          const double sdotd = A.det_run ? preduce<NW, 0>(x * out[1], red, rslot) : 0.0;
          double val;
          if (skip) {
            val = xm + x;
          } else {
            const double pert = cf[v] * out[2 + v] + rtpp_diag(A, pt, v) * x;
            val = analysis_value(xm, x, beta, pert, sdot);
            if (A.q_sprd_max > 0.0 && v == A.iv_q_first) {
              const double q_mean = preduce<NW, 0>(lane < k ? val : 0.0, red, rslot) / (double)k;
              const double dq = (lane < k) ? val - q_mean : 0.0;
              const double q_sprd = sqrt(preduce<NW, 0>(dq * dq, red, rslot) / km1) / q_mean;
              val = q_clamped(val, q_mean, dq, q_sprd, A.q_sprd_max);
            }
          }
          const bool inclass = (A.var_mask >> v) & 1u;
          if (lane < k && inclass) *ap = val;
          ap += A.sv;
          if (A.det_run && lane == 0 && inclass)
            a0[(k + 1) * A.sm + v * A.sv] = skip ? xdt : xdt + sdotd * beta;     // :489-497
        }
        if (A.infl_adaptive) {                       // (rules_dev::var_updated, restated; also without obs: the class copies its first slot), after every parm read above
#pragma unroll
          for (int v = 0; v < NV; ++v) {
            const bool skip = qskip && v >= A.iv_q_first && v <= A.iv_q_last;
            if (!skip && lane == 0 && ((A.var_mask >> v) & 1u)) A.infl[pt + A.infl_sv * (long)v] = infl_new;
          }
        }
      } else if (A.infl_adaptive && n > 0 && lane == 0) {
        A.infl[pt] = infl_new;
      }
    }

    // ------------------------------------------------------------ optional outputs
    if constexpr (NW == 1) {
      KernArgs* const Ao = fresh_args<NW>(Ak0);
      if (double* const t_ = Ao->transm_out; t_ && lane < k) t_[(size_t)pt * k + lane] = out[0];
      if (double* const t_ = Ao->transmd_out; t_ && lane < k) t_[(size_t)pt * k + lane] = out[1];
    } else {
      if (A.transm_out && lane < k) A.transm_out[(size_t)pt * k + lane] = out[0];
      if (A.transmd_out && lane < k) A.transmd_out[(size_t)pt * k + lane] = out[1];
    }
    if (KKOUT && (A.trans_out || A.pa_out)) {
      // T = V diag(sc1) V^T and Pa = V diag(sc2) V^T: same row-gather with C[j][:] = sc * v_j
      #pragma unroll 1
      for (int which = 0; which < 2; ++which) {
        double* dst = which == 0 ? A.trans_out : A.pa_out;
        if (!dst) continue;
        dst += (size_t)pt * k * k;
        const double sc = which == 0 ? sc1 : sc2;
        double kk[KR];
#pragma unroll
        for (int r = 0; r < KR; ++r) kk[r] = 0.0;
        double* ckk = bmat;                       // [kChunk][KR], B vectors are dead by now
        const int ncol = (k + 1) & ~1;
        for (int j0 = 0; j0 < ncol; j0 += kChunk) {
          psync<NW>();
          if (lane >= j0 && lane < j0 + kChunk) {
            const int jj = lane - j0;
#pragma unroll
            for (int r = 0; r < KR; ++r) {
              vbuf[r * kVld + jj] = g[r];
              ckk[jj * KR + r] = sc * g[r];
            }
          }
          psync<NW>();
          const int mrow = lane < KR ? lane : KR - 1;
          const int nj = min(kChunk, ncol - j0);
          for (int jj = 0; jj < nj; ++jj) {
            const double vv = vbuf[mrow * kVld + jj];
#pragma unroll
            for (int r = 0; r < KR; r += 2) {
              const double2 c2 = *reinterpret_cast<const double2*>(&ckk[jj * KR + r]);
              kk[r] = fma(vv, c2.x, kk[r]);
              kk[r + 1] = fma(vv, c2.y, kk[r + 1]);
            }
          }
        }
        psync<NW>();
        // lane m holds row m; the matrices are symmetric, so write it as column m (coalescing is irrelevant here)
        if (lane < k) {
          const double add = (which == 0 && A.add_wbar_to_trans) ? 1.0 : 0.0;
          // trans(i,j) += w-bar(i) (common_letkf.f90:221-225): row i gets w-bar_i in every column
#pragma unroll
          for (int r = 0; r < KR; ++r)
            if (r < k) dst[(size_t)r * k + lane] = kk[r] + add * out[0];
        }
      }
    }
    PROF_MARK(8)
    if constexpr (NW == 1) {
      KernArgs* const As = fresh_args<NW>(Ak0);
      if (lane == 0) {
        if (int* const o_ = As->status) o_[pt] = st;
        if (int* const o_ = As->nsweep) o_[pt] = sweeps;
        if (int* const o_ = As->nobs_out) o_[pt] = n;
      }
    } else if (lane == 0) {
      if (A.status) A.status[pt] = st;
      if (A.nsweep) A.nsweep[pt] = sweeps;
      if (A.nobs_out) A.nobs_out[pt] = n;
    }
   }
  }
  PROF_FLUSH
}

// ------------------------------------------------------------------ host launcher
template <int KR, int NV, bool KKOUT, int NW, int FUSED = 0>
static hipError_t launch_wave(const PointArgs& a, int num_cu, hipStream_t st) {
  const size_t lds = (size_t)(NW == 1 ? 4 : 1) * wave_slice_doubles(KR, NV, NW) * sizeof(double);
  if (a.k < wave_kmin(KR, NW) || a.k > KR) return hipErrorInvalidValue;   // the Gram assumes its full member blocks
  if (NV > 0 && a.mode == 1) return hipErrorInvalidValue;                 // ... and, with variables to analyse, rows of the obs table
  if (hipError_t e = lds_opt_in(&letkf_wave_kernel<KR, NV, KKOUT, NW, FUSED>, lds)) return e;
  // (the PROF twin's static dealing launches the shape's unclamped grid and needs no occupancy)
  const int occ = a.sched ? resident_blocks(&letkf_wave_kernel<KR, NV, KKOUT, NW, FUSED>, NW == 1 ? 256 : 128, lds, NW == 1 ? 2 : 1) : 0;
  const LaunchShape s = launch_shape(false, a.k, a.mode, a.npts, a.warm_stride, a.run_len, num_cu, occ, a.sched != nullptr, wave_grid_per_cu());
  static_assert(NW != 1 || wave_occupancy(KR, NW) == (KR <= 20 ? LETKF_SMALL_OCC : 2), "launch_shape counts resident_per_xcd with these");
  PointArgs b = a;
  b.run_len = s.run_len;
  b.plan = s.plan;
  if (hipError_t e = sched_reset_counters(s, a.sched, st)) return e;
  hipLaunchKernelGGL((letkf_wave_kernel<KR, NV, KKOUT, NW, FUSED>), dim3(s.grid), dim3(NW == 1 ? 256 : 128), lds, st, b);
  return hipGetLastError();
}

// the dispatch of launch_wave_kernel (letkf_wave.hip) and launch_wave_kernel_two (letkf_wave2.hip): instantiation <KR, NW> for
// k up to KR (one wave: up to 62), by the call's mode and outputs
#define LETKF_WAVE_CASE(KR, NW)                                                                                 \
  if (k <= (NW == 1 ? (KR < 62 ? KR : 62) : KR)) {                                                              \
    if constexpr (NW == 1) {                                                                                    \
      if (a.mode == 2) return launch_wave<KR, 11, false, NW, 2>(a, num_cu, st);                                 \
      if (a.mode == 3) return launch_wave<KR, 11, false, NW, 3>(a, num_cu, st);                                 \
    }                                                                                                           \
    if (a.mode != 1)                                                                                            \
      return kkout ? launch_wave<KR, 11, true, NW>(a, num_cu, st) : launch_wave<KR, 11, false, NW>(a, num_cu, st); \
    return launch_wave<KR, 0, true, NW>(a, num_cu, st);                                                         \
  }

}  // namespace letkf
