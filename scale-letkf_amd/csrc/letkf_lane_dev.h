// letkf_lane_dev.h -- cross-lane and scalarisation primitives of a 64-lane wavefront (gfx950), each defined once for every
// unit: DPP moves of a double, wave reductions, lane reads into scalar registers, shuffles, the scheduling pin, the
// row-broadcast FMA, the wave-level LDS hand-off, the XCD remap.  Device code only; everything is inlined.
#pragma once
#include <hip/hip_runtime.h>

namespace letkf {
namespace lane_dev {

__device__ __forceinline__ double wshfl_xor(double v, int mask) { return __shfl_xor(v, mask, 64); }
__device__ __forceinline__ double wshfl(double v, int src) { return __shfl(v, src, 64); }

// 64-lane sum by the xor butterfly through __shfl_xor (two ds_bpermute per stage): the units that sum rarely
__device__ __forceinline__ double wsum(double v) {
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) v += wshfl_xor(v, m);
  return v;
}

// DPP cross-lane move of a double (two 32-bit VALU movs, no LDS crossbar).  CTRL is a gfx9 dpp_ctrl code:
// 0xB1 quad_perm[1,0,3,2] (lane^1), 0x4E quad_perm[2,3,0,1] (lane^2), 0x1B quad_perm[3,2,1,0] (lane^3),
// 0x141 row_half_mirror (lane^7), 0x140 row_mirror (lane^15), 0x130 wave_shl:1, 0x138 wave_shr:1.
// Two forms, and they are NOT interchangeable as far as hipcc's code goes:
//   dpp_mov0      mov_dpp with bound_ctrl: a lane whose source lane does not exist or is switched off gets 0 (the "no partner"
//                 case at the ends of a Jacobi line), and no old value is asked for -- one v_mov_b32_dpp per dword.  Taken by
//                 the shifts, by the quad_perm controls, and by the 8-lane sums of letkf_kernels.hip (0x141 included).
//   dpp_mov_self  update_dpp with the lane's own value as the old one, bound_ctrl off.  Taken by wave_sum / wave_max / wave_min
//                 for the mirror controls 0x140 / 0x141.  These have a valid source in every lane, so dpp_mov0 would serve, and
//                 here hipcc puts a v_mov_b32 copy of the old value in front of every v_mov_b32_dpp (seen in letkf_wave's and
//                 letkf_trio's assembly) -- but swapping the form changes the code of the kernels that reduce, the k = 50 kernel
//                 among them (levers left): to be measured on the device, not assumed.
template <int CTRL>
__device__ __forceinline__ double dpp_mov0(double v) {
  int lo = __double2loint(v), hi = __double2hiint(v);
  lo = __builtin_amdgcn_mov_dpp(lo, CTRL, 0xF, 0xF, true);
  hi = __builtin_amdgcn_mov_dpp(hi, CTRL, 0xF, 0xF, true);
  return __hiloint2double(hi, lo);
}
template <int CTRL>
__device__ __forceinline__ double dpp_mov_self(double v) {
  int lo = __double2loint(v), hi = __double2hiint(v);
  lo = __builtin_amdgcn_update_dpp(lo, lo, CTRL, 0xF, 0xF, false);
  hi = __builtin_amdgcn_update_dpp(hi, hi, CTRL, 0xF, 0xF, false);
  return __hiloint2double(hi, lo);
}

// a value known to be identical in every lane -> scalar registers (frees VGPRs, lets FMAs take a scalar operand; what hipcc
// loads through plain pointers it otherwise keeps in vector registers and spills inside the loops)
__device__ __forceinline__ int uniform(const int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ double uniform(double v) {
  const int lo = __builtin_amdgcn_readfirstlane(__double2loint(v));
  const int hi = __builtin_amdgcn_readfirstlane(__double2hiint(v));
  return __hiloint2double(hi, lo);
}

// lane `src` (wave-uniform) of v -> SGPR pair
__device__ __forceinline__ double readlane_d(double v, int src) {
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), src);
  const int hi = __builtin_amdgcn_readlane(__double2hiint(v), src);
  return __hiloint2double(hi, lo);
}

// Reductions over the 64 lanes (every lane active).  (r4) The xor butterfly through __shfl_xor compiles to two ds_bpermute per
// stage -- six dependent LDS round trips per sum, and the analysis members take 11 .. 33 sums per point (found in the ISA of
// letkf_trio.hip: 636 ds_bpermute; the phase was 14 % of its wave time).  Same tree without LDS: inside a row of 16 lanes by DPP
// (lane ^ 1, lane ^ 2, then the mirrors: lanes of a quad / of eight hold the same partial sum by then, so lane ^ 7 and lane ^ 15
// deliver what lane ^ 4 and lane ^ 8 would), the four rows by v_readlane -- ((r0 + r1) + (r2 + r3)), the butterfly's own
// association: bitwise the same result.
__device__ __forceinline__ double wave_sum(double v) {
  v += dpp_mov0<0xB1>(v);
  v += dpp_mov0<0x4E>(v);
  v += dpp_mov_self<0x141>(v);
  v += dpp_mov_self<0x140>(v);
  return (readlane_d(v, 0) + readlane_d(v, 16)) + (readlane_d(v, 32) + readlane_d(v, 48));
}
__device__ __forceinline__ double wave_max(double v) {
  v = fmax(v, dpp_mov0<0xB1>(v));
  v = fmax(v, dpp_mov0<0x4E>(v));
  v = fmax(v, dpp_mov_self<0x141>(v));
  v = fmax(v, dpp_mov_self<0x140>(v));
  return fmax(fmax(readlane_d(v, 0), readlane_d(v, 16)), fmax(readlane_d(v, 32), readlane_d(v, 48)));
}
__device__ __forceinline__ double wave_min(double v) {
  v = fmin(v, dpp_mov0<0xB1>(v));
  v = fmin(v, dpp_mov0<0x4E>(v));
  v = fmin(v, dpp_mov_self<0x141>(v));
  v = fmin(v, dpp_mov_self<0x140>(v));
  return fmin(fmin(readlane_d(v, 0), readlane_d(v, 16)), fmin(readlane_d(v, 32), readlane_d(v, 48)));
}

// number of set bits of a wave mask below this lane (v_mbcnt_lo / _hi: two instructions)
__device__ __forceinline__ int mbcnt(const unsigned long long m) {
  return (int)__builtin_amdgcn_mbcnt_hi((unsigned int)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned int)m, 0u));
}

// the wave mask of the lanes below `lane`, for __popcll(m & lanes_below(lane)) where the mask is kept over many ballots
__device__ __forceinline__ unsigned long long lanes_below(const int lane) {
  return (lane == 0) ? 0ull : (~0ull >> (64 - lane));
}

// LDS written by some lanes of this wave, read by others: DS instructions of one wave execute in
// order, so only the compiler has to be kept from reordering across the hand-off.
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Scheduling pin: makes every accumulator an in/out operand of an empty asm with a memory clobber.  The FMAs that
// produce the accumulators must then retire before it and the next LDS loads issue after it, which stops the
// compiler from issuing all unrolled broadcast loads first and spilling them (measured: 5 KB of scratch per lane).
template <int NB>
__device__ __forceinline__ void pin_acc(double (&c)[NB]) {
  if constexpr (NB == 2) {
    asm volatile("" : "+v"(c[0]), "+v"(c[1])::"memory");
  } else if constexpr (NB == 13) {
    asm volatile(""
                 : "+v"(c[0]), "+v"(c[1]), "+v"(c[2]), "+v"(c[3]), "+v"(c[4]), "+v"(c[5]), "+v"(c[6]), "+v"(c[7]),
                   "+v"(c[8]), "+v"(c[9]), "+v"(c[10]), "+v"(c[11]), "+v"(c[12])::"memory");
  } else {
#pragma unroll
    for (int b = 0; b < NB; ++b) asm volatile("" : "+v"(c[b])::"memory");
  }
}

// acc += (ys of lane A of this lane's row of 16) * y: ONE instruction -- FP64 instructions take exactly one DPP control on
// gfx950, row_newbcast (tools/ubench_newbcast.hip: correct in every row, ~10 cycles of a SIMD per instruction beside the matrix
// instructions).  NOP: two wait states in front (a DPP read of a register a vector instruction has just written; the compiler's
// hazard recogniser does not see into inline asm) -- set on the first one of a group.
template <int A, bool NOP>
__device__ __forceinline__ void fmac_row_bcast(double& acc, const double ys, const double y) {
#define LETKF_FMAC_BCAST(N)                                                                                                      \
  if constexpr (A == N) {                                                                                                        \
    if constexpr (NOP) asm volatile("s_nop 1\n\tv_fmac_f64_dpp %0, %1, %2 row_newbcast:" #N " row_mask:0xf bank_mask:0xf" : "+v"(acc) : "v"(ys), "v"(y)); \
    else asm volatile("v_fmac_f64_dpp %0, %1, %2 row_newbcast:" #N " row_mask:0xf bank_mask:0xf" : "+v"(acc) : "v"(ys), "v"(y)); \
  }
  LETKF_FMAC_BCAST(0) LETKF_FMAC_BCAST(1) LETKF_FMAC_BCAST(2) LETKF_FMAC_BCAST(3) LETKF_FMAC_BCAST(4) LETKF_FMAC_BCAST(5)
#undef LETKF_FMAC_BCAST
}

// Bijective XCD-aware remap (blocks b and b+8 share an XCD and its L2): consecutive logical
// work items go to the same XCD so neighbouring grid points, which read almost the same obs
// rows, hit the same L2.  Speed only, never correctness.
__device__ __forceinline__ long xcd_remap(long orig, long n) {
  const long q = n >> 3, r = n & 7;
  const long xcd = orig & 7, j = orig >> 3;
  const long base = (xcd < r) ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
  return base + j;
}

}  // namespace lane_dev
}  // namespace letkf
