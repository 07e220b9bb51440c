// letkf_interp.hip -- weight interpolation (include/letkf_amd_interp.h): the coarse set, the gather
// of the coarse points' local lists into letkf_core's batch form, and the kernel that blends the kept T / w-bar of a
// cell's corners and applies them, with the per-point rules of letkf_rules_dev.h, at the cell's fine points.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "../../include/letkf_amd_interp_window.h"
#include "letkf_interp_dev.h"
#include "letkf_rules_dev.h"

extern "C" int letkf_interp_coarse_axis(int32_t n, int32_t stride, int32_t* idx, int32_t* count) {
  if (n < 1 || stride < 1 || !count) return LETKF_E_INVALID;
  int32_t m = 0, last = -1;
  for (int64_t i = 0; i < n; i += stride) {
    last = (int32_t)i;
    if (idx) idx[m] = last;
    ++m;
  }
  if (last != n - 1) {   // (the end closes the set where the stride does not land on it)
    if (idx) idx[m] = n - 1;
    ++m;
  }
  *count = m;
  return LETKF_OK;
}

extern "C" int letkf_interp_window_axis(int32_t gn, int32_t stride, int32_t g0, int32_t n, int32_t o0, int32_t on, int32_t* idx,
                                        int32_t* count) {
  return letkf::interp_window_axis(gn, stride, g0, n, o0, on, idx, count, nullptr);
}

namespace letkf {

int interp_window_axis(int32_t gn, int32_t stride, int32_t g0, int32_t n, int32_t o0, int32_t on, int32_t* idx, int32_t* count,
                       int32_t* bad) {
  if (gn < 1 || stride < 1 || n < 1 || on < 1 || !count) return LETKF_E_INVALID;
  if (g0 < 0 || (int64_t)g0 + n > gn || o0 < 0 || (int64_t)o0 + on > n) return LETKF_E_INVALID;
  // the global lines: multiples of the stride below gn, and gn - 1 (letkf_interp_coarse_axis)
  const int64_t p = (int64_t)g0 + o0, q = p + on - 1;
  const bool p_on = p % stride == 0 || p == gn - 1;
  int64_t l = p_on ? p : p / stride * stride;   // (p itself, or its predecessor)
  int32_t m = 0;
  for (;;) {
    if (l < g0 || l >= (int64_t)g0 + n) {
      if (bad) *bad = (int32_t)l;
      return LETKF_E_INVALID;
    }
    if (idx) idx[m] = (int32_t)(l - g0);
    ++m;
    if (l >= q) break;                          // (q itself, or its successor)
    l = std::min<int64_t>(l + stride, gn - 1);
  }
  *count = m;
  return LETKF_OK;
}

namespace {

using namespace rules_dev;
using d4 = __attribute__((ext_vector_type(4))) double;

__global__ __launch_bounds__(256) void interp_coords_kernel(const InterpCoordArgs a) {
  const InterpGrid& G = a.G;
  const long ncc = (long)G.ncx * G.ncy, nij1 = (long)G.nx * G.ny, n = ncc * G.nlev;
  for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (long)gridDim.x * blockDim.x) {
    const long cc = e % ncc, lev = e / ncc;
    const long col = G.ix[cc % G.ncx] + (long)G.nx * G.iy[cc / G.ncx];
    if (lev == 0) {
      a.crig[cc] = a.rig[col];
      a.crjg[cc] = a.rjg[col];
    }
    a.crlev[e] = a.rlev[col + nij1 * lev];
    a.crz[e] = a.rz[col + nij1 * lev];
  }
}

// one workgroup per coarse point of the slab
__global__ __launch_bounds__(256) void interp_gather_kernel(const InterpGatherArgs a) {
  const InterpGrid& G = a.G;
  const PointArgs& A = a.A;
  const long ncc = (long)G.ncx * G.ncy, nij1 = (long)G.nx * G.ny, nb = ncc * a.nl;
  const int k = A.k, tid = threadIdx.x;
  for (long b = blockIdx.x; b < nb; b += gridDim.x) {
    const long cc = b % ncc, lev = a.l0 + b / ncc;
    const long pt = G.ix[cc % G.ncx] + (long)G.nx * G.iy[cc / G.ncx] + nij1 * lev;
    const long gp = cc + ncc * lev;
    const long off0 = a.obs_off[gp];
    long nl = a.obs_off[gp + 1] - off0;
    if (nl > a.nobs) nl = a.nobs;   // (the host sized nobs as the slab's longest list)
    const int n = (int)nl;
    if (tid == 0) {
      a.nobsl[b] = n;
      const double* xmean = A.gues + pt * A.sp + (long)k * A.sm;
      a.rho[b] = solve_inflation(A, pt, A.nv, q_update_skipped(A, xmean, A.sv));
    }
    // every element of the problem is written: the rows beyond the point's own list hold zeros, whoever reads them
    for (int i = tid; i < a.nobs; i += blockDim.x) {
      const bool in = i < n;
      const long row = in ? a.obs_idx[off0 + i] : 0;
      a.rdiag[b * a.nobs + i] = in ? a.rdiag_l[off0 + i] : 0.0;
      a.rloc[b * a.nobs + i] = in ? a.rloc_l[off0 + i] : 0.0;
      a.dep[b * a.nobs + i] = in ? A.dep[row] : 0.0;
      if (a.depd) a.depd[b * a.nobs + i] = in ? A.ensval[row * A.kld + k] : 0.0;
    }
    // (consecutive threads walk down a column of hdxb: unit-stride writes; the table's rows come back from the cache)
    double* h = a.hdxb + (size_t)b * (size_t)k * (size_t)a.nobs;
    for (long e = tid; e < (long)a.nobs * k; e += blockDim.x) {
      const int m = (int)(e / a.nobs), i = (int)(e - (long)m * a.nobs);
      h[e] = i < n ? A.ensval[(long)a.obs_idx[off0 + i] * A.kld + m] : 0.0;
    }
  }
}

// the sum of x over the 16 lanes that hold one row of a 16 x 16 result tile (lanes with the same lane >> 4): a butterfly,
// the same order of additions in every lane
__device__ __forceinline__ double row16_sum(double x) {
#pragma unroll
  for (int o = 1; o < 16; o <<= 1) x += __shfl_xor(x, o, 64);
  return x;
}

// One workgroup per (cell, level).  Rows are (owned fine point q, variable v), row = q + npo * v, in chunks of 16 * NW, a
// tile of 16 rows per wave; columns are the k members in NCT tiles of 16.  Per chunk and corner: T_c goes to LDS
// (Ts[i][m] = T_c(i, m), zero beyond k in both directions), acc = X' T_c on v_mfma_f64_16x16x4_f64 (operand layout of
// the matrix instruction: A lane l = X'[row l & 15][i = 4 step + (l >> 4)], B lane l = Ts[i][col l & 15], D register r of
// lane l = row (l >> 4) + 4 r, col l & 15), out += w_c acc for the rows whose w_c is not 0.  The epilogue stays in the D
// layout: the row sums var_g, var_a, x' . w-bar go over the column tiles in order and then over the 16 lanes of the row.
template <int NCT, int NW>
__global__ __launch_bounds__(64 * NW) void letkf_interp_apply_kernel(const InterpApplyArgs S) {
  extern __shared__ double lds[];
  constexpr int KC = NCT * 16, LD = KC + 1, NSTEP = NCT * 4;
  const InterpGrid& G = S.G;
  const PointArgs& A = S.A;
  const int k = A.k, nv = A.nv;
  const int KP = (k + 3) & ~3;
  double* Ts = lds;
  double* wb = Ts + (size_t)KP * LD;   // [4][KC] w-bar of the corners
  double* wbd = wb + 4 * KC;           // [4][KC] w-bar_det
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int lrow = lane >> 4, lcol = lane & 15;
  const int ncelx = G.ncx > 1 ? G.ncx - 1 : 1, ncely = G.ncy > 1 ? G.ncy - 1 : 1;
  const long bid = blockIdx.x;
  const int cx = (int)(bid % ncelx), cy = (int)((bid / ncelx) % ncely), ll = (int)(bid / ((long)ncelx * ncely));
  const long lev = S.l0 + ll;
  const int cxb = cx + 1 < G.ncx ? cx + 1 : G.ncx - 1, cyb = cy + 1 < G.ncy ? cy + 1 : G.ncy - 1;
  const int ia = G.ix[cx], ib = G.ix[cxb], jc = G.iy[cy], jd = G.iy[cyb];
  // the cell owns i in [ia, ib) and j in [jc, jd), the last cell of a direction also its far line; of these the call's own:
  // the first cell of a direction may start above its near line, the last stop below its far line
  int ilo, ihi, jlo, jhi;
  interp_cell_lines(cx, G.ncx, ia, ib, G.ox0, G.ox1, &ilo, &ihi);
  interp_cell_lines(cy, G.ncy, jc, jd, G.oy0, G.oy1, &jlo, &jhi);
  const int nox = ihi - ilo + 1, noy = jhi - jlo + 1;
  if (nox < 1 || noy < 1) return;   // (no cell of a call is without an owned point: the host has checked)
  const int npo = nox * noy, nrows = npo * nv;
  // A corner that weighs 0 at every owned row of the cell is not staged: the far one where the cell's own lines are the
  // near line alone, the near one where they are the far line alone (the last cell of a window that begins on it).
  const bool far_x_unused = ihi == ia, near_x_unused = ilo == ib && ib > ia;
  const bool far_y_unused = jhi == jc, near_y_unused = jlo == jd && jd > jc;
  const long ncc = (long)G.ncx * G.ncy, nij1 = (long)G.nx * G.ny;
  const double km1 = (double)(k - 1);
  const bool det = A.det_run && S.wbard;

  auto corner = [&](const int c) -> long { return ((c & 1) ? cxb : cx) + (long)G.ncx * ((c & 2) ? cyb : cy) + ncc * ll; };
  // w-bar (and w-bar_det) of the four corners, once per cell and level
  for (int e = tid; e < 4 * KC; e += 64 * NW) {
    const int c = e / KC, m = e - c * KC;
    const long cp = corner(c);
    wb[e] = m < k ? S.wbar[cp * k + m] : 0.0;
    wbd[e] = (det && m < k) ? S.wbard[cp * k + m] : 0.0;
  }
  int cst[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) cst[c] = S.cstatus[corner(c)];

  for (int row0 = 0; row0 < nrows; row0 += 16 * NW) {
    const int base = row0 + 16 * wv;
    // ---- this lane's rows in the D layout
    bool valid[4];
    long pt[4];
    int vv[4];
    double wx[4], wy[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = base + lrow + 4 * r;
      valid[r] = row < nrows;
      const int v = valid[r] ? row / npo : 0, q = valid[r] ? row - v * npo : 0;
      const int qj = q / nox, qi = q - qj * nox;
      vv[r] = v;
      pt[r] = (ilo + qi) + (long)G.nx * (jlo + qj) + nij1 * lev;
      wx[r] = ib > ia ? (double)(ilo + qi - ia) / (double)(ib - ia) : 0.0;
      wy[r] = jd > jc ? (double)(jlo + qj - jc) / (double)(jd - jc) : 0.0;
    }
    // ---- and its row as the A operand: X' of the row, k-tail masked
    double ax[NSTEP];
    {
      const int row = base + lcol;
      const bool va = row < nrows;
      const int v = va ? row / npo : 0, q = va ? row - v * npo : 0;
      const int qj = q / nox, qi = q - qj * nox;
      const double* g0 = A.gues + ((ilo + qi) + (long)G.nx * (jlo + qj) + nij1 * lev) * A.sp + (long)v * A.sv;
#pragma unroll
      for (int s = 0; s < NSTEP; ++s) {
        const int i = 4 * s + lrow;
        ax[s] = (va && i < k) ? g0[(long)i * A.sm] : 0.0;
      }
    }
    d4 out[NCT];
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct) out[ct] = d4{0.0, 0.0, 0.0, 0.0};

#pragma unroll 1
    for (int c = 0; c < 4; ++c) {
      if (((c & 1) ? far_x_unused : near_x_unused) || ((c & 2) ? far_y_unused : near_y_unused)) continue;
      const double* Tc = S.T + (size_t)corner(c) * (size_t)k * (size_t)k;
      __syncthreads();
      for (int e = tid; e < KP * KC; e += 64 * NW) {
        const int m = e / KP, i = e - m * KP;
        Ts[(size_t)i * LD + m] = (i < k && m < k) ? Tc[(size_t)m * k + i] : 0.0;
      }
      __syncthreads();
      d4 acc[NCT];
#pragma unroll
      for (int ct = 0; ct < NCT; ++ct) acc[ct] = d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int s = 0; s < NSTEP; ++s) {
        if (4 * s < KP) {
          const double* trow = Ts + (size_t)(4 * s + lrow) * LD + lcol;
#pragma unroll
          for (int ct = 0; ct < NCT; ++ct) acc[ct] = __builtin_amdgcn_mfma_f64_16x16x4f64(ax[s], trow[16 * ct], acc[ct], 0, 0, 0);
        }
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const double w = ((c & 1) ? wx[r] : 1.0 - wx[r]) * ((c & 2) ? wy[r] : 1.0 - wy[r]);
        if (w != 0.0) {
#pragma unroll
          for (int ct = 0; ct < NCT; ++ct) out[ct][r] = fma(w, acc[ct][r], out[ct][r]);
        }
      }
    }

    // ---- the rules at the fine point, row by row
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const bool ok = valid[r];
      const long p = pt[r];
      const int v = vv[r];
      const double* g0 = A.gues + p * A.sp;
      double* a0 = A.anal + p * A.sp;
      const double beta = (ok && A.beta) ? A.beta[p] : 1.0;
      const bool qskip = ok && q_update_skipped(A, g0 + (long)k * A.sm, A.sv);
      const bool skip = var_skipped(A, qskip, v);
      const bool mine = ok && in_class(A, v);
      const double xm = ok ? g0[(long)k * A.sm + (long)v * A.sv] : 0.0;
      double wc[4];
      int st = 0;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        wc[c] = ((c & 1) ? wx[r] : 1.0 - wx[r]) * ((c & 2) ? wy[r] : 1.0 - wy[r]);
        if (wc[c] != 0.0 && cst[c] > st) st = cst[c];
      }
      double xp[NCT];
      double var_g = 0.0, var_a = 0.0, sdot = 0.0, sdotd = 0.0;
#pragma unroll
      for (int ct = 0; ct < NCT; ++ct) {
        const int m = 16 * ct + lcol;
        xp[ct] = (ok && m < k) ? g0[(long)m * A.sm + (long)v * A.sv] : 0.0;
        double wbl = 0.0, wbdl = 0.0;
#pragma unroll
        for (int c = 0; c < 4; ++c)
          if (wc[c] != 0.0) {
            wbl = fma(wc[c], wb[c * KC + m], wbl);
            wbdl = fma(wc[c], wbd[c * KC + m], wbdl);
          }
        const double o = m < k ? out[ct][r] : 0.0;
        var_g = fma(xp[ct], xp[ct], var_g);
        var_a = fma(o, o, var_a);
        sdot = fma(xp[ct], wbl, sdot);
        sdotd = fma(xp[ct], wbdl, sdotd);
      }
      var_g = row16_sum(var_g);
      var_a = row16_sum(var_a) / km1;
      sdot = row16_sum(sdot);
      sdotd = row16_sum(sdotd);
      const bool copy = beta == 0.0;                     // letkf_tools.f90:333-359: the first guess stays
      const double parm = ok ? relax_parm(A, p, v) : 1.0;
      const double cf = relax_factor(A, parm, var_g, var_a, km1);
      const double cd = rtpp_diag(A, parm);
      double val[NCT];
      double qsum = 0.0;
#pragma unroll
      for (int ct = 0; ct < NCT; ++ct) {
        const int m = 16 * ct + lcol;
        val[ct] = (skip || copy) ? xm + xp[ct] : analysis_value(xm, xp[ct], beta, cf * out[ct][r] + cd * xp[ct], sdot);
        qsum += m < k ? val[ct] : 0.0;
      }
      const bool clampq = A.q_sprd_max > 0.0 && !qskip && !copy && v == A.iv_q_first;   // variable iv3d_q only
      // (the two sums are taken by every lane: the butterfly needs the whole wave)
      const double q_mean = row16_sum(qsum) / (double)k;
      double ss = 0.0;
#pragma unroll
      for (int ct = 0; ct < NCT; ++ct) {
        const double d = (16 * ct + lcol < k) ? val[ct] - q_mean : 0.0;
        ss = fma(d, d, ss);
      }
      ss = row16_sum(ss);
      if (clampq) {
        const double q_sprd = sqrt(ss / km1) / q_mean;
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct) val[ct] = q_clamped(val[ct], q_mean, val[ct] - q_mean, q_sprd, A.q_sprd_max);
      }
      if (mine) {
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct) {
          const int m = 16 * ct + lcol;
          if (m < k) a0[(long)m * A.sm + (long)v * A.sv] = val[ct];
        }
        if (lcol == 0) {
          if (A.det_run) {
            const double xd = g0[(long)(k + 1) * A.sm + (long)v * A.sv];
            a0[(long)(k + 1) * A.sm + (long)v * A.sv] = (skip || copy) ? xd : xd + sdotd * beta;   // :489-497
          }
          if (A.rtps_out) A.rtps_out[p + A.infl_sv * (long)v] = copy ? 1.0 : rtps_reported(A, skip, cf);
        }
      }
      if (ok && v == 0 && lcol == 0 && A.status) A.status[p] = copy ? 0 : st;
    }
  }
}

template <int NCT, int NW>
hipError_t launch_apply(const InterpApplyArgs& a, hipStream_t st) {
  const size_t lds = interp_apply_lds_bytes(a.A.k);
  auto kern = letkf_interp_apply_kernel<NCT, NW>;
  if (hipError_t e = lds_opt_in(kern, lds)) return e;
  const long ncelx = a.G.ncx > 1 ? a.G.ncx - 1 : 1, ncely = a.G.ncy > 1 ? a.G.ncy - 1 : 1;
  const long grid = ncelx * ncely * a.nl;
  if (grid < 1 || grid > 0x7fffffffL) return hipErrorInvalidValue;
  hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(64 * NW), lds, st, a);
  return hipGetLastError();
}

}  // namespace

int interp_apply_nct(int k) {
  const int t = (k + 15) / 16;
  return t <= 1 ? 1 : t <= 2 ? 2 : t <= 4 ? 4 : 8;
}
// the instantiations up to 64 members run 8 waves; the largest keeps its three register tiles of 64 within one wave per SIMD
static int interp_apply_nw(int k) { return interp_apply_nct(k) == 8 ? 4 : 8; }

size_t interp_apply_lds_bytes(int k) {
  const int kc = 16 * interp_apply_nct(k), kp = (k + 3) & ~3;
  return ((size_t)kp * (size_t)(kc + 1) + 8 * (size_t)kc) * sizeof(double);
}

std::string interp_apply_kernel_name(int k) {
  return "letkf_interp_apply_kernel<NCT=" + std::to_string(interp_apply_nct(k)) + ",NW=" + std::to_string(interp_apply_nw(k)) + ">";
}

hipError_t launch_interp_apply(const InterpApplyArgs& a, hipStream_t st) {
  if (a.A.k < 2 || a.A.k > 128) return hipErrorInvalidValue;
  switch (interp_apply_nct(a.A.k)) {
    case 1: return launch_apply<1, 8>(a, st);
    case 2: return launch_apply<2, 8>(a, st);
    case 4: return launch_apply<4, 8>(a, st);
    default: return launch_apply<8, 4>(a, st);
  }
}

hipError_t launch_interp_coords(const InterpCoordArgs& a, int num_cu, hipStream_t st) {
  const long n = (long)a.G.ncx * a.G.ncy * a.G.nlev;
  hipLaunchKernelGGL(interp_coords_kernel, dim3(grid_for(n, 256, num_cu)), dim3(256), 0, st, a);
  return hipGetLastError();
}

hipError_t launch_interp_gather(const InterpGatherArgs& a, int num_cu, hipStream_t st) {
  const long nb = (long)a.G.ncx * a.G.ncy * a.nl;
  const long cap = (long)num_cu * 16;
  hipLaunchKernelGGL(interp_gather_kernel, dim3((unsigned)std::max<long>(1, std::min(nb, cap))), dim3(256), 0, st, a);
  return hipGetLastError();
}

}  // namespace letkf
