// Device check of scale-letkf_amd/csrc/letkf_rules_dev.h: one kernel evaluates every helper of the header over a table of
// input tuples; the host restates the same rules in plain C from the reference's lines (scale/letkf/letkf_tools.f90,
// common/common_letkf.f90, common/common_mtx.f90) without the header and compares.  Integer and boolean results must be
// equal.  Floating results: device and host may contract multiply-adds differently and no helper does more than eight
// roundings that contraction can move, so the bound is 8 x 2^-53 relative to the largest intermediate of the tuple (the
// cancellation in the adaptive inflation makes "relative to the result" the wrong scale).  Prints the largest observed
// ratio to that bound and, last, "mismatches N".
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "letkf_rules_dev.h"

constexpr int NV = 11;
constexpr int NI = 8, ND = 13;

struct Case {
  // switches of PointArgs
  double relax_alpha, relax_alpha_spread, q_update_top, q_sprd_max;
  int relax_to_inflated_prior, iv_p, iv_q_first, iv_q_last, max_sweep, nv;
  unsigned var_mask;
  // the point
  double p_mean, slot[NV];
  int qskip, v;
  double var_g, var_a, km1;
  double xm, x, beta, tx, sdot;
  double val, q_mean, q_sprd;
  double infl_old, parm1, parm2, parm3;
  int jconv, colvalid;
  double lmx, lmn, lam;
};
struct Out {
  int i[NI];
  double d[ND];
};

__global__ void eval(const Case* cs, const int n, double* infl, const double* xmean, Out* out) {
  using namespace letkf::rules_dev;
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  const Case& c = cs[t];
  letkf::PointArgs A;
  memset(&A, 0, sizeof(A));
  A.relax_alpha = c.relax_alpha;
  A.relax_alpha_spread = c.relax_alpha_spread;
  A.q_update_top = c.q_update_top;
  A.q_sprd_max = c.q_sprd_max;
  A.relax_to_inflated_prior = c.relax_to_inflated_prior;
  A.iv_p = c.iv_p;
  A.iv_q_first = c.iv_q_first;
  A.iv_q_last = c.iv_q_last;
  A.max_sweep = c.max_sweep;
  A.var_mask = c.var_mask;
  A.nv = c.nv;
  A.infl = infl;
  A.infl_sv = n;
  const long pt = t;
  Out o;
  o.i[0] = q_update_skipped(A, xmean + (long)t * NV, 1);
  o.i[1] = var_skipped(A, c.qskip, c.v);
  o.i[2] = in_class(A, c.v);
  o.i[3] = var_updated(A, c.qskip, c.v);
  o.i[4] = first_updated_var(A, c.nv, c.qskip);
  o.i[5] = wants_variances(A);
  o.i[6] = eig_status(c.jconv, c.max_sweep, c.lmx, c.lmn);
  o.i[7] = spectrum_status(c.jconv != 0, c.lmx, c.lmn);
  const double parm = relax_parm(A, pt, c.v);
  o.d[0] = solve_inflation(A, pt, c.nv, c.qskip);
  o.d[1] = parm;
  o.d[2] = rtpp_factor(A);
  o.d[3] = rtps_factor(A, parm, c.var_g, c.var_a, c.km1);
  o.d[4] = relax_factor(A, parm, c.var_g, c.var_a, c.km1);
  o.d[5] = rtps_reported(A, o.i[1], o.d[4]);
  o.d[6] = rtpp_diag(A, parm);
  o.d[7] = rtpp_diag(A, pt, c.v);
  o.d[8] = analysis_value(c.xm, c.x, c.beta, o.d[4] * c.tx + o.d[6] * c.x, c.sdot);
  o.d[9] = q_clamped(c.val, c.q_mean, c.val - c.q_mean, c.q_sprd, c.q_sprd_max);
  o.d[10] = adaptive_inflation(c.infl_old, c.parm1, c.parm2, c.parm3);
  const Spectra sc = spectra(c.lam, c.km1, c.colvalid);
  o.d[11] = sc.sc1;
  o.d[12] = sc.sc2;
  out[t] = o;
}

// ---------------------------------------------------------------- the host's restatement
static double big;   // largest |intermediate| of the value being computed
static double T(double v) {
  if (fabs(v) > big && isfinite(v)) big = fabs(v);
  return v;
}

static void host_eval(const Case& c, Out& o, double* scale) {
  // letkf_tools.f90:333-359: q is not updated where the mean pressure is below Q_UPDATE_TOP
  const bool top = c.q_update_top > 0.0 && c.p_mean < c.q_update_top;
  o.i[0] = top;
  const bool isq = c.v >= c.iv_q_first && c.v <= c.iv_q_last;
  o.i[1] = c.qskip && isq;
  o.i[2] = (c.var_mask & (1u << c.v)) != 0;
  o.i[3] = o.i[2] && !o.i[1];
  // :387-418: the first variable of the class that is updated carries the point's inflation
  int v0 = c.nv;
  for (int v = c.nv - 1; v >= 0; --v) {
    const bool q = v >= c.iv_q_first && v <= c.iv_q_last;
    if ((c.var_mask & (1u << v)) && !(c.qskip && q)) v0 = v;
  }
  o.i[4] = v0;
  const bool rtpp = c.relax_alpha != 0.0, rtps = !rtpp && c.relax_alpha_spread != 0.0;
  o.i[5] = rtps;
  // common_mtx.f90:66-78
  {
    int st = 0;
    if (c.lmn < c.lmx * 1.4901161193847656e-08) st = 3;
    if (!(c.lmx > 0.0)) st = 2;
    o.i[7] = c.jconv ? st : 1;
    o.i[6] = (!c.jconv && c.max_sweep >= 60) ? 1 : st;
  }
  big = 0.0;
  o.d[0] = T(v0 < c.nv ? c.slot[v0] : 1.0);
  scale[0] = big;
  big = 0.0;
  const double parm = T(c.relax_to_inflated_prior ? c.slot[c.v] : 1.0);   // :387-391
  o.d[1] = parm;
  scale[1] = big;
  big = 0.0;
  o.d[2] = rtpp ? T(1.0 - T(c.relax_alpha)) : T(1.0);                      // :1953-1966
  scale[2] = big;
  // :1971-2002
  big = 1.0;
  double rs = 1.0;
  if (c.var_g > 0.0 && c.var_a > 0.0) {
    const double ratio = T(T(T(c.var_g) * parm) / T(T(c.var_a) * c.km1));
    const double root = T(sqrt(ratio));
    rs = T(T(T(T(c.relax_alpha_spread) * root) - c.relax_alpha_spread) + 1.0);
  }
  o.d[3] = rs;
  scale[3] = big;
  o.d[4] = rtpp ? o.d[2] : (c.relax_alpha_spread != 0.0 ? rs : 1.0);
  scale[4] = rtpp ? scale[2] : scale[3];
  o.d[5] = (rtps && !o.i[1]) ? o.d[4] : 1.0;                               // :460-462
  scale[5] = scale[4];
  big = 0.0;
  o.d[6] = rtpp ? T(T(c.relax_alpha) * T(sqrt(parm))) : 0.0;               // :1960-1963
  o.d[7] = o.d[6];
  scale[6] = scale[7] = big;
  // :472-487 with the beta blend
  big = scale[4] > scale[6] ? scale[4] : scale[6];
  {
    const double pert = T(T(o.d[4] * T(c.tx)) + T(o.d[6] * T(c.x)));
    const double incr = T(T(c.beta) * T(pert + T(c.sdot)));
    const double keep = T(T(1.0 - c.beta) * c.x);
    o.d[8] = T(T(T(c.xm) + incr) + keep);
  }
  scale[8] = big;
  // :500-513
  big = 0.0;
  o.d[9] = T(c.val);
  if (c.q_sprd > c.q_sprd_max) o.d[9] = T(T(c.q_mean) + T(T(T(c.val - c.q_mean) * T(c.q_sprd_max)) / T(c.q_sprd)));
  scale[9] = big;
  // common_letkf.f90:233-254
  big = 0.0;
  {
    const double parm4 = T(T(T(T(c.parm1) - T(c.parm3)) / T(c.parm2)) - T(c.infl_old));
    const double root = T(T(T(c.infl_old * c.parm2) + c.parm3) / c.parm2);
    const double sigma_o = T(T(2.0 / c.parm3) * T(root * root));
    const double sigma_b = T(0.04 * 0.04);
    const double gain = T(sigma_b / T(sigma_o + sigma_b));
    o.d[10] = T(c.infl_old + T(gain * parm4));
  }
  scale[10] = big;
  big = 0.0;
  o.d[11] = c.colvalid ? T(sqrt(T(T(c.km1) / T(c.lam)))) : 0.0;
  scale[11] = big;
  big = 0.0;
  o.d[12] = c.colvalid ? T(1.0 / T(c.lam)) : 0.0;
  scale[12] = big;
}

int main() {
  std::vector<Case> cs;
  const double eps_s = 1.4901161193847656e-08;
  const double alphas[3][2] = {{0.7, 0.0}, {0.0, 0.95}, {0.0, 0.0}};          // RTPP, RTPS, neither
  const double vars[3][2] = {{0.0, 5.0}, {5.0, 0.0}, {7.3, 0.021}};           // var_g = 0, var_a = 0, both positive
  const int vs[4] = {4, 5, 9, 10};                                            // iv_q_first - 1, iv_q_first, iv_q_last, iv_q_last + 1
  const unsigned masks[4] = {0x7FFu, 0x7F8u, 0x000u, 0x3E0u};                 // all; first updated = 3; none; only the q variables
  const double betas[3] = {0.0, 0.5, 1.0};
  const double lmx0 = 3.7;
  const double st[8][4] = {{1, 60, 10.0, 1.0},  {0, 59, 10.0, 1.0},           {0, 60, 10.0, 1.0},
                           {1, 60, 0.0, 0.0},   {1, 60, lmx0, lmx0 * eps_s},  {1, 60, lmx0, nextafter(lmx0 * eps_s, 0.0)},
                           {1, 60, lmx0, nextafter(lmx0 * eps_s, 1.0)},       {0, 60, 0.0, 0.0}};
  const double qmax = 0.1;
  const double qs[5] = {nextafter(qmax, 0.0), nextafter(qmax, 1.0), qmax, 0.25, 0.0};
  const double pm[4] = {29999.0, 30001.0, 30000.0, 101325.0};
  for (int pass = 0; pass < 2; ++pass)
    for (int a = 0; a < 3; ++a)
      for (int pr = 0; pr < 2; ++pr)
        for (int g = 0; g < 3; ++g)
          for (int qk = 0; qk < 2; ++qk)
            for (int iv = 0; iv < 4; ++iv) {
              const int i = (int)cs.size();
              Case c;
              memset(&c, 0, sizeof(c));
              c.relax_alpha = alphas[a][0];
              c.relax_alpha_spread = alphas[a][1];
              c.relax_to_inflated_prior = pr;
              c.q_update_top = (i % 3 == 2) ? 0.0 : 30000.0;
              c.q_sprd_max = qmax;
              c.iv_p = 3;
              c.iv_q_first = 5;
              c.iv_q_last = 9;
              c.max_sweep = (int)st[(i + i / 8) % 8][1];
              c.nv = NV;
              c.var_mask = masks[(i / 8 + iv + pass) % 4];
              c.p_mean = pm[(i / 3) % 4];
              for (int v = 0; v < NV; ++v) c.slot[v] = 1.0 + 0.013 * v + 1e-3 * (i % 7);
              c.qskip = qk;
              c.v = vs[iv];
              c.var_g = vars[g][0] * (1.0 + 0.1 * pass);
              c.var_a = vars[g][1];
              c.km1 = 49.0 - 30.0 * pass;
              c.xm = 285.3 + i;
              c.x = ((i % 5) - 2) * 0.731;
              c.beta = betas[i % 3];
              c.tx = ((i % 7) - 3) * 0.413;
              c.sdot = ((i % 4) - 1.5) * 0.059;
              c.q_mean = 0.0123;
              c.val = c.q_mean * (1.0 + ((i % 9) - 4) * 0.07);
              c.q_sprd = qs[i % 5];
              c.infl_old = 1.0 + 0.05 * (i % 6);
              c.parm3 = 20.0 + (i % 11);
              c.parm1 = c.parm3 * (0.8 + 0.1 * (i % 5));
              c.parm2 = 3.0 + 0.37 * (i % 13);
              c.jconv = (int)st[(i + i / 8) % 8][0];
              c.lmx = st[(i + i / 8) % 8][2];
              c.lmn = st[(i + i / 8) % 8][3];
              c.lam = 49.0 / c.infl_old + 0.3 * (i % 10);
              c.colvalid = (i % 6) != 5;
              cs.push_back(c);
            }
  const int n = (int)cs.size();
  std::vector<double> infl((size_t)n * NV), xmean((size_t)n * NV, 1.0);
  for (int i = 0; i < n; ++i) {
    for (int v = 0; v < NV; ++v) infl[i + (size_t)n * v] = cs[i].slot[v];
    xmean[(size_t)i * NV + cs[i].iv_p] = cs[i].p_mean;
  }
  Case* d_cs;
  double *d_infl, *d_xm;
  Out* d_out;
  if (hipMalloc(&d_cs, n * sizeof(Case)) != hipSuccess || hipMalloc(&d_infl, infl.size() * 8) != hipSuccess ||
      hipMalloc(&d_xm, xmean.size() * 8) != hipSuccess || hipMalloc(&d_out, n * sizeof(Out)) != hipSuccess)
    return 2;
  (void)hipMemcpy(d_cs, cs.data(), n * sizeof(Case), hipMemcpyHostToDevice);
  (void)hipMemcpy(d_infl, infl.data(), infl.size() * 8, hipMemcpyHostToDevice);
  (void)hipMemcpy(d_xm, xmean.data(), xmean.size() * 8, hipMemcpyHostToDevice);
  hipLaunchKernelGGL(eval, dim3((n + 63) / 64), dim3(64), 0, 0, d_cs, n, d_infl, d_xm, d_out);
  std::vector<Out> out(n);
  if (hipMemcpy(out.data(), d_out, n * sizeof(Out), hipMemcpyDeviceToHost) != hipSuccess) return 2;

  static const char* iname[NI] = {"q_update_skipped", "var_skipped", "in_class", "var_updated", "first_updated_var", "wants_variances", "eig_status", "spectrum_status"};
  static const char* dname[ND] = {"solve_inflation", "relax_parm", "rtpp_factor", "rtps_factor", "relax_factor", "rtps_reported", "rtpp_diag(parm)",
                                  "rtpp_diag(pt, v)", "analysis_value", "q_clamped", "adaptive_inflation", "spectra.sc1", "spectra.sc2"};
  int bad = 0;
  double worst[ND] = {0.0};
  int seen[NI][4] = {{0}}, first_later = 0, first_none = 0;
  for (int i = 0; i < n; ++i) {
    Out h;
    double scale[ND];
    host_eval(cs[i], h, scale);
    if (h.i[4] > 0 && h.i[4] < NV) first_later = 1;
    if (h.i[4] == NV) first_none = 1;
    for (int j = 0; j < NI; ++j) {
      if (h.i[j] >= 0 && h.i[j] < 4) seen[j][h.i[j]] = 1;
      if (out[i].i[j] != h.i[j]) {
        if (bad++ < 10) printf("case %d %s: device %d host %d\n", i, iname[j], out[i].i[j], h.i[j]);
      }
    }
    for (int j = 0; j < ND; ++j) {
      const double bound = 8.0 * 0x1p-53 * scale[j];
      const double err = fabs(out[i].d[j] - h.d[j]);
      const bool ok = (out[i].d[j] == h.d[j]) || err <= bound;
      const double ratio = err == 0.0 ? 0.0 : err / bound;
      if (ok && ratio > worst[j]) worst[j] = ratio;
      if (!ok) {
        if (bad++ < 10) printf("case %d %s: device %.17g host %.17g bound %.3g\n", i, dname[j], out[i].d[j], h.d[j], bound);
      }
    }
  }
  // the table must reach every answer of the predicates and every status
  for (int j = 0; j < NI; ++j) {
    const int need = (j == 6 || j == 7) ? 4 : (j == 4 ? 0 : 2);
    for (int r = 0; r < need; ++r)
      if (!seen[j][r]) {
        printf("%s never gave %d\n", iname[j], r);
        ++bad;
      }
  }
  if (!first_later || !first_none) {
    printf("first_updated_var: no class with a later first variable (%d) or with none (%d)\n", first_later, first_none);
    ++bad;
  }
  printf("%d tuples\n", n);
  for (int j = 0; j < ND; ++j) printf("%-20s largest error / bound %.3f\n", dname[j], worst[j]);
  printf("mismatches %d\n", bad);
  return bad ? 1 : 0;
}
