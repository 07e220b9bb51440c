// semantics probe (MI355X): wave_shl:1 / wave_shr:1 DPP moves with bound_ctrl and EXEC-masked source lanes,
// and v_permlane32_swap.  The kp* rows probe the other half of the bound_ctrl rule, which jacobi_split relies on at the two ends of
// its line: with bound_ctrl = 0 a lane whose source lane does not exist (lane 0 under wave_shr:1, lane 63 under wave_shl:1) or is
// switched off keeps the old value of its destination (-1000 - lane here).  The last line is v_rsq_f64(1.0) and the third-order
// step on top of it, which must both be exactly 1 for a pair that is not rotated to leave its scales alone.  Build: hipcc --offload-arch=gfx950 -O3 tools/ubench_dpp.hip -o tools/ubench_dpp
#include <hip/hip_runtime.h>
#include <cstdio>

__global__ void probe_rsq(double* out) {
  const double x = 1.0 + out[2];   // (out[2] = 0: keeps the compiler from folding the seed)
  const double y = __builtin_amdgcn_rsq(x);
  const double e = fma(-x * y, y, 1.0);
  out[0] = y;
  out[1] = fma(y, e * fma(0.375, e, 0.5), y);
}

__global__ void probe(int* out, int nact) {
  const int lane = threadIdx.x;
  int shl = -7, shr = -7, sw0 = -7, sw1 = -7, kpl = -7, kpr = -7;
  const int slot = lane & 31;
  if (slot < nact) {
    const int v = 100 + lane;
    shl = __builtin_amdgcn_mov_dpp(v, 0x130, 0xF, 0xF, true);
    shr = __builtin_amdgcn_mov_dpp(v, 0x138, 0xF, 0xF, true);
    kpl = __builtin_amdgcn_update_dpp(-1000 - lane, v, 0x130, 0xF, 0xF, false);
    kpr = __builtin_amdgcn_update_dpp(-1000 - lane, v, 0x138, 0xF, 0xF, false);
#if __has_builtin(__builtin_amdgcn_permlane32_swap)
    auto r = __builtin_amdgcn_permlane32_swap(v, v, false, false);
    sw0 = r[0];
    sw1 = r[1];
#endif
  }
  out[lane] = shl;
  out[64 + lane] = shr;
  out[128 + lane] = sw0;
  out[192 + lane] = sw1;
  out[256 + lane] = kpl;
  out[320 + lane] = kpr;
}

int main() {
  int* d;
  hipMalloc(&d, 384 * 4);
  int h[384];
  for (int nact : {32, 25}) {
    hipLaunchKernelGGL(probe, dim3(1), dim3(64), 0, 0, d, nact);
    hipMemcpy(h, d, sizeof(h), hipMemcpyDeviceToHost);
    printf("nact=%d\n", nact);
    const char* nm[6] = {"shl", "shr", "sw0", "sw1", "kpl", "kpr"};
    for (int a = 0; a < 6; ++a) {
      printf("%s:", nm[a]);
      for (int l = 0; l < 64; ++l) printf(" %d", h[64 * a + l]);
      printf("\n");
    }
  }
  // the rule jacobi_split builds on, checked: exit code 1 if the hardware does otherwise (h[] holds the run with 25 active slots)
  int bad = 0;
  for (int l = 0; l < 64; ++l) {
    if ((l & 31) >= 25) continue;
    const bool srcl = l + 1 < 64 && ((l + 1) & 31) < 25, srcr = l >= 1 && ((l - 1) & 31) < 25;
    bad += h[256 + l] != (srcl ? 100 + l + 1 : -1000 - l);
    bad += h[320 + l] != (srcr ? 100 + l - 1 : -1000 - l);
  }
  double* dd;
  double hd[3] = {0.0, 0.0, 0.0};
  hipMalloc(&dd, sizeof(hd));
  hipMemcpy(dd, hd, sizeof(hd), hipMemcpyHostToDevice);
  hipLaunchKernelGGL(probe_rsq, dim3(1), dim3(1), 0, 0, dd);
  hipMemcpy(hd, dd, sizeof(hd), hipMemcpyDeviceToHost);
  printf("rsq(1.0) = %.17g, refined %.17g\n", hd[0], hd[1]);
  bad += hd[0] != 1.0 || hd[1] != 1.0;
  printf("bound_ctrl = 0 keeps the destination, rsq(1) = 1: %s\n", bad ? "NO" : "yes");
  return bad ? 1 : 0;
}
