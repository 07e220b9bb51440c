// ubench_issue_cost.hip -- what one vector instruction of the Jacobi rotation's scalar chain costs a SIMD, in cycles per
// wave-instruction, at the occupancy the k = 50 wave kernel runs at (two waves per SIMD) and at one wave per SIMD.
// (round 11, DESIGN 4.1 (r11): the price table the integer threshold tests, the per-step-pair vote and the 32-bit seed of
// 1/sqrt(w) were priced from before they were written.)
// One workgroup per CU, 256 or 512 threads.  Every wave runs ITERS x 32 copies of one instruction on 8 independent registers
// (four rounds of eight: no copy waits for the one before it), so the figure is the issue cost, not the latency.
// cycles = wall time x the clock the runtime reports / (instructions per wave x waves per SIMD); the last column is the same
// figure relative to v_fma_f64's, which does not depend on the clock the chip really ran at.
// Build: hipcc --offload-arch=gfx950 -O3 tools/ubench_issue_cost.hip -o tools/ubench_issue_cost
#include <hip/hip_runtime.h>
#include <cstdio>

enum Op { MUL_F64, CMP_F64, FMA_F64, RSQ_F64, RCP_F64, RSQ_F32_CVT, RSQ_F32, CVT_F32_F64, CVT_F64_F32, SUB_U32, CMP_I32, MAX_I32, CNDMASK, NOPS };
static const char* kName[NOPS] = {"v_mul_f64", "v_cmp_gt_f64", "v_fma_f64", "v_rsq_f64", "v_rcp_f64", "v_cvt_f32_f64 + v_rsq_f32 + v_cvt_f64_f32 (3)",
                                  "v_rsq_f32", "v_cvt_f32_f64", "v_cvt_f64_f32", "v_sub_u32", "v_cmp_gt_i32", "v_max_i32", "v_cndmask_b32"};
static const int kPerCopy[NOPS] = {1, 1, 1, 1, 1, 3, 1, 1, 1, 1, 1, 1, 1};

template <int OP>
__device__ __forceinline__ void one(double& x, int& i, float& f, const double a, const double b, const int j) {
  if constexpr (OP == MUL_F64) asm volatile("v_mul_f64 %0, %0, %1" : "+v"(x) : "v"(a));
  else if constexpr (OP == CMP_F64) asm volatile("v_cmp_gt_f64 vcc, %0, %1" : : "v"(x), "v"(a) : "vcc");
  else if constexpr (OP == FMA_F64) asm volatile("v_fma_f64 %0, %0, %1, %2" : "+v"(x) : "v"(a), "v"(b));
  else if constexpr (OP == RSQ_F64) asm volatile("v_rsq_f64 %0, %0" : "+v"(x));
  else if constexpr (OP == RCP_F64) asm volatile("v_rcp_f64 %0, %0" : "+v"(x));
  else if constexpr (OP == RSQ_F32_CVT)
    asm volatile("v_cvt_f32_f64 %1, %0\n\tv_rsq_f32 %1, %1\n\tv_cvt_f64_f32 %0, %1" : "+v"(x), "+v"(f));
  else if constexpr (OP == RSQ_F32) asm volatile("v_rsq_f32 %0, %0" : "+v"(f));
  else if constexpr (OP == CVT_F32_F64) asm volatile("v_cvt_f32_f64 %0, %1" : "+v"(f) : "v"(x));
  else if constexpr (OP == CVT_F64_F32) asm volatile("v_cvt_f64_f32 %0, %1" : "+v"(x) : "v"(f));
  else if constexpr (OP == SUB_U32) asm volatile("v_sub_u32 %0, %0, %1" : "+v"(i) : "v"(j));
  else if constexpr (OP == CMP_I32) asm volatile("v_cmp_gt_i32 vcc, %0, %1" : : "v"(i), "v"(j) : "vcc");
  else if constexpr (OP == MAX_I32) asm volatile("v_max_i32 %0, %0, %1" : "+v"(i) : "v"(j));
  else if constexpr (OP == CNDMASK) asm volatile("v_cndmask_b32 %0, %0, %1, vcc" : "+v"(i) : "v"(j) : "vcc");
}

template <int OP>
__global__ void __launch_bounds__(512) k(const int iters, double* out) {
  double x[8];
  int i[8];
  float f[8];
  const double a = 1.0000001, b = 1e-9;
  const int j = 1 + (threadIdx.x & 1);
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    x[r] = 1.25 + threadIdx.x * 1e-6 + r;
    i[r] = 0x40000000 + threadIdx.x + r;
    f[r] = 1.25f + r;
  }
  for (int it = 0; it < iters; ++it) {
#pragma unroll
    for (int rep = 0; rep < 4; ++rep)
#pragma unroll
      for (int r = 0; r < 8; ++r) one<OP>(x[r], i[r], f[r], a, b, j);
  }
  double s = 0.0;
#pragma unroll
  for (int r = 0; r < 8; ++r) s += x[r] + i[r] + f[r];
  if (s == 12345.678) out[threadIdx.x] = s;   // (never: keeps the registers alive; out holds 512 doubles)
}

template <int OP>
static float run(const int ncu, const int threads, const int iters, double* out) {
  hipEvent_t e0, e1;
  hipEventCreate(&e0);
  hipEventCreate(&e1);
  float ms = 0.f;
  for (int rep = 0; rep < 3; ++rep) {   // the third launch is the one reported
    hipEventRecord(e0);
    hipLaunchKernelGGL(k<OP>, dim3(ncu), dim3(threads), 0, 0, iters, out);
    hipEventRecord(e1);
    hipEventSynchronize(e1);
    hipEventElapsedTime(&ms, e0, e1);
  }
  hipEventDestroy(e0);
  hipEventDestroy(e1);
  return ms;
}

typedef float (*RunFn)(int, int, int, double*);
static const RunFn kRun[NOPS] = {run<MUL_F64>, run<CMP_F64>, run<FMA_F64>, run<RSQ_F64>, run<RCP_F64>, run<RSQ_F32_CVT>, run<RSQ_F32>,
                                 run<CVT_F32_F64>, run<CVT_F64_F32>, run<SUB_U32>, run<CMP_I32>, run<MAX_I32>, run<CNDMASK>};

int main() {
  hipSetDevice(0);
  hipDeviceProp_t pr;
  hipGetDeviceProperties(&pr, 0);
  const int ncu = pr.multiProcessorCount, iters = 20000;
  double* out;
  if (hipMalloc(&out, 512 * sizeof(double)) != hipSuccess) return 1;
  printf("CUs %d, clock %d MHz, %d x 32 copies per wave\n", ncu, pr.clockRate / 1000, iters);
  for (int wps = 1; wps <= 2; ++wps) {
    const int threads = 256 * wps;
    const double fma_ms = kRun[FMA_F64](ncu, threads, iters, out);
    printf("-- %d wave(s) per SIMD\n", wps);
    for (int op = 0; op < NOPS; ++op) {
      const double ms = kRun[op](ncu, threads, iters, out);
      const double n = (double)iters * 32.0 * kPerCopy[op];
      const double cyc = ms * 1e-3 * (pr.clockRate * 1e3) / (n * wps);
      printf("%-48s %8.3f ms  %6.2f cycles per wave-instruction  %5.2f x v_fma_f64\n", kName[op], ms, cyc, ms / kPerCopy[op] / fma_ms);
    }
  }
  if (hipDeviceSynchronize() != hipSuccess) return 1;
  hipFree(out);
  return 0;
}
