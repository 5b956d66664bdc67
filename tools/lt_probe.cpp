// hipBLASLt vs pcnn_deep GEMM probe — driven from C++ so no torch
// dispatch overhead contaminates the comparison (round-1 finding:
// standalone Lt kernels beat ours 1.6-3.3x via torch, but in-step torch
// dispatch added ~110 us host wall; VERDICT r1 #3a asks for the direct
// C++ measurement).
//
// Measures, interleaved in ONE process (guide rule 24), median of R
// rounds: hipblasLtMatmul (bf16 in, fp32 compute, bf16 out, heuristic
// algo) vs pcnn_deep_gemm on the DeepCNN bs=256 step shapes.
//
// Build (done by tools/build_lt_probe.sh or setup.py is NOT needed):
//   hipcc --offload-arch=gfx950 -O3 tools/lt_probe.cpp \
//       csrc/hip/conv_kernels.o -lhipblaslt -o tools/lt_probe
// Run on a GPU box: ./tools/lt_probe
#include <hip/hip_bf16.h>
#include <hip/hip_runtime.h>
#include <hipblaslt/hipblaslt.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../csrc/pcnn_launch.h"

#define CK(x)                                                      \
  do {                                                             \
    auto e_ = (x);                                                 \
    if (e_ != hipSuccess) {                                        \
      fprintf(stderr, "HIP error %d at %s:%d\n", (int)e_, __FILE__, \
              __LINE__);                                           \
      exit(1);                                                     \
    }                                                              \
  } while (0)
#define CKL(x)                                                        \
  do {                                                                \
    auto e_ = (x);                                                    \
    if (e_ != HIPBLAS_STATUS_SUCCESS) {                               \
      fprintf(stderr, "hipblasLt error %d at %s:%d\n", (int)e_,       \
              __FILE__, __LINE__);                                    \
      exit(1);                                                        \
    }                                                                 \
  } while (0)

struct Shape {
  const char* name;
  long long M;
  int N, K;
};

template <typename F>
static double bench(F&& fn, int iters = 100, int warm = 10) {
  for (int i = 0; i < warm; ++i) fn();
  CK(hipDeviceSynchronize());
  auto t0 = std::chrono::high_resolution_clock::now();
  for (int i = 0; i < iters; ++i) fn();
  CK(hipDeviceSynchronize());
  auto t1 = std::chrono::high_resolution_clock::now();
  return std::chrono::duration<double, std::micro>(t1 - t0).count() / iters;
}

int main() {
  hipblasLtHandle_t handle;
  CKL(hipblasLtCreate(&handle));
  void* ws;
  const size_t ws_size = 64u << 20;
  CK(hipMalloc(&ws, ws_size));

  // DeepCNN bs=256 step shapes: fwd st0/st1/st2, dgrad st1/st2
  Shape shapes[] = {
      {"fwd-st0 (M=262144,N=32,K=96)", 262144, 32, 96},
      {"fwd-st1 (M=65536,N=64,K=800)", 65536, 64, 800},
      {"fwd-st2 (M=16384,N=64,K=1600)", 16384, 64, 1600},
      {"dgrad-st1 (M=65536,N=32,K=1600)", 65536, 32, 1600},
      {"dgrad-st2 (M=16384,N=64,K=1600)", 16384, 64, 1600},
  };

  for (const auto& sh : shapes) {
    const long long M = sh.M;
    const int N = sh.N, K = sh.K;
    __hip_bfloat16 *A, *C;
    float* Bf;
    __hip_bfloat16* Bb;
    float* c32;
    CK(hipMalloc(&A, sizeof(__hip_bfloat16) * M * K));
    CK(hipMalloc(&C, sizeof(__hip_bfloat16) * M * N));
    CK(hipMalloc(&Bf, sizeof(float) * K * N));
    CK(hipMalloc(&Bb, sizeof(__hip_bfloat16) * K * N));
    // split-K scratch sized like the engine's (so "ours" is the exact
    // engine configuration, split included)
    CK(hipMalloc(&c32, sizeof(float) * 8 * M * N));
    CK(hipMemset(A, 0x3c, sizeof(__hip_bfloat16) * M * K));
    CK(hipMemset(Bf, 0x3d, sizeof(float) * K * N));
    CK(hipMemset(Bb, 0x3c, sizeof(__hip_bfloat16) * K * N));

    // ---- hipBLASLt: row-major C[M][N] = A[M][K] @ B[K][N] expressed
    // col-major as C'[N][M] = B'[N][K] @ A'[K][M] (opN/opN, operands
    // swapped) -------------------------------------------------------
    hipblasLtMatmulDesc_t op;
    CKL(hipblasLtMatmulDescCreate(&op, HIPBLAS_COMPUTE_32F, HIP_R_32F));
    hipblasLtMatrixLayout_t la, lb, lc;
    // B' = our B viewed col-major: N rows x K cols, ld = N
    CKL(hipblasLtMatrixLayoutCreate(&lb, HIP_R_16BF, N, K, N));
    // A' = our A viewed col-major: K rows x M cols, ld = K
    CKL(hipblasLtMatrixLayoutCreate(&la, HIP_R_16BF, K, M, K));
    CKL(hipblasLtMatrixLayoutCreate(&lc, HIP_R_16BF, N, M, N));
    hipblasLtMatmulPreference_t pref;
    CKL(hipblasLtMatmulPreferenceCreate(&pref));
    CKL(hipblasLtMatmulPreferenceSetAttribute(
        pref, HIPBLASLT_MATMUL_PREF_MAX_WORKSPACE_BYTES, &ws_size,
        sizeof(ws_size)));
    hipblasLtMatmulHeuristicResult_t heur[4];
    int nheur = 0;
    CKL(hipblasLtMatmulAlgoGetHeuristic(handle, op, lb, la, lc, lc, pref, 4,
                                        heur, &nheur));
    if (nheur == 0) {
      printf("%-34s  Lt: NO ALGO\n", sh.name);
    } else {
      float alpha = 1.f, beta = 0.f;
      auto lt = [&]() {
        hipblasLtMatmul(handle, op, &alpha, Bb, lb, A, la, &beta, C, lc, C,
                        lc, &heur[0].algo, ws, ws_size, 0);
      };
      double t_lt = bench(lt);
      auto ours = [&]() {
        pcnn_deep_gemm(A, Bf, Bb, nullptr, C, M, K, N, K, N, 1, 0,
                       nullptr, 0, 0, 0, 0, 0, nullptr, nullptr, nullptr, 0,
                       c32, 8 * M * N, 1, nullptr);
      };
      double t_ours = bench(ours);
      // interleave a second round (process-variance guard)
      double t_lt2 = bench(lt);
      double t_ours2 = bench(ours);
      printf("%-34s  Lt: %7.2f/%7.2f us   ours: %7.2f/%7.2f us   ratio %.2fx\n",
             sh.name, t_lt, t_lt2, t_ours, t_ours2,
             std::min(t_ours, t_ours2) / std::min(t_lt, t_lt2));
    }
    hipblasLtMatmulPreferenceDestroy(pref);
    hipblasLtMatrixLayoutDestroy(la);
    hipblasLtMatrixLayoutDestroy(lb);
    hipblasLtMatrixLayoutDestroy(lc);
    hipblasLtMatmulDescDestroy(op);
    CK(hipFree(A));
    CK(hipFree(C));
    CK(hipFree(Bf));
    CK(hipFree(Bb));
    CK(hipFree(c32));
  }
  CK(hipFree(ws));
  hipblasLtDestroy(handle);
  return 0;
}
