// fri_fold.hip — the FRI fold chain (values only) for CDNA4 (gfx950):
// y'_i = y_i + beta * y_{i+len/2} (crates/sezkp-stark/src/v1/prover.rs:200-239),
// one fold per pass (k_fold) or F = 2..4 folds per pass (k_foldm). The folds
// fused into a tree kernel are in merkle_dev.h (fold_load), the replays of
// the small layers in fri_forest.hip.
#include "dev_common.h"
#include "sezkp_internal.h"

namespace sezkp {

constexpr int FOLD_THREADS = 256;

// y'_i = y_i + beta * y_{i+len}, 4 per lane.
__global__ void __launch_bounds__(FOLD_THREADS) k_fold(const uint64_t* __restrict__ in, uint64_t* __restrict__ out,
                                                       int logLen, uint64_t beta, const uint64_t* __restrict__ dbeta) {
  const uint64_t len = 1ULL << logLen;
  if (dbeta) beta = *dbeta;
  const uint64_t i = ((uint64_t)blockIdx.x * FOLD_THREADS + threadIdx.x) * 4;
  if (i >= len) return;
  const ulonglong2* p = reinterpret_cast<const ulonglong2*>(in + i);
  const ulonglong2* q = reinterpret_cast<const ulonglong2*>(in + i + len);
  ulonglong2* o = reinterpret_cast<ulonglong2*>(out + i);
  const ulonglong2 a0 = p[0], a1 = p[1], b0 = q[0], b1 = q[1];
  o[0] = make_ulonglong2(gl_add(a0.x, gl_mul(beta, b0.x)), gl_add(a0.y, gl_mul(beta, b0.y)));
  o[1] = make_ulonglong2(gl_add(a1.x, gl_mul(beta, b1.x)), gl_add(a1.y, gl_mul(beta, b1.y)));
}

// F folds per pass (F = 2..4): layer r + m (m = 1..F) at index i + j L, j <
// 2^(F-m), L = len(layer r + F), is y_m = y_{m-1}[i + j L] + b_m
// y_{m-1}[i + (j + 2^(F-m)) L]; a lane holds two adjacent i, reads its 2^F
// strided pairs of layer r once and writes every intermediate layer once.
template <int F>
__global__ void __launch_bounds__(FOLD_THREADS) k_foldm(const uint64_t* __restrict__ in, FoldOuts O, int logLenF) {
  constexpr int W = 1 << F;
  const uint64_t L = 1ULL << logLenF;
  const uint64_t i = ((uint64_t)blockIdx.x * FOLD_THREADS + threadIdx.x) * 2;
  if (i >= L) return;
  uint64_t x0[W], x1[W];
#pragma unroll
  for (int j = 0; j < W; j++) {
    const ulonglong2 v = *reinterpret_cast<const ulonglong2*>(in + i + (uint64_t)j * L);
    x0[j] = v.x;
    x1[j] = v.y;
  }
#pragma unroll
  for (int m = 1; m <= F; m++) {
    const int half = W >> m;
    const uint64_t b = O.beta[m - 1];
    uint64_t* out = O.out[m - 1];
#pragma unroll
    for (int j = 0; j < half; j++) {
      x0[j] = gl_add(x0[j], gl_mul(b, x0[j + half]));
      x1[j] = gl_add(x1[j], gl_mul(b, x1[j + half]));
      *reinterpret_cast<ulonglong2*>(out + i + (uint64_t)j * L) = make_ulonglong2(x0[j], x1[j]);
    }
  }
}

hipError_t launch_fold(hipStream_t st, const uint64_t* in, uint64_t* out, int logLen, uint64_t beta,
                       const uint64_t* dbeta) {
  if (logLen < 2) return hipErrorInvalidValue;
  const uint64_t per = (uint64_t)FOLD_THREADS * 4;
  const unsigned grid = (unsigned)(((1ULL << logLen) + per - 1) / per);
  hipLaunchKernelGGL(k_fold, dim3(grid), dim3(FOLD_THREADS), 0, st, in, out, logLen, beta, dbeta);
  return hipGetLastError();
}

hipError_t launch_foldm(hipStream_t st, const uint64_t* in, const FoldOuts& outs, int F, int logLenF) {
  if (logLenF < 1 || F < 2 || F > FOLD_MAX) return hipErrorInvalidValue;
  const uint64_t per = (uint64_t)FOLD_THREADS * 2;
  const unsigned grid = (unsigned)(((1ULL << logLenF) + per - 1) / per);
  switch (F) {
    case 2: hipLaunchKernelGGL(k_foldm<2>, dim3(grid), dim3(FOLD_THREADS), 0, st, in, outs, logLenF); break;
    case 3: hipLaunchKernelGGL(k_foldm<3>, dim3(grid), dim3(FOLD_THREADS), 0, st, in, outs, logLenF); break;
    default: hipLaunchKernelGGL(k_foldm<4>, dim3(grid), dim3(FOLD_THREADS), 0, st, in, outs, logLenF); break;
  }
  return hipGetLastError();
}

}  // namespace sezkp
