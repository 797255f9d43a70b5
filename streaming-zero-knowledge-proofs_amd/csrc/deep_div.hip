// deep_div.hip — the per-point DEEP division for CDNA4 (gfx950):
// out_i = y_i * (3*w_N^i - z)^-1 (crates/sezkp-stark/src/v1/lde.rs:76-93).
//
// 16 consecutive elements per lane, one Montgomery batch inversion per
// workgroup (4096 elements): wave prefix/suffix product scans + one Fermat
// inversion in lane 0 of wave 0.
#include "dev_common.h"
#include "sezkp_internal.h"

namespace sezkp {

constexpr int DEEP_THREADS = 256;
constexpr int DEEP_PER = 16;
__global__ void __launch_bounds__(DEEP_THREADS) k_deep(uint64_t* __restrict__ y, int logN, uint64_t z, NttTables T,
                                                       int logP, uint32_t g, uint64_t shift) {
  __shared__ uint64_t wtot[DEEP_THREADS / 64];
  __shared__ uint64_t s_inv;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint64_t i0 = ((uint64_t)blockIdx.x * DEEP_THREADS + tid) * DEEP_PER;
  const uint64_t N = 1ULL << (logN - logP);  // local length
  const bool act = i0 < N;
  uint64_t d[DEEP_PER], a[DEEP_PER];
  uint64_t P = 1;
  if (act) {
    // x_j = shift * w_N^(g + P j) (shift = 3 in the prover); first from the
    // two-level table, then incremental
    const uint64_t e = ((uint64_t)g + (i0 << logP)) << (T.K - logN);
    uint64_t x = gl_mul(gl_mul(T.hi[e >> T.S], T.lo[e & ((1ULL << T.S) - 1)]), shift);
    uint64_t wN;
    {
      const uint64_t e1 = 1ULL << (T.K - logN + logP);
      wN = gl_mul(T.hi[e1 >> T.S], T.lo[e1 & ((1ULL << T.S) - 1)]);
    }
#pragma unroll
    for (int j = 0; j < DEEP_PER; j++) {
      d[j] = i0 + j < N ? gl_sub(x, z) : 1;  // N < 16 (tiny kernel-level calls): neutral tail
      P = gl_mul(P, d[j]);
      a[j] = P;
      x = gl_mul(x, wN);
    }
  }
  // wave inclusive prefix S and exclusive suffix Q of the lane products
  uint64_t S = P, Tq = P;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    uint64_t u = __shfl_up(S, o, 64);
    if (lane >= o) S = gl_mul(S, u);
    uint64_t v = __shfl_down(Tq, o, 64);
    if (lane + o < 64) Tq = gl_mul(Tq, v);
  }
  uint64_t Q = __shfl_down(Tq, 1, 64);
  if (lane == 63) Q = 1;
  uint64_t Sprev = __shfl_up(S, 1, 64);
  if (lane == 0) Sprev = 1;
  if (lane == 63) wtot[wave] = S;
  __syncthreads();
  if (tid == 0) {
    uint64_t t = 1;
#pragma unroll
    for (int w = 0; w < DEEP_THREADS / 64; w++) t = gl_mul(t, wtot[w]);
    s_inv = gl_inv(t);
  }
  __syncthreads();
  uint64_t invW = s_inv;  // inverse of this wave's total = inv(all) * prod(other waves)
#pragma unroll
  for (int w = 0; w < DEEP_THREADS / 64; w++)
    if (w != wave) invW = gl_mul(invW, wtot[w]);
  // inv(S_lane) = invW * Q ; inv(P_lane) = inv(S_lane) * S_{lane-1}
  uint64_t inv_run = gl_mul(gl_mul(invW, Q), Sprev);
  if (!act) return;
#pragma unroll
  for (int j = DEEP_PER - 1; j >= 0; j--) {
    uint64_t inv_dj = j ? gl_mul(inv_run, a[j - 1]) : inv_run;
    inv_run = gl_mul(inv_run, d[j]);
    if (i0 + j < N) y[i0 + j] = gl_mul(y[i0 + j], inv_dj);
  }
}

hipError_t launch_deep(hipStream_t st, uint64_t* y, int logN, uint64_t z, const NttTables& tw, int logP, uint32_t g,
                       uint64_t shift) {
  if (logP > logN) return hipErrorInvalidValue;
  const uint64_t N = 1ULL << (logN - logP);
  const uint64_t per_wg = (uint64_t)DEEP_THREADS * DEEP_PER;
  const unsigned grid = (unsigned)((N + per_wg - 1) / per_wg);
  hipLaunchKernelGGL(k_deep, dim3(grid), dim3(DEEP_THREADS), 0, st, y, logN, z, tw, logP, g, shift);
  return hipGetLastError();
}

}  // namespace sezkp
