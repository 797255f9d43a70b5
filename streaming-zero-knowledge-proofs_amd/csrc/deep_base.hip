// deep_base.hip — the DEEP quotient on the base domain (DeepPoly,
// sezkp_internal.h): D_j and the partial sums of f(z), the q tables, and the
// coset pre-scaling of the kernel-level LDE. No transform runs here.
#include <algorithm>

#include "compose.h"
#include "ntt_dev.h"

namespace sezkp {

// ------------------------------------------- DEEP quotient (base domain)
// See DeepPoly (sezkp_internal.h). k_inv_base: D_j = C_j / (w_n^j - z) for the
// base points j in [row0, row0 + nrows), C_j the composition value of the
// row (compose.h, from k_compose_terms' sums: the composition's
// transcript-dependent half runs here), DQ_PER per lane, one Montgomery batch
// per WG, and the per-WG partial sums of D_j w_n^j; WG b of the range
// writes partial[b] (sharded ranks each own a block of rows and allgather
// their partials with the INTT coefficients, so every rank reduces the same sum).
template <int DQ_PER>
__global__ void __launch_bounds__(NTT_THREADS) k_inv_base(ComposeTerms Tm, uint64_t* __restrict__ Dout,
                                                          uint64_t* __restrict__ partial, int logn,
                                                          const DevChal* __restrict__ ch, NttTables T, uint64_t row0,
                                                          uint64_t nrows) {
  const uint64_t z = ch->z;
  __shared__ uint64_t wtot[NTT_THREADS / 64];
  __shared__ uint64_t s_inv;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  // the WG's rows wg0 + j NTT_THREADS + tid (j < DQ_PER): every load and
  // store of a j step is one coalesced row range (lane-consecutive rows
  // touched 8x the cache lines per instruction)
  const uint64_t wg0 = row0 + (uint64_t)blockIdx.x * NTT_THREADS * DQ_PER, end = row0 + nrows;
  uint64_t d[DQ_PER], a[DQ_PER], cv[DQ_PER];
  uint64_t Pp = 1;
  {
    const ComposeCoef K = compose_coef(ch);
    // exponents mod 2^K (w^(2^K) = 1): rows past a small n stay inside the
    // twiddle tables (their values are never used)
    const uint64_t kmask = (1ULL << T.K) - 1;
    const uint64_t e = ((wg0 + tid) << (T.K - logn)) & kmask;
    uint64_t x = gl_mul(T.hi[e >> T.S], T.lo[e & ((1ULL << T.S) - 1)]);
    const uint64_t e1 = ((uint64_t)NTT_THREADS << (T.K - logn)) & kmask;
    const uint64_t ws = gl_mul(T.hi[e1 >> T.S], T.lo[e1 & ((1ULL << T.S) - 1)]);  // w_n^NTT_THREADS
#pragma unroll
    for (int j = 0; j < DQ_PER; j++) {
      const uint64_t row = wg0 + (uint64_t)j * NTT_THREADS + tid;
      if (row < end) {
        cv[j] = compose_value(Tm, K, row, x);  // C_row (air.rs:49-136 + mask)
        d[j] = gl_sub(x, z);
      } else {  // past the block: a unit factor in the batch
        cv[j] = 0;
        d[j] = 1;
      }
      Pp = j ? gl_mul(Pp, d[j]) : d[j];
      a[j] = Pp;
      x = gl_mul(x, ws);
    }
  }
  uint64_t S = Pp, Tq = Pp;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint64_t u = __shfl_up(S, o, 64);
    if (lane >= o) S = gl_mul(S, u);
    const uint64_t v = __shfl_down(Tq, o, 64);
    if (lane + o < 64) Tq = gl_mul(Tq, v);
  }
  uint64_t Q = __shfl_down(Tq, 1, 64);
  if (lane == 63) Q = 1;
  uint64_t Sprev = __shfl_up(S, 1, 64);
  if (lane == 0) Sprev = 1;
  if (lane == 63) wtot[wave] = S;
  __syncthreads();
  if (tid == 0) {
    uint64_t t = wtot[0];
#pragma unroll
    for (int w = 1; w < NTT_THREADS / 64; w++) t = gl_mul(t, wtot[w]);
    s_inv = gl_inv(t);
  }
  __syncthreads();
  uint64_t invW = s_inv;
#pragma unroll
  for (int w = 0; w < NTT_THREADS / 64; w++)
    if (w != wave) invW = gl_mul(invW, wtot[w]);
  uint64_t inv_run = gl_mul(gl_mul(invW, Q), Sprev);
  uint64_t acc = 0;
#pragma unroll
  for (int j = DQ_PER - 1; j >= 0; j--) {
    const uint64_t ij = j ? gl_mul(inv_run, a[j - 1]) : inv_run;
    if (j) inv_run = gl_mul(inv_run, d[j]);
    const uint64_t row = wg0 + (uint64_t)j * NTT_THREADS + tid;
    if (row < end) {
      const uint64_t xj = gl_add(d[j], z);  // w_n^row
      const uint64_t Dj = gl_mul(cv[j], ij);
      Dout[row] = Dj;
      acc = gl_add(acc, gl_mul(Dj, xj));
    }
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) acc = gl_add(acc, __shfl_xor(acc, o, 64));
  __syncthreads();
  if (lane == 0) wtot[wave] = acc;
  __syncthreads();
  if (tid == 0) {
    uint64_t t = wtot[0];
#pragma unroll
    for (int w = 1; w < NTT_THREADS / 64; w++) t = gl_add(t, wtot[w]);
    partial[blockIdx.x] = t;
  }
}

// Coset scaling for a shift other than the prover's 3 (kernel-level ABI):
// a[p] *= base^e, e = bitrev_logn(p), from base^e = lo[e & 2047] hi[e >> 11].
__global__ void __launch_bounds__(NTT_THREADS) k_pow_tables(uint64_t* __restrict__ lo, uint64_t* __restrict__ hi,
                                                            uint64_t base, uint32_t nhi) {
  const uint32_t t = blockIdx.x * NTT_THREADS + threadIdx.x;
  if (t < 2048) lo[t] = gl_pow_dev(base, t);
  if (t < nhi) hi[t] = gl_pow_dev(base, 2048ull * t);
}
__global__ void __launch_bounds__(NTT_THREADS) k_scale_pow_bitrev(uint64_t* __restrict__ a, int logn,
                                                                  const uint64_t* __restrict__ lo,
                                                                  const uint64_t* __restrict__ hi) {
  const uint64_t p = blockIdx.x * (uint64_t)NTT_THREADS + threadIdx.x;
  if (p >> logn) return;
  const uint32_t e = logn ? __brev((uint32_t)p) >> (32 - logn) : 0;
  a[p] = gl_mul(a[p], gl_mul(lo[e & 2047], hi[e >> 11]));
}
hipError_t launch_scale_pow_bitrev(hipStream_t st, uint64_t* a, int logn, uint64_t base, uint64_t* scratch) {
  if (logn > 31) return hipErrorInvalidValue;
  const uint32_t nhi = logn > 11 ? 1u << (logn - 11) : 1u;
  uint64_t* lo = scratch;
  uint64_t* hi = scratch + 2048;
  const uint32_t nt = std::max<uint32_t>(2048, nhi);
  hipLaunchKernelGGL(k_pow_tables, dim3((nt + NTT_THREADS - 1) / NTT_THREADS), dim3(NTT_THREADS), 0, st, lo, hi, base,
                     nhi);
  const uint64_t n = 1ULL << logn;
  hipLaunchKernelGGL(k_scale_pow_bitrev, dim3((unsigned)((n + NTT_THREADS - 1) / NTT_THREADS)), dim3(NTT_THREADS), 0,
                     st, a, logn, lo, hi);
  return hipGetLastError();
}

// Every WG reduces the partials (S; f(z) = K1 S, c' = f(z) K2, kappa = K3 S),
// then grid-strides over the tables: rlo[t] = r^t, rhi[t] = c' r^(4096 t),
// rhk[t] = kappa r^(4096 t); or, for the closed-form first LDE stages
// (gk != null): rlo, rhu[t] = r^(4096 t) and gk[s] = c' G[s] - kappa.
__global__ void __launch_bounds__(NTT_THREADS) k_q_tables(const uint64_t* __restrict__ partial, uint32_t nparts,
                                                          const DevChal* __restrict__ ch, uint64_t* __restrict__ rlo,
                                                          uint64_t* __restrict__ rhi, uint32_t nhi,
                                                          uint64_t* __restrict__ rhk, uint32_t nhk,
                                                          uint64_t* __restrict__ rhu, uint64_t* __restrict__ gk) {
  const uint64_t K1 = ch->K1, K2 = ch->K2, K3 = ch->K3, r = ch->rho, r4096 = ch->rho4096;
  __shared__ uint64_t wsum[NTT_THREADS / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  uint64_t acc = 0;
  for (uint32_t i = tid; i < nparts; i += NTT_THREADS) acc = gl_add(acc, partial[i]);
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) acc = gl_add(acc, __shfl_xor(acc, o, 64));
  if (lane == 0) wsum[wave] = acc;
  __syncthreads();
  uint64_t S = wsum[0];
#pragma unroll
  for (int w = 1; w < NTT_THREADS / 64; w++) S = gl_add(S, wsum[w]);
  const uint64_t fz = gl_mul(K1, S), cp = gl_mul(fz, K2), kappa = gl_mul(K3, S);
  const uint64_t g0 = (uint64_t)blockIdx.x * NTT_THREADS + tid, gs = (uint64_t)gridDim.x * NTT_THREADS;
  for (uint64_t t = g0; t < 4096; t += gs) rlo[t] = gl_pow_dev(r, t);
  if (gk) {
    for (uint64_t t = g0; t < nhk; t += gs) rhu[t] = gl_pow_dev(r4096, t);
    if (g0 < 8) gk[g0] = gl_sub(gl_mul(cp, ch->G[g0]), kappa);
    return;
  }
  for (uint64_t t = g0; t < nhi; t += gs) rhi[t] = gl_mul(cp, gl_pow_dev(r4096, t));
  for (uint64_t t = g0; t < nhk; t += gs) rhk[t] = gl_mul(kappa, gl_pow_dev(r4096, t));
}

uint64_t dq_rows_per_part(uint64_t nrows) {
  // 8 rows per lane (the composition values of the lane stay in registers:
  // 16 took 158 VGPRs); 4 when that leaves fewer than 512 workgroups (a
  // sharded rank's block: its batch inversions then run twice as parallel)
  return (uint64_t)NTT_THREADS * (nrows >= 512ull * NTT_THREADS * 8 ? 8 : 4);
}

hipError_t launch_inv_base(hipStream_t st, const ComposeTerms& Tm, uint64_t* D, uint64_t* partial, int logn,
                           const DevChal* ch, const NttTables& T, uint64_t row0, uint64_t nrows, uint64_t per) {
  if (logn < 4 || (per != 8 * NTT_THREADS && per != 4 * NTT_THREADS) || nrows % 16 || row0 % per ||
      row0 + nrows > (1ULL << logn))
    return hipErrorInvalidValue;
  const dim3 grid((unsigned)((nrows + per - 1) / per));
  if (per == 8 * NTT_THREADS)
    hipLaunchKernelGGL(k_inv_base<8>, grid, dim3(NTT_THREADS), 0, st, Tm, D, partial + row0 / per, logn, ch, T, row0,
                       nrows);
  else
    hipLaunchKernelGGL(k_inv_base<4>, grid, dim3(NTT_THREADS), 0, st, Tm, D, partial + row0 / per, logn, ch, T, row0,
                       nrows);
  return hipGetLastError();
}

hipError_t launch_q_tables(hipStream_t st, const uint64_t* partial, int logn, int logN, const DevChal* ch,
                           uint64_t* rlo, uint64_t* rhi, uint64_t* rhk, uint64_t* rhu, uint64_t* gk, bool closed,
                           uint64_t per) {
  if (logn < 4 || logN < logn || logN > 32 || !per || (closed && (!rhu || !gk))) return hipErrorInvalidValue;
  const uint64_t n = 1ULL << logn;
  const uint32_t nparts = (uint32_t)((n + per - 1) / per);
  const uint32_t nhi = logN > 12 ? (1u << (logN - 12)) : 1u;
  const uint32_t nhk = logn > 12 ? (1u << (logn - 12)) : 1u;
  const uint64_t work = std::max<uint64_t>(4096, closed ? nhk : nhi);
  const unsigned grid = (unsigned)std::min<uint64_t>(1024, (work + NTT_THREADS - 1) / NTT_THREADS);
  hipLaunchKernelGGL(k_q_tables, dim3(grid), dim3(NTT_THREADS), 0, st, partial, nparts, ch, rlo, rhi, nhi, rhk, nhk,
                     closed ? rhu : nullptr, closed ? gk : nullptr);
  return hipGetLastError();
}
}  // namespace sezkp
