// ntt_pass.hip — Goldilocks NTT passes for CDNA4 (gfx950).
//
// Mathematically the reference's transforms (crates/sezkp-ffts/src/ntt.rs:79-155):
// forward y_k = sum_j a_j w_N^{jk}, inverse = (1/n) sum_k y_k w_N^{-jk}, with
// w_{2^s} = 7^((p-1)>>s) (lib.rs:237-242). Field arithmetic is exact, so any
// factorisation produces the reference's bits.
//
// Structure: a transform of 2^logN points is a sequence of LDS passes. A pass
// owns m consecutive radix-2 stages whose smallest half-size is L = 2^sL; it
// treats every group {base + low + t*L : t < 2^m} (low < L) as one 2^m-point
// sub-transform done in LDS with internal twiddles w_{2^m}, plus ONE element-
// wise twiddle w_{2^m L}^{low * bitrev_m(t)} (post-multiply for DIF, pre-
// multiply for DIT; the four-step identity). Tiles are C <= 16 groups with
// consecutive `low` (128-B row segments) or, when L < C, one contiguous run.
//   DIF: natural -> bit-reversed order.   DIT: bit-reversed -> natural order.
// Which kernel takes which pass is ntt_plan.h's decision; launch_pass256 at
// the end maps a planned pass to its instantiation.
#include <map>
#include <mutex>
#include <tuple>

#include "gl_pow2.h"
#include "ntt_dev.h"
#include "ntt_plan.h"

namespace sezkp {

__device__ __forceinline__ uint64_t pow3(const NttTables& T, uint64_t e) {
  return gl_mul(T.p3_hi[e >> T.S], T.p3_lo[e & ((1ULL << T.S) - 1)]);
}
// tw_pow(T, i << T.S, inverse) without its product: the exponent's low part is
// zero and lo[0] = 1, so the factor is one entry of the hi table (the inverse
// mirrors the index as tw_pow mirrors the exponent)
__device__ __forceinline__ uint64_t tw_hi(const NttTables& T, uint64_t i, bool inverse) {
  const uint64_t mask = (1ULL << (T.K - T.S)) - 1;
  return T.hi[(inverse ? 0 - i : i) & mask];
}

// slot of coefficient e (= bitrev of the load position k) in the replicated
// source: k itself after one n-point DIF INTT, or the sharded INTT's
// allgathered layout (NttPassArgs::src_logP)
__device__ __forceinline__ uint64_t src_slot(const NttPassArgs& P, uint64_t k, uint32_t e) {
  if (!P.src_logP) return k;
  const int lm = P.log_src - P.src_logP;
  const uint64_t hi = (uint64_t)e >> P.src_logP;
  return ((uint64_t)(e & ((1u << P.src_logP) - 1)) << lm) | (lm ? (__brev((uint32_t)hi) >> (32 - lm)) : 0);
}

// DEEP-quotient coefficient at bit-reversed position p of the N-point DIT
// input: e = bitrev(p); the q part only where p's low b = log(N/n) bits are 0
__device__ __forceinline__ uint64_t dp_load(const NttPassArgs& P, const NttTables& T, uint64_t p, int b) {
  const uint64_t e = (uint64_t)(__brev((uint32_t)p) >> (32 - P.dp_logN));
  uint64_t v = gl_mul(P.dp_rhi[e >> 12], P.dp_rlo[e & 4095]);
  if ((p & ((1ULL << b) - 1)) == 0) {
    const uint64_t k = p >> b;
    const uint32_t rk = P.log_src ? (__brev((uint32_t)k) >> (32 - P.log_src)) : 0;  // = e
    uint64_t qv = gl_mul(gl_mul(P.src[src_slot(P, k, rk)], P.inv_n), pow3(T, rk));
    if (P.coset_e) qv = gl_mul(qv, tw_pow(T, ((uint64_t)rk * P.coset_e) & ((1ULL << T.K) - 1), false));  // (w_N^g)^e
    // q_e = d_e - f(z) z^(n-1-e) / (1 - z^n): minus kappa r^e (DeepPoly)
    v = gl_sub(gl_add(v, qv), gl_mul(P.dp_rhk[e >> 12], P.dp_rlo[e & 4095]));
  }
  return v;
}
// The same coefficients after the first B DIT stages, in closed form
// (DeepPoly): the F1 points from p0 (a multiple of F1) are F1 >> B groups;
// group g = p >> B holds qv_g + r^e0 gk[s] in slot s, e0 = bitrev(g). One
// bit reversal, one r^e0 and one qv per group; one product and one sum per
// point. The caller goes on with fft_dit_regs<M1, INV, B>.
template <int F1, int B>
__device__ __forceinline__ void dp_load_closed(const NttPassArgs& P, const NttTables& T, uint64_t p0,
                                               uint64_t (&x)[F1]) {
  static_assert((1 << B) <= F1 && B >= 1 && B <= 3, "a group lies inside one thread's points");
  uint64_t gk[1 << B];
#pragma unroll
  for (int s = 0; s < (1 << B); s++) gk[s] = P.dp_gk[s];
#pragma unroll
  for (int r = 0; r < F1; r += (1 << B)) {
    const uint64_t k = (p0 + r) >> B;
    const uint32_t e0 = P.log_src ? (__brev((uint32_t)k) >> (32 - P.log_src)) : 0;
    uint64_t qv = gl_mul(gl_mul(P.src[src_slot(P, k, e0)], P.inv_n), pow3(T, e0));
    if (P.coset_e) qv = gl_mul(qv, tw_pow(T, ((uint64_t)e0 * P.coset_e) & ((1ULL << T.K) - 1), false));  // (w_N^g)^e
    const uint64_t re = gl_mul(P.dp_rhu[e0 >> 12], P.dp_rlo[e0 & 4095]);
#pragma unroll
    for (int s = 0; s < (1 << B); s++) x[r + s] = gl_add(qv, gl_mul(re, gk[s]));
  }
}

template <bool DIF>
__global__ void __launch_bounds__(NTT_THREADS) k_ntt_pass(NttPassArgs P) {
  __shared__ uint64_t sh[(1 << NTT_MMAX) * NTT_PADC];
  __shared__ uint64_t W[(1 << NTT_MMAX) / 2];
  const int m = P.m, R = 1 << m, sL = P.sL;
  const uint64_t L = 1ULL << sL;
  const int logC = P.logC, C = 1 << logC;
  const int tid = threadIdx.x;
  const uint64_t tile = blockIdx.x;
  const NttTables& T = P.tw;

  for (int x = tid; x < R / 2; x += NTT_THREADS) W[x] = tw_pow(T, (uint64_t)x << (T.K - m), P.inverse);

  const int nel = R << logC;
  const bool wide = L >= (uint64_t)C;  // tile = C consecutive `low` columns
  uint64_t blk_base = 0, low0 = 0;
  if (wide) {
    uint64_t tiles_per_blk = L >> logC;
    blk_base = (tile / tiles_per_blk) * ((uint64_t)R << sL);
    low0 = (tile % tiles_per_blk) << logC;
  }
  const int tw_shift = T.K - m - sL;  // exponent scale into w_{2^K}
  // ---- load (+ DIT pre-twiddle)
  for (int q = tid; q < nel; q += NTT_THREADS) {
    int t, c;
    uint64_t low, pos;
    if (wide) {
      t = q >> logC; c = q & (C - 1); low = low0 + c;
      pos = blk_base + low + ((uint64_t)t << sL);
    } else {
      low = q & (L - 1);
      t = (q >> sL) & (R - 1);
      c = ((q >> (sL + m)) << sL) | (int)low;
      pos = tile * (uint64_t)nel + q;
    }
    uint64_t v;
    if (P.dp_rlo) {
      v = dp_load(P, T, pos, P.dp_logN - P.log_src);
    } else if (P.src) {  // LDE replicated load: B[2^skip k + s] = A[k] * n^-1 * (3 w^g)^bitrev(k)
      uint64_t k = pos >> P.skip;
      uint32_t rk = P.log_src ? (__brev((uint32_t)k) >> (32 - P.log_src)) : 0;
      v = gl_mul(gl_mul(P.src[src_slot(P, k, rk)], P.inv_n), pow3(T, rk));
      if (P.coset_e) v = gl_mul(v, tw_pow(T, ((uint64_t)rk * P.coset_e) & ((1ULL << T.K) - 1), false));
    } else {
      v = P.a[pos];
    }
    if (!DIF && low != 0) {
      uint32_t bt = __brev((uint32_t)t) >> (32 - m);
      v = gl_mul(v, tw_pow(T, (low * bt) << tw_shift, P.inverse));
    }
    sh[t * NTT_PADC + c] = v;
  }
  __syncthreads();
  // ---- internal radix-2 stages over t
  const int nbf = (R / 2) << logC;
  for (int it = 0; it < m - P.skip; it++) {
    const int s = DIF ? (m - 1 - it) : (it + P.skip);
    const int h = 1 << s;
    for (int b = tid; b < nbf; b += NTT_THREADS) {
      const int c = b & (C - 1), u = b >> logC;
      const int j = u & (h - 1);
      const int t0 = ((u >> s) << (s + 1)) | j, t1 = t0 + h;
      const uint64_t w = W[j << (m - 1 - s)];
      uint64_t x = sh[t0 * NTT_PADC + c], y = sh[t1 * NTT_PADC + c];
      if (DIF) {
        sh[t0 * NTT_PADC + c] = gl_add(x, y);
        sh[t1 * NTT_PADC + c] = gl_mul(gl_sub(x, y), w);
      } else {
        y = gl_mul(y, w);
        sh[t0 * NTT_PADC + c] = gl_add(x, y);
        sh[t1 * NTT_PADC + c] = gl_sub(x, y);
      }
    }
    __syncthreads();
  }
  // ---- (DIF post-twiddle +) store
  for (int q = tid; q < nel; q += NTT_THREADS) {
    int t, c;
    uint64_t low, pos;
    if (wide) {
      t = q >> logC; c = q & (C - 1); low = low0 + c;
      pos = blk_base + low + ((uint64_t)t << sL);
    } else {
      low = q & (L - 1);
      t = (q >> sL) & (R - 1);
      c = ((q >> (sL + m)) << sL) | (int)low;
      pos = tile * (uint64_t)nel + q;
    }
    uint64_t v = sh[t * NTT_PADC + c];
    if (DIF && low != 0) {
      uint32_t bt = __brev((uint32_t)t) >> (32 - m);
      v = gl_mul(v, tw_pow(T, (low * bt) << tw_shift, P.inverse));
    }
    P.a[pos] = v;
  }
}

// ------------------------------------------------ four-step register passes
// A pass of m = M1 + M2 stages as ONE exchange through LDS instead of m
// LDS round trips: two register-resident radix-2^M FFTs (<= 16 points) whose
// internal twiddles are powers of w_16 = 2^156 (w_16^-1 = 2^36), i.e. shifts
// plus one 128->64 reduction instead of general products, and one general
// twiddle w_{2^m}^(j1*k2) between them (LDS table). Same tile geometry and
// per-pass twiddle as k_ntt_pass; the two kernels are interchangeable per pass.
//   DIT (bit-reversed in, natural out): position F1*u + r holds a[j1 + F2*j2],
//     j1 = rev_M2(u), j2 = rev_M1(r). Step 1 (thread per u): F1-point DIT over
//     j2 -> Y[j1][k2]; * w^(j1 k2); step 2 (thread per k2): F2-point DIT over
//     j1 (slot u holds j1 = rev(u)) -> X[k2 + F1*k1].
//   DIF (natural in, bit-reversed out): step 1 (thread per r): F2-point DIF
//     over x[F1*u + r] -> slot q holds k_lo = rev_M2(q); * w^(r k_lo);
//     step 2 (thread per q): F1-point DIF over r -> X[k_lo + F2*k_hi] lands at
//     position q*F1 + q' (k_hi = rev_M1(q')).

// Fused DEEP (last forward DIT pass of the LDE only): out_i = y_i / (x_i - z),
// x_i = 3 w_N^(g + P i) (deep_div.hip k_deep, lde.rs:76-93). A thread's F2
// outputs sit F1 << sL apart, so consecutive x differ by w_F2 (a power of
// two: a shift); one Montgomery batch inversion per workgroup (4096 points).
template <int F, class Emit>
__device__ __forceinline__ void deep_tile(uint64_t x, uint64_t z, Emit emit) {
  __shared__ uint64_t wtot[NTT_THREADS / 64];
  __shared__ uint64_t s_inv;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  uint64_t d[F], a[F];
  uint64_t Pp = 1;
#pragma unroll
  for (int j = 0; j < F; j++) {
    d[j] = gl_sub(x, z);
    Pp = j ? gl_mul(Pp, d[j]) : d[j];
    a[j] = Pp;
    if (j + 1 < F) x = tw_small<false>(x, 1, F / 2);  // * w_F
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
  uint64_t inv_run = gl_mul(gl_mul(invW, Q), Sprev);  // 1 / (this thread's product)
#pragma unroll
  for (int j = F - 1; j >= 0; j--) {
    emit(j, j ? gl_mul(inv_run, a[j - 1]) : inv_run);  // 1 / d_j
    if (j) inv_run = gl_mul(inv_run, d[j]);
  }
}

// NARROW (sL = 0, the first DIT / last DIF pass): a tile is 16 contiguous
// sub-transforms of R elements, so a thread's R points are consecutive and
// the lanes of one load or store instruction are R elements apart (64 cache
// lines per wave instruction). Those passes move the tile between HBM and the
// LDS image with lane-consecutive addresses (element e = j * 256 + tid of the
// tile: row e mod R, column e / R) and the register FFTs read / write the LDS.
template <int R>
__device__ __forceinline__ void narrow_to_lds(uint64_t* sh, const uint64_t* __restrict__ a, uint64_t tile) {
  constexpr int m = __builtin_ctz(R);
  const uint64_t* src = a + tile * (uint64_t)(NTT_CMAX * R);
#pragma unroll
  for (int j = 0; j < NTT_CMAX * R / NTT_THREADS; j++) {
    const int e = j * NTT_THREADS + threadIdx.x;
    sh[(e & (R - 1)) * NTT_PADC + (e >> m)] = src[e];
  }
}
template <int R>
__device__ __forceinline__ void lds_to_narrow(const uint64_t* sh, uint64_t* __restrict__ a, uint64_t tile) {
  constexpr int m = __builtin_ctz(R);
  uint64_t* dst = a + tile * (uint64_t)(NTT_CMAX * R);
#pragma unroll
  for (int j = 0; j < NTT_CMAX * R / NTT_THREADS; j++) {
    const int e = j * NTT_THREADS + threadIdx.x;
    dst[e] = sh[(e & (R - 1)) * NTT_PADC + (e >> m)];
  }
}

// nat_out: the tile's point p = tile * 16R + e holds frequency bitrev(p); it
// goes straight to out[bitrev(p)] (one word per 128-B line per tile; the 16
// tiles sharing those lines run back to back on one XCD, see nat_tile, so the
// partial lines merge in its L2 before they are written back)
template <int R>
__device__ __forceinline__ void lds_to_natural(const uint64_t* sh, const NttPassArgs& P, uint64_t tile) {
  constexpr int m = __builtin_ctz(R);
  const uint64_t p0 = tile * (uint64_t)(NTT_CMAX * R);
  const int sh_r = 32 - P.nat_logN;
#pragma unroll
  for (int j = 0; j < NTT_CMAX * R / NTT_THREADS; j++) {
    const int e = j * NTT_THREADS + threadIdx.x;
    uint64_t v = sh[(e & (R - 1)) * NTT_PADC + (e >> m)];
    if (P.out_scale != 1) v = gl_mul(v, P.out_scale);
    P.out[__brev((uint32_t)(p0 + e)) >> sh_r] = v;
  }
}
// nat_tr (the last, narrow DIF pass of a natural-order transform, 2^m-point
// sub-transforms, m <= 8): after the earlier passes block B (2^m contiguous
// points) holds the sub-transforms whose outputs land at
// X[k 2^(N-m) + bitrev_{N-m}(B)], k = bitrev_m(row). Tile T takes the 16
// blocks B_i = bitrev_{N-m}(16 T + i), i < 16, so for every k its 16 outputs
// are one contiguous 128-B segment: whole-segment loads (each block is 2^m
// contiguous points) and whole-segment stores, no bit-reversal pass.
template <int R>
__device__ __forceinline__ void gather_to_lds(uint64_t* sh, const uint64_t* __restrict__ a, uint64_t tile, int logN) {
  constexpr int m = __builtin_ctz(R);
  const int sb = 32 - (logN - m);
#pragma unroll
  for (int j = 0; j < NTT_CMAX * R / NTT_THREADS; j++) {
    const int e = j * NTT_THREADS + threadIdx.x, i = e >> m, row = e & (R - 1);
    const uint64_t B = __brev((uint32_t)(tile * NTT_CMAX + i)) >> sb;
    sh[row * NTT_PADC + i] = a[(B << m) + row];
  }
}
template <int R>
__device__ __forceinline__ void lds_to_transposed(const uint64_t* sh, const NttPassArgs& P, uint64_t tile) {
  constexpr int m = __builtin_ctz(R);
  const int lo = P.nat_logN - m;
#pragma unroll
  for (int j = 0; j < NTT_CMAX * R / NTT_THREADS; j++) {
    // lanes walk consecutive LDS rows (conflict-free reads; consecutive k =
    // rows R/4 apart put a wave's four k on the same banks); each k's 16
    // outputs stay one 128-B segment
    const int e = j * NTT_THREADS + threadIdx.x, i = e & (NTT_CMAX - 1), row = e >> 4;
    const uint64_t k = __brev((uint32_t)row) >> (32 - m);
    uint64_t v = sh[row * NTT_PADC + i];
    if (P.out_scale != 1) v = gl_mul(v, P.out_scale);
    P.out[(k << lo) + tile * NTT_CMAX + i] = v;
  }
}

// nat_tr on the DIT side (the first, narrow pass of a natural-order DIT
// transform, m <= 8): slot p of the DIT input holds x[bitrev_N(p)]. Tile T
// takes the 16 blocks B_i = bitrev_{N-m}(16 T + i): for every in-block slot e
// their inputs x[bitrev_m(e) 2^(N-m) + 16 T + i] are one contiguous 128-B
// segment; the blocks go back to their own slots (2^m contiguous points
// each). (An X16 tile, one 2^(m+4)-point sub-transform, would read single
// points 2^(N-m-4) apart and rely on L2 sharing between 16 tiles: measured
// 2^25 1267 vs 1053 us and 2^26 2493 vs 2109 us per round trip against the DIF
// transposed store, so it is not built.)
template <int R>
__device__ __forceinline__ void gather_dit_to_lds(uint64_t* sh, const uint64_t* __restrict__ x, uint64_t tile,
                                                  int logN) {
  constexpr int m = __builtin_ctz(R);
#pragma unroll
  for (int j = 0; j < NTT_CMAX * R / NTT_THREADS; j++) {
    const int e = j * NTT_THREADS + threadIdx.x, i = e & (NTT_CMAX - 1), row = e >> 4;
    sh[row * NTT_PADC + i] = x[((uint64_t)(__brev((uint32_t)row) >> (32 - m)) << (logN - m)) + tile * NTT_CMAX + i];
  }
}
template <int R>
__device__ __forceinline__ void lds_to_blocks(const uint64_t* sh, uint64_t* __restrict__ a, uint64_t tile, int logN) {
  constexpr int m = __builtin_ctz(R);
  const int sb = 32 - (logN - m);
#pragma unroll
  for (int j = 0; j < NTT_CMAX * R / NTT_THREADS; j++) {
    const int e = j * NTT_THREADS + threadIdx.x, i = e >> m, row = e & (R - 1);
    const uint64_t B = __brev((uint32_t)(tile * NTT_CMAX + i)) >> sb;
    a[(B << m) + row] = sh[row * NTT_PADC + i];
  }
}

// X16 (a NARROW pass extended by one radix-16 step inside its tile): a
// NARROW tile is 16 * R contiguous points, so it also holds every 16-point
// sub-transform {row + R t : t < 16} of the neighbouring pass with sL = log R.
// One thread per row runs it on the LDS image (element (row, t) at
// sh[row * NTT_PADC + t]) with the pass twiddle w_{16R}^(row * rev4(t)),
// pre-multiplied for DIT (after the R-point stages), post-multiplied for DIF
// (before them). A 2^12 tile then does 12 stages with one HBM round trip.
template <int R, bool DIF, bool INV>
__device__ __forceinline__ void tile_radix16(uint64_t* sh, const NttTables& T) {
  constexpr int m = __builtin_ctz(R);
  const int row = threadIdx.x;
  if (row >= R) return;
  uint64_t x[16];
#pragma unroll
  for (int t = 0; t < 16; t++) x[t] = sh[row * NTT_PADC + t];
  if constexpr (DIF) fft_dif_regs<4, INV>(x);
  if (row) {  // x[rev4(q)] *= w^(row q), the chain applied as it goes
    const uint64_t s1 = tw_pow(T, (uint64_t)row << (T.K - m - 4), INV);
    uint64_t t = s1;
#pragma unroll
    for (int q = 1; q < 16; q++) {
      x[rev<4>(q)] = gl_mul(x[rev<4>(q)], t);
      if (q + 1 < 16) t = gl_mul(t, s1);
    }
  }
  if constexpr (!DIF) fft_dit_regs<4, INV, 0>(x);
#pragma unroll
  for (int t = 0; t < 16; t++) sh[row * NTT_PADC + t] = x[t];
}

template <bool DIF, bool INV, int M1, int M2, int SKIP, bool DEEP = false, bool NARROW = false,
          bool X16 = false>
__global__ void __launch_bounds__(NTT_THREADS, 4) k_ntt4(NttPassArgs P) {
  constexpr int F1 = 1 << M1, F2 = 1 << M2, m = M1 + M2, R = 1 << m;
  static_assert(!(NARROW && DEEP), "the fused DEEP pass is a wide pass");
  static_assert(!X16 || (NARROW && SKIP == 0), "the in-tile radix-16 step extends a plain NARROW pass");
  __shared__ uint64_t sh[R * NTT_PADC];
  __shared__ uint64_t W[R];
  const int tid = threadIdx.x;
  const NttTables& T = P.tw;
  // x << (K - m) has no low part (m <= K - S): with the tables on, a load
  for (int x = tid; x < R; x += NTT_THREADS)
    W[x] = P.tw_tab ? tw_hi(T, (uint64_t)x << (T.K - T.S - m), INV) : tw_pow(T, (uint64_t)x << (T.K - m), INV);
  Tile G;
  G.sL = P.sL;
  G.m = m;
  G.tile = (NARROW && P.nat_out) ? nat_tile(blockIdx.x, gridDim.x) : blockIdx.x;
  G.wide = (1ULL << G.sL) >= (uint64_t)NTT_CMAX;
  G.blk_base = 0;
  G.low0 = 0;
  if (G.wide) {
    const uint64_t tiles_per_blk = (1ULL << G.sL) / NTT_CMAX;
    G.blk_base = (G.tile / tiles_per_blk) * ((uint64_t)R << G.sL);
    G.low0 = (G.tile % tiles_per_blk) * NTT_CMAX;
  }
  const int tw_shift = T.K - m - G.sL;
  // pass twiddle w_{2^(m + sL)}^(low j) of a wide pass with m + sL <= K - S:
  // one load per element from the pass's own table (pass_twiddles), row j,
  // column low, so the 16 lanes of a tile row read one 128-B segment as they
  // do for the data: no chain, no tw_pow
  const bool pass_tab = !NARROW && P.tw_pass != nullptr;
  const int c = tid & (NTT_CMAX - 1), g = tid / NTT_CMAX;
  // a plain NARROW load stages the tile through the LDS image first
  const bool staged_load = NARROW && !P.dp_rlo && !P.src;
  if constexpr (NARROW && DIF && !X16) {
    if (P.nat_tr) gather_to_lds<R>(sh, P.a, G.tile, P.nat_logN);
    else if (staged_load) narrow_to_lds<R>(sh, P.a, G.tile);
  } else if constexpr (NARROW && !DIF && SKIP == 0 && !X16) {
    if (staged_load && P.nat_tr) gather_dit_to_lds<R>(sh, P.a, G.tile, P.nat_logN);
    else if (staged_load) narrow_to_lds<R>(sh, P.a, G.tile);
  } else if (staged_load) {
    narrow_to_lds<R>(sh, P.a, G.tile);
  }
  __syncthreads();
  if constexpr (X16 && DIF) {  // the previous DIF pass's 4 stages, in the tile
    tile_radix16<R, true, INV>(sh, T);
    __syncthreads();
  }
  if constexpr (!DIF) {
    uint64_t x[F1];
    if (g < F2) {  // step 1: thread (c, u), registers r
      const int u = g;
      uint64_t low = 0;
      bool closed = false;  // the load came with its first b stages done (dp_load_closed)
      if (P.dp_rlo) {  // DEEP-quotient LDE load (first pass, sL = 0, low = 0, SKIP = 0)
        const uint64_t p0 = tile_pos(G, F1 * u, c, low);
        const int b = P.dp_logN - P.log_src;
        if constexpr (NARROW && SKIP == 0 && !X16 && !INV) {
          if (P.dp_gk) {  // b in 1..3 (ntt_pass_dp_closed): a kernel argument, so wave-uniform
            closed = true;
            if (b == 3) {
              dp_load_closed<F1, 3>(P, T, p0, x);
              fft_dit_regs<M1, INV, 3>(x);
            } else if (b == 2) {
              dp_load_closed<F1, 2>(P, T, p0, x);
              fft_dit_regs<M1, INV, 2>(x);
            } else {
              dp_load_closed<F1, 1>(P, T, p0, x);
              fft_dit_regs<M1, INV, 1>(x);
            }
          }
        }
        if (!closed) {
#pragma unroll
          for (int r = 0; r < F1; r++) x[r] = dp_load(P, T, p0 + r, b);
        }
      } else if (P.src) {  // LDE replicated load (first pass, sL = 0, low = 0)
        const uint64_t p0 = tile_pos(G, F1 * u, c, low);
#pragma unroll
        for (int r = 0; r < F1; r += (1 << SKIP)) {
          const uint64_t k = (p0 + r) >> P.skip;
          const uint32_t rk = P.log_src ? (__brev((uint32_t)k) >> (32 - P.log_src)) : 0;
          uint64_t v = gl_mul(gl_mul(P.src[src_slot(P, k, rk)], P.inv_n), pow3(T, rk));
          if (P.coset_e) v = gl_mul(v, tw_pow(T, ((uint64_t)rk * P.coset_e) & ((1ULL << T.K) - 1), false));
#pragma unroll
          for (int s = 0; s < (1 << SKIP); s++) x[r + s] = v;
        }
      } else if (NARROW) {
#pragma unroll
        for (int r = 0; r < F1; r++) x[r] = sh[(F1 * u + r) * NTT_PADC + c];
      } else {
#pragma unroll
        for (int r = 0; r < F1; r++) x[r] = P.a[tile_pos(G, F1 * u + r, c, low)];
        // out_scale > 1 (the last pass of an inverse natural-order transform):
        // n^-1 rides on the pre-twiddle chain (one product per thread), the
        // rare low = 0 column is scaled point by point
        const bool scale = P.out_scale > 1;
        if (scale && low == 0) {
#pragma unroll
          for (int r = 0; r < F1; r++) x[r] = gl_mul(x[r], P.out_scale);
        }
        if (low != 0 && pass_tab) {  // pre-twiddle w^(low * (j1 + F2 j2)), j2 = rev(r), from the table
          const int j1 = rev<M2>(u);
#pragma unroll
          for (int q = 0; q < F1; q++) {
            uint64_t f = P.tw_pass[((uint64_t)(j1 + F2 * q) << G.sL) + low];
            if (scale) f = gl_mul(f, P.out_scale);
            x[rev<M1>(q)] = gl_mul(x[rev<M1>(q)], f);
          }
        } else if (low != 0) {  // the same factors as a chain
          const int j1 = rev<M2>(u);
          uint64_t t = tw_pow(T, (low * (uint64_t)j1) << tw_shift, INV);
          if (scale) t = gl_mul(t, P.out_scale);
          const uint64_t s1 = tw_pow(T, (low * (uint64_t)F2) << tw_shift, INV);
#pragma unroll
          for (int q = 0; q < F1; q++) {  // x[rev(q)] *= t s1^q, the chain applied as it goes
            x[rev<M1>(q)] = gl_mul(x[rev<M1>(q)], t);
            if (q + 1 < F1) t = gl_mul(t, s1);
          }
        }
      }
      if (!closed) fft_dit_regs<M1, INV, SKIP>(x);
    }
    if (staged_load) __syncthreads();  // every thread has read its points from the image
    if (g < F2) {
      const int u = g, j1 = rev<M2>(u);
#pragma unroll
      for (int k2 = 0; k2 < F1; k2++) {
        const uint64_t v = k2 && j1 ? gl_mul(x[k2], W[j1 * k2]) : x[k2];
        sh[(u * F1 + k2) * NTT_PADC + c] = v;
      }
    }
    __syncthreads();
    uint64_t y[F2];
    if (g < F1) {  // step 2: thread (c, k2), registers u
      const int k2 = g;
#pragma unroll
      for (int u = 0; u < F2; u++) y[u] = sh[(u * F1 + k2) * NTT_PADC + c];
      fft_dit_regs<M2, INV, 0>(y);
      uint64_t low;
      if constexpr (DEEP) {
        static_assert(F1 * NTT_CMAX == NTT_THREADS && !INV && !DIF, "fused DEEP needs every thread in step 2");
        // park y in this thread's own LDS slots (read above) to free registers
#pragma unroll
        for (int k1 = 0; k1 < F2; k1++) sh[(k1 * F1 + k2) * NTT_PADC + c] = y[k1];
        const uint64_t pos0 = tile_pos(G, k2, c, low);
        const uint64_t e = ((uint64_t)P.deep_g + (pos0 << P.deep_logP)) << (T.K - P.deep_logN);
        const uint64_t x0 = gl_mul(gl_mul(T.hi[e >> T.S], T.lo[e & ((1ULL << T.S) - 1)]), 3);
        deep_tile<F2>(x0, P.deep_z, [&](int k1, uint64_t inv) {
          P.a[tile_pos(G, k2 + F1 * k1, c, low)] = gl_mul(sh[(k1 * F1 + k2) * NTT_PADC + c], inv);
        });
      } else if (!NARROW) {
        uint64_t* dst = P.out ? P.out : P.a;
#pragma unroll
        for (int k1 = 0; k1 < F2; k1++) dst[tile_pos(G, k2 + F1 * k1, c, low)] = y[k1];
      }
    }
    if constexpr (NARROW) {  // rows k2 + F1 k1 back through the image, lane-consecutive stores
      __syncthreads();
      if (g < F1) {
#pragma unroll
        for (int k1 = 0; k1 < F2; k1++) sh[(g + F1 * k1) * NTT_PADC + c] = y[k1];
      }
      __syncthreads();
      if constexpr (X16) {  // the next DIT pass's 4 stages, in the tile
        tile_radix16<R, false, INV>(sh, T);
        __syncthreads();
      }
      if (!X16 && P.nat_tr) lds_to_blocks<R>(sh, P.out ? P.out : P.a, G.tile, P.nat_logN);
      else lds_to_narrow<R>(sh, P.out ? P.out : P.a, G.tile);
    }
  } else {
    uint64_t x[F2];
    if (g < F1) {  // step 1: thread (c, r), registers u (natural)
      const int r = g;
      uint64_t low;
#pragma unroll
      for (int u = 0; u < F2; u++)
        x[u] = NARROW ? sh[(F1 * u + r) * NTT_PADC + c] : P.a[tile_pos(G, F1 * u + r, c, low)];
      fft_dif_regs<M2, INV>(x);
    }
    if (NARROW) __syncthreads();
    if (g < F1) {
      const int r = g;
#pragma unroll
      for (int q = 0; q < F2; q++) {
        const int klo = rev<M2>(q);
        const uint64_t v = klo && r ? gl_mul(x[q], W[r * klo]) : x[q];
        sh[(q * F1 + r) * NTT_PADC + c] = v;
      }
    }
    __syncthreads();
    uint64_t y[F1];
    if (g < F2) {  // step 2: thread (c, q), registers r
      const int q = g;
#pragma unroll
      for (int r = 0; r < F1; r++) y[r] = sh[(q * F1 + r) * NTT_PADC + c];
      fft_dif_regs<M1, INV>(y);
      uint64_t low;
      (void)tile_pos(G, q * F1, c, low);
      if (low != 0 && pass_tab) {  // post-twiddle w^(low * (k_lo + F2 k_hi)), k_hi = rev(q'), from the table
        const int klo = rev<M2>(q);
#pragma unroll
        for (int kh = 0; kh < F1; kh++)
          y[rev<M1>(kh)] = gl_mul(y[rev<M1>(kh)], P.tw_pass[((uint64_t)(klo + F2 * kh) << G.sL) + low]);
      } else if (low != 0) {  // the same factors as a chain
        uint64_t t = tw_pow(T, (low * (uint64_t)rev<M2>(q)) << tw_shift, INV);
        const uint64_t s1 = tw_pow(T, (low * (uint64_t)F2) << tw_shift, INV);
#pragma unroll
        for (int kh = 0; kh < F1; kh++) {
          y[rev<M1>(kh)] = gl_mul(y[rev<M1>(kh)], t);
          if (kh + 1 < F1) t = gl_mul(t, s1);
        }
      }
      if (!NARROW) {
        uint64_t* dst = P.out ? P.out : P.a;
#pragma unroll
        for (int qq = 0; qq < F1; qq++) dst[tile_pos(G, q * F1 + qq, c, low)] = y[qq];
      }
    }
    if constexpr (NARROW) {
      __syncthreads();
      if (g < F2) {
#pragma unroll
        for (int qq = 0; qq < F1; qq++) sh[(g * F1 + qq) * NTT_PADC + c] = y[qq];
      }
      __syncthreads();
      if (!X16 && P.nat_tr) lds_to_transposed<R>(sh, P, G.tile);
      else if (P.nat_out) lds_to_natural<R>(sh, P, G.tile);
      else lds_to_narrow<R>(sh, P.a, G.tile);
    }
  }
}

// The pass twiddles of a wide k_ntt4 pass as a table: entry (j << sL) + low =
// w_{2^(m + sL)}^(+-low j) for j < 2^m, low < 2^sL. While m + sL <= K - S the
// exponent (low j) << (K - m - sL) has no low part, so every entry is a copy
// of one hi entry (exact). Read straight from hi, the 16 lanes of a tile row
// would fetch 16 entries j apart (a cache line each: the m = 8, sL = 8 pass of
// a 2^24-point transform measured 94 against 89 us with the chain); in this
// order they read one 128-B segment, as for the data. At most 2^(K - S)
// entries (512 KB) per geometry, built on first use and kept for the
// process, per device; the few geometries a prover's sizes use stay in L2.
__global__ void __launch_bounds__(NTT_THREADS) k_pass_twiddles(NttTables T, uint64_t* __restrict__ tab, int sL, int m,
                                                               int inverse) {
  const uint64_t i = (uint64_t)blockIdx.x * NTT_THREADS + threadIdx.x;
  if (i >> (sL + m)) return;
  const uint64_t low = i & ((1ULL << sL) - 1), j = i >> sL;
  tab[i] = tw_hi(T, (low * j) << (T.K - T.S - m - sL), inverse != 0);
}
const uint64_t* pass_twiddles(hipStream_t st, const NttTables& T, int sL, int m, bool inverse) {
  static std::mutex mu;
  static std::map<std::tuple<int, const uint64_t*, int, int, int, int, bool>, uint64_t*> tabs;
  if (sL < 4 || m + sL > T.K - T.S) return nullptr;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return nullptr;
  std::lock_guard<std::mutex> lk(mu);
  const auto key = std::make_tuple(dev, T.hi, T.K, T.S, sL, m, inverse);
  auto it = tabs.find(key);
  if (it != tabs.end()) return it->second;
  // first use: built on the caller's stream and waited for, so that a launch
  // on any other stream finds it complete. A failure leaves the chain for
  // this launch (the error is peeked at, not cleared: an earlier one stays
  // for the caller's own check). The tables live as long as the process, as
  // the hi / lo tables they copy do.
  uint64_t* d = nullptr;
  const uint64_t cnt = 1ULL << (sL + m);
  if (hipMalloc((void**)&d, cnt * 8) != hipSuccess) return nullptr;
  hipLaunchKernelGGL(k_pass_twiddles, dim3((unsigned)((cnt + NTT_THREADS - 1) / NTT_THREADS)), dim3(NTT_THREADS), 0, st,
                     T, d, sL, m, inverse ? 1 : 0);
  if (hipPeekAtLastError() != hipSuccess || hipStreamSynchronize(st) != hipSuccess) {
    (void)hipFree(d);
    return nullptr;
  }
  tabs.emplace(key, d);
  return d;
}

// ---------------------------------------------------------------- launch
// A planned pass (ntt_plan.h) to its instantiation: direction, then the split
// of its stages, then the form. The plan has checked the pass's shape; false
// = a form that is not built (nothing launched).
template <bool DIF, bool INV, int M1, int M2, int SK>
static void launch_ntt4(hipStream_t st, const NttPass& p, const NttPassArgs& P) {
  if (p.form == NTT4_NARROW)
    hipLaunchKernelGGL((k_ntt4<DIF, INV, M1, M2, SK, false, true>), dim3(p.tiles), dim3(p.threads), 0, st, P);
  else
    hipLaunchKernelGGL((k_ntt4<DIF, INV, M1, M2, SK>), dim3(p.tiles), dim3(p.threads), 0, st, P);
}
template <bool DIF, bool INV, int M1, int M2>
static bool launch_form(hipStream_t st, const NttPass& p, const NttPassArgs& P) {
  switch (p.form) {
    case NTT4_X16:
      hipLaunchKernelGGL((k_ntt4<DIF, INV, M1, M2, 0, false, true, true>), dim3(p.tiles), dim3(p.threads), 0, st, P);
      return true;
    case NTT4_DEEP:
      if constexpr (!DIF && !INV && M1 == 4) {
        hipLaunchKernelGGL((k_ntt4<false, false, 4, M2, 0, true>), dim3(p.tiles), dim3(p.threads), 0, st, P);
        return true;
      }
      return false;
    case NTT4_WIDE:
    case NTT4_NARROW:
      if (p.SKIP == 0) {
        launch_ntt4<DIF, INV, M1, M2, 0>(st, p, P);
        return true;
      }
      if constexpr (!DIF) {  // the LDE's replicated load: its first 1..3 stages are trivial
        switch (p.SKIP) {
          case 1: launch_ntt4<false, INV, M1, M2, 1>(st, p, P); return true;
          case 2: launch_ntt4<false, INV, M1, M2, 2>(st, p, P); return true;
          case 3: launch_ntt4<false, INV, M1, M2, 3>(st, p, P); return true;
          default: break;
        }
      }
      return false;
    default:
      return false;
  }
}
template <bool DIF, bool INV>
static bool launch_split(hipStream_t st, const NttPass& p, const NttPassArgs& P) {
  switch (p.M1 * 8 + p.M2) {
    case 4 * 8 + 4: return launch_form<DIF, INV, 4, 4>(st, p, P);
    case 4 * 8 + 3: return launch_form<DIF, INV, 4, 3>(st, p, P);
    case 3 * 8 + 3: return launch_form<DIF, INV, 3, 3>(st, p, P);
    default: return false;
  }
}
bool launch_pass256(hipStream_t st, const NttPass& p, bool dif, bool inverse, const NttPassArgs& P) {
  if (p.form == NTT_GENERIC) {
    if (dif) hipLaunchKernelGGL(k_ntt_pass<true>, dim3(p.tiles), dim3(p.threads), 0, st, P);
    else hipLaunchKernelGGL(k_ntt_pass<false>, dim3(p.tiles), dim3(p.threads), 0, st, P);
    return true;
  }
  return dif ? (inverse ? launch_split<true, true>(st, p, P) : launch_split<true, false>(st, p, P))
             : (inverse ? launch_split<false, true>(st, p, P) : launch_split<false, false>(st, p, P));
}
}  // namespace sezkp
