// ntt_pass512.hip — the 512-lane DIF passes: the 9-stage wide pass of the
// 2^21 INTT and of the natural-order 2^25 / 2^26 transforms, and the two
// radix-8 passes of the natural-order 2^20 transform. Same tile geometry,
// pass twiddle and store as k_ntt4's DIF passes (ntt_pass.hip).
#include "gl_pow2.h"
#include "ntt_dev.h"
#include "ntt_plan.h"

namespace sezkp {

// Wide DIF pass of m = 9 stages for the natural-order transforms of 2^25 and
// 2^26 points: their last pass stays at 8 stages (the transposed store of
// nat_tr needs a 16-block tile), so the other 17 / 18 stages take passes of 9,
// keeping 3 passes. Tile = 16 columns x 512 rows (70 KB of LDS, 512 threads,
// two workgroups per CU: 16 waves, as four k_ntt4 workgroups). Four-step
// 512 = 32 x 16: step 1, thread (c, r) for r < 32, a 16-point DIF over u
// (x[32 u + r]), then * w_512^(r k_lo); step 2, thread (c, q) for q < 16, a
// 32-point DIF over r (w_32 = 2^78: shifts). Same row order, pass twiddle and
// out-of-place store as k_ntt4's wide DIF pass.
// LDS slot of (q, r, c): 16 u64 (32 banks) of padding after every q-block. A
// q-block is 32 rows = 64 * NTT_PADC dwords, so without it the four q of a
// step-2 wave hit the same 32 banks (a 2x serialised read).
template <int F1>
__device__ __forceinline__ int dif9_slot(int q, int r, int c) {
  return (q * F1 + r) * NTT_PADC + c + (q << 4);
}
template <bool INV>
__global__ void __launch_bounds__(512, 2) k_ntt_dif9(NttPassArgs P) {
  constexpr int M1 = 5, M2 = 4, F1 = 1 << M1, F2 = 1 << M2, m = M1 + M2, R = 1 << m, NT = 512;
  __shared__ uint64_t sh[R * NTT_PADC + 16 * (1 << M2)];
  __shared__ uint64_t W[R];
  const int tid = threadIdx.x;
  const NttTables& T = P.tw;
  for (int x = tid; x < R; x += NT) W[x] = tw_pow(T, (uint64_t)x << (T.K - m), INV);
  Tile G;
  G.sL = P.sL;
  G.m = m;
  G.tile = blockIdx.x;
  G.wide = true;
  const uint64_t tiles_per_blk = (1ULL << G.sL) / NTT_CMAX;
  G.blk_base = (G.tile / tiles_per_blk) * ((uint64_t)R << G.sL);
  G.low0 = (G.tile % tiles_per_blk) * NTT_CMAX;
  const int tw_shift = T.K - m - G.sL;
  const int c = tid & (NTT_CMAX - 1), g = tid / NTT_CMAX;  // g < F1
  uint64_t low;
  {  // step 1: thread (c, r), registers u
    const int r = g;
    uint64_t x[F2];
#pragma unroll
    for (int u = 0; u < F2; u++) x[u] = P.a[tile_pos(G, F1 * u + r, c, low)];
    fft_dif_regs<M2, INV>(x);
    __syncthreads();  // W
#pragma unroll
    for (int q = 0; q < F2; q++) {
      const int klo = rev<M2>(q);
      sh[dif9_slot<F1>(q, r, c)] = klo && r ? gl_mul(x[q], W[r * klo]) : x[q];
    }
  }
  __syncthreads();
  {  // step 2: the 32-point DIF over r of column q as two threads (c, q, h):
     // its first radix-2 stage (pairs r, r + 16; twiddle w_32^r, a shift) is
     // split by output half, h = 0 the sums, h = 1 the differences, then each
     // thread runs a 16-point DIF. Slot s of thread h is slot s + 16 h of
     // the 32-point output, i.e. k_hi = 2 rev4(s) + h. All 512 threads busy.
    const int q = g & (F2 - 1), h = g >> M2;
    uint64_t y[16];
#pragma unroll
    for (int r = 0; r < 16; r++) {
      const uint64_t a = sh[dif9_slot<F1>(q, r, c)], b = sh[dif9_slot<F1>(q, r + 16, c)];
      if (h == 0) {
        y[r] = gl_add(a, b);
      } else {
        const int e = r ? tw_exp<INV>(r, 16) : 0;
        const bool neg = e >= 96;
        y[r] = gl_mul2e(neg ? gl_sub(b, a) : gl_sub(a, b), neg ? e - 96 : e);
      }
    }
    fft_dif_regs<4, INV>(y);
    (void)tile_pos(G, q * F1, c, low);
    if (low != 0) {  // post-twiddle w^(low * (k_lo + F2 k_hi)), k_hi = 2 k' + h, slot rev4(k')
      uint64_t t = tw_pow(T, (low * ((uint64_t)rev<M2>(q) + (uint64_t)F2 * h)) << tw_shift, INV);
      const uint64_t s2 = tw_pow(T, (low * (uint64_t)(2 * F2)) << tw_shift, INV);
#pragma unroll
      for (int kp = 0; kp < 16; kp++) {
        y[rev<4>(kp)] = gl_mul(y[rev<4>(kp)], t);
        if (kp + 1 < 16) t = gl_mul(t, s2);
      }
    }
    uint64_t* dst = P.out ? P.out : P.a;
#pragma unroll
    for (int s = 0; s < 16; s++) dst[tile_pos(G, q * F1 + 16 * h + s, c, low)] = y[s];
  }
}

// ---- 512-thread radix-8 DIF passes (8 points per lane, two waves per SIMD)
// The two passes of a 2^20-point DIF ([8, 12] stages) and the 12-stage
// narrow pass of other DIFs launch 256 workgroups of 4096 points: one
// workgroup per CU. With 256 lanes (16 points each, k_ntt4) that is one wave
// per SIMD and ~45% of its cycles wait on memory (round 3 PMC); with 512 lanes
// each SIMD holds two waves. Radix-8 steps: a lane loads 8 points L apart,
// runs an 8-point DIF (w_8 powers: shifts), multiplies slot q by
// w_{8L}^(low * rev3(q)) and stores them back (the four-step identity of
// k_ntt4's DIF, three stages per LDS exchange).
constexpr int R8_NT = 512;
// LDS hand-off between lanes of ONE wave: a wave's LDS instructions execute
// in issue order, so only the compiler has to keep its reads after its writes
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
__device__ __forceinline__ int r8_pad(int e) { return e + (e >> 3); }  // conflict-free strides 64 / 8 / 1
// slot rev3(k) *= w1^k, k = 1..7 (w1 = w_{8L}^low)
__device__ __forceinline__ void r8_twiddle(uint64_t (&x)[8], uint64_t w1) {
  uint64_t t = w1;
#pragma unroll
  for (int k = 1; k < 8; k++) {
    x[rev<3>(k)] = gl_mul(x[rev<3>(k)], t);
    if (k < 7) t = gl_mul(t, w1);
  }
}

// Wide DIF pass of 8 stages (tile = 16 columns x 256 rows, rows 2^sL apart),
// 256 = 8 x 8 x 4: lane (c, g), g < 32. Same pass twiddle and out-of-place
// store as k_ntt4's wide DIF pass.
template <bool INV>
__global__ void __launch_bounds__(R8_NT, 2) k_ntt_w8r8(NttPassArgs P) {
  __shared__ uint64_t sh[256 * NTT_PADC];
  const int tid = threadIdx.x, c = tid & (NTT_CMAX - 1), g = tid >> 4;
  const NttTables& T = P.tw;
  Tile G;
  G.sL = P.sL;
  G.m = 8;
  G.tile = blockIdx.x;
  G.wide = true;
  const uint64_t tiles_per_blk = (1ULL << G.sL) / NTT_CMAX;
  G.blk_base = (G.tile / tiles_per_blk) * (256ULL << G.sL);
  G.low0 = (G.tile % tiles_per_blk) * NTT_CMAX;
  const int tw_shift = T.K - 8 - G.sL;
  uint64_t low;
  (void)tile_pos(G, 0, c, low);
  // stages 1..0 take rows 4h..4h+3, h = h0 and h0 + 4: the 32 rows stages
  // 4..2 of this wave (g >> 2) wrote, so the last exchange stays in the wave.
  // Every table twiddle depends on the lane only: fetched beside the data.
  const int h0 = 8 * (g >> 2) + (g & 3);
  const uint64_t w1 = tw_pow(T, (uint64_t)g << (T.K - 8), INV);  // w_256^g
  uint64_t ta[2], tb = 1;
  if (low) {  // pass twiddle w_{2^(8+sL)}^(low rev8(t)), rev8(4h + rev2(k)) = 64 k + rev6(h)
#pragma unroll
    for (int hh = 0; hh < 2; hh++)
      ta[hh] = tw_pow(T, (low * (uint64_t)(__brev((uint32_t)(h0 + 4 * hh)) >> 26)) << tw_shift, INV);
    tb = tw_pow(T, (low * 64ULL) << tw_shift, INV);
  }
  uint64_t x[8];
  // stages 7..5 (stride 32), straight from HBM
#pragma unroll
  for (int d = 0; d < 8; d++) x[d] = P.a[tile_pos(G, g + 32 * d, c, low)];
  fft_dif_regs<3, INV>(x);
  if (g) r8_twiddle(x, w1);  // w_256^(g k)
#pragma unroll
  for (int q = 0; q < 8; q++) sh[(g + 32 * q) * NTT_PADC + c] = x[q];
  __syncthreads();
  {  // stages 4..2 (stride 4) on rows 32 (g >> 2) + ..., twiddles w_32^(lo k): shifts
    const int lo = g & 3, base = (g >> 2) * 32 + lo;
#pragma unroll
    for (int d = 0; d < 8; d++) x[d] = sh[(base + 4 * d) * NTT_PADC + c];
    fft_dif_regs<3, INV>(x);
    if (lo) {
#pragma unroll
      for (int k = 1; k < 8; k++) x[rev<3>(k)] = tw_small<INV>(x[rev<3>(k)], lo * k, 16);
    }
#pragma unroll
    for (int d = 0; d < 8; d++) sh[(base + 4 * d) * NTT_PADC + c] = x[d];
  }
  wave_lds_sync();
  uint64_t* dst = P.out ? P.out : P.a;
#pragma unroll
  for (int hh = 0; hh < 2; hh++) {
    const int h = h0 + 4 * hh;
    uint64_t y[4];
#pragma unroll
    for (int d = 0; d < 4; d++) y[d] = sh[(4 * h + d) * NTT_PADC + c];
    fft_dif_regs<2, INV>(y);
    if (low) {
      uint64_t t = ta[hh];
#pragma unroll
      for (int k = 0; k < 4; k++) {
        y[rev<2>(k)] = gl_mul(y[rev<2>(k)], t);
        if (k < 3) t = gl_mul(t, tb);
      }
    }
#pragma unroll
    for (int d = 0; d < 4; d++) dst[tile_pos(G, 4 * h + d, c, low)] = y[d];
  }
}

// LDS slot of point e = 512 a + 64 b + 8 c + d of the 4096-point tile: the XOR
// swizzle 512 a + 64 b + 8 (c ^ (b & 3)) + (d ^ c) (a permutation, no padding).
// Every access of k_ntt_n12r8 is then conflict-free: a ds_read_b64 serves 32
// lanes per LDS cycle (bank = slot mod 32 must differ) and a ds_write_b64 16
// lanes (slot mod 16); the half-wave sets are (c low 2 bits, d), (b low 2
// bits, d) and (b low 2 bits, c), each mapped one to one onto the bank bits
// (round 5's pad e + e / 8 cost 31% of the LDS cycles in conflicts).
__device__ __forceinline__ int n12_slot(int e) {
  const int b = (e >> 6) & 7, c = (e >> 3) & 7, d = e & 7;
  return (e & ~63) | ((c ^ (b & 3)) << 3) | (d ^ c);
}

// Narrow DIF pass of 12 stages on 4096 contiguous points (sL = 0),
// 4096 = 8^4: lane g < 512; the natural-order store (nat_out): position
// p = 4096 tile + e goes to out[bitrev(p)] * out_scale (workgroup order as
// k_ntt4's nat_out).
template <bool INV>
__global__ void __launch_bounds__(R8_NT, 2) k_ntt_n12r8(NttPassArgs P) {
  __shared__ uint64_t sh[4096];
  const int g = threadIdx.x;
  const NttTables& T = P.tw;
  const uint64_t tile = nat_tile(blockIdx.x, gridDim.x);
  const uint64_t p0 = tile << 12;
  uint64_t x[8];
  // both table twiddles depend on the lane only: fetched beside the data
  const int lo2 = g & 63;
  const uint64_t w1 = tw_pow(T, (uint64_t)g << (T.K - 12), INV);    // w_4096^g
  const uint64_t w2 = tw_pow(T, (uint64_t)lo2 << (T.K - 9), INV);   // w_512^lo
  // stages 11..9 (stride 512), straight from HBM
#pragma unroll
  for (int d = 0; d < 8; d++) x[d] = P.a[p0 + g + 512 * d];
  fft_dif_regs<3, INV>(x);
  if (g) r8_twiddle(x, w1);
#pragma unroll
  for (int q = 0; q < 8; q++) sh[n12_slot(g + 512 * q)] = x[q];
  __syncthreads();
  // stages 8..0 stay inside 512-point block g >> 6: wave w's own block, so
  // the exchanges below are between lanes of one wave
  {  // stages 8..6 (stride 64)
    const int base = (g >> 6) * 512 + lo2;
#pragma unroll
    for (int d = 0; d < 8; d++) x[d] = sh[n12_slot(base + 64 * d)];
    fft_dif_regs<3, INV>(x);
    if (lo2) r8_twiddle(x, w2);
#pragma unroll
    for (int d = 0; d < 8; d++) sh[n12_slot(base + 64 * d)] = x[d];
  }
  wave_lds_sync();
  {  // stages 5..3 (stride 8), twiddles w_64^(lo k): shifts
    const int lo = g & 7, base = (g >> 3) * 64 + lo;
#pragma unroll
    for (int d = 0; d < 8; d++) x[d] = sh[n12_slot(base + 8 * d)];
    fft_dif_regs<3, INV>(x);
    if (lo) {
#pragma unroll
      for (int k = 1; k < 8; k++) x[rev<3>(k)] = gl_mul_pow2(x[rev<3>(k)], tw_exp64<INV>(lo * k));
    }
#pragma unroll
    for (int d = 0; d < 8; d++) sh[n12_slot(base + 8 * d)] = x[d];
  }
  wave_lds_sync();
  // stages 2..0 on 8 consecutive points
#pragma unroll
  for (int d = 0; d < 8; d++) x[d] = sh[n12_slot(8 * g + d)];
  fft_dif_regs<3, INV>(x);
  const int sh_r = 32 - P.nat_logN;
  const bool scale = P.out_scale > 1;
#pragma unroll
  for (int q = 0; q < 8; q++)
    P.out[__brev((uint32_t)(p0 + 8 * g + q)) >> sh_r] = scale ? gl_mul(x[q], P.out_scale) : x[q];
}

// A planned pass (ntt_plan.h) to its kernel; false = not one of this unit's forms.
bool launch_pass512(hipStream_t st, const NttPass& p, bool inverse, const NttPassArgs& P) {
  const dim3 g(p.tiles), b(p.threads);
  switch (p.form) {
    case NTT_DIF9:
      if (inverse) hipLaunchKernelGGL(k_ntt_dif9<true>, g, b, 0, st, P);
      else hipLaunchKernelGGL(k_ntt_dif9<false>, g, b, 0, st, P);
      return true;
    case NTT_W8R8:
      if (inverse) hipLaunchKernelGGL(k_ntt_w8r8<true>, g, b, 0, st, P);
      else hipLaunchKernelGGL(k_ntt_w8r8<false>, g, b, 0, st, P);
      return true;
    case NTT_N12R8:
      if (inverse) hipLaunchKernelGGL(k_ntt_n12r8<true>, g, b, 0, st, P);
      else hipLaunchKernelGGL(k_ntt_n12r8<false>, g, b, 0, st, P);
      return true;
    default:
      return false;
  }
}
}  // namespace sezkp
