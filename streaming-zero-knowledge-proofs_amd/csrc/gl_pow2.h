// gl_pow2.h — Goldilocks products by powers of two and the register
// butterflies built on them (the four-step register passes of ntt_pass.hip).
// 2 has order 192 mod p, so every root of unity w_{2^k} with k <= 6 is a power
// of two and x * w^j is limb placement plus one or two add/sub fix-ups.
#pragma once
#include "dev_common.h"

namespace sezkp {

__device__ __forceinline__ uint64_t gl_neg(uint64_t x) { return x ? GL_P - x : 0; }
// x * 2^e mod p for 0 <= e < 96 with e a compile-time constant after
// unrolling, by 32-bit limb placement (2^64 = 2^32 - 1, 2^96 = -1) instead of
// a 128-bit reduction. gl_add(A, B) is canonical for any A < 2^64 when
// B = h eps with h < 2^32 (mul_eps32), i.e. B <= eps^2 = p - 2^32: then
// A + B < 2p, so one subtraction of p suffices. (Not for every B < p:
// A = 2^64 - 1, B = p - 1 leaves 2^64 - 2.)
//   e < 32:  x 2^e = A + y2 2^64 = A + y2 eps,   A = x << e, y2 = x >> (64-e)
//   e < 64:  x 2^e = A 2^32 + y2 2^96 = (A_lo << 32) + A_hi eps - y2, A = x << (e-32)
//   e < 96:  x 2^e = (x 2^(e-64)) 2^64 = y 2^32 - y
__device__ __forceinline__ uint64_t mul_eps32(uint32_t h) { return ((uint64_t)h << 32) - h; }  // h * eps < p
__device__ __forceinline__ uint64_t gl_mul2e_lo(uint64_t x, int e) {  // 0 <= e < 32
  if (e == 0) return x;
  const uint64_t A = x << e;
  const uint32_t y2 = (uint32_t)(x >> (64 - e));
  return gl_add(A, mul_eps32(y2));
}
__device__ __forceinline__ uint64_t gl_mul2e(uint64_t x, int e) {
  if (e < 32) return gl_mul2e_lo(x, e);
  if (e < 64) {
    const int r = e - 32;
    const uint64_t A = r ? x << r : x;
    const uint32_t y2 = r ? (uint32_t)(x >> (64 - r)) : 0u;
    const uint64_t t = gl_add(A << 32, mul_eps32((uint32_t)(A >> 32)));
    return r ? gl_sub(t, y2) : t;
  }
  const uint64_t y = gl_mul2e_lo(x, e - 64);
  return gl_sub(gl_add(y << 32, mul_eps32((uint32_t)(y >> 32))), y);
}
// x * 2^e mod p, 0 <= e < 192 (2^96 = -1)
__device__ __forceinline__ uint64_t gl_mul_pow2(uint64_t x, int e) {
  return e >= 96 ? gl_neg(gl_mul2e(x, e - 96)) : gl_mul2e(x, e);
}
// exponent of w_{2h}^j as a power of two: w_32 = 2^78 (w_32^-1 = 2^114), so
// w_16 = 2^156 (w_16^-1 = 2^36); 2 has order 192 mod p, every w_{2^k} with
// k <= 6 is a power of two (w_64 = 2^39), the reference's roots included
template <bool INV>
__device__ __forceinline__ constexpr int tw_exp(int j, int h) { return ((INV ? 114 : 78) * j * (16 / h)) % 192; }
// x * w_{2h}^j for 2h <= 32
template <bool INV>
__device__ __forceinline__ uint64_t tw_small(uint64_t x, int j, int h) {
  return gl_mul_pow2(x, tw_exp<INV>(j, h));
}
// Butterflies take the sign of w^j = -2^(e-96) into the add/sub instead of negating.
template <int LOGF, bool INV, int SKIP>
__device__ __forceinline__ void fft_dit_regs(uint64_t (&x)[1 << LOGF]) {
#pragma unroll
  for (int s = SKIP; s < LOGF; s++) {
    const int h = 1 << s;
#pragma unroll
    for (int t0 = 0; t0 < (1 << LOGF); t0++) {
      if (!(t0 & h)) {
        const int j = t0 & (h - 1);
        const int e = j ? tw_exp<INV>(j, h) : 0;
        const bool neg = e >= 96;
        const uint64_t y = gl_mul2e(x[t0 + h], neg ? e - 96 : e);
        const uint64_t a = x[t0];
        x[t0] = neg ? gl_sub(a, y) : gl_add(a, y);
        x[t0 + h] = neg ? gl_add(a, y) : gl_sub(a, y);
      }
    }
  }
}
template <int LOGF, bool INV>
__device__ __forceinline__ void fft_dif_regs(uint64_t (&x)[1 << LOGF]) {
#pragma unroll
  for (int s = LOGF - 1; s >= 0; s--) {
    const int h = 1 << s;
#pragma unroll
    for (int t0 = 0; t0 < (1 << LOGF); t0++) {
      if (!(t0 & h)) {
        const int j = t0 & (h - 1);
        const int e = j ? tw_exp<INV>(j, h) : 0;
        const bool neg = e >= 96;
        const uint64_t a = x[t0], b = x[t0 + h];
        x[t0] = gl_add(a, b);
        x[t0 + h] = gl_mul2e(neg ? gl_sub(b, a) : gl_sub(a, b), neg ? e - 96 : e);
      }
    }
  }
}
template <int M>
__device__ __forceinline__ constexpr int rev(int x) {
  int r = 0;
  for (int i = 0; i < M; i++) r |= ((x >> i) & 1) << (M - 1 - i);
  return r;
}
// w_64 = 2^39, w_64^-1 = 2^153 (2 has order 192)
template <bool INV>
__device__ __forceinline__ constexpr int tw_exp64(int j) { return ((INV ? 153 : 39) * j) % 192; }

}  // namespace sezkp
