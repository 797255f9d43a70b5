// trace_image.hip — the trace image for CDNA4 (gfx950): the block view's step
// arrays transposed to tape-major, and the row expansion (block ids, first /
// last flags, block-local heads) that every later column kernel reads.
//
// Reference semantics: RowIter values (openings.rs:227-273; ==
// TraceColumns::build columns.rs:252-365).
#include "dev_common.h"
#include "col_dev.h"
#include "sezkp_internal.h"

namespace sezkp {

// ------------------------------------------------------------ trace image
// The block view's step arrays are row-major [n][tau]; the kernels read them
// tape-major [tau][n]. One lane per row: the lane's tau cells are adjacent on
// the read side, and a wave's stores to one tape are 64 consecutive cells.
// wsym is zeroed where has_write is false (the reference reads the
// symbol only under the flag: `op.write.unwrap_or(0)`, columns.rs:71-72).
__global__ void __launch_bounds__(TR_THREADS) k_trace_image(const int8_t* __restrict__ raw_mv,
                                                          const uint8_t* __restrict__ raw_hw,
                                                          const uint16_t* __restrict__ raw_ws, uint64_t n, int tau,
                                                          int8_t* __restrict__ mv, uint8_t* __restrict__ wf,
                                                          uint16_t* __restrict__ ws, uint64_t r0, uint64_t r1) {
  const uint64_t s = r0 + (uint64_t)blockIdx.x * TR_THREADS + threadIdx.x;
  if (s >= r1) return;
  const size_t i0 = (size_t)s * tau;
  for (int r = 0; r < tau; r++) {
    const size_t o = (size_t)r * n + s;
    const bool w = raw_hw[i0 + r] != 0;
    mv[o] = raw_mv[i0 + r];
    wf[o] = w ? 1 : 0;
    ws[o] = w ? raw_ws[i0 + r] : 0;
  }
}

// tau = 8 (the headline shape): a lane takes 8 consecutive steps, loads their
// 64 + 64 + 128 raw bytes as 16-byte vectors, transposes the 8 x 8 byte /
// u16 matrices in registers (three XOR-swap stages, 64-bit words) and stores
// 8 bytes / 16 bytes per tape: the same image as k_trace_image with wide
// coalesced accesses instead of byte loads and stores.
__device__ __forceinline__ void swap_bits(uint64_t& a, uint64_t& b, int sh, uint64_t m) {
  const uint64_t t = ((a >> sh) ^ b) & m;
  a ^= t << sh;
  b ^= t;
}
__device__ __forceinline__ void transpose8x8_u8(uint64_t (&r)[8]) {
#pragma unroll
  for (int i = 0; i < 4; i++) swap_bits(r[i], r[i + 4], 32, 0x00000000FFFFFFFFull);
#pragma unroll
  for (int i = 0; i < 8; i++)
    if ((i & 2) == 0) swap_bits(r[i], r[i + 2], 16, 0x0000FFFF0000FFFFull);
#pragma unroll
  for (int i = 0; i < 8; i += 2) swap_bits(r[i], r[i + 1], 8, 0x00FF00FF00FF00FFull);
}
// rows of 8 u16 as (lo = elements 0..3, hi = 4..7)
__device__ __forceinline__ void transpose8x8_u16(uint64_t (&lo)[8], uint64_t (&hi)[8]) {
#pragma unroll
  for (int i = 0; i < 4; i++) {
    const uint64_t t = hi[i];
    hi[i] = lo[i + 4];
    lo[i + 4] = t;
  }
#pragma unroll
  for (int i = 0; i < 8; i++)
    if ((i & 2) == 0) {
      swap_bits(lo[i], lo[i + 2], 32, 0x00000000FFFFFFFFull);
      swap_bits(hi[i], hi[i + 2], 32, 0x00000000FFFFFFFFull);
    }
#pragma unroll
  for (int i = 0; i < 8; i += 2) {
    swap_bits(lo[i], lo[i + 1], 16, 0x0000FFFF0000FFFFull);
    swap_bits(hi[i], hi[i + 1], 16, 0x0000FFFF0000FFFFull);
  }
}
// bytes -> 0 / 1 (any nonzero byte is a write)
__device__ __forceinline__ uint64_t bytes_nonzero(uint64_t x) {
  x |= x >> 4;
  x |= x >> 2;
  x |= x >> 1;
  return x & 0x0101010101010101ull;
}
// 4 bytes of 0 / 1 (low half of b) -> 4 u16 masks of 0 / 0xFFFF
__device__ __forceinline__ uint64_t spread_mask16(uint32_t b) {
  const uint64_t s = (uint64_t)(b & 0xFF) | ((uint64_t)(b & 0xFF00) << 8) | ((uint64_t)(b & 0xFF0000) << 16) |
                     ((uint64_t)(b & 0xFF000000u) << 24);
  return (s << 16) - s;
}
__global__ void __launch_bounds__(TR_THREADS) k_trace_image8(const int8_t* __restrict__ raw_mv,
                                                           const uint8_t* __restrict__ raw_hw,
                                                           const uint16_t* __restrict__ raw_ws, uint64_t n,
                                                           int8_t* __restrict__ mv, uint8_t* __restrict__ wf,
                                                           uint16_t* __restrict__ ws, uint64_t r0, uint64_t r1) {
  // rows [r0, r1): r0 a multiple of 8
  const uint64_t s0 = r0 + ((uint64_t)blockIdx.x * TR_THREADS + threadIdx.x) * 8;
  if (s0 >= r1) return;
  if (s0 + 8 > r1) {  // ragged tail: element by element
    for (uint64_t s = s0; s < r1; s++)
      for (int r = 0; r < 8; r++) {
        const bool w = raw_hw[s * 8 + r] != 0;
        mv[(uint64_t)r * n + s] = raw_mv[s * 8 + r];
        wf[(uint64_t)r * n + s] = w ? 1 : 0;
        ws[(uint64_t)r * n + s] = w ? raw_ws[s * 8 + r] : 0;
      }
    return;
  }
  uint64_t m[8], h[8], wl[8], wh[8];
  {
    const uint4* pm = reinterpret_cast<const uint4*>(raw_mv + s0 * 8);
    const uint4* ph = reinterpret_cast<const uint4*>(raw_hw + s0 * 8);
    const uint4* pw = reinterpret_cast<const uint4*>(raw_ws + s0 * 8);
#pragma unroll
    for (int q = 0; q < 4; q++) {
      const uint4 a = pm[q], b = ph[q];
      m[2 * q] = (uint64_t)a.x | ((uint64_t)a.y << 32);
      m[2 * q + 1] = (uint64_t)a.z | ((uint64_t)a.w << 32);
      h[2 * q] = (uint64_t)b.x | ((uint64_t)b.y << 32);
      h[2 * q + 1] = (uint64_t)b.z | ((uint64_t)b.w << 32);
    }
#pragma unroll
    for (int q = 0; q < 8; q++) {
      const uint4 c = pw[q];
      wl[q] = (uint64_t)c.x | ((uint64_t)c.y << 32);
      wh[q] = (uint64_t)c.z | ((uint64_t)c.w << 32);
    }
  }
  // mask the symbols of steps that write nothing (row = step here)
#pragma unroll
  for (int i = 0; i < 8; i++) {
    h[i] = bytes_nonzero(h[i]);
    wl[i] &= spread_mask16((uint32_t)h[i]);
    wh[i] &= spread_mask16((uint32_t)(h[i] >> 32));
  }
  transpose8x8_u8(m);
  transpose8x8_u8(h);
  transpose8x8_u16(wl, wh);
#pragma unroll
  for (int r = 0; r < 8; r++) {
    const uint64_t o = (uint64_t)r * n + s0;
    *reinterpret_cast<uint64_t*>(mv + o) = m[r];
    *reinterpret_cast<uint64_t*>(wf + o) = h[r];
    *reinterpret_cast<uint4*>(ws + o) =
        make_uint4((uint32_t)wl[r], (uint32_t)(wl[r] >> 32), (uint32_t)wh[r], (uint32_t)(wh[r] >> 32));
  }
}

// ------------------------------------------------------------ expansion
// One workgroup per block: row -> block id, first/last flags, and the
// post-move head prefix sums per tape (head starts at 0 in every block).
// The head columns are stored as i32 (the reference keeps i64 heads,
// air.rs:54): a block whose head leaves the i32 range (more than ~2^24 rows of
// large moves) sets the guard word to GUARD_HEAD_RANGE and the proof fails.
__global__ void __launch_bounds__(TR_THREADS) k_expand(TraceDev T, uint32_t b0, uint32_t* __restrict__ err) {
  const uint32_t b = b0 + blockIdx.x;
  const uint64_t s = T.blk_start[b], e = T.blk_start[b + 1];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (uint64_t r = s + tid; r < e; r += TR_THREADS) {
    T.row_blk[r] = b;
    T.row_flags[r] = (uint8_t)((r == s ? 1 : 0) | (r + 1 == e ? 2 : 0));
  }
  // head = block-local inclusive prefix sum of the tape's moves. One wave per
  // tape (no WG barriers): two rows per lane, 32-bit wave scan (|sum| <= 128
  // rows * 128), 64-bit carry from lane 63. The block's min / max head goes to
  // head_rng, so the dictionary plan need not re-read the head columns.
  for (int tp = wave; tp < T.tau; tp += TR_THREADS / 64) {
    const int8_t* mv = T.mv + (uint64_t)tp * T.n;
    int32_t* hd = T.head + (uint64_t)tp * T.n;
    int64_t carry = 0, lo = INT64_MAX, hi = INT64_MIN;
    // even block start (n is even): a lane's row pair is one 2-byte load and
    // one 8-byte store
    const bool paired = (s & 1) == 0;
    for (uint64_t r0 = s; r0 < e; r0 += 128) {
      const uint64_t r = r0 + 2 * (uint64_t)lane;
      int32_t m0 = 0, m1 = 0;
      if (paired && r + 1 < e) {
        const uint16_t w = *reinterpret_cast<const uint16_t*>(mv + r);
        m0 = (int8_t)(w & 0xFF);
        m1 = (int8_t)(w >> 8);
      } else {
        m0 = r < e ? (int32_t)mv[r] : 0;
        m1 = r + 1 < e ? (int32_t)mv[r + 1] : 0;
      }
      int32_t x = m0 + m1;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const int32_t y = __shfl_up(x, o, 64);
        if (lane >= o) x += y;
      }
      const int64_t h1 = carry + (int64_t)x;  // through row r + 1
      if (r < e) {
        lo = min(lo, h1 - m1);
        hi = max(hi, h1 - m1);
      }
      if (r + 1 < e) {
        lo = min(lo, h1);
        hi = max(hi, h1);
      }
      if (paired && r + 1 < e) {
        *reinterpret_cast<int2*>(hd + r) = make_int2((int32_t)(h1 - m1), (int32_t)h1);
      } else {
        if (r < e) hd[r] = (int32_t)(h1 - m1);
        if (r + 1 < e) hd[r + 1] = (int32_t)h1;
      }
      carry += __shfl(x, 63, 64);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      lo = min(lo, __shfl_xor(lo, o, 64));
      hi = max(hi, __shfl_xor(hi, o, 64));
    }
    if (lane == 0) {
      T.head_rng[2 * ((uint64_t)tp * T.nblk + b)] = lo;
      T.head_rng[2 * ((uint64_t)tp * T.nblk + b) + 1] = hi;
      if (lo < (int64_t)INT32_MIN || hi > (int64_t)INT32_MAX) atomicOr(err, GUARD_HEAD_RANGE);
    }
  }
}

// ------------------------------------------------------------------ host
hipError_t launch_trace_image(hipStream_t st, const int8_t* raw_mv, const uint8_t* raw_hw, const uint16_t* raw_ws,
                              uint64_t n, int tau, int8_t* mv, uint8_t* wf, uint16_t* ws, uint64_t r0, uint64_t r1) {
  if (r1 > n) r1 = n;
  if (r0 >= r1 || tau <= 0) return hipSuccess;
  if (tau == 8) {
    r0 &= ~7ull;  // the rows in front of the slice are the raw buffer's other contents: never read
    const uint64_t g8 = ((r1 - r0 + 7) / 8 + TR_THREADS - 1) / TR_THREADS;
    if (g8 > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_trace_image8, dim3((unsigned)g8), dim3(TR_THREADS), 0, st, raw_mv, raw_hw, raw_ws, n, mv, wf,
                       ws, r0, r1);
    return hipGetLastError();
  }
  const uint64_t g = (r1 - r0 + TR_THREADS - 1) / TR_THREADS;
  if (g > 0x7FFFFFFFull) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_trace_image, dim3((unsigned)g), dim3(TR_THREADS), 0, st, raw_mv, raw_hw, raw_ws, n, tau, mv,
                     wf, ws, r0, r1);
  return hipGetLastError();
}
hipError_t launch_expand(hipStream_t st, const TraceDev& T, uint32_t blk_lo, uint32_t blk_cnt, uint32_t* d_err) {
  if (blk_cnt == 0) return hipSuccess;
  if ((uint64_t)blk_lo + blk_cnt > T.nblk) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_expand, dim3(blk_cnt), dim3(TR_THREADS), 0, st, T, blk_lo, d_err);
  return hipGetLastError();
}

}  // namespace sezkp
