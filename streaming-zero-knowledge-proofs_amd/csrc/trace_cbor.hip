// trace_cbor.hip — TraceFile CBOR bytes to the four step arrays on the device
// (gfx950), for sezkp_ctx_upload_trace_cbor / sezkp_ctx_decode_trace_cbor.
//
// The file's bytes lie in device memory; trace_cbor_plan.h holds the canonical
// form, the strict step parser and the tiling. Four launches on one stream:
//   k_cbor_marks<false>  per tile of 4096 bytes: how many positions start the
//                        signature A2 68 "input_mv" (the candidates);
//   k_cbor_tile_scan     one workgroup: the exclusive scan of the tile counts
//                        and the number of candidates;
//   k_cbor_marks<true>   the same marks again, now stored in file order (the
//                        first t of them): wave64 ballots and popcounts give a
//                        lane its place in the wave, four words of LDS a wave
//                        its place in the tile, the scan the tile's place;
//   k_cbor_parse         one lane per stored candidate parses a whole step
//                        strictly into row i and checks its link of the chain.
// Nothing here decides: the verdict words go home and the host accepts the
// arrays or runs its own decoder (ctx_trace_cbor.cpp). Every read of the file
// goes through cbor_at / cbor_load16, which never read at or past len.
#include <hip/hip_runtime.h>

#include "sezkp_internal.h"
#include "trace_cbor_plan.h"

namespace sezkp {

constexpr int TC_THREADS = (int)TRACE_CBOR_THREADS;
static_assert(TC_THREADS == 256 && TRACE_CBOR_LANE_BYTES == 16, "four waves of 64 lanes, one 16-byte load per lane");

// the candidates among the 16 positions from pos (bit s: pos + s), none before lo
__device__ __forceinline__ uint32_t lane_marks(const CborSpan& s, uint64_t lo, uint64_t pos) {
  if (pos >= s.len) return 0;
  uint32_t m = cbor_sig_mask(cbor_load16(s, pos), cbor_load16(s, pos + 16));
  if (pos < lo) m = lo - pos >= 16 ? 0u : m & (0xFFFFu << (uint32_t)(lo - pos)) & 0xFFFFu;
  return m;
}

// A signature is 10 bytes and its first byte occurs nowhere else in it, so two
// candidates lie at least 10 positions apart: a lane's 16 positions hold at
// most two. Two ballots (one or more, two) count and place them.
template <bool STORE>
__global__ void __launch_bounds__(TC_THREADS) k_cbor_marks(CborSpan s, uint64_t lo, uint32_t* __restrict__ counts,
                                                           const uint64_t* __restrict__ offs,
                                                           uint64_t* __restrict__ cand, uint64_t t) {
  __shared__ uint32_t sh[TC_THREADS / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint64_t pos = (uint64_t)blockIdx.x * TRACE_CBOR_TILE + (uint64_t)threadIdx.x * TRACE_CBOR_LANE_BYTES;
  const uint32_t m = lane_marks(s, lo, pos);
  const uint32_t c = (uint32_t)__popc(m);
  const unsigned long long b1 = __ballot(c >= 1), b2 = __ballot(c >= 2);
  if (lane == 0) sh[wave] = (uint32_t)(__popcll(b1) + __popcll(b2));
  __syncthreads();
  if constexpr (!STORE) {
    if (threadIdx.x == 0) counts[blockIdx.x] = sh[0] + sh[1] + sh[2] + sh[3];
  } else {
    if (!m) return;
    uint32_t before = 0;
#pragma unroll
    for (int w = 0; w < TC_THREADS / 64; w++)
      if (w < wave) before += sh[w];
    const unsigned long long below = (1ull << lane) - 1ull;
    uint64_t idx = offs[blockIdx.x] + before + (uint64_t)(__popcll(b1 & below) + __popcll(b2 & below));
    uint32_t rest = m;
    while (rest) {
      const uint32_t bit = (uint32_t)__ffs((int)rest) - 1u;
      rest &= rest - 1u;
      if (idx < t) cand[idx] = pos + bit;
      idx++;
    }
  }
}

// offs[i] = the candidates in the tiles before i; *total = all of them
__global__ void __launch_bounds__(TC_THREADS) k_cbor_tile_scan(const uint32_t* __restrict__ counts, uint64_t ntiles,
                                                               uint64_t* __restrict__ offs, uint64_t* total_out) {
  __shared__ unsigned long long sh[TC_THREADS / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  constexpr uint32_t PER = TRACE_CBOR_SCAN_PASS / TRACE_CBOR_THREADS;
  unsigned long long carry = 0;
  for (uint64_t base = 0; base < ntiles; base += TRACE_CBOR_SCAN_PASS) {
    const uint64_t i0 = base + (uint64_t)threadIdx.x * PER;
    uint32_t c[PER];
    unsigned long long sum = 0;
#pragma unroll
    for (uint32_t k = 0; k < PER; k++) {
      c[k] = i0 + k < ntiles ? counts[i0 + k] : 0u;
      sum += c[k];
    }
    unsigned long long x = sum;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const unsigned long long y = __shfl_up(x, o, 64);
      if (lane >= o) x += y;
    }
    if (lane == 63) sh[wave] = x;
    __syncthreads();
    unsigned long long before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < TC_THREADS / 64; w++) {
      const unsigned long long v = sh[w];
      if (w < wave) before += v;
      total += v;
    }
    __syncthreads();
    unsigned long long excl = carry + before + x - sum;
#pragma unroll
    for (uint32_t k = 0; k < PER; k++)
      if (i0 + k < ntiles) {
        offs[i0 + k] = excl;
        excl += c[k];
      }
    carry += total;
  }
  if (threadIdx.x == 0) *total_out = carry;
}
// the scan alone, for blocks_cbor.hip: n counts (candidates per tile, steps
// per block) to their exclusive scan and, in a device word, their sum
hipError_t launch_cbor_tile_scan(hipStream_t st, const uint32_t* counts, uint64_t n, uint64_t* offs, uint64_t* total) {
  hipLaunchKernelGGL(k_cbor_tile_scan, dim3(1), dim3(TC_THREADS), 0, st, counts, n, offs, total);
  return hipGetLastError();
}

// Step i from candidate i, and its link: step 0 starts at lo, step i + 1 where
// step i ends. With fewer than t candidates nothing is parsed (the host
// declines on the count). The first failures by index: 64-bit atomic minima,
// taken only by lanes that fail.
__global__ void __launch_bounds__(TC_THREADS) k_cbor_parse(CborSpan s, uint64_t lo, const uint64_t* __restrict__ cand,
                                                           uint64_t t, uint32_t tau, int8_t* __restrict__ input_mv,
                                                           int8_t* __restrict__ mv, uint8_t* __restrict__ has_write,
                                                           uint16_t* __restrict__ wsym, TraceCborVerdict* V) {
  const uint64_t i = (uint64_t)blockIdx.x * TC_THREADS + threadIdx.x;
  if (i >= t || V->candidates < t) return;
  const uint64_t c = cand[i], o = i * tau;
  const uint64_t end = cbor_parse_step(s, c, tau, input_mv + i, mv + o, has_write + o, wsym + o);
  if (!end) {
    atomicMin(reinterpret_cast<unsigned long long*>(&V->bad_step), (unsigned long long)i);
    return;
  }
  if (i == 0 && c != lo) atomicMin(reinterpret_cast<unsigned long long*>(&V->bad_link), 0ull);
  if (i + 1 < t) {
    if (cand[i + 1] != end) atomicMin(reinterpret_cast<unsigned long long*>(&V->bad_link), (unsigned long long)(i + 1));
  } else {
    V->tail_off = end;
  }
}

// counts / offs: trace_cbor_tiles(len) words each; cand: t words; the arrays:
// t and t * tau elements. t >= 1 and t <= len / cbor_step_min_len(tau)
// (trace_cbor_head), d_bytes on a 16-byte boundary.
hipError_t launch_trace_cbor_decode(hipStream_t st, const uint8_t* d_bytes, uint64_t len, uint64_t steps_off, uint64_t t,
                                    uint32_t tau, uint32_t* counts, uint64_t* offs, uint64_t* cand, int8_t* input_mv,
                                    int8_t* mv, uint8_t* has_write, uint16_t* wsym, TraceCborVerdict* verdict) {
  const uint64_t ntiles = trace_cbor_tiles(len), pgrid = (t + TC_THREADS - 1) / TC_THREADS;
  if (!t || !ntiles || ntiles > 0x7FFFFFFFull || pgrid > 0x7FFFFFFFull) return hipErrorInvalidValue;
  if (reinterpret_cast<uintptr_t>(d_bytes) & 15u) return hipErrorInvalidValue;
  const CborSpan s{d_bytes, len};
  hipError_t e = hipMemsetAsync(verdict, 0xFF, sizeof(TraceCborVerdict), st);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_cbor_marks<false>, dim3((uint32_t)ntiles), dim3(TC_THREADS), 0, st, s, steps_off, counts, nullptr,
                     nullptr, t);
  hipLaunchKernelGGL(k_cbor_tile_scan, dim3(1), dim3(TC_THREADS), 0, st, counts, ntiles, offs, &verdict->candidates);
  hipLaunchKernelGGL(k_cbor_marks<true>, dim3((uint32_t)ntiles), dim3(TC_THREADS), 0, st, s, steps_off, nullptr, offs,
                     cand, t);
  hipLaunchKernelGGL(k_cbor_parse, dim3((uint32_t)pgrid), dim3(TC_THREADS), 0, st, s, steps_off, cand, t, tau, input_mv,
                     mv, has_write, wsym, verdict);
  return hipGetLastError();
}

}  // namespace sezkp
