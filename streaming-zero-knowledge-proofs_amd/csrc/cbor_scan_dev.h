// cbor_scan_dev.h — the one-workgroup exclusive scan of 32-bit counts that the
// CBOR decoders (cbor_decode.hip: candidates per tile, steps per block) and
// the CBOR encoder (cbor_encode.hip: step bytes per tile, head and tail bytes
// per block) share. Device code: included by those two units only.
#pragma once
#include <hip/hip_runtime.h>

#include "trace_cbor_plan.h"

namespace sezkp {

// offs[i] = the sum of the counts before i; *total = all of them
static __global__ void __launch_bounds__(TRACE_CBOR_THREADS)
    k_cbor_tile_scan(const uint32_t* __restrict__ counts, uint64_t ntiles, uint64_t* __restrict__ offs,
                     uint64_t* total_out) {
  constexpr int THREADS = (int)TRACE_CBOR_THREADS;
  __shared__ unsigned long long sh[THREADS / 64];
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
    for (int w = 0; w < THREADS / 64; w++) {
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

static inline hipError_t cbor_scan(hipStream_t st, const uint32_t* counts, uint64_t n, uint64_t* offs, uint64_t* total) {
  hipLaunchKernelGGL(k_cbor_tile_scan, dim3(1), dim3(TRACE_CBOR_THREADS), 0, st, counts, n, offs, total);
  return hipGetLastError();
}

}  // namespace sezkp
