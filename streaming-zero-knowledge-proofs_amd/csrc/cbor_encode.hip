// cbor_encode.hip — a block file (Vec<BlockSummary>) or a TraceFile written as
// CBOR on the device (gfx950), from step arrays and block tables in device
// memory (sezkp_ctx_encode_trace_blocks_cbor / sezkp_ctx_encode_blocks_cbor /
// sezkp_ctx_encode_trace_cbor). cbor_emit_plan.h holds the byte layout, the
// tiling and the body of every per-index pass, so a kernel here is its index,
// one or two calls and, for the steps, the staging of a tile in LDS. On one
// stream, 256 lanes a workgroup, no atomics:
//   k_cbor_emit_step_lens   per tile of S steps (S from tau), one lane a step:
//                           the record's length, summed over the tile;
//   k_cbor_emit_block_lens  one lane per block: its head + tail length;
//   k_cbor_tile_scan        both, exclusive, and their totals (cbor_scan_dev.h);
// the two totals go home, the host sizes the file's memory, and then
//   k_cbor_emit_steps       per tile: every lane recomputes its step's length,
//                           the workgroup scans them, the lane writes its
//                           record into LDS at its tile-local offset, and all
//                           lanes copy the tile out, run by run (a run: the
//                           tile's steps of one block, contiguous in the file),
//                           consecutive lanes to consecutive bytes;
//   k_cbor_emit_blocks      one lane per block: its head in front of its first
//                           step, its tail behind its last one.
// A step's LDS offset stays below S * cbor_step_max_len(tau) <= CBOR_EMIT_LDS;
// a file offset is below the length the same code measured, and the copy-out
// checks it against out_len all the same.
#include <hip/hip_runtime.h>

#include "cbor_emit_plan.h"
#include "cbor_scan_dev.h"
#include "sezkp_internal.h"

namespace sezkp {

constexpr int CE_THREADS = (int)CBOR_EMIT_THREADS;
static_assert(CE_THREADS == 256, "four waves of 64 lanes");

// a lane's place in the workgroup's scan of x: the sum over the lanes before
// it, and the workgroup's total. sh: one word per wave; two barriers.
__device__ inline uint32_t ce_scan(uint32_t v, uint32_t* sh, uint32_t& total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint32_t x = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t y = __shfl_up(x, o, 64);
    if (lane >= o) x += y;
  }
  if (lane == 63) sh[wave] = x;
  __syncthreads();
  uint32_t before = 0;
  total = 0;
#pragma unroll
  for (int w = 0; w < CE_THREADS / 64; w++) {
    const uint32_t s = sh[w];
    if (w < wave) before += s;
    total += s;
  }
  __syncthreads();
  return before + x - v;
}

__global__ void __launch_bounds__(CE_THREADS)
    k_cbor_emit_step_lens(CborEmitSteps A, uint64_t t, uint32_t tau, uint32_t S, uint32_t* __restrict__ counts) {
  __shared__ uint32_t sh[CE_THREADS / 64];
  const uint64_t i = (uint64_t)blockIdx.x * S + threadIdx.x;
  const uint32_t len = threadIdx.x < S && i < t ? cbor_emit_step_len(A, tau, i) : 0u;
  uint32_t total;
  (void)ce_scan(len, sh, total);
  if (threadIdx.x == 0) counts[blockIdx.x] = total;
}

__global__ void __launch_bounds__(CE_THREADS) k_cbor_emit_block_lens(CborEmitShape sh, CborEmitTables T, uint32_t* blen) {
  cbor_emit_block_len_pass(sh, T, blen, (uint64_t)blockIdx.x * CE_THREADS + threadIdx.x);
}

__global__ void __launch_bounds__(CE_THREADS)
    k_cbor_emit_steps(CborEmitShape sh, CborEmitSteps A, uint32_t S, const uint64_t* __restrict__ offs, CborEmitScans sc,
                      uint8_t* __restrict__ out, uint64_t out_len) {
  __shared__ uint8_t stage[CBOR_EMIT_LDS];
  __shared__ uint32_t run_lo[CE_THREADS + 1];
  __shared__ uint64_t run_shift[CE_THREADS];
  __shared__ uint32_t w_sum[CE_THREADS / 64];
  const uint32_t tid = threadIdx.x;
  const uint64_t i = (uint64_t)blockIdx.x * S + tid;
  const bool active = tid < S && i < sh.t;
  const uint32_t len = active ? cbor_emit_step_len(A, sh.tau, i) : 0u;
  uint32_t total;
  const uint32_t at = ce_scan(len, w_sum, total);  // at + len <= total <= S * cbor_step_max_len(tau)
  bool first = false;
  uint64_t dst = 0;
  if (active) {
    dst = cbor_emit_step_place(sh, sc, i, offs[blockIdx.x] + at, first);
    CborBytes o{stage + at};
    cbor_emit_step(o, A, sh.tau, i);
  }
  // the runs: one starts at the tile's first step and at every first step of a block
  const bool start = active && (tid == 0 || first);
  uint32_t runs;
  const uint32_t r = ce_scan(start ? 1u : 0u, w_sum, runs);
  if (start) {
    run_lo[r] = at;
    run_shift[r] = dst - at;
  }
  if (tid == 0) run_lo[runs] = total;
  __syncthreads();
  for (uint32_t q = 0; q < runs; q++) {
    const uint32_t hi = run_lo[q + 1];
    const uint64_t shift = run_shift[q];
    for (uint32_t x = run_lo[q] + tid; x < hi; x += CE_THREADS)
      if (shift + x < out_len) out[shift + x] = stage[x];
  }
}

__global__ void __launch_bounds__(CE_THREADS)
    k_cbor_emit_blocks(CborEmitShape sh, CborEmitTables T, CborEmitScans sc, uint8_t* out, uint64_t out_len) {
  cbor_emit_block_pass(sh, T, sc, CborBounded{out, 0, out_len}, (uint64_t)blockIdx.x * CE_THREADS + threadIdx.x);
}

static uint64_t grid_of(uint64_t n) { return (n + CE_THREADS - 1) / CE_THREADS; }
static bool grid_fits(uint64_t g) { return g && g <= 0x7FFFFFFFull; }

hipError_t launch_cbor_emit_lengths(hipStream_t st, const CborEmitShape& sh, const CborEmitSteps& A,
                                    const CborEmitTables& T, uint32_t* counts, uint64_t* offs, uint32_t* blen,
                                    uint64_t* pre, uint64_t* words) {
  const uint32_t S = cbor_emit_tile_steps(sh.tau);
  const uint64_t tiles = cbor_emit_tiles(sh.t, S), bgrid = grid_of(sh.B);
  if (!grid_fits(bgrid) || (sh.t && !grid_fits(tiles))) return hipErrorInvalidValue;
  hipError_t e = hipMemsetAsync(words, 0, 16, st);
  if (e != hipSuccess) return e;
  if (sh.t) {
    hipLaunchKernelGGL(k_cbor_emit_step_lens, dim3((uint32_t)tiles), dim3(CE_THREADS), 0, st, A, sh.t, sh.tau, S, counts);
    if ((e = cbor_scan(st, counts, tiles, offs, words)) != hipSuccess) return e;
  }
  hipLaunchKernelGGL(k_cbor_emit_block_lens, dim3((uint32_t)bgrid), dim3(CE_THREADS), 0, st, sh, T, blen);
  return cbor_scan(st, blen, sh.B, pre, words + 1);
}

hipError_t launch_cbor_emit(hipStream_t st, const CborEmitShape& sh, const CborEmitSteps& A, const CborEmitTables& T,
                            const uint64_t* offs, const uint32_t* blen, const uint64_t* pre, uint64_t* first,
                            uint64_t steps_total, uint8_t* out, uint64_t out_len) {
  const uint32_t S = cbor_emit_tile_steps(sh.tau);
  const uint64_t tiles = cbor_emit_tiles(sh.t, S), bgrid = grid_of(sh.B);
  if (!grid_fits(bgrid) || (sh.t && !grid_fits(tiles))) return hipErrorInvalidValue;
  const CborEmitScans sc{pre, blen, first, steps_total};
  if (sh.t) {
    hipLaunchKernelGGL(k_cbor_emit_steps, dim3((uint32_t)tiles), dim3(CE_THREADS), 0, st, sh, A, S, offs, sc, out, out_len);
    if (const hipError_t e = hipGetLastError(); e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(k_cbor_emit_blocks, dim3((uint32_t)bgrid), dim3(CE_THREADS), 0, st, sh, T, sc, out, out_len);
  return hipGetLastError();
}

}  // namespace sezkp
