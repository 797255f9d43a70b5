// blocks_cbor.hip — block-file CBOR bytes (Vec<BlockSummary>) to the block
// tables and the four step arrays on the device (gfx950), for
// sezkp_ctx_ingest_blocks_cbor / sezkp_ctx_decode_blocks_cbor.
//
// The file's bytes lie in device memory; blocks_cbor_plan.h holds the
// canonical form, the strict parsers and the chain argument, trace_cbor_plan.h
// the tiling and the step parser. On one stream:
//   k_blocks_marks<false>  per tile of 4096 bytes: how many positions start
//                          AE 67 "version" (block candidates) and how many
//                          A2 68 "input_mv" (step candidates);
//   tile scan (x2)         trace_cbor.hip's one-workgroup scan, per kind;
//   k_blocks_marks<true>   the same marks again, stored in file order (the
//                          first B and the first t_max of them);
//   k_blocks_heads         one lane per block candidate: the head, strictly,
//                          into the tables' row k, with n_k and steps_off_k;
//   tile scan              over n_k: step_start on the device, t in the verdict;
//   k_blocks_steps         one lane per step candidate below t: the step,
//                          strictly, into row i; its end; its link;
//   k_blocks_chain         one lane per block: the first step at steps_off_k,
//                          the tail behind the last one up to the next block.
// Nothing here decides: the verdict words go home and the host accepts the
// arrays or runs its own decoder (ctx_blocks_cbor.cpp). Every read of the file
// goes through cbor_at / cbor_load16, which never read at or past len; every
// index into a candidate or row array is below the count the array was sized by.
#include <hip/hip_runtime.h>

#include "blocks_cbor_plan.h"
#include "sezkp_internal.h"

namespace sezkp {

constexpr int BC_THREADS = (int)TRACE_CBOR_THREADS;
static_assert(BC_THREADS == 256 && TRACE_CBOR_LANE_BYTES == 16, "four waves of 64 lanes, one 16-byte load per lane");
static_assert(BLOCKS_CBOR_SIG_LEN >= 9 && TRACE_CBOR_SIG_LEN >= 9, "at most two candidates of a kind in 16 positions");

__device__ __forceinline__ unsigned long long* u64a(uint64_t* p) { return reinterpret_cast<unsigned long long*>(p); }

// A signature's first byte occurs nowhere else in it, so two candidates of one
// kind lie at least 9 positions apart: a lane's 16 positions hold at most two
// of each. Two ballots per kind (one or more, two) count and place them.
template <bool STORE>
__global__ void __launch_bounds__(BC_THREADS)
    k_blocks_marks(CborSpan s, uint64_t lo, uint32_t* __restrict__ counts_b, uint32_t* __restrict__ counts_s,
                   const uint64_t* __restrict__ offs_b, const uint64_t* __restrict__ offs_s,
                   uint64_t* __restrict__ cand_b, uint64_t* __restrict__ cand_s, uint64_t cap_b, uint64_t cap_s) {
  __shared__ uint32_t sh[2][BC_THREADS / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint64_t pos = (uint64_t)blockIdx.x * TRACE_CBOR_TILE + (uint64_t)threadIdx.x * TRACE_CBOR_LANE_BYTES;
  uint32_t m[2] = {0u, 0u};
  if (pos < s.len) {
    const Cbor16 a = cbor_load16(s, pos), b = cbor_load16(s, pos + 16);
    m[0] = cbor_block_sig_mask(a, b);
    m[1] = cbor_sig_mask(a, b);
    if (pos < lo) {
      const uint32_t keep = lo - pos >= 16 ? 0u : (0xFFFFu << (uint32_t)(lo - pos)) & 0xFFFFu;
      m[0] &= keep;
      m[1] &= keep;
    }
  }
  unsigned long long b1[2], b2[2];
#pragma unroll
  for (int q = 0; q < 2; q++) {
    const uint32_t c = (uint32_t)__popc(m[q]);
    b1[q] = __ballot(c >= 1);
    b2[q] = __ballot(c >= 2);
    if (lane == 0) sh[q][wave] = (uint32_t)(__popcll(b1[q]) + __popcll(b2[q]));
  }
  __syncthreads();
  if constexpr (!STORE) {
    if (threadIdx.x == 0) {
      counts_b[blockIdx.x] = sh[0][0] + sh[0][1] + sh[0][2] + sh[0][3];
      counts_s[blockIdx.x] = sh[1][0] + sh[1][1] + sh[1][2] + sh[1][3];
    }
  } else {
    const unsigned long long below = (1ull << lane) - 1ull;
#pragma unroll
    for (int q = 0; q < 2; q++) {
      if (!m[q]) continue;
      uint32_t before = 0;
#pragma unroll
      for (int w = 0; w < BC_THREADS / 64; w++)
        if (w < wave) before += sh[q][w];
      uint64_t idx = (q ? offs_s : offs_b)[blockIdx.x] + before +
                     (uint64_t)(__popcll(b1[q] & below) + __popcll(b2[q] & below));
      uint64_t* cand = q ? cand_s : cand_b;
      const uint64_t cap = q ? cap_s : cap_b;
      uint32_t rest = m[q];
      while (rest) {
        const uint32_t bit = (uint32_t)__ffs((int)rest) - 1u;
        rest &= rest - 1u;
        if (idx < cap) cand[idx] = pos + bit;
        idx++;
      }
    }
  }
}

// Block k's head from block candidate k. With fewer than B candidates nothing
// is parsed (the host declines on the count), but n_k is written all the same:
// the scan reads all B of them.
__global__ void __launch_bounds__(BC_THREADS) k_blocks_heads(CborSpan s, uint64_t lo, const uint64_t* __restrict__ cand_b,
                                                             uint64_t B, uint32_t tau, BlocksCborTables T,
                                                             BlocksCborVerdict* V) {
  const uint64_t k = (uint64_t)blockIdx.x * BC_THREADS + threadIdx.x;
  if (k >= B) return;
  if (V->block_candidates < B) {
    T.n_steps[k] = 0;
    T.steps_off[k] = 0;
    return;
  }
  const uint64_t c = cand_b[k], o = k * tau;
  BlockCborHead h{};
  uint64_t end = cbor_parse_block_head(s, c, tau, false, h, T.win_left + o, T.win_right + o, T.off_in + o, T.off_out + o);
  if (k == 0 && c != lo) end = 0;
  blocks_cbor_store_head(T, k, h, end);
  if (!end) atomicMin(u64a(&V->bad_head), (unsigned long long)k);
}

// Step i from step candidate i, its end, and its link: step i + 1 starts where
// step i ends unless it is the first of a block (then k_blocks_chain checks
// both sides). The search through step_start runs only for lanes at a
// mismatch: B - 1 of them in a canonical file.
__global__ void __launch_bounds__(BC_THREADS)
    k_blocks_steps(CborSpan s, const uint64_t* __restrict__ cand_s, uint64_t t_max, uint64_t B,
                   const uint64_t* __restrict__ step_start, uint32_t tau, int8_t* __restrict__ input_mv,
                   int8_t* __restrict__ mv, uint8_t* __restrict__ has_write, uint16_t* __restrict__ wsym,
                   uint64_t* __restrict__ ends, BlocksCborVerdict* V) {
  const uint64_t i = (uint64_t)blockIdx.x * BC_THREADS + threadIdx.x;
  const uint64_t t = V->t;
  if (V->block_candidates < B || V->bad_head != ~0ull || t > t_max || V->step_candidates < t || i >= t) return;
  const uint64_t c = cand_s[i], o = i * tau;
  const uint64_t end = cbor_parse_step(s, c, tau, input_mv + i, mv + o, has_write + o, wsym + o);
  ends[i] = end;
  if (!end) {
    atomicMin(u64a(&V->bad_step), (unsigned long long)i);
    return;
  }
  if (i + 1 < t && cand_s[i + 1] != end) {
    const uint64_t k = blocks_cbor_block_of(step_start, B, i + 1);
    if (step_start[k] != i + 1) atomicMin(u64a(&V->bad_link), (unsigned long long)(i + 1));
  }
}

// Block k's two ends: its first step lies right behind its head, and behind
// its last step the tail runs up to the next block candidate (to len for the
// last block).
__global__ void __launch_bounds__(BC_THREADS)
    k_blocks_chain(CborSpan s, const uint64_t* __restrict__ cand_b, const uint64_t* __restrict__ cand_s, uint64_t t_max,
                   uint64_t B, uint32_t tau, BlocksCborTables T, const uint64_t* __restrict__ ends,
                   BlocksCborVerdict* V) {
  const uint64_t k = (uint64_t)blockIdx.x * BC_THREADS + threadIdx.x;
  const uint64_t t = V->t;
  if (V->block_candidates < B || V->bad_head != ~0ull || t > t_max || V->step_candidates < t || k >= B) return;
  const uint64_t a = T.step_start[k], n = T.n_steps[k];  // n >= 1, a + n <= t
  if (cand_s[a] != T.steps_off[k]) atomicMin(u64a(&V->bad_link), (unsigned long long)a);
  const uint64_t e = ends[a + n - 1];
  if (!e) return;  // the step did not parse: bad_step has it
  const uint64_t tail_end = cbor_parse_block_tail(s, e, tau);
  const uint64_t want = k + 1 < B ? cand_b[k + 1] : s.len;
  if (!tail_end || tail_end != want) atomicMin(u64a(&V->bad_tail), (unsigned long long)k);
}

// counts_* / offs_*: trace_cbor_tiles(len) words each; cand_b: B words; cand_s
// and ends: t_max words; the arrays: t_max and t_max * tau elements; T: the
// tables of B blocks in device memory. B >= 1, t_max >= 1 (blocks_cbor_head),
// d_bytes on a 16-byte boundary.
hipError_t launch_blocks_cbor_decode(hipStream_t st, const uint8_t* d_bytes, uint64_t len, uint64_t first_off,
                                     uint64_t B, uint32_t tau, uint64_t t_max, uint32_t* counts_b, uint32_t* counts_s,
                                     uint64_t* offs_b, uint64_t* offs_s, uint64_t* cand_b, uint64_t* cand_s,
                                     uint64_t* ends, const BlocksCborTables& T, int8_t* input_mv, int8_t* mv,
                                     uint8_t* has_write, uint16_t* wsym, BlocksCborVerdict* verdict) {
  const uint64_t ntiles = trace_cbor_tiles(len), bgrid = (B + BC_THREADS - 1) / BC_THREADS,
                 sgrid = (t_max + BC_THREADS - 1) / BC_THREADS;
  if (!B || !t_max || !ntiles || ntiles > 0x7FFFFFFFull || bgrid > 0x7FFFFFFFull || sgrid > 0x7FFFFFFFull)
    return hipErrorInvalidValue;
  if (reinterpret_cast<uintptr_t>(d_bytes) & 15u) return hipErrorInvalidValue;
  const CborSpan s{d_bytes, len};
  hipError_t e = hipMemsetAsync(verdict, 0xFF, sizeof(BlocksCborVerdict), st);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_blocks_marks<false>, dim3((uint32_t)ntiles), dim3(BC_THREADS), 0, st, s, first_off, counts_b,
                     counts_s, nullptr, nullptr, nullptr, nullptr, B, t_max);
  if ((e = launch_cbor_tile_scan(st, counts_b, ntiles, offs_b, &verdict->block_candidates)) != hipSuccess) return e;
  if ((e = launch_cbor_tile_scan(st, counts_s, ntiles, offs_s, &verdict->step_candidates)) != hipSuccess) return e;
  hipLaunchKernelGGL(k_blocks_marks<true>, dim3((uint32_t)ntiles), dim3(BC_THREADS), 0, st, s, first_off, nullptr,
                     nullptr, offs_b, offs_s, cand_b, cand_s, B, t_max);
  hipLaunchKernelGGL(k_blocks_heads, dim3((uint32_t)bgrid), dim3(BC_THREADS), 0, st, s, first_off, cand_b, B, tau, T,
                     verdict);
  if ((e = launch_cbor_tile_scan(st, T.n_steps, B, T.step_start, &verdict->t)) != hipSuccess) return e;
  hipLaunchKernelGGL(k_blocks_steps, dim3((uint32_t)sgrid), dim3(BC_THREADS), 0, st, s, cand_s, t_max, B, T.step_start,
                     tau, input_mv, mv, has_write, wsym, ends, verdict);
  hipLaunchKernelGGL(k_blocks_chain, dim3((uint32_t)bgrid), dim3(BC_THREADS), 0, st, s, cand_b, cand_s, t_max, B, tau, T,
                     ends, verdict);
  return hipGetLastError();
}

}  // namespace sezkp
