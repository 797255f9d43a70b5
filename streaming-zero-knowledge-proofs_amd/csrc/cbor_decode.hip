// cbor_decode.hip — CBOR bytes to the four step arrays on the device (gfx950):
// a TraceFile (sezkp_ctx_upload_trace_cbor / sezkp_ctx_decode_trace_cbor) and a
// block file, Vec<BlockSummary>, which has block tables besides
// (sezkp_ctx_ingest_blocks_cbor / sezkp_ctx_decode_blocks_cbor). A TraceFile's
// step records are a block file's, so its decoder is the block decoder's step
// half: the same mark, scan and compact kernels at one signature kind where
// the block file has two, and one parse pass where it has three.
//
// The file's bytes lie in device memory; trace_cbor_plan.h and
// blocks_cbor_plan.h hold the canonical forms, the strict parsers, the tiling,
// the chain argument and the body of every per-index pass, so a kernel here is
// its index and one call. On one stream:
//   k_cbor_marks<KINDS, false>  per tile of 4096 bytes: how many positions
//                               start A2 68 "input_mv" (step candidates) and,
//                               at KINDS = 2, AE 67 "version" (block candidates);
//   k_cbor_tile_scan            one workgroup, once per kind: the exclusive scan
//                               of the tile counts and the number of candidates
//                               (cbor_scan_dev.h, shared with the encoder);
//   k_cbor_marks<KINDS, true>   the same marks again, now stored in file order
//                               (the first cap of each kind): wave64 ballots
//                               and popcounts give a lane its place in the
//                               wave, four words of LDS a wave its place in
//                               the tile, the scan the tile's place;
// then for a TraceFile
//   k_cbor_parse                one lane per step candidate: the step, strictly,
//                               into row i, and its link of the chain;
// and for a block file
//   k_cbor_block_heads          one lane per block candidate: the head, strictly,
//                               into the tables' row k, with n_k and steps_off_k;
//   k_cbor_tile_scan            over n_k: step_start on the device, t in the verdict;
//   k_cbor_block_steps          one lane per step candidate below t: the step,
//                               strictly, into row i; its end; its link;
//   k_cbor_block_chain          one lane per block: the first step at steps_off_k,
//                               the tail behind the last one up to the next block.
// Nothing here decides: the verdict words go home and the host accepts the
// arrays or runs its own decoder (ctx_cbor.cpp). Every read of the file goes
// through cbor_at / cbor_load16, which never read at or past len; every index
// into a candidate or row array is below the count the array was sized by.
#include <hip/hip_runtime.h>

#include "blocks_cbor_plan.h"
#include "cbor_scan_dev.h"
#include "sezkp_internal.h"

namespace sezkp {

constexpr int TC_THREADS = (int)TRACE_CBOR_THREADS;
static_assert(TC_THREADS == 256 && TRACE_CBOR_LANE_BYTES == 16, "four waves of 64 lanes, one 16-byte load per lane");

// the first failure by index: a 64-bit atomic minimum, taken only by lanes that fail
struct AtomicMin {
  __device__ void operator()(uint64_t* word, uint64_t i) const {
    atomicMin(reinterpret_cast<unsigned long long*>(word), (unsigned long long)i);
  }
};

// per kind: the tile counts (count pass), their scan and the candidates with
// their cap (store pass)
template <int KINDS>
struct CborMarkArgs {
  uint32_t* counts[KINDS];
  const uint64_t* offs[KINDS];
  uint64_t* cand[KINDS];
  uint64_t cap[KINDS];
};

// A lane's 16 positions hold at most two candidates of a kind
// (cbor_lane_marks). Two ballots per kind (one or more, two) count and place them.
template <int KINDS, bool STORE>
__global__ void __launch_bounds__(TC_THREADS) k_cbor_marks(CborSpan s, uint64_t lo, CborMarkArgs<KINDS> a) {
  __shared__ uint32_t sh[KINDS][TC_THREADS / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint64_t pos = (uint64_t)blockIdx.x * TRACE_CBOR_TILE + (uint64_t)threadIdx.x * TRACE_CBOR_LANE_BYTES;
  uint32_t m[KINDS];
  cbor_lane_marks<KINDS>(s, lo, pos, m);
  unsigned long long b1[KINDS], b2[KINDS];
#pragma unroll
  for (int q = 0; q < KINDS; q++) {
    const uint32_t c = (uint32_t)__popc(m[q]);
    b1[q] = __ballot(c >= 1);
    b2[q] = __ballot(c >= 2);
    if (lane == 0) sh[q][wave] = (uint32_t)(__popcll(b1[q]) + __popcll(b2[q]));
  }
  __syncthreads();
  if constexpr (!STORE) {
    if (threadIdx.x == 0) {
#pragma unroll
      for (int q = 0; q < KINDS; q++) a.counts[q][blockIdx.x] = sh[q][0] + sh[q][1] + sh[q][2] + sh[q][3];
    }
  } else {
    const unsigned long long below = (1ull << lane) - 1ull;
#pragma unroll
    for (int q = 0; q < KINDS; q++) {
      if (!m[q]) continue;
      uint32_t before = 0;
#pragma unroll
      for (int w = 0; w < TC_THREADS / 64; w++)
        if (w < wave) before += sh[q][w];
      const uint64_t idx = a.offs[q][blockIdx.x] + before + (uint64_t)(__popcll(b1[q] & below) + __popcll(b2[q] & below));
      cbor_store_marks(m[q], pos, idx, a.cand[q], a.cap[q]);
    }
  }
}

__global__ void __launch_bounds__(TC_THREADS) k_cbor_parse(CborSpan s, uint64_t lo, const uint64_t* __restrict__ cand,
                                                           uint64_t t, uint32_t tau, int8_t* __restrict__ input_mv,
                                                           int8_t* __restrict__ mv, uint8_t* __restrict__ has_write,
                                                           uint16_t* __restrict__ wsym, TraceCborVerdict* V) {
  const uint64_t i = (uint64_t)blockIdx.x * TC_THREADS + threadIdx.x;
  trace_cbor_step_pass(s, lo, cand, t, tau, input_mv, mv, has_write, wsym, V, i, AtomicMin{});
}

__global__ void __launch_bounds__(TC_THREADS) k_cbor_block_heads(CborSpan s, uint64_t lo,
                                                                 const uint64_t* __restrict__ cand_b, uint64_t B,
                                                                 uint32_t tau, BlocksCborTables T, BlocksCborVerdict* V) {
  const uint64_t k = (uint64_t)blockIdx.x * TC_THREADS + threadIdx.x;
  blocks_cbor_head_pass(s, lo, cand_b, B, tau, T, V, k, AtomicMin{});
}

__global__ void __launch_bounds__(TC_THREADS)
    k_cbor_block_steps(CborSpan s, const uint64_t* __restrict__ cand_s, uint64_t t_max, uint64_t B,
                       const uint64_t* __restrict__ step_start, uint32_t tau, int8_t* __restrict__ input_mv,
                       int8_t* __restrict__ mv, uint8_t* __restrict__ has_write, uint16_t* __restrict__ wsym,
                       uint64_t* __restrict__ ends, BlocksCborVerdict* V) {
  const uint64_t i = (uint64_t)blockIdx.x * TC_THREADS + threadIdx.x;
  blocks_cbor_step_pass(s, cand_s, t_max, B, step_start, tau, input_mv, mv, has_write, wsym, ends, V, i, AtomicMin{});
}

__global__ void __launch_bounds__(TC_THREADS)
    k_cbor_block_chain(CborSpan s, const uint64_t* __restrict__ cand_b, const uint64_t* __restrict__ cand_s,
                       uint64_t t_max, uint64_t B, uint32_t tau, BlocksCborTables T, const uint64_t* __restrict__ ends,
                       BlocksCborVerdict* V) {
  const uint64_t k = (uint64_t)blockIdx.x * TC_THREADS + threadIdx.x;
  blocks_cbor_chain_pass(s, cand_b, cand_s, t_max, B, tau, T, ends, V, k, AtomicMin{});
}

static uint64_t grid_of(uint64_t n) { return (n + TC_THREADS - 1) / TC_THREADS; }
static bool grids_fit(std::initializer_list<uint64_t> grids) {
  for (uint64_t g : grids)
    if (!g || g > 0x7FFFFFFFull) return false;
  return true;
}
// mark, scan and compact: the first cap[q] candidates of each kind from lo on
// into cand[q], the number of all of them into *total[q]. Nothing is launched
// behind a scan that failed to launch.
template <int KINDS>
static hipError_t mark_and_compact(hipStream_t st, const CborSpan& s, uint64_t lo, uint64_t ntiles, uint32_t* const* counts,
                                   uint64_t* const* offs, uint64_t* const* cand, const uint64_t* cap,
                                   uint64_t* const* total) {
  CborMarkArgs<KINDS> a{};
  for (int q = 0; q < KINDS; q++) a.counts[q] = counts[q], a.cap[q] = cap[q];
  hipLaunchKernelGGL((k_cbor_marks<KINDS, false>), dim3((uint32_t)ntiles), dim3(TC_THREADS), 0, st, s, lo, a);
  for (int q = KINDS; q-- > 0;) {
    if (const hipError_t e = cbor_scan(st, counts[q], ntiles, offs[q], total[q]); e != hipSuccess) return e;
    a.counts[q] = nullptr, a.offs[q] = offs[q], a.cand[q] = cand[q];
  }
  hipLaunchKernelGGL((k_cbor_marks<KINDS, true>), dim3((uint32_t)ntiles), dim3(TC_THREADS), 0, st, s, lo, a);
  return hipSuccess;
}

// counts / offs: trace_cbor_tiles(len) words each; cand: t words; the arrays:
// t and t * tau elements. t >= 1 and t <= len / cbor_step_min_len(tau)
// (trace_cbor_head), d_bytes on a 16-byte boundary.
hipError_t launch_trace_cbor_decode(hipStream_t st, const uint8_t* d_bytes, uint64_t len, uint64_t steps_off, uint64_t t,
                                    uint32_t tau, uint32_t* counts, uint64_t* offs, uint64_t* cand, int8_t* input_mv,
                                    int8_t* mv, uint8_t* has_write, uint16_t* wsym, TraceCborVerdict* verdict) {
  const uint64_t ntiles = trace_cbor_tiles(len), pgrid = grid_of(t);
  if (!grids_fit({ntiles, pgrid}) || (reinterpret_cast<uintptr_t>(d_bytes) & 15u)) return hipErrorInvalidValue;
  const CborSpan s{d_bytes, len};
  hipError_t e = hipMemsetAsync(verdict, 0xFF, sizeof(TraceCborVerdict), st);
  if (e != hipSuccess) return e;
  uint64_t* const total = &verdict->candidates;
  if ((e = mark_and_compact<1>(st, s, steps_off, ntiles, &counts, &offs, &cand, &t, &total)) != hipSuccess) return e;
  hipLaunchKernelGGL(k_cbor_parse, dim3((uint32_t)pgrid), dim3(TC_THREADS), 0, st, s, steps_off, cand, t, tau, input_mv,
                     mv, has_write, wsym, verdict);
  return hipGetLastError();
}

// counts / offs / cand by kind (0: steps, 1: blocks): trace_cbor_tiles(len)
// words each for counts and offs; cand[0] and ends: t_max words; cand[1]: B
// words; the arrays: t_max and t_max * tau elements; T: the tables of B blocks
// in device memory. B >= 1, t_max >= 1 (blocks_cbor_head), d_bytes on a
// 16-byte boundary.
hipError_t launch_blocks_cbor_decode(hipStream_t st, const uint8_t* d_bytes, uint64_t len, uint64_t first_off,
                                     uint64_t B, uint32_t tau, uint64_t t_max, uint32_t* const counts[2],
                                     uint64_t* const offs[2], uint64_t* const cand[2], uint64_t* ends,
                                     const BlocksCborTables& T, int8_t* input_mv, int8_t* mv, uint8_t* has_write,
                                     uint16_t* wsym, BlocksCborVerdict* verdict) {
  const uint64_t ntiles = trace_cbor_tiles(len), bgrid = grid_of(B), sgrid = grid_of(t_max);
  if (!grids_fit({ntiles, bgrid, sgrid}) || (reinterpret_cast<uintptr_t>(d_bytes) & 15u)) return hipErrorInvalidValue;
  const CborSpan s{d_bytes, len};
  hipError_t e = hipMemsetAsync(verdict, 0xFF, sizeof(BlocksCborVerdict), st);
  if (e != hipSuccess) return e;
  const uint64_t cap[2] = {t_max, B};
  uint64_t* const total[2] = {&verdict->step_candidates, &verdict->block_candidates};
  if ((e = mark_and_compact<2>(st, s, first_off, ntiles, counts, offs, cand, cap, total)) != hipSuccess) return e;
  hipLaunchKernelGGL(k_cbor_block_heads, dim3((uint32_t)bgrid), dim3(TC_THREADS), 0, st, s, first_off, cand[1], B, tau, T,
                     verdict);
  if ((e = cbor_scan(st, T.n_steps, B, T.step_start, &verdict->t)) != hipSuccess) return e;
  hipLaunchKernelGGL(k_cbor_block_steps, dim3((uint32_t)sgrid), dim3(TC_THREADS), 0, st, s, cand[0], t_max, B,
                     T.step_start, tau, input_mv, mv, has_write, wsym, ends, verdict);
  hipLaunchKernelGGL(k_cbor_block_chain, dim3((uint32_t)bgrid), dim3(TC_THREADS), 0, st, s, cand[1], cand[0], t_max, B, tau,
                     T, ends, verdict);
  return hipGetLastError();
}

}  // namespace sezkp
