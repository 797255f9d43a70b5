// trace_plan.h — what the host and the device must agree on when a trace is
// uploaded as a raw movement log (sezkp_ctx_upload_trace) and partitioned on
// the device (partition.hip): the uniform block boundaries of partition_trace
// (partition.rs:43-150), the manifest leaf message (sezkp-merkle lib.rs:85-117),
// the tiling of the input-head scan and the condition under which the device
// hashes the leaves. Plain C++, no HIP type: tools/trace_plan_check.cpp prints
// all of it on a machine without a GPU, as tools/prove_plan_check.cpp does for
// prove_plan.h.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define TRACE_PLAN_HD __host__ __device__
#else
#define TRACE_PLAN_HD
#endif

namespace sezkp {

// ------------------------------------------------------------ block shape
// partition_trace cuts a trace of t steps into blocks of b steps: block k
// covers rows [k b, min((k + 1) b, t)) (partition.rs:60-66).
TRACE_PLAN_HD inline uint64_t trace_nblk(uint64_t t, uint64_t b) { return b ? (t + b - 1) / b : 0; }
TRACE_PLAN_HD inline uint64_t trace_step_start(uint64_t k, uint64_t t, uint64_t b) {
  // k <= nblk <= t, b <= 2^32: no overflow for t <= 2^32; larger t saturates
  const uint64_t lim = b ? t / b : 0;
  return k > lim ? t : (k * b < t ? k * b : t);
}

// ------------------------------------------------------------ sharded traces
// Rank g of P = 2^logP commits the column chunks shard_range (prove_plan.h)
// gives it and reads the whole blocks over their rows [r0, r1] (r1: the halo
// row). With uniform boundaries the block of a row is row / b, so a rank's
// rows and blocks follow from (t, b) alone, without a step_start array.
// Rank g OWNS block k exactly when the block's first row k b lies in the
// rank's own rows [r0, r_end): every block has one owner, the owner holds all
// of the block's rows (k b >= r0, and the block ends at or before the end of
// the block of r1), and a rank whose rows start no block owns none. The owner
// sums the block's input_mv and hashes its manifest leaf (partition.hip).
constexpr int TRACE_SHARD_CHUNK_LOG2 = 10;  // = COL_CHUNK_LOG2 (prover_ctx.h asserts it)
struct TraceShard {
  uint64_t row0 = 0, nrows = 0;       // the rows the rank reads (whole blocks): sezkp_shard_rows
  uint32_t blk_lo = 0, blk_cnt = 0;   // the blocks it reads
  uint32_t own_lo = 0, own_cnt = 0;   // the blocks it owns (inside the read range)
};
// false: a shape the sharded prover does not take (the caller's SEZKP_E_INVALID)
inline bool trace_shard_plan(uint64_t t, uint64_t b, int64_t rank, int64_t world, TraceShard& s) {
  if (b == 0 || b > 0xFFFFFFFFull || t == 0 || (t & (t - 1)) != 0) return false;
  if (world != 1 && world != 2 && world != 4 && world != 8) return false;
  if (rank < 0 || rank >= world) return false;
  if (world > 1 && t < 4096ull * (uint64_t)world) return false;
  if (trace_nblk(t, b) > 0xFFFFFFFFull) return false;
  const uint64_t chunk_rows = t < (1ull << TRACE_SHARD_CHUNK_LOG2) ? t : 1ull << TRACE_SHARD_CHUNK_LOG2;
  const uint64_t per_rank = (t / chunk_rows) / (uint64_t)world;  // chunks per rank
  const uint64_t r0 = per_rank * (uint64_t)rank * chunk_rows, r_end = r0 + per_rank * chunk_rows;
  const uint64_t r1 = r_end < t - 1 ? r_end : t - 1;
  const uint64_t lo = r0 / b, hi = r1 / b;
  s.blk_lo = (uint32_t)lo;
  s.blk_cnt = (uint32_t)(hi - lo + 1);
  s.row0 = trace_step_start(lo, t, b);
  s.nrows = trace_step_start(hi + 1, t, b) - s.row0;
  const uint64_t o0 = (r0 + b - 1) / b, o1 = (r_end + b - 1) / b;  // first blocks starting at or after r0 / r_end
  s.own_lo = (uint32_t)o0;
  s.own_cnt = (uint32_t)(o1 - o0);
  return true;
}

// ------------------------------------------------------------ input-head scan
// in_head_in / in_head_out are the exclusive / inclusive prefix sums of the
// blocks' input_mv sums, exact in i64. Three launches: every tile of
// TRACE_SCAN_TILE consecutive blocks is summed (k_inhead_tile_sums), one
// workgroup scans the tile sums (k_inhead_tile_scan), and every tile scans its
// own blocks from its offset (k_inhead_add). A workgroup of 256 lanes takes
// TRACE_SCAN_PER_LANE consecutive blocks per lane.
constexpr uint32_t TRACE_SCAN_THREADS = 256;
constexpr uint32_t TRACE_SCAN_PER_LANE = 4;
constexpr uint32_t TRACE_SCAN_TILE = TRACE_SCAN_THREADS * TRACE_SCAN_PER_LANE;  // 1024 blocks
TRACE_PLAN_HD inline uint64_t trace_scan_tiles(uint64_t nblk) { return (nblk + TRACE_SCAN_TILE - 1) / TRACE_SCAN_TILE; }
// blocks [lo, hi) of tile `tile`
TRACE_PLAN_HD inline void trace_scan_tile_range(uint64_t tile, uint64_t nblk, uint64_t& lo, uint64_t& hi) {
  lo = tile * TRACE_SCAN_TILE;
  hi = lo + TRACE_SCAN_TILE < nblk ? lo + TRACE_SCAN_TILE : nblk;
  if (lo > nblk) lo = nblk;
}
// a block's input_mv sum: one lane per block below this many rows per block,
// one wave per block from it on (k_inhead_block_sums)
constexpr uint32_t TRACE_SUM_WAVE_ROWS = 64;

// ------------------------------------------------------------ manifest leaf
// leaf_hash (lib.rs:85-117) hashes these little-endian fields back to back:
//   u16 version, u32 block_id, u64 step_lo, u64 step_hi, u16 ctrl_in,
//   u16 ctrl_out, i64 in_head_in, i64 in_head_out, u64 tau,
//   tau x (i64 left, i64 right), tau x u32 head_in_offset,
//   tau x u32 head_out_offset, u64 steps
// 58 + 24 tau bytes. For a partitioned trace version = 1, block_id = k + 1,
// step_lo = k b + 1, step_hi = the block's end row, ctrl_in = ctrl_out = 0.
// Every field starts at an offset that is 2 mod 4, so the message is best seen
// as 29 + 12 tau 16-bit halves (manifest_leaf_half).
TRACE_PLAN_HD inline uint32_t manifest_leaf_len(uint32_t tau) { return 58u + 24u * tau; }
// The device hashes a leaf as one BLAKE3 chunk (b3_chunk_block, dev_common.h):
// the message must fit 1024 bytes, tau <= 40. Above that the host hashes the
// leaves from the metadata image that comes home; same bytes, same hashes.
constexpr uint32_t MANIFEST_LEAF_DEV_MAX_TAU = 40;
TRACE_PLAN_HD inline bool manifest_leaf_on_device(uint32_t tau) { return manifest_leaf_len(tau) <= 1024u; }

// Block k's fields as the metadata image holds them ([nblk][tau] rows).
struct LeafFields {
  uint64_t k, t, b;
  uint32_t tau;
  int64_t in_head_in, in_head_out;
  const int64_t* win_left;   // [tau] of this block
  const int64_t* win_right;  // [tau]
  const uint32_t* off_in;    // [tau]
  const uint32_t* off_out;   // [tau]
};
TRACE_PLAN_HD inline uint32_t leaf_half_of(uint64_t x, uint32_t part) { return (uint32_t)(x >> (16 * part)) & 0xFFFFu; }
// 16-bit half i (little endian: bytes 2 i, 2 i + 1) of the leaf message
TRACE_PLAN_HD inline uint32_t manifest_leaf_half(const LeafFields& f, uint32_t i) {
  const uint64_t lo = trace_step_start(f.k, f.t, f.b), hi = trace_step_start(f.k + 1, f.t, f.b);
  if (i == 0) return 1u;                                              // version
  if (i < 3) return leaf_half_of(f.k + 1, i - 1);                     // block_id
  if (i < 7) return leaf_half_of(lo + 1, i - 3);                      // step_lo (1-based)
  if (i < 11) return leaf_half_of(hi, i - 7);                         // step_hi (inclusive)
  if (i < 13) return 0u;                                              // ctrl_in, ctrl_out
  if (i < 17) return leaf_half_of((uint64_t)f.in_head_in, i - 13);
  if (i < 21) return leaf_half_of((uint64_t)f.in_head_out, i - 17);
  if (i < 25) return leaf_half_of(f.tau, i - 21);
  uint32_t j = i - 25;
  if (j < 8 * f.tau) {
    const uint32_t r = j >> 3;
    return leaf_half_of((uint64_t)((j & 4) ? f.win_right[r] : f.win_left[r]), j & 3);
  }
  j -= 8 * f.tau;
  if (j < 2 * f.tau) return leaf_half_of(f.off_in[j >> 1], j & 1);
  j -= 2 * f.tau;
  if (j < 2 * f.tau) return leaf_half_of(f.off_out[j >> 1], j & 1);
  j -= 2 * f.tau;
  return j < 4 ? leaf_half_of(hi - lo, j) : 0u;                       // steps; 0 past the end (padding)
}
// the message bytes (manifest_leaf_len(tau) of them)
inline void manifest_leaf_message(const LeafFields& f, uint8_t* out) {
  const uint32_t halves = manifest_leaf_len(f.tau) / 2;
  for (uint32_t i = 0; i < halves; i++) {
    const uint32_t h = manifest_leaf_half(f, i);
    out[2 * i] = (uint8_t)h;
    out[2 * i + 1] = (uint8_t)(h >> 8);
  }
}

}  // namespace sezkp
