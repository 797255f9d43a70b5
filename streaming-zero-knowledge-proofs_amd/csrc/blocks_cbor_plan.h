// blocks_cbor_plan.h — what the host and the device agree on when a block file
// (Vec<BlockSummary> as CBOR, sezkp-core io.rs:57-65, types.rs:116-151) is
// decoded from its bytes on the device (cbor_decode.hip,
// sezkp_ctx_ingest_blocks_cbor): the canonical form, the strict parsers of a
// block's head and tail, the head check, and the body of the heads, steps and
// chain passes. Plain C++, no HIP type: tools/cbor_check.cpp calls the same
// passes index by index under the sanitizers on a machine without a GPU. The
// accessors, both signatures, the mark passes, the integer heads and the step
// parser are trace_cbor_plan.h's: a TraceFile's decoder is this one's step
// half.
//
// The canonical form is what ciborium and encode_blocks_cbor write:
//   file   array(B) head, B >= 1
//   block  AE | 67 "version" uint<=u16 | 68 "block_id" uint<=u32 | 67 "step_lo" uint | 67 "step_hi" uint |
//          67 "ctrl_in" uint<=u16 | 68 "ctrl_out" uint<=u16 | 6A "in_head_in" int(i64) | 6B "in_head_out" int(i64) |
//          67 "windows" array(tau) x (A2 | 64 "left" int(i64) | 65 "right" int(i64)) |
//          6F "head_in_offsets" array(tau) x uint<=u32 | 70 "head_out_offsets" array(tau) x uint<=u32 |
//          6C "movement_log" | A1 | 65 "steps" | array(n_k), n_k >= 1 | n_k x step (trace_cbor_plan.h) |
//          68 "pre_tags" array(tau) x (90 | 16 x uint<=255) | 69 "post_tags" the same
//   end    the last block's tail ends at len
// with every integer in its minimal-length head and inside its field's type
// (the host decoder casts what is outside; the device declines it, so the
// host answers). tau <= 255 is block 0's window count.
//
// The decode (index by index in the check tool, one kernel each on the device):
//   mark     every position from first_off on that starts AE 67 "version" is
//            a block candidate, every one that starts A2 68 "input_mv" a step
//            candidate; the first B and the first t_max in file order are stored;
//   heads    block candidate k is parsed strictly as a block's head, up to
//            and with the head of its steps array: the block tables' row k,
//            n_k and steps_off_k (the first byte behind that array head);
//   scan     S = the exclusive scan of n_k, t = S_B;
//   steps    step candidate i < t is parsed strictly as a whole step into row
//            i; end_i is where it ends. A step whose successor candidate is
//            not at its end must be the last of its block (i + 1 is some S_k);
//   chain    per block k: candidate 0 is first_off; step candidate S_k is
//            steps_off_k; behind the end of step S_k + n_k - 1 the tail parses
//            strictly and ends at block candidate k + 1 (at len for k = B - 1).
// When all of it holds, a sequential parse visits exactly these offsets: it
// starts block 0 at first_off, walks block k's head to steps_off_k = c[S_k],
// its n_k steps link by link, its tail to block candidate k + 1, and ends at
// len. So the tables and the rows are the host decoder's. Nothing on the
// device decides: the verdict words go home and the host accepts or runs
// decode_blocks_cbor, which alone reports errors.
#pragma once
#include "trace_cbor_plan.h"

namespace sezkp {

// ------------------------------------------------------------ strict items
// a text key of n <= 16 bytes (head byte included), little endian in lo | hi
TRACE_CBOR_HD inline bool cbor_key(const CborSpan& s, uint64_t& pos, uint64_t lo, uint64_t hi, int n) {
  if (!cbor_match(s, pos, lo, n < 8 ? n : 8)) return false;
  if (n > 8 && !cbor_match(s, pos + 8, hi, n - 8)) return false;
  pos += (uint64_t)n;
  return true;
}
// an unsigned integer <= max, minimal, in at most max_bytes bytes
TRACE_CBOR_HD inline bool cbor_uint_max(const CborSpan& s, uint64_t& pos, int max_bytes, uint64_t max, uint64_t& out) {
  uint32_t mj, adv;
  uint64_t v;
  cbor_head_min(s, pos, max_bytes, mj, v, adv);
  if (!adv || mj != 0 || v > max) return false;
  out = v;
  pos += adv;
  return true;
}
// a signed integer of i64, minimal
TRACE_CBOR_HD inline bool cbor_int64(const CborSpan& s, uint64_t& pos, int64_t& out) {
  uint32_t mj, adv;
  uint64_t v;
  cbor_head_min(s, pos, 9, mj, v, adv);
  if (!adv || mj > 1 || v > 0x7FFFFFFFFFFFFFFFull) return false;
  out = mj ? -1 - (int64_t)v : (int64_t)v;
  pos += adv;
  return true;
}
// the head of an array of exactly n <= 255 items
TRACE_CBOR_HD inline bool cbor_array_of(const CborSpan& s, uint64_t& pos, uint32_t n) {
  if (n < 24) {
    if (cbor_at(s, pos) != (0x80u | n)) return false;
    pos += 1;
  } else {
    if (cbor_at(s, pos) != 0x98u || cbor_at(s, pos + 1) != n) return false;
    pos += 2;
  }
  return true;
}

// the keys, head byte first
constexpr uint64_t BK_VERSION = 0x6E6F697372657667ull;                                    // 67 "version"
constexpr uint64_t BK_BLOCK_ID_LO = 0x695F6B636F6C6268ull, BK_BLOCK_ID_HI = 0x64ull;      // 68 "block_id"
constexpr uint64_t BK_STEP_LO = 0x6F6C5F7065747367ull;                                    // 67 "step_lo"
constexpr uint64_t BK_STEP_HI = 0x69685F7065747367ull;                                    // 67 "step_hi"
constexpr uint64_t BK_CTRL_IN = 0x6E695F6C72746367ull;                                    // 67 "ctrl_in"
constexpr uint64_t BK_CTRL_OUT_LO = 0x756F5F6C72746368ull, BK_CTRL_OUT_HI = 0x74ull;      // 68 "ctrl_out"
constexpr uint64_t BK_IN_HEAD_IN_LO = 0x646165685F6E696Aull, BK_IN_HEAD_IN_HI = 0x6E695Full;      // 6A "in_head_in"
constexpr uint64_t BK_IN_HEAD_OUT_LO = 0x646165685F6E696Bull, BK_IN_HEAD_OUT_HI = 0x74756F5Full;  // 6B "in_head_out"
constexpr uint64_t BK_WINDOWS = 0x73776F646E697767ull;                                    // 67 "windows"
constexpr uint64_t BK_LEFT = 0x7466656C64A2ull;                                           // A2 | 64 "left"
constexpr uint64_t BK_RIGHT = 0x746867697265ull;                                          // 65 "right"
constexpr uint64_t BK_OFF_IN_LO = 0x6E695F646165686Full, BK_OFF_IN_HI = 0x7374657366666F5Full;    // 6F "head_in_offsets"
constexpr uint64_t BK_OFF_OUT_LO = 0x756F5F6461656870ull;                                 // 70 "head_ou"
constexpr uint64_t BK_OFF_OUT_HI = 0x7374657366666F5Full;                                 // "_offsets" (behind a 't')
constexpr uint64_t BK_MOVLOG_LO = 0x6E656D65766F6D6Cull, BK_MOVLOG_HI = 0x676F6C5F74ull;  // 6C "movement_log"
constexpr uint64_t BK_STEPS = 0x737065747365A1ull;                                        // A1 | 65 "steps"
constexpr uint64_t BK_PRE_TAGS_LO = 0x6761745F65727068ull, BK_PRE_TAGS_HI = 0x73ull;      // 68 "pre_tags"
constexpr uint64_t BK_POST_TAGS_LO = 0x61745F74736F7069ull, BK_POST_TAGS_HI = 0x7367ull;  // 69 "post_tags"

// what a block is long at the least (one step, every integer in one byte):
// bounds B by the file's length before anything is sized by it
TRACE_CBOR_HD inline uint64_t cbor_block_min_len(uint32_t tau) {
  const uint64_t h = tau < 24 ? 1u : 2u;
  return 1 + 9 + 10 + 9 + 9 + 9 + 10 + 12 + 13 + (8 + h + 14ull * tau) + (16 + h + tau) + (17 + h + tau) + 13 + 7 + 1 +
         cbor_step_min_len(tau) + (9 + h + 17ull * tau) + (10 + h + 17ull * tau);
}

// One block's head at pos, strictly, up to and with the head of its steps
// array: the offset behind that head (where the first step starts), or 0 at
// the first deviation. tau_any: the window count is read, not given (block 0,
// on the host); else it must be `tau`. win_left .. off_out: tau cells each, or
// null (the head check reads no array).
struct BlockCborHead {
  uint16_t version, ctrl_in, ctrl_out;
  uint32_t block_id, tau, n_steps;
  uint64_t step_lo, step_hi;
  int64_t in_head_in, in_head_out;
};
TRACE_CBOR_HD inline uint64_t cbor_parse_block_head(const CborSpan& s, uint64_t pos, uint32_t tau, bool tau_any,
                                                    BlockCborHead& h, int64_t* win_left, int64_t* win_right,
                                                    uint32_t* off_in, uint32_t* off_out) {
  uint64_t v;
  if (cbor_at(s, pos) != 0xAEu) return 0;
  pos += 1;
  if (!cbor_key(s, pos, BK_VERSION, 0, 8) || !cbor_uint_max(s, pos, 3, 0xFFFFu, v)) return 0;
  h.version = (uint16_t)v;
  if (!cbor_key(s, pos, BK_BLOCK_ID_LO, BK_BLOCK_ID_HI, 9) || !cbor_uint_max(s, pos, 5, 0xFFFFFFFFull, v)) return 0;
  h.block_id = (uint32_t)v;
  if (!cbor_key(s, pos, BK_STEP_LO, 0, 8) || !cbor_uint_max(s, pos, 9, ~0ull, h.step_lo)) return 0;
  if (!cbor_key(s, pos, BK_STEP_HI, 0, 8) || !cbor_uint_max(s, pos, 9, ~0ull, h.step_hi)) return 0;
  if (!cbor_key(s, pos, BK_CTRL_IN, 0, 8) || !cbor_uint_max(s, pos, 3, 0xFFFFu, v)) return 0;
  h.ctrl_in = (uint16_t)v;
  if (!cbor_key(s, pos, BK_CTRL_OUT_LO, BK_CTRL_OUT_HI, 9) || !cbor_uint_max(s, pos, 3, 0xFFFFu, v)) return 0;
  h.ctrl_out = (uint16_t)v;
  if (!cbor_key(s, pos, BK_IN_HEAD_IN_LO, BK_IN_HEAD_IN_HI, 11) || !cbor_int64(s, pos, h.in_head_in)) return 0;
  if (!cbor_key(s, pos, BK_IN_HEAD_OUT_LO, BK_IN_HEAD_OUT_HI, 12) || !cbor_int64(s, pos, h.in_head_out)) return 0;
  if (!cbor_key(s, pos, BK_WINDOWS, 0, 8)) return 0;
  if (tau_any) {
    uint32_t mj, adv;
    cbor_head_min(s, pos, 2, mj, v, adv);
    if (!adv || mj != 4) return 0;  // two bytes: at most 255
    tau = (uint32_t)v;
    pos += adv;
  } else if (!cbor_array_of(s, pos, tau)) {
    return 0;
  }
  h.tau = tau;
  for (uint32_t r = 0; r < tau; r++) {
    int64_t l, rr;
    if (!cbor_match(s, pos, BK_LEFT, 6)) return 0;
    pos += 6;
    if (!cbor_int64(s, pos, l)) return 0;
    if (!cbor_match(s, pos, BK_RIGHT, 6)) return 0;
    pos += 6;
    if (!cbor_int64(s, pos, rr)) return 0;
    if (win_left) {
      win_left[r] = l;
      win_right[r] = rr;
    }
  }
  if (!cbor_key(s, pos, BK_OFF_IN_LO, BK_OFF_IN_HI, 16) || !cbor_array_of(s, pos, tau)) return 0;
  for (uint32_t r = 0; r < tau; r++) {
    if (!cbor_uint_max(s, pos, 5, 0xFFFFFFFFull, v)) return 0;
    if (off_in) off_in[r] = (uint32_t)v;
  }
  if (!cbor_match(s, pos, BK_OFF_OUT_LO, 8) || cbor_at(s, pos + 8) != 0x74u) return 0;  // 70 "head_ou" | 't'
  pos += 9;
  if (!cbor_match(s, pos, BK_OFF_OUT_HI, 8)) return 0;
  pos += 8;
  if (!cbor_array_of(s, pos, tau)) return 0;
  for (uint32_t r = 0; r < tau; r++) {
    if (!cbor_uint_max(s, pos, 5, 0xFFFFFFFFull, v)) return 0;
    if (off_out) off_out[r] = (uint32_t)v;
  }
  if (!cbor_key(s, pos, BK_MOVLOG_LO, BK_MOVLOG_HI, 13)) return 0;
  if (!cbor_match(s, pos, BK_STEPS, 7)) return 0;
  pos += 7;
  uint32_t mj, adv;
  cbor_head_min(s, pos, 5, mj, v, adv);
  if (!adv || mj != 4 || v < 1) return 0;  // five bytes: at most 2^32 - 1
  h.n_steps = (uint32_t)v;
  return pos + adv;
}

// array(tau) x (90 | 16 x uint <= 255)
TRACE_CBOR_HD inline bool cbor_tag_arrays(const CborSpan& s, uint64_t& pos, uint32_t tau) {
  if (!cbor_array_of(s, pos, tau)) return false;
  for (uint32_t r = 0; r < tau; r++) {
    if (cbor_at(s, pos) != 0x90u) return false;
    pos += 1;
    for (int k = 0; k < 16; k++) {
      uint64_t v;
      if (!cbor_uint_max(s, pos, 2, 255, v)) return false;
    }
  }
  return true;
}
// One block's tail at pos (behind its last step), strictly: its end, or 0
TRACE_CBOR_HD inline uint64_t cbor_parse_block_tail(const CborSpan& s, uint64_t pos, uint32_t tau) {
  if (!cbor_key(s, pos, BK_PRE_TAGS_LO, BK_PRE_TAGS_HI, 9) || !cbor_tag_arrays(s, pos, tau)) return 0;
  if (!cbor_key(s, pos, BK_POST_TAGS_LO, BK_POST_TAGS_HI, 10) || !cbor_tag_arrays(s, pos, tau)) return 0;
  return pos;
}

// ------------------------------------------------------------ the head
struct BlocksCborHead {
  uint32_t n_blocks = 0;
  uint32_t tau = 0;
  uint64_t first_off = 0;  // block 0: the first byte after the array head
  uint64_t t_max = 0;      // no more steps than this fit the file
};
// true: the bytes start with array(B), B >= 1, and a canonical head of block
// 0, and B blocks can fit the rest
inline bool blocks_cbor_head(const CborSpan& s, BlocksCborHead& h) {
  uint32_t mj, adv;
  uint64_t v;
  cbor_head_min(s, 0, 5, mj, v, adv);
  if (!adv || mj != 4 || v < 1) return false;
  BlockCborHead b0;
  if (!cbor_parse_block_head(s, adv, 0, true, b0, nullptr, nullptr, nullptr, nullptr)) return false;
  if (v > (s.len - adv) / cbor_block_min_len(b0.tau)) return false;
  h.n_blocks = (uint32_t)v;
  h.tau = b0.tau;
  h.first_off = adv;
  h.t_max = (s.len - adv) / cbor_step_min_len(b0.tau);
  return true;
}

// ------------------------------------------------------------ the tables
// One block of memory holds what comes home: the widest fields first, every
// array on its own alignment. B blocks, nt = B * tau cells.
struct BlocksCborTables {
  uint64_t *step_lo, *step_hi, *steps_off, *step_start;
  int64_t *in_head_in, *in_head_out, *win_left, *win_right;
  uint32_t *off_in, *off_out, *block_id, *n_steps;
  uint16_t *version, *ctrl_in, *ctrl_out;
};
inline size_t blocks_cbor_tables_bytes(uint64_t B, uint32_t tau) { return (size_t)(B * (62 + 24ull * tau)); }
inline BlocksCborTables blocks_cbor_tables_at(uint8_t* base, uint64_t B, uint32_t tau) {
  const uint64_t nt = B * tau;
  BlocksCborTables t;
  uint64_t* q = reinterpret_cast<uint64_t*>(base);
  t.step_lo = q;
  t.step_hi = q + B;
  t.steps_off = q + 2 * B;
  t.step_start = q + 3 * B;
  t.in_head_in = reinterpret_cast<int64_t*>(q + 4 * B);
  t.in_head_out = reinterpret_cast<int64_t*>(q + 5 * B);
  t.win_left = reinterpret_cast<int64_t*>(q + 6 * B);
  t.win_right = reinterpret_cast<int64_t*>(q + 6 * B + nt);
  uint32_t* d = reinterpret_cast<uint32_t*>(q + 6 * B + 2 * nt);
  t.off_in = d;
  t.off_out = d + nt;
  t.block_id = d + 2 * nt;
  t.n_steps = d + 2 * nt + B;
  uint16_t* w = reinterpret_cast<uint16_t*>(d + 2 * nt + 2 * B);
  t.version = w;
  t.ctrl_in = w + B;
  t.ctrl_out = w + 2 * B;
  return t;
}

// row k of the tables from a parsed head (a failed head leaves n_steps = 0)
TRACE_CBOR_HD inline void blocks_cbor_store_head(const BlocksCborTables& T, uint64_t k, const BlockCborHead& h,
                                                 uint64_t steps_off) {
  T.version[k] = h.version;
  T.block_id[k] = h.block_id;
  T.step_lo[k] = h.step_lo;
  T.step_hi[k] = h.step_hi;
  T.ctrl_in[k] = h.ctrl_in;
  T.ctrl_out[k] = h.ctrl_out;
  T.in_head_in[k] = h.in_head_in;
  T.in_head_out[k] = h.in_head_out;
  T.n_steps[k] = steps_off ? h.n_steps : 0u;
  T.steps_off[k] = steps_off;
}

// the largest k < B with step_start[k] <= i (step_start[0] = 0)
TRACE_CBOR_HD inline uint64_t blocks_cbor_block_of(const uint64_t* step_start, uint64_t B, uint64_t i) {
  uint64_t lo = 0, hi = B;
  while (hi - lo > 1) {
    const uint64_t mid = lo + (hi - lo) / 2;
    if (step_start[mid] <= i) lo = mid;
    else hi = mid;
  }
  return lo;
}

// ------------------------------------------------------------ the verdict
// the first failures by index, ~0 when none; t = the sum of n_k
struct BlocksCborVerdict {
  uint64_t block_candidates;
  uint64_t step_candidates;
  uint64_t t;
  uint64_t bad_head;  // block whose head does not parse (or block 0 not at first_off)
  uint64_t bad_step;  // step that does not parse
  uint64_t bad_link;  // step that does not start where its block's head or its predecessor ends
  uint64_t bad_tail;  // block whose tail does not parse or does not end at the next block / at len
};

// Heads are good and t fits: all B heads parsed, so t is the file's step
// count, and that many rows and candidates are there. The step and chain
// passes run only then.
TRACE_CBOR_HD inline bool blocks_cbor_heads_fit(const BlocksCborVerdict& v, uint64_t B, uint64_t t_max) {
  return v.block_candidates >= B && v.bad_head == ~0ull && v.t <= t_max && v.step_candidates >= v.t;
}

// ------------------------------------------------------------ the passes
// The body of each per-index pass, for the kernels of cbor_decode.hip and,
// index by index, for the check tool. cand_b: B words; cand_s, ends: t_max
// words; the arrays: t_max and t_max * tau elements; T: the tables of B
// blocks. V starts as all ones but for the two candidate counts. `lower`: see
// CborSerialMin.
//
// heads, index k: block k's head from block candidate k. With fewer than B
// candidates nothing is parsed, but n_k is written all the same: the scan
// reads all B of them.
template <class Min>
TRACE_CBOR_HD inline void blocks_cbor_head_pass(const CborSpan& s, uint64_t lo, const uint64_t* cand_b, uint64_t B,
                                                uint32_t tau, const BlocksCborTables& T, BlocksCborVerdict* V,
                                                uint64_t k, Min lower) {
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
  if (!end) lower(&V->bad_head, k);
}
// steps, index i: step i from step candidate i, its end, and its link: step
// i + 1 starts where step i ends unless it is the first of a block (then the
// chain pass checks both sides). The search through step_start runs only at a
// mismatch: B - 1 times in a canonical file.
template <class Min>
TRACE_CBOR_HD inline void blocks_cbor_step_pass(const CborSpan& s, const uint64_t* cand_s, uint64_t t_max, uint64_t B,
                                                const uint64_t* step_start, uint32_t tau, int8_t* input_mv, int8_t* mv,
                                                uint8_t* has_write, uint16_t* wsym, uint64_t* ends,
                                                BlocksCborVerdict* V, uint64_t i, Min lower) {
  const uint64_t t = V->t;
  if (!blocks_cbor_heads_fit(*V, B, t_max) || i >= t) return;
  const uint64_t c = cand_s[i], o = i * tau;
  const uint64_t end = cbor_parse_step(s, c, tau, input_mv + i, mv + o, has_write + o, wsym + o);
  ends[i] = end;
  if (!end) {
    lower(&V->bad_step, i);
    return;
  }
  if (i + 1 < t && cand_s[i + 1] != end) {
    const uint64_t k = blocks_cbor_block_of(step_start, B, i + 1);
    if (step_start[k] != i + 1) lower(&V->bad_link, i + 1);
  }
}
// chain, index k: block k's two ends: its first step lies right behind its
// head, and behind its last step the tail runs up to the next block candidate
// (to len for the last block).
template <class Min>
TRACE_CBOR_HD inline void blocks_cbor_chain_pass(const CborSpan& s, const uint64_t* cand_b, const uint64_t* cand_s,
                                                 uint64_t t_max, uint64_t B, uint32_t tau, const BlocksCborTables& T,
                                                 const uint64_t* ends, BlocksCborVerdict* V, uint64_t k, Min lower) {
  if (!blocks_cbor_heads_fit(*V, B, t_max) || k >= B) return;
  const uint64_t a = T.step_start[k], n = T.n_steps[k];  // n >= 1, a + n <= t
  if (cand_s[a] != T.steps_off[k]) lower(&V->bad_link, a);
  const uint64_t e = ends[a + n - 1];
  if (!e) return;  // the step did not parse: bad_step has it
  const uint64_t tail_end = cbor_parse_block_tail(s, e, tau);
  const uint64_t want = k + 1 < B ? cand_b[k + 1] : s.len;
  if (!tail_end || tail_end != want) lower(&V->bad_tail, k);
}

// What the host makes of the verdict: SEZKP_BLOCKS_R_* by value (sezkp_stark.h)
// and the index that goes with it. Shared with the check tool.
inline CborDecision blocks_cbor_decide(const BlocksCborVerdict& v, const BlocksCborHead& h) {
  CborDecision d;
  if (!blocks_cbor_heads_fit(v, h.n_blocks, h.t_max)) {
    if (v.block_candidates < h.n_blocks) d.reason = 2;
    else if (v.bad_head != ~0ull) d.reason = 4, d.index = v.bad_head;
    else d.reason = 3;
  } else if (v.bad_step != ~0ull && v.bad_step <= v.bad_link) d.reason = 5, d.index = v.bad_step;
  else if (v.bad_link != ~0ull) d.reason = 6, d.index = v.bad_link;
  else if (v.bad_tail != ~0ull) d.reason = 7, d.index = v.bad_tail;
  return d;
}

}  // namespace sezkp
