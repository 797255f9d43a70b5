// cbor_emit_plan.h — what the host and the device agree on when a block file
// (Vec<BlockSummary>) or a TraceFile is written as CBOR on the device
// (cbor_encode.hip, sezkp_ctx_encode_*): the byte layout from the writing
// side, the tiling, and the body of every per-index pass. The layout is the
// one blocks_cbor_plan.h and trace_cbor_plan.h read, and the bytes are
// encode_blocks_cbor's / encode_trace_cbor's (codec.cpp). Plain C++, no HIP
// type: tools/cbor_encode_check.cpp runs the same passes index by index under
// the sanitizers on a machine without a GPU.
//
// A file is B blocks, each a head, its n_k step records and a tail:
//   block file  head  [array(B), block 0 only] AE | the 8 scalar fields | windows | the two offset
//                     arrays | 6C "movement_log" A1 65 "steps" array(n_k)
//               tail  68 "pre_tags" array(tau) x (90 | 16 x 00) | 69 "post_tags" the same
//   TraceFile   one pseudo-block: head A4 67 "version" 01 63 "tau" uint 65 "steps" array(t),
//               tail 64 "meta" F6
// Everything is written through a byte sink (put(byte), at(offset)), and a
// length is the same code run into a sink that only counts: what a pass
// measures is what a later pass writes.
//
// The encode, in five passes (one kernel each on the device):
//   step lengths   step i's record length; one sum per tile of S steps;
//   block lengths  block k's head + tail length;
//   scans          both, exclusive (cbor_scan_dev.h); the file's length is the two totals;
//   steps          step i's record at  P(i) + pre[k] + head_k,  P(i) the step
//                  bytes before i, pre[k] the heads and tails of the blocks
//                  before k = the block of i; the first step of block k
//                  leaves P(i) in first[k];
//   blocks         block k's head at pre[k] + P(step_start[k]) and its tail
//                  in front of block k + 1's head (at the file's end for the last).
// Every byte of the file is written by exactly one index of one pass.
#pragma once
#include "blocks_cbor_plan.h"
#include "trace_plan.h"

namespace sezkp {

// ------------------------------------------------------------ tiling
// A workgroup of 256 lanes assembles a tile of S consecutive steps in LDS, one
// lane per step, and copies the tile out with all lanes. S is the largest
// power of two, at most 256, whose worst-case span fits CBOR_EMIT_LDS: 256
// steps up to 11 tapes (35.6 KB at 8), then 128 (to 24), 64 (to 49), 32 (to
// 101), 16 (to 203), 8 (255 tapes: 3,845 bytes a record).
constexpr uint32_t CBOR_EMIT_THREADS = 256;
constexpr uint32_t CBOR_EMIT_LDS = 48u << 10;
TRACE_CBOR_HD inline uint32_t cbor_emit_tile_steps(uint32_t tau) {
  uint32_t s = CBOR_EMIT_THREADS;
  while (s > 1 && s * cbor_step_max_len(tau) > CBOR_EMIT_LDS) s >>= 1;
  return s;
}
TRACE_CBOR_HD inline uint64_t cbor_emit_tiles(uint64_t t, uint32_t S) { return (t + S - 1) / S; }

// ------------------------------------------------------------ sinks
// counts the bytes put
struct CborCount {
  uint64_t n = 0;
  TRACE_CBOR_HD void put(uint8_t) { n++; }
};
// writes them, unchecked: the caller has sized the memory by the counts
struct CborBytes {
  uint8_t* p;
  TRACE_CBOR_HD void put(uint8_t b) { *p++ = b; }
  TRACE_CBOR_HD CborBytes at(uint64_t off) const { return CborBytes{p + off}; }
};

// the same into memory of len bytes: a byte at or past len is dropped, whatever
// the counts said (the heads and tails, which go straight to the file image)
struct CborBounded {
  uint8_t* base;
  uint64_t pos, len;
  TRACE_CBOR_HD void put(uint8_t b) {
    if (pos < len) base[pos] = b;
    pos++;
  }
  TRACE_CBOR_HD CborBounded at(uint64_t off) const { return CborBounded{base, off, len}; }
};

// ------------------------------------------------------------ items
// cb_head (codec.cpp): major type and argument in the minimal length
template <class O>
TRACE_CBOR_HD inline void cbor_put_head(O& o, uint32_t major, uint64_t v) {
  const uint8_t m = (uint8_t)(major << 5);
  if (v < 24) {
    o.put(m | (uint8_t)v);
    return;
  }
  const int nb = v < 0x100ull ? 1 : v < 0x10000ull ? 2 : v < 0x100000000ull ? 4 : 8;
  o.put(m | (uint8_t)(nb == 1 ? 24 : nb == 2 ? 25 : nb == 4 ? 26 : 27));
  for (int i = nb - 1; i >= 0; i--) o.put((uint8_t)(v >> (8 * i)));
}
// a negative x is major type 1 of -1 - x
template <class O>
TRACE_CBOR_HD inline void cbor_put_int(O& o, int64_t x) {
  if (x >= 0) cbor_put_head(o, 0, (uint64_t)x);
  else cbor_put_head(o, 1, (uint64_t)(-1 - x));
}
// n <= 16 literal bytes, little endian in lo | hi (the keys of the two plan headers)
template <class O>
TRACE_CBOR_HD inline void cbor_put_lit(O& o, uint64_t lo, uint64_t hi, int n) {
  for (int k = 0; k < n; k++) o.put((uint8_t)((k < 8 ? lo >> (8 * k) : hi >> (8 * (k - 8))) & 0xFFu));
}

// ------------------------------------------------------------ the inputs
// the four step arrays, step-major (t and t * tau elements)
struct CborEmitSteps {
  const int8_t* input_mv;
  const int8_t* mv;
  const uint8_t* has_write;
  const uint16_t* wsym;
};
// kind 0: a block file of B blocks; kind 1: a TraceFile (B = 1). Uniform
// blocks of b steps (a partitioned trace, a TraceFile's pseudo-block) need no
// step_start array: b != 0 says so.
struct CborEmitShape {
  uint32_t kind;
  uint32_t tau;
  uint64_t B, t;
  uint64_t b;
  const uint64_t* step_start;  // B + 1 words when b = 0
};
TRACE_CBOR_HD inline uint64_t cbor_emit_step_start(const CborEmitShape& sh, uint64_t k) {
  return sh.b ? trace_step_start(k, sh.t, sh.b) : sh.step_start[k];
}
// the block of step i < t: the largest k with step_start[k] <= i (never an empty block)
TRACE_CBOR_HD inline uint64_t cbor_emit_block_of(const CborEmitShape& sh, uint64_t i) {
  return sh.b ? i / sh.b : blocks_cbor_block_of(sh.step_start, sh.B, i);
}
// The block fields. version = null: those of partition_trace (version 1,
// block_id k + 1, step_lo and step_hi from the boundaries, ctrl 0), the rest
// from the device's metadata image. A TraceFile reads none.
struct CborEmitTables {
  const uint16_t *version, *ctrl_in, *ctrl_out;
  const uint32_t *block_id, *off_in, *off_out;
  const uint64_t *step_lo, *step_hi;
  const int64_t *in_head_in, *in_head_out, *win_left, *win_right;
};

// ------------------------------------------------------------ a step record
template <class O>
TRACE_CBOR_HD inline void cbor_emit_step(O& o, const CborEmitSteps& A, uint32_t tau, uint64_t i) {
  cbor_put_lit(o, CBOR_SIG_LO, CBOR_SIG_HI, 10);  // A2 68 "input_mv"
  cbor_put_int(o, A.input_mv[i]);
  cbor_put_lit(o, CBOR_KEY_TAPES, 0, 6);
  cbor_put_head(o, 4, tau);
  const uint64_t c0 = i * tau;
  for (uint32_t r = 0; r < tau; r++) {
    cbor_put_lit(o, CBOR_KEY_WRITE, 0, 7);
    if (A.has_write[c0 + r]) cbor_put_head(o, 0, A.wsym[c0 + r]);
    else o.put(0xF6);
    cbor_put_lit(o, CBOR_KEY_MV, 0, 3);
    cbor_put_int(o, A.mv[c0 + r]);
  }
}
TRACE_CBOR_HD inline uint32_t cbor_emit_step_len(const CborEmitSteps& A, uint32_t tau, uint64_t i) {
  CborCount c;
  cbor_emit_step(c, A, tau, i);
  return (uint32_t)c.n;
}

// ------------------------------------------------------------ heads and tails
template <class O>
TRACE_CBOR_HD inline void cbor_emit_head(O& o, const CborEmitShape& sh, const CborEmitTables& T, uint64_t k) {
  const uint32_t tau = sh.tau;
  const uint64_t lo = cbor_emit_step_start(sh, k), hi = cbor_emit_step_start(sh, k + 1);
  if (sh.kind == 1) {
    o.put(0xA4);
    cbor_put_lit(o, BK_VERSION, 0, 8);
    o.put(0x01);
    cbor_put_lit(o, 0x75617463ull, 0, 4);  // 63 "tau"
    cbor_put_head(o, 0, tau);
    cbor_put_lit(o, 0x737065747365ull, 0, 6);  // 65 "steps"
    cbor_put_head(o, 4, sh.t);
    return;
  }
  if (k == 0) cbor_put_head(o, 4, sh.B);
  const bool synth = T.version == nullptr;
  o.put(0xAE);
  cbor_put_lit(o, BK_VERSION, 0, 8);
  cbor_put_head(o, 0, synth ? 1u : T.version[k]);
  cbor_put_lit(o, BK_BLOCK_ID_LO, BK_BLOCK_ID_HI, 9);
  cbor_put_head(o, 0, synth ? (uint32_t)(k + 1) : T.block_id[k]);
  cbor_put_lit(o, BK_STEP_LO, 0, 8);
  cbor_put_head(o, 0, synth ? lo + 1 : T.step_lo[k]);
  cbor_put_lit(o, BK_STEP_HI, 0, 8);
  cbor_put_head(o, 0, synth ? hi : T.step_hi[k]);
  cbor_put_lit(o, BK_CTRL_IN, 0, 8);
  cbor_put_head(o, 0, synth ? 0u : T.ctrl_in[k]);
  cbor_put_lit(o, BK_CTRL_OUT_LO, BK_CTRL_OUT_HI, 9);
  cbor_put_head(o, 0, synth ? 0u : T.ctrl_out[k]);
  cbor_put_lit(o, BK_IN_HEAD_IN_LO, BK_IN_HEAD_IN_HI, 11);
  cbor_put_int(o, T.in_head_in[k]);
  cbor_put_lit(o, BK_IN_HEAD_OUT_LO, BK_IN_HEAD_OUT_HI, 12);
  cbor_put_int(o, T.in_head_out[k]);
  cbor_put_lit(o, BK_WINDOWS, 0, 8);
  cbor_put_head(o, 4, tau);
  const uint64_t c0 = k * tau;
  for (uint32_t r = 0; r < tau; r++) {
    cbor_put_lit(o, BK_LEFT, 0, 6);
    cbor_put_int(o, T.win_left[c0 + r]);
    cbor_put_lit(o, BK_RIGHT, 0, 6);
    cbor_put_int(o, T.win_right[c0 + r]);
  }
  cbor_put_lit(o, BK_OFF_IN_LO, BK_OFF_IN_HI, 16);
  cbor_put_head(o, 4, tau);
  for (uint32_t r = 0; r < tau; r++) cbor_put_head(o, 0, T.off_in[c0 + r]);
  cbor_put_lit(o, BK_OFF_OUT_LO, 0, 8);  // 70 "head_ou"
  o.put(0x74);                           // 't'
  cbor_put_lit(o, BK_OFF_OUT_HI, 0, 8);  // "_offsets"
  cbor_put_head(o, 4, tau);
  for (uint32_t r = 0; r < tau; r++) cbor_put_head(o, 0, T.off_out[c0 + r]);
  cbor_put_lit(o, BK_MOVLOG_LO, BK_MOVLOG_HI, 13);
  cbor_put_lit(o, BK_STEPS, 0, 7);
  cbor_put_head(o, 4, hi - lo);
}
template <class O>
TRACE_CBOR_HD inline void cbor_emit_tail(O& o, const CborEmitShape& sh) {
  if (sh.kind == 1) {
    cbor_put_lit(o, 0xF66174656D64ull, 0, 6);  // 64 "meta" F6
    return;
  }
  for (int q = 0; q < 2; q++) {
    if (q == 0) cbor_put_lit(o, BK_PRE_TAGS_LO, BK_PRE_TAGS_HI, 9);
    else cbor_put_lit(o, BK_POST_TAGS_LO, BK_POST_TAGS_HI, 10);
    cbor_put_head(o, 4, sh.tau);
    for (uint32_t r = 0; r < sh.tau; r++) {
      o.put(0x90);
      for (int z = 0; z < 16; z++) o.put(0x00);
    }
  }
}
// a constant of the kind and tau: 19 + 2 h + 34 tau for a block, 6 for a TraceFile
TRACE_CBOR_HD inline uint32_t cbor_emit_tail_len(const CborEmitShape& sh) {
  return sh.kind == 1 ? 6u : 19u + 2u * (sh.tau < 24 ? 1u : 2u) + 34u * sh.tau;
}
// what no head exceeds (every integer at its type's longest; array(B) and
// array(n_k) at 9 bytes), so that a length can be checked against the shape
// before anything is sized by it
TRACE_CBOR_HD inline uint64_t cbor_emit_head_max(uint32_t kind, uint32_t tau) {
  if (kind == 1) return 1 + 8 + 1 + 4 + 2 + 6 + 9;
  const uint64_t h = tau < 24 ? 1u : 2u;
  return 1 + (8 + 3) + (9 + 5) + (8 + 9) + (8 + 9) + (8 + 3) + (9 + 3) + (11 + 9) + (12 + 9) + (8 + h + 30ull * tau) +
         (16 + h + 5ull * tau) + (17 + h + 5ull * tau) + 13 + 7 + 9;
}
TRACE_CBOR_HD inline uint64_t cbor_emit_len_bound(const CborEmitShape& sh) {
  return sh.B * (cbor_emit_head_max(sh.kind, sh.tau) + cbor_emit_tail_len(sh)) + sh.t * cbor_step_max_len(sh.tau) + 9;
}

// ------------------------------------------------------------ the passes
// block lengths, index k: head + tail
TRACE_CBOR_HD inline void cbor_emit_block_len_pass(const CborEmitShape& sh, const CborEmitTables& T, uint32_t* blen,
                                                   uint64_t k) {
  if (k >= sh.B) return;
  CborCount c;
  cbor_emit_head(c, sh, T, k);
  blen[k] = (uint32_t)c.n + cbor_emit_tail_len(sh);
}
// What the scans leave: pre[k] the head and tail bytes of the blocks before k,
// blen[k] block k's own, first[k] the step bytes in front of a non-empty
// block's first step (written by the steps pass), steps_total all step bytes.
struct CborEmitScans {
  const uint64_t* pre;
  const uint32_t* blen;
  uint64_t* first;
  uint64_t steps_total;
};
// steps, index i, with P = the step bytes before i (the tile's scanned offset
// plus the lengths of the tile's steps before i): where the record goes. The
// first step of a block leaves P for the blocks pass.
TRACE_CBOR_HD inline uint64_t cbor_emit_step_place(const CborEmitShape& sh, const CborEmitScans& sc, uint64_t i,
                                                   uint64_t P, bool& first_of_block) {
  const uint64_t k = cbor_emit_block_of(sh, i);
  first_of_block = cbor_emit_step_start(sh, k) == i;
  if (first_of_block) sc.first[k] = P;
  return P + sc.pre[k] + sc.blen[k] - cbor_emit_tail_len(sh);
}
// the step bytes before block k's steps; k = B: all of them. An empty block
// lies where the next non-empty one starts.
TRACE_CBOR_HD inline uint64_t cbor_emit_steps_before(const CborEmitShape& sh, const CborEmitScans& sc, uint64_t k) {
  for (; k < sh.B; k++)
    if (cbor_emit_step_start(sh, k + 1) > cbor_emit_step_start(sh, k)) return sc.first[k];
  return sc.steps_total;
}
// blocks, index k: the head in front of the block's first step, the tail
// behind its last one
template <class Sink>
TRACE_CBOR_HD inline void cbor_emit_block_pass(const CborEmitShape& sh, const CborEmitTables& T, const CborEmitScans& sc,
                                               const Sink& file, uint64_t k) {
  if (k >= sh.B) return;
  Sink head = file.at(sc.pre[k] + cbor_emit_steps_before(sh, sc, k));
  cbor_emit_head(head, sh, T, k);
  Sink tail = file.at(sc.pre[k] + sc.blen[k] - cbor_emit_tail_len(sh) + cbor_emit_steps_before(sh, sc, k + 1));
  cbor_emit_tail(tail, sh);
}

}  // namespace sezkp
