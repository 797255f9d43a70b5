// trace_cbor_plan.h — what the host and the device agree on when a TraceFile
// (sezkp-trace format.rs:59-68, io.rs) is decoded from its CBOR bytes on the
// device (cbor_decode.hip, sezkp_ctx_upload_trace_cbor): the canonical form, the
// signatures that start a record, the strict step parser, the head check, and
// the body of every per-index pass: a kernel is its index and one call of
// cbor_lane_marks / cbor_store_marks / trace_cbor_step_pass. Plain C++, no HIP
// type: tools/cbor_check.cpp calls the same passes index by index under the
// sanitizers on a machine without a GPU.
//
// The canonical form is what ciborium and sezkp_trace_encode_cbor write:
//   head  A4 | 67 "version" | uint | 63 "tau" | uint <= 255 | 65 "steps" | array(t)
//   step  A2 | 68 "input_mv" | int | 65 "tapes" | array(tau) |
//         tau x (A2 | 65 "write" | F6 or uint | 62 "mv" | int)
//   tail  64 "meta" | one flat item (null, a number, a string; no array, map
//         or tag), ending at len
// with every integer in its minimal-length head. A step is 17 + h + 12 tau to
// 18 + h + 15 tau bytes (h = 1 below 24 tapes, else 2). The device path takes
// exactly this form and declines everything else; a declined file goes to the
// host pull parser (codec.cpp), which alone reports errors.
//
// The decode, in four passes (index by index in the check tool, one kernel
// each on the device):
//   mark     every byte position from steps_off on that starts the 10-byte
//            signature A2 68 "input_mv" is a candidate;
//   compact  the candidates in file order, the first t stored, all counted;
//   parse    candidate i is parsed strictly as a whole step into row i;
//   chain    c[0] = steps_off, c[i] + len_i = c[i + 1], and the tail that
//            starts at c[t - 1] + len_{t - 1} is "meta" and one flat item up to len.
// When the chain holds, a sequential parse visits exactly c[0..t), so the rows
// are the host decoder's. The step records of blocks.cbor and of the JSONL
// block files' CBOR twin are the same, so cbor_parse_step is kept free of
// anything that belongs to the TraceFile around it.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define TRACE_CBOR_HD __host__ __device__
#else
#define TRACE_CBOR_HD
#endif

namespace sezkp {

// ------------------------------------------------------------ tiling
// The mark and compact kernels give one workgroup of 256 lanes a tile of
// TRACE_CBOR_TILE consecutive bytes, 16 per lane (one 16-byte load, plus the
// next 16 for the signatures that start in the lane's bytes and end behind
// them). The tile counts are scanned by one workgroup, TRACE_CBOR_SCAN_PASS
// tiles per pass.
constexpr uint32_t TRACE_CBOR_THREADS = 256;
constexpr uint32_t TRACE_CBOR_LANE_BYTES = 16;
constexpr uint32_t TRACE_CBOR_TILE = TRACE_CBOR_THREADS * TRACE_CBOR_LANE_BYTES;  // 4096 bytes
constexpr uint32_t TRACE_CBOR_SCAN_PASS = TRACE_CBOR_THREADS * 4;                 // 1024 tiles
constexpr uint32_t TRACE_CBOR_SIG_LEN = 10;
TRACE_CBOR_HD inline uint64_t trace_cbor_tiles(uint64_t len) { return (len + TRACE_CBOR_TILE - 1) / TRACE_CBOR_TILE; }

// ------------------------------------------------------------ the accessor
// Every read of file bytes goes through these two. Past the end a byte reads
// as CBOR_END, which is no byte value: it equals no key byte and no integer
// head, so a parse that runs off a truncated file stops there.
struct CborSpan {
  const uint8_t* data;
  uint64_t len;
};
constexpr uint32_t CBOR_END = 0x100u;
TRACE_CBOR_HD inline uint32_t cbor_at(const CborSpan& s, uint64_t pos) { return pos < s.len ? s.data[pos] : CBOR_END; }

// 16 bytes from pos (little endian: byte 0 in lo's low bits); bytes past the
// end read as 0xFF, which no signature byte is. pos a multiple of 16.
struct alignas(16) Cbor16 {
  uint64_t lo, hi;
};
TRACE_CBOR_HD inline Cbor16 cbor_load16(const CborSpan& s, uint64_t pos) {
  Cbor16 r;
  if (pos < s.len && s.len - pos >= 16) {
#if defined(__HIP_DEVICE_COMPILE__)
    // the device copy of the file starts on a 16-byte boundary: one dwordx4 load
    r = *reinterpret_cast<const Cbor16*>(s.data + pos);
#else
    memcpy(&r.lo, s.data + pos, 8);
    memcpy(&r.hi, s.data + pos + 8, 8);
#endif
    return r;
  }
  r.lo = r.hi = 0;
  for (int k = 0; k < 16; k++) {
    const uint32_t b = cbor_at(s, pos + (uint64_t)k);
    const uint64_t v = b == CBOR_END ? 0xFFu : b;
    if (k < 8) r.lo |= v << (8 * k);
    else r.hi |= v << (8 * (k - 8));
  }
  return r;
}

// ------------------------------------------------------------ mark
// The signatures by kind: 0 starts a step record (A2 68 "input_mv"), 1 a block
// of a block file (AE 67 "version", blocks_cbor_plan.h). The first 8 bytes in
// lo, the rest in hi under hi_mask. A signature's first byte occurs nowhere
// else in it, so two candidates of one kind lie at least len positions apart.
constexpr uint64_t CBOR_SIG_LO = 0x5F7475706E6968A2ull;  // A2 68 'i' 'n' 'p' 'u' 't' '_'
constexpr uint32_t CBOR_SIG_HI = 0x766Du;                // 'm' 'v'
constexpr uint32_t BLOCKS_CBOR_SIG_LEN = 9;
struct CborSig {
  uint64_t lo;
  uint32_t hi, hi_mask;
};
constexpr CborSig CBOR_SIGS[2] = {{CBOR_SIG_LO, CBOR_SIG_HI, 0xFFFFu},
                                  {0x6F697372657667AEull, 0x6Eu, 0xFFu}};  // AE 67 'v' 'e' 'r' 's' 'i' 'o' | 'n'
// bit s: the signature of KIND starts at byte s of a (it may end in b, the 16 bytes after a)
template <int KIND>
TRACE_CBOR_HD inline uint32_t cbor_sig_mask(const Cbor16& a, const Cbor16& b) {
  constexpr CborSig S = CBOR_SIGS[KIND];
  const uint64_t w[4] = {a.lo, a.hi, b.lo, b.hi};
  uint32_t m = 0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (int s = 0; s < 16; s++) {
    const int q = s >> 3, r = (s & 7) * 8;
    const uint64_t x = r ? (w[q] >> r) | (w[q + 1] << (64 - r)) : w[q];
    const uint64_t y = r ? (w[q + 1] >> r) | (w[q + 2] << (64 - r)) : w[q + 1];
    if (x == S.lo && (uint32_t)(y & S.hi_mask) == S.hi) m |= 1u << s;
  }
  return m;
}
// One lane of the mark passes: the candidates of the first KINDS kinds among
// the 16 positions from pos (bit s of m[kind]: pos + s), none before lo. At
// most two of a kind (both signatures are 9 bytes or longer).
static_assert(BLOCKS_CBOR_SIG_LEN >= 9 && TRACE_CBOR_SIG_LEN >= 9, "at most two candidates of a kind in 16 positions");
template <int KINDS>
TRACE_CBOR_HD inline void cbor_lane_marks(const CborSpan& s, uint64_t lo, uint64_t pos, uint32_t (&m)[KINDS]) {
  for (int q = 0; q < KINDS; q++) m[q] = 0u;
  if (pos >= s.len) return;
  const Cbor16 a = cbor_load16(s, pos), b = cbor_load16(s, pos + 16);
  m[0] = cbor_sig_mask<0>(a, b);
  if constexpr (KINDS > 1) m[1] = cbor_sig_mask<1>(a, b);
  if (pos < lo) {
    const uint32_t keep = lo - pos >= 16 ? 0u : (0xFFFFu << (uint32_t)(lo - pos)) & 0xFFFFu;
    for (int q = 0; q < KINDS; q++) m[q] &= keep;
  }
}
// One lane of the compact pass: its marks of one kind are candidates idx,
// idx + 1, ... in file order; those below cap are stored. The index behind them.
TRACE_CBOR_HD inline uint64_t cbor_store_marks(uint32_t m, uint64_t pos, uint64_t idx, uint64_t* cand, uint64_t cap) {
  while (m) {
    if (idx < cap) cand[idx] = pos + (uint32_t)__builtin_ctz(m);
    m &= m - 1u;
    idx++;
  }
  return idx;
}

// ------------------------------------------------------------ strict items
// n <= 8 literal bytes (little endian in lit) at pos
TRACE_CBOR_HD inline bool cbor_match(const CborSpan& s, uint64_t pos, uint64_t lit, int n) {
  for (int k = 0; k < n; k++)
    if (cbor_at(s, pos + (uint64_t)k) != (uint32_t)((lit >> (8 * k)) & 0xFFu)) return false;
  return true;
}
// An item head of major type 0..7 with its argument in minimal length, of at
// most max_bytes bytes in all (1, 2, 3, 5 or 9). adv = 0: none such at pos.
TRACE_CBOR_HD inline void cbor_head_min(const CborSpan& s, uint64_t pos, int max_bytes, uint32_t& major, uint64_t& arg,
                                        uint32_t& adv) {
  adv = 0;
  major = 0;
  arg = 0;
  const uint32_t b = cbor_at(s, pos);
  if (b == CBOR_END) return;
  major = b >> 5;
  const uint32_t ai = b & 31u;
  if (ai < 24) {
    arg = ai;
    adv = 1;
    return;
  }
  if (ai > 27) return;
  const int nb = 1 << (ai - 24);
  if (1 + nb > max_bytes) return;
  uint64_t v = 0;
  for (int k = 0; k < nb; k++) {
    const uint32_t c = cbor_at(s, pos + 1 + (uint64_t)k);
    if (c == CBOR_END) return;
    v = (v << 8) | c;
  }
  // minimal: the value needs this many bytes
  const uint64_t floor_v = nb == 1 ? 24u : nb == 2 ? 0x100ull : nb == 4 ? 0x10000ull : 0x100000000ull;
  if (v < floor_v) return;
  arg = v;
  adv = 1u + (uint32_t)nb;
}
// a signed integer in [lo, hi] with a head of 1 to 3 bytes
TRACE_CBOR_HD inline bool cbor_small_int(const CborSpan& s, uint64_t& pos, int32_t lo, int32_t hi, int32_t& out) {
  uint32_t mj, adv;
  uint64_t v;
  cbor_head_min(s, pos, 3, mj, v, adv);
  if (!adv || mj > 1) return false;
  const int32_t x = mj ? -1 - (int32_t)v : (int32_t)v;  // v < 2^16
  if (x < lo || x > hi) return false;
  out = x;
  pos += adv;
  return true;
}

// ------------------------------------------------------------ the step parser
constexpr uint64_t CBOR_KEY_TAPES = 0x736570617465ull;    // 65 "tapes"
constexpr uint64_t CBOR_KEY_WRITE = 0x657469727765A2ull;  // A2 | 65 "write"
constexpr uint64_t CBOR_KEY_MV = 0x766D62ull;             // 62 "mv"
TRACE_CBOR_HD inline uint32_t cbor_step_min_len(uint32_t tau) { return 17u + (tau < 24 ? 1u : 2u) + 12u * tau; }
TRACE_CBOR_HD inline uint32_t cbor_step_max_len(uint32_t tau) { return 18u + (tau < 24 ? 1u : 2u) + 15u * tau; }
// One whole step record at pos, strictly: its end offset, or 0 at the first
// deviation (a wrong key byte, a non-minimal head, a value outside i8 / u16,
// the end of the bytes). Writes the step's input_mv and its tau tape cells
// (wsym = 0 where there is no write); what a failed parse has written is
// garbage the caller discards.
TRACE_CBOR_HD inline uint64_t cbor_parse_step(const CborSpan& s, uint64_t pos, uint32_t tau, int8_t* input_mv,
                                              int8_t* mv, uint8_t* has_write, uint16_t* wsym) {
  if (!cbor_match(s, pos, CBOR_SIG_LO, 8) || !cbor_match(s, pos + 8, CBOR_SIG_HI, 2)) return 0;
  pos += TRACE_CBOR_SIG_LEN;
  int32_t x;
  if (!cbor_small_int(s, pos, -128, 127, x)) return 0;
  *input_mv = (int8_t)x;
  if (!cbor_match(s, pos, CBOR_KEY_TAPES, 6)) return 0;
  pos += 6;
  if (tau < 24) {
    if (cbor_at(s, pos) != (0x80u | tau)) return 0;
    pos += 1;
  } else {
    if (cbor_at(s, pos) != 0x98u || cbor_at(s, pos + 1) != tau) return 0;
    pos += 2;
  }
  for (uint32_t r = 0; r < tau; r++) {
    if (!cbor_match(s, pos, CBOR_KEY_WRITE, 7)) return 0;
    pos += 7;
    if (cbor_at(s, pos) == 0xF6u) {
      pos += 1;
      has_write[r] = 0;
      wsym[r] = 0;
    } else {
      if (!cbor_small_int(s, pos, 0, 65535, x)) return 0;
      has_write[r] = 1;
      wsym[r] = (uint16_t)x;
    }
    if (!cbor_match(s, pos, CBOR_KEY_MV, 3)) return 0;
    pos += 3;
    if (!cbor_small_int(s, pos, -128, 127, x)) return 0;
    mv[r] = (int8_t)x;
  }
  return pos;
}

// ------------------------------------------------------------ the head
struct TraceCborHead {
  uint64_t t = 0;
  uint32_t tau = 0;
  uint64_t steps_off = 0;  // the first byte after the array head
};
// true: the bytes start with a canonical head whose t steps can fit the rest
inline bool trace_cbor_head(const CborSpan& s, TraceCborHead& h) {
  uint64_t pos = 0, v;
  uint32_t mj, adv;
  if (cbor_at(s, pos) != 0xA4u) return false;
  pos += 1;
  if (!cbor_match(s, pos, 0x6E6F697372657667ull, 8)) return false;  // 67 "version"
  pos += 8;
  cbor_head_min(s, pos, 9, mj, v, adv);
  if (!adv || mj != 0) return false;
  pos += adv;
  if (!cbor_match(s, pos, 0x75617463ull, 4)) return false;  // 63 "tau"
  pos += 4;
  cbor_head_min(s, pos, 9, mj, v, adv);
  if (!adv || mj != 0 || v > 255) return false;
  h.tau = (uint32_t)v;
  pos += adv;
  if (!cbor_match(s, pos, 0x737065747365ull, 6)) return false;  // 65 "steps"
  pos += 6;
  cbor_head_min(s, pos, 9, mj, v, adv);
  if (!adv || mj != 4) return false;
  pos += adv;
  if (pos > s.len || v > (s.len - pos) / cbor_step_min_len(h.tau)) return false;
  h.t = v;
  h.steps_off = pos;
  return true;
}

// ------------------------------------------------------------ the verdict
// what the parse pass leaves for the chain check: the first step that did not
// parse, the first link c[i] + len_i = c[i + 1] (or c[0] = steps_off, index 0)
// that does not hold, both ~0 when none, and the end of step t - 1
struct TraceCborVerdict {
  uint64_t candidates;
  uint64_t bad_step;
  uint64_t bad_link;
  uint64_t tail_off;
};
// How a failing index is lowered into a verdict word is all that differs
// between the device and a serial run: an atomic minimum there (cbor_decode.hip),
// this one here.
struct CborSerialMin {
  void operator()(uint64_t* word, uint64_t i) const {
    if (i < *word) *word = i;
  }
};

// ------------------------------------------------------------ the step pass
// Index i of the parse pass: step i from candidate i into row i of the arrays
// (t and t * tau elements), and its link: step 0 starts at lo, step i + 1
// where step i ends. With fewer than t candidates nothing is parsed. V starts
// as all ones but for candidates.
template <class Min>
TRACE_CBOR_HD inline void trace_cbor_step_pass(const CborSpan& s, uint64_t lo, const uint64_t* cand, uint64_t t,
                                               uint32_t tau, int8_t* input_mv, int8_t* mv, uint8_t* has_write,
                                               uint16_t* wsym, TraceCborVerdict* V, uint64_t i, Min lower) {
  if (i >= t || V->candidates < t) return;
  const uint64_t c = cand[i], o = i * tau;
  const uint64_t end = cbor_parse_step(s, c, tau, input_mv + i, mv + o, has_write + o, wsym + o);
  if (!end) {
    lower(&V->bad_step, i);
    return;
  }
  if (i == 0 && c != lo) lower(&V->bad_link, 0);
  if (i + 1 < t) {
    if (cand[i + 1] != end) lower(&V->bad_link, i + 1);
  } else {
    V->tail_off = end;
  }
}

// What the host makes of the verdict: SEZKP_INGEST_R_* by value (sezkp_stark.h)
// and the index that goes with it; 0: the steps are taken, the tail at
// v.tail_off is the caller's to check (codec.cpp's trace_cbor_tail_ok). A file
// of no steps has the verdict {0, ~0, ~0, steps_off}. Shared with the check tool.
struct CborDecision {
  uint32_t reason = 0;
  uint64_t index = 0;
};
inline CborDecision trace_cbor_decide(const TraceCborVerdict& v, const TraceCborHead& h) {
  CborDecision d;
  if (v.candidates < h.t) d.reason = 2;
  else if (v.bad_step != ~0ull && v.bad_step <= v.bad_link) d.reason = 3, d.index = v.bad_step;
  else if (v.bad_link != ~0ull) d.reason = 4, d.index = v.bad_link;
  return d;
}

}  // namespace sezkp
