// abi_host.cpp — the part of the C ABI (include/sezkp_stark.h) that never
// touches the device: versions, the codecs of blocks, traces and manifests,
// the manifest commitment, the simulator. No HIP header: it also builds with a
// plain host compiler, which is how tools/host_abi_check.cpp runs it under the
// sanitizers.
#include <memory>
#include <new>
#include <string>
#include <vector>

#include "abi_blocks.h"
#include "abi_util.h"
#include "codec.h"
#include "host_crypto.h"
#include "blocks_cbor_plan.h"
#include "trace_cbor_plan.h"
#include "trace_plan.h"

using namespace sezkp;

extern "C" {

uint32_t sezkp_abi_version(void) { return SEZKP_ABI_VERSION; }
const char* sezkp_version(void) { return "sezkp-mi355x 0.1.0 (stark-v1, gfx950)"; }

void sezkp_buf_free(sezkp_buf* b) {
  if (b && b->data) {
    free(b->data);
    b->data = nullptr;
    b->len = 0;
  }
}

// ---------------------------------------------------------- host helpers
int32_t sezkp_manifest_root(const sezkp_block_view* blocks, uint8_t out[32]) {
  if (!blocks || !out) return SEZKP_E_INVALID;
  manifest_root(*blocks, out);
  return SEZKP_OK;
}
int32_t sezkp_manifest_frontier_root(const sezkp_block_view* blocks, uint8_t out[32]) {
  if (!blocks || !out) return SEZKP_E_INVALID;
  manifest_frontier_root(*blocks, out);
  return SEZKP_OK;
}

// a sharded rank's rows and blocks of a raw trace (trace_plan.h: what
// sezkp_shard_rows gives for the uniform boundaries of (t, b), in closed form)
int32_t sezkp_trace_shard_rows(uint64_t t, uint32_t b, int32_t rank, int32_t world, uint64_t* row0, uint64_t* nrows) {
  TraceShard s;
  if (!row0 || !nrows || !trace_shard_plan(t, b, rank, world, s)) return SEZKP_E_INVALID;
  *row0 = s.row0;
  *nrows = s.nrows;
  return SEZKP_OK;
}
int32_t sezkp_trace_shard_blocks(uint64_t t, uint32_t b, int32_t rank, int32_t world, uint32_t* blk_lo,
                                 uint32_t* blk_cnt, uint32_t* own_lo, uint32_t* own_cnt) {
  TraceShard s;
  if (!blk_lo || !blk_cnt || !own_lo || !own_cnt || !trace_shard_plan(t, b, rank, world, s)) return SEZKP_E_INVALID;
  *blk_lo = s.blk_lo;
  *blk_cnt = s.blk_cnt;
  *own_lo = s.own_lo;
  *own_cnt = s.own_cnt;
  return SEZKP_OK;
}

// TraceFile CBOR (sezkp-trace io.rs; format.rs:59-68)
int32_t sezkp_trace_decode_cbor(const uint8_t* data, size_t len, sezkp_trace** out, char* err, size_t err_len) {
  if (!out || (!data && len)) return SEZKP_E_INVALID;
  try {
    std::unique_ptr<sezkp_trace> t(new sezkp_trace());
    std::string e;
    if (!decode_trace_cbor(data, len, t->s, e)) {
      set_err(err, err_len, e);
      return SEZKP_E_DECODE;
    }
    t->bind();
    *out = t.release();
    return SEZKP_OK;
  } catch (const std::exception& e) {
    set_err(err, err_len, e.what());
    return SEZKP_E_NOMEM;
  }
}
int32_t sezkp_trace_encode_cbor(const sezkp_trace_view* trace, sezkp_buf* out) {
  try {
    if (!trace || !out || trace->tau > 255 ||
        (trace->t && (!trace->input_mv || (trace->tau && (!trace->mv || !trace->has_write || !trace->wsym)))))
      return SEZKP_E_INVALID;
    to_buf(encode_trace_cbor(*trace), out);
    return SEZKP_OK;
  } catch (const Err& e) {
    return e.code;
  } catch (const std::exception&) {
    return SEZKP_E_NOMEM;
  }
}
// the canonical head the device decoder takes (trace_cbor_plan.h)
int32_t sezkp_trace_cbor_head(const uint8_t* data, size_t len, uint64_t* t, uint32_t* tau, uint64_t* steps_off) {
  TraceCborHead h;
  if (!data || !t || !tau || !steps_off || !trace_cbor_head(CborSpan{data, len}, h)) return 0;
  *t = h.t;
  *tau = h.tau;
  *steps_off = h.steps_off;
  return 1;
}
// the canonical head of a block file the device decoder takes (blocks_cbor_plan.h)
int32_t sezkp_blocks_cbor_head(const uint8_t* data, size_t len, uint32_t* n_blocks, uint32_t* tau, uint64_t* first_off) {
  BlocksCborHead h;
  if (!data || !n_blocks || !tau || !first_off || !blocks_cbor_head(CborSpan{data, len}, h)) return 0;
  *n_blocks = h.n_blocks;
  *tau = h.tau;
  *first_off = h.first_off;
  return 1;
}
const sezkp_trace_view* sezkp_trace_view_of(const sezkp_trace* t) { return t ? &t->view : nullptr; }
void sezkp_trace_free(sezkp_trace* t) { delete t; }

int32_t sezkp_blocks_decode_jsonl_meta(const uint8_t* data, size_t len, uint64_t lo, uint64_t hi, sezkp_blocks** out,
                                       char* err, size_t err_len) {
  return sezkp_blocks_decode_jsonl_lines(data, len, lo, hi, 0, out, err, err_len);
}
int32_t sezkp_blocks_decode_jsonl_lines(const uint8_t* data, size_t len, uint64_t lo, uint64_t hi, int32_t steps,
                                        sezkp_blocks** out, char* err, size_t err_len) {
  if (!out || (!data && len) || lo > hi) return SEZKP_E_INVALID;
  std::unique_ptr<sezkp_blocks> b(new sezkp_blocks());
  std::string e;
  if (!decode_blocks_jsonl_meta(reinterpret_cast<const char*>(data), len, lo, hi, b->s, b->line_off, e, steps != 0)) {
    set_err(err, err_len, e);
    return SEZKP_E_DECODE;
  }
  *out = b.release();
  return SEZKP_OK;
}
int32_t sezkp_blocks_line_offsets(const sezkp_blocks* b, const uint64_t** offsets, size_t* n) {
  if (!b || !offsets || !n) return SEZKP_E_INVALID;
  *offsets = b->line_off.data();
  *n = b->line_off.size();
  return SEZKP_OK;
}
int32_t sezkp_manifest_leaf_hashes(const sezkp_block_view* blocks, uint8_t* out) {
  if (!blocks || (!out && blocks->n_blocks)) return SEZKP_E_INVALID;
  for (uint32_t k = 0; k < blocks->n_blocks; k++) manifest_leaf_hash(*blocks, k, out + 32ull * k);
  return SEZKP_OK;
}
int32_t sezkp_merkle_root_of_leaves(const uint8_t* leaves, size_t n, int32_t frontier, uint8_t out[32]) {
  if (!out || (!leaves && n)) return SEZKP_E_INVALID;
  merkle_root_of_leaves(leaves, n, frontier != 0, out);
  return SEZKP_OK;
}
int32_t sezkp_blocks_decode_cbor(const uint8_t* data, size_t len, sezkp_blocks** out, char* err, size_t err_len) {
  if (!out || (!data && len)) return SEZKP_E_INVALID;
  std::unique_ptr<sezkp_blocks> b(new sezkp_blocks());
  std::string e;
  if (!decode_blocks_cbor(data, len, b->s, e)) {
    set_err(err, err_len, e);
    return SEZKP_E_DECODE;
  }
  *out = b.release();
  return SEZKP_OK;
}
int32_t sezkp_blocks_decode_jsonl(const uint8_t* data, size_t len, sezkp_blocks** out, char* err, size_t err_len) {
  if (!out || (!data && len)) return SEZKP_E_INVALID;
  std::unique_ptr<sezkp_blocks> b(new sezkp_blocks());
  std::string e;
  if (!decode_blocks_jsonl(reinterpret_cast<const char*>(data), len, b->s, e)) {
    set_err(err, err_len, e);
    return SEZKP_E_DECODE;
  }
  *out = b.release();
  return SEZKP_OK;
}
// `sezkp-cli simulate --t T --b b --tau tau` (main.rs:317-350): generate_trace
// (tracegen.cpp, rand 0.9 StdRng bit-exact; the reference fixes seed 42) +
// partition_trace into blocks of b steps.
int32_t sezkp_simulate_blocks(uint64_t t, uint32_t b, uint32_t tau, uint64_t seed, sezkp_blocks** out, char* err,
                              size_t err_len) {
  try {
    if (!out || b == 0 || tau > 255 || t == 0 || t > (1ULL << 32)) {
      set_err(err, err_len, "simulate: need 0 < t <= 2^32, b > 0, tau <= 255");
      return SEZKP_E_INVALID;
    }
    std::vector<int8_t> imv(t), mv(t * tau);
    std::vector<uint8_t> hw(t * tau);
    std::vector<uint16_t> ws(t * tau);
    int32_t rc = sezkp_simulate_trace(t, tau, seed, imv.data(), mv.data(), hw.data(), ws.data());
    if (rc != SEZKP_OK) return rc;
    std::unique_ptr<sezkp_blocks> bl(new sezkp_blocks());
    partition_trace(bl->s, t, tau, b, imv.data(), mv.data(), hw.data(), ws.data());
    *out = bl.release();
    return SEZKP_OK;
  } catch (const std::bad_alloc&) {
    set_err(err, err_len, "simulate: out of host memory");
    return SEZKP_E_NOMEM;
  }
}
int32_t sezkp_blocks_encode_cbor(const sezkp_block_view* blocks, sezkp_buf* out) {
  try {
    if (!blocks || !out) return SEZKP_E_INVALID;
    to_buf(encode_blocks_cbor(*blocks), out);
    return SEZKP_OK;
  } catch (const std::exception&) {
    return SEZKP_E_NOMEM;
  }
}
int32_t sezkp_blocks_encode_jsonl(const sezkp_block_view* blocks, sezkp_buf* out) {
  try {
    if (!blocks || !out) return SEZKP_E_INVALID;
    to_buf(encode_blocks_jsonl(*blocks), out);
    return SEZKP_OK;
  } catch (const Err& e) {
    return e.code;
  } catch (const std::exception&) {
    return SEZKP_E_NOMEM;
  }
}
int32_t sezkp_manifest_decode(const uint8_t* data, size_t len, int32_t is_json, uint8_t root[32],
                              uint32_t* n_leaves, char* err, size_t err_len) {
  if (!data || !root) return SEZKP_E_INVALID;
  std::string e;
  const bool ok = is_json ? decode_manifest_json(reinterpret_cast<const char*>(data), len, root, n_leaves, e)
                          : decode_manifest_cbor(data, len, root, n_leaves, e);
  if (!ok) {
    set_err(err, err_len, e);
    return SEZKP_E_DECODE;
  }
  return SEZKP_OK;
}
const sezkp_block_view* sezkp_blocks_view(const sezkp_blocks* b) { return b ? &b->s.view : nullptr; }
void sezkp_blocks_free(sezkp_blocks* b) { delete b; }
void sezkp_blake3(const uint8_t* data, size_t len, uint8_t* out, size_t out_len) {
  Blake3 h;
  h.update(data, len);
  h.finalize(out, out_len);
}

}  // extern "C"
