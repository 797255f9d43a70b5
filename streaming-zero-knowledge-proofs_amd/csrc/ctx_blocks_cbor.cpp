// ctx_blocks_cbor.cpp — a context's block-file ingest (prover_ctx.h): the
// CBOR bytes of a Vec<BlockSummary> go to the device, blocks_cbor.hip decodes
// them there into the block tables and the four step arrays, and the host
// decides on the verdict words that come home (blocks_cbor_plan.h). Only the
// block tables follow them home: the step arrays stay in the context's ingest
// buffers until sezkp_ctx_upload_ingested copies them, device to device, into
// the trace image. A file the device path declines, for whatever reason, is
// decoded by the host pull parser (codec.cpp), which alone words the errors.
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <string>

#include "prover_ctx.h"

namespace sezkp::detail {
void BlocksCborBuffers::release() {
  for (void* p : {(void*)d_counts, (void*)d_offs, (void*)d_cand, (void*)d_ends, (void*)d_tables, (void*)d_verdict})
    if (p) (void)hipFree(p);
  if (h_verdict) (void)hipHostFree(h_verdict);
  *this = BlocksCborBuffers{};
}
}  // namespace sezkp::detail

// true: the block fields and step_start are in `out`, the step arrays in
// cbor.d_arrays (st synchronised), `steps` points at them. false: declined,
// bcbor.info.reason says why. Throws only for device errors.
bool sezkp_ctx::decode_blocks_cbor_device(const uint8_t* data, size_t len, BlockStore& out, sezkp_block_view& steps) {
  sezkp_blocks_ingest_info& info = bcbor.info;
  const char* force = getenv("SEZKP_BLOCKS_CBOR_HOST");  // read per call
  if (force && !strcmp(force, "1")) {
    info.reason = SEZKP_BLOCKS_R_FORCED;
    return false;
  }
  BlocksCborHead h;
  if (!blocks_cbor_head(CborSpan{data, len}, h)) {
    info.reason = SEZKP_BLOCKS_R_HEAD;
    return false;
  }
  info.n_blocks = h.n_blocks;
  info.tau = h.tau;
  const uint64_t B = h.n_blocks, t_max = h.t_max, cells = t_max * h.tau;  // t_max <= len / 18, B <= len / 186
  HIP_OR_THROW(hipSetDevice(device));
  // buffers of an earlier call may still be read by the upload it fed
  HIP_OR_THROW(hipStreamSynchronize(st));
  cbor_grow(cbor.d_arrays, cbor.arrays_cap, (size_t)(4 * cells + t_max));
  uint16_t* d_ws = reinterpret_cast<uint16_t*>(cbor.d_arrays);
  int8_t* d_mv = reinterpret_cast<int8_t*>(cbor.d_arrays + 2 * cells);
  uint8_t* d_hw = cbor.d_arrays + 3 * cells;
  int8_t* d_imv = reinterpret_cast<int8_t*>(cbor.d_arrays + 4 * cells);
  const size_t ntiles = (size_t)trace_cbor_tiles(len);
  auto tile_words = [&](uint32_t*& counts, uint64_t*& offs, size_t& cap) {
    if (ntiles <= cap && counts) return;
    size_t c0 = 0, c1 = 0;
    if (counts) (void)hipFree(counts);
    if (offs) (void)hipFree(offs);
    counts = nullptr;
    offs = nullptr;
    cap = 0;
    cbor_grow(counts, c0, ntiles * 4);
    cbor_grow(offs, c1, ntiles * 8);
    cap = ntiles;
  };
  tile_words(cbor.d_counts, cbor.d_offs, cbor.tiles_cap);
  tile_words(bcbor.d_counts, bcbor.d_offs, bcbor.tiles_cap);
  cbor_grow(cbor.d_cand, cbor.cand_cap, (size_t)t_max * 8);
  cbor_grow(bcbor.d_cand, bcbor.cand_cap, (size_t)B * 8);
  cbor_grow(bcbor.d_ends, bcbor.ends_cap, (size_t)t_max * 8);
  const size_t tab_bytes = blocks_cbor_tables_bytes(B, h.tau);
  cbor_grow(bcbor.d_tables, bcbor.tables_cap, tab_bytes);
  if (!bcbor.d_verdict) {
    void* q = nullptr;
    HIP_OR_THROW(hipMalloc(&q, sizeof(BlocksCborVerdict)));
    bcbor.d_verdict = static_cast<BlocksCborVerdict*>(q);
    HIP_OR_THROW(hipHostMalloc(&q, sizeof(BlocksCborVerdict), hipHostMallocDefault));
    bcbor.h_verdict = static_cast<BlocksCborVerdict*>(q);
  }
  cbor_bytes_to_device(data, len);
  const BlocksCborTables dT = blocks_cbor_tables_at(bcbor.d_tables, B, h.tau);
  HIP_OR_THROW(launch_blocks_cbor_decode(st, cbor.d_bytes, len, h.first_off, B, h.tau, t_max, bcbor.d_counts,
                                         cbor.d_counts, bcbor.d_offs, cbor.d_offs, bcbor.d_cand, cbor.d_cand,
                                         bcbor.d_ends, dT, d_imv, d_mv, d_hw, d_ws, bcbor.d_verdict));
  HIP_OR_THROW(hipEventRecord(cbor.ev[2], st));
  HIP_OR_THROW(hipMemcpyAsync(bcbor.h_verdict, bcbor.d_verdict, sizeof(BlocksCborVerdict), hipMemcpyDeviceToHost, st));
  HIP_OR_THROW(hipStreamSynchronize(st));
  float ms = 0;
  HIP_OR_THROW(hipEventElapsedTime(&ms, cbor.ev[0], cbor.ev[1]));
  info.ms_h2d = ms;
  HIP_OR_THROW(hipEventElapsedTime(&ms, cbor.ev[1], cbor.ev[2]));
  info.ms_decode = ms;
  const BlocksCborVerdict& v = *bcbor.h_verdict;
  info.block_candidates = v.block_candidates;
  info.step_candidates = v.step_candidates;
  const BlocksCborDecision d = blocks_cbor_decide(v, h);
  if (d.reason) {
    info.reason = d.reason;
    info.index = d.index;
    return false;
  }
  // ---- the tables come home: one copy, then into the store's vectors
  std::vector<uint64_t> home((tab_bytes + 7) / 8);
  HIP_OR_THROW(hipMemcpyAsync(home.data(), bcbor.d_tables, tab_bytes, hipMemcpyDeviceToHost, st));
  HIP_OR_THROW(hipStreamSynchronize(st));
  const BlocksCborTables T = blocks_cbor_tables_at(reinterpret_cast<uint8_t*>(home.data()), B, h.tau);
  const size_t nb = (size_t)B, nt = nb * h.tau;
  out = BlockStore();
  out.tau = h.tau;
  out.version.assign(T.version, T.version + nb);
  out.block_id.assign(T.block_id, T.block_id + nb);
  out.step_lo.assign(T.step_lo, T.step_lo + nb);
  out.step_hi.assign(T.step_hi, T.step_hi + nb);
  out.ctrl_in.assign(T.ctrl_in, T.ctrl_in + nb);
  out.ctrl_out.assign(T.ctrl_out, T.ctrl_out + nb);
  out.in_head_in.assign(T.in_head_in, T.in_head_in + nb);
  out.in_head_out.assign(T.in_head_out, T.in_head_out + nb);
  out.win_left.assign(T.win_left, T.win_left + nt);
  out.win_right.assign(T.win_right, T.win_right + nt);
  out.off_in.assign(T.off_in, T.off_in + nt);
  out.off_out.assign(T.off_out, T.off_out + nt);
  out.step_start.assign(T.step_start, T.step_start + nb);
  out.step_start.push_back(v.t);
  out.bind();
  info.t = v.t;
  steps = sezkp_block_view{};
  steps.input_mv = d_imv;
  steps.mv = d_mv;
  steps.has_write = d_hw;
  steps.wsym = d_ws;
  return true;
}

void sezkp_ctx::decode_blocks_cbor(const uint8_t* data, size_t len, BlockStore& out, sezkp_block_view& steps) {
  bcbor.drop_pending();
  bcbor.info = sezkp_blocks_ingest_info{};
  bcbor.info.bytes = len;
  bcbor.have_info = true;
  if (decode_blocks_cbor_device(data, len, out, steps)) {
    bcbor.info.path = SEZKP_INGEST_DEVICE;
    return;
  }
  bcbor.info.path = SEZKP_INGEST_HOST;
  using clk = std::chrono::steady_clock;
  const auto t0 = clk::now();
  std::string e;
  const bool ok = sezkp::decode_blocks_cbor(data, len, out, e);
  bcbor.info.ms_host = std::chrono::duration<double, std::milli>(clk::now() - t0).count();
  if (!ok) throw Err{SEZKP_E_DECODE, e};
  // the shape of what was decoded, whatever the head said (or did not say)
  bcbor.info.n_blocks = out.view.n_blocks;
  bcbor.info.tau = out.tau;
  bcbor.info.t = out.input_mv.size();
  steps = out.view;
}

void sezkp_ctx::ingest_blocks_cbor(const uint8_t* data, size_t len) {
  sezkp_block_view steps{};
  decode_blocks_cbor(data, len, bcbor.pend, steps);
  bcbor.steps = steps;
  bcbor.pending = true;
}

// sezkp_ctx_upload of the pending ingest: the block tables from the host, the
// step arrays from where the decode left them. On a sharded context only the
// rows of the rank's blocks are handed on (sezkp_shard_rows).
void sezkp_ctx::upload_ingested() {
  if (!bcbor.pending) throw Err{SEZKP_E_INVALID, "upload_ingested: no ingest is pending (call sezkp_ctx_ingest_blocks_cbor)"};
  struct Drop {
    BlocksCborBuffers& b;
    ~Drop() { b.drop_pending(); }
  } drop{bcbor};
  bcbor.pend.bind();
  sezkp_block_view v = bcbor.pend.view;
  const uint32_t nblk = v.n_blocks, tau = v.tau;
  uint64_t row0 = 0, nrows = ~0ull;
  const uint64_t n = nblk ? v.step_start[nblk] : 0;
  if (sharded() && world > 1 && n && !(n & (n - 1)) && v.step_start[0] == 0) {
    const int logn = ilog2(n);
    if (logn >= 12 + logP) {
      uint64_t ch_lo, ch_hi;
      uint32_t blk_lo, blk_cnt;
      shard_range(v.step_start, nblk, logn, rank, logP, ch_lo, ch_hi, blk_lo, blk_cnt);
      row0 = v.step_start[blk_lo];
      nrows = v.step_start[blk_lo + blk_cnt] - row0;
    }
  }
  v.input_mv = bcbor.steps.input_mv + row0;
  v.mv = bcbor.steps.mv + row0 * tau;
  v.has_write = bcbor.steps.has_write + row0 * tau;
  v.wsym = bcbor.steps.wsym + row0 * tau;
  upload(v, row0, nrows);
}
