// ctx_cbor.cpp — a context's ingest of CBOR files (prover_ctx.h): a TraceFile
// or a block file (Vec<BlockSummary>). The file's bytes go to the device,
// cbor_decode.hip decodes them there into the four step arrays (and, for a
// block file, the block tables), and the host decides on the verdict words
// that come home (trace_cbor_plan.h, blocks_cbor_plan.h). Of a block file only
// the tables follow them home: the step arrays stay in the context's ingest
// buffers until sezkp_ctx_upload_ingested copies them, device to device, into
// the trace image. A file the device path declines, for whatever reason, is
// decoded by the host pull parser (codec.cpp), which alone words the errors.
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <string>

#include "prover_ctx.h"

// ------------------------------------------------------------ the shared blocks
namespace sezkp::detail {
void cbor_grow(void** p, size_t& cap, size_t bytes) {
  if (*p && bytes <= cap) return;
  if (*p) (void)hipFree(*p);
  *p = nullptr;
  cap = 0;
  const size_t want = bytes + bytes / 4 + 64;
  HIP_OR_THROW(hipMalloc(p, want));
  cap = want;
}
void CborBuffers::release() {
  for (void* p : {(void*)d_bytes, (void*)d_counts[0], (void*)d_counts[1], (void*)d_offs[0], (void*)d_offs[1],
                  (void*)d_cand[0], (void*)d_cand[1], (void*)d_ends, (void*)d_tables, (void*)d_arrays, d_verdict})
    if (p) (void)hipFree(p);
  if (h_verdict) (void)hipHostFree(h_verdict);
  if (h_stage) (void)hipHostFree(h_stage);
  for (auto& e : stage_ev)
    if (e) (void)hipEventDestroy(e);
  for (auto& e : ev)
    if (e) (void)hipEventDestroy(e);
  *this = CborBuffers{};
}
CborStepArrays CborBuffers::step_arrays(uint64_t rows, uint32_t tau) {
  const uint64_t cells = rows * tau;
  cbor_grow(d_arrays, arrays_cap, (size_t)(4 * cells + rows));
  return {reinterpret_cast<uint16_t*>(d_arrays), reinterpret_cast<int8_t*>(d_arrays + 2 * cells), d_arrays + 3 * cells,
          reinterpret_cast<int8_t*>(d_arrays + 4 * cells)};
}
void CborBuffers::tile_words(int kind, size_t ntiles) {
  if (ntiles <= tiles_cap[kind] && d_counts[kind]) return;
  size_t c0 = 0, c1 = 0;
  if (d_counts[kind]) (void)hipFree(d_counts[kind]);
  if (d_offs[kind]) (void)hipFree(d_offs[kind]);
  d_counts[kind] = nullptr;
  d_offs[kind] = nullptr;
  tiles_cap[kind] = 0;
  cbor_grow(d_counts[kind], c0, ntiles * 4);
  cbor_grow(d_offs[kind], c1, ntiles * 8);
  tiles_cap[kind] = ntiles;
}
void CborBuffers::verdict_pair() {
  if (d_verdict) return;
  HIP_OR_THROW(hipMalloc(&d_verdict, VERDICT_BYTES));
  HIP_OR_THROW(hipHostMalloc(&h_verdict, VERDICT_BYTES, hipHostMallocDefault));
}
}  // namespace sezkp::detail

namespace {
// page-locked host memory the runtime knows (hipHostMalloc, hipHostRegister):
// copied from directly; anything else goes through the staging block
bool host_pinned(const void* p) {
  hipPointerAttribute_t a{};
  if (hipPointerGetAttributes(&a, p) != hipSuccess) {
    (void)hipGetLastError();  // not an error of ours
    return false;
  }
  return a.type == hipMemoryTypeHost;
}
// SEZKP_TRACE_CBOR_HOST=1 / SEZKP_BLOCKS_CBOR_HOST=1, read per call
bool forced_to_host(const char* env) {
  const char* force = getenv(env);
  return force && !strcmp(force, "1");
}
// The device path's answer, or else the host pull parser's, timed: a refusal
// of its is Err SEZKP_E_DECODE with its message.
template <class Info, class Device, class Host>
void device_else_host(Info& info, Device device, Host host) {
  if (device()) {
    info.path = SEZKP_INGEST_DEVICE;
    return;
  }
  info.path = SEZKP_INGEST_HOST;
  using clk = std::chrono::steady_clock;
  const auto t0 = clk::now();
  std::string e;
  const bool ok = host(e);
  info.ms_host = std::chrono::duration<double, std::milli>(clk::now() - t0).count();
  if (!ok) throw Err{SEZKP_E_DECODE, e};
}
}  // namespace

void sezkp_ctx::cbor_claim() {
  HIP_OR_THROW(hipSetDevice(device));
  HIP_OR_THROW(hipStreamSynchronize(st));
  bcbor.drop_pending();
}

void sezkp_ctx::cbor_stage_block() {
  if (cbuf.h_stage) return;
  void* q = nullptr;
  HIP_OR_THROW(hipHostMalloc(&q, 2 * CborBuffers::STAGE_HALF, hipHostMallocDefault));
  cbuf.h_stage = static_cast<uint8_t*>(q);
  for (auto& e : cbuf.stage_ev) HIP_OR_THROW(hipEventCreateWithFlags(&e, hipEventDisableTiming));
}

void sezkp_ctx::cbor_bytes_to_device(const uint8_t* data, size_t len) {
  for (auto& e : cbuf.ev)
    if (!e) HIP_OR_THROW(hipEventCreate(&e));
  cbor_grow(cbuf.d_bytes, cbuf.bytes_cap, len);
  // ---- the bytes: straight from pinned memory, else through the staging block
  HIP_OR_THROW(hipEventRecord(cbuf.ev[0], st));
  if (host_pinned(data)) {
    copy_chunked(cbuf.d_bytes, data, len, COPY_CHUNK, hipMemcpyHostToDevice, st);
  } else {
    constexpr size_t H = CborBuffers::STAGE_HALF;
    cbor_stage_block();
    size_t k = 0;
    for (size_t o = 0; o < len; k++) {
      const size_t n = std::min(H, len - o), half = k & 1;
      if (k >= 2) HIP_OR_THROW(hipEventSynchronize(cbuf.stage_ev[half]));  // the half's previous copy
      memcpy(cbuf.h_stage + half * H, data + o, n);
      HIP_OR_THROW(hipMemcpyAsync(cbuf.d_bytes + o, cbuf.h_stage + half * H, n, hipMemcpyHostToDevice, st));
      HIP_OR_THROW(hipEventRecord(cbuf.stage_ev[half], st));
      o += n;
    }
  }
  HIP_OR_THROW(hipEventRecord(cbuf.ev[1], st));
}

const void* sezkp_ctx::cbor_verdict_home(size_t bytes, double& ms_h2d, double& ms_decode) {
  HIP_OR_THROW(hipEventRecord(cbuf.ev[2], st));
  HIP_OR_THROW(hipMemcpyAsync(cbuf.h_verdict, cbuf.d_verdict, bytes, hipMemcpyDeviceToHost, st));
  HIP_OR_THROW(hipStreamSynchronize(st));
  float ms = 0;
  HIP_OR_THROW(hipEventElapsedTime(&ms, cbuf.ev[0], cbuf.ev[1]));
  ms_h2d = ms;
  HIP_OR_THROW(hipEventElapsedTime(&ms, cbuf.ev[1], cbuf.ev[2]));
  ms_decode = ms;
  return cbuf.h_verdict;
}

// ------------------------------------------------------------ a TraceFile
// true: the arrays are in cbuf.d_arrays (st synchronised), tv points at them.
// false: declined, cbor.info.reason says why. Throws only for device errors.
bool sezkp_ctx::decode_trace_cbor_device(const uint8_t* data, size_t len, sezkp_trace_view& tv) {
  sezkp_trace_ingest_info& info = cbor.info;
  if (forced_to_host("SEZKP_TRACE_CBOR_HOST")) {
    info.reason = SEZKP_INGEST_R_FORCED;
    return false;
  }
  TraceCborHead h;
  if (!trace_cbor_head(CborSpan{data, len}, h)) {
    info.reason = SEZKP_INGEST_R_HEAD;
    return false;
  }
  info.t = h.t;
  info.tau = h.tau;
  const uint64_t t = h.t;  // t <= len / 18
  cbor_claim();
  const CborStepArrays A = cbuf.step_arrays(t, h.tau);
  TraceCborVerdict v{0, ~0ull, ~0ull, h.steps_off};  // of a file of no steps
  if (t) {
    cbuf.tile_words(0, (size_t)trace_cbor_tiles(len));
    cbor_grow(cbuf.d_cand[0], cbuf.cand_cap[0], (size_t)t * 8);
    cbuf.verdict_pair();
    cbor_bytes_to_device(data, len);
    HIP_OR_THROW(launch_trace_cbor_decode(st, cbuf.d_bytes, len, h.steps_off, t, h.tau, cbuf.d_counts[0], cbuf.d_offs[0],
                                          cbuf.d_cand[0], A.input_mv, A.mv, A.has_write, A.wsym,
                                          static_cast<TraceCborVerdict*>(cbuf.d_verdict)));
    v = *static_cast<const TraceCborVerdict*>(cbor_verdict_home(sizeof v, info.ms_h2d, info.ms_decode));
    info.candidates = v.candidates;
  }
  const CborDecision d = trace_cbor_decide(v, h);
  if (d.reason) {
    info.reason = d.reason;
    info.index = d.index;
    return false;
  }
  if (v.tail_off > len || !trace_cbor_tail_ok(data, len, (size_t)v.tail_off)) {
    info.reason = SEZKP_INGEST_R_TAIL;
    return false;
  }
  tv = sezkp_trace_view{};
  tv.t = t;
  tv.tau = h.tau;
  tv.input_mv = A.input_mv;
  tv.mv = A.mv;
  tv.has_write = A.has_write;
  tv.wsym = A.wsym;
  return true;
}

void sezkp_ctx::decode_trace_cbor(const uint8_t* data, size_t len, BlockStore& host, sezkp_trace_view& tv) {
  cbor.info = sezkp_trace_ingest_info{};
  cbor.info.bytes = len;
  cbor.have_info = true;
  device_else_host(
      cbor.info, [&] { return decode_trace_cbor_device(data, len, tv); },
      [&](std::string& e) { return sezkp::decode_trace_cbor(data, len, host, e); });
  if (cbor.info.path == SEZKP_INGEST_DEVICE) return;
  // the shape of what was decoded, whatever the head said (or did not say)
  cbor.info.t = host.input_mv.size();
  cbor.info.tau = host.tau;
  tv = sezkp_trace_view{};
  tv.t = host.input_mv.size();
  tv.tau = host.tau;
  tv.input_mv = host.input_mv.data();
  tv.mv = host.mv.data();
  tv.has_write = host.has_write.data();
  tv.wsym = host.wsym.data();
}

// ------------------------------------------------------------ a block file
// true: the block fields and step_start are in `out`, the step arrays in
// cbuf.d_arrays (st synchronised), `steps` points at them. false: declined,
// bcbor.info.reason says why. Throws only for device errors.
bool sezkp_ctx::decode_blocks_cbor_device(const uint8_t* data, size_t len, BlockStore& out, sezkp_block_view& steps) {
  sezkp_blocks_ingest_info& info = bcbor.info;
  if (forced_to_host("SEZKP_BLOCKS_CBOR_HOST")) {
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
  const uint64_t B = h.n_blocks, t_max = h.t_max;  // t_max <= len / 18, B <= len / 186
  cbor_claim();
  const CborStepArrays A = cbuf.step_arrays(t_max, h.tau);
  const uint64_t caps[2] = {t_max, B};
  for (int kind = 0; kind < 2; kind++) {
    cbuf.tile_words(kind, (size_t)trace_cbor_tiles(len));
    cbor_grow(cbuf.d_cand[kind], cbuf.cand_cap[kind], (size_t)caps[kind] * 8);
  }
  cbor_grow(cbuf.d_ends, cbuf.ends_cap, (size_t)t_max * 8);
  const size_t tab_bytes = blocks_cbor_tables_bytes(B, h.tau);
  cbor_grow(cbuf.d_tables, cbuf.tables_cap, tab_bytes);
  cbuf.verdict_pair();
  cbor_bytes_to_device(data, len);
  const BlocksCborTables dT = blocks_cbor_tables_at(cbuf.d_tables, B, h.tau);
  HIP_OR_THROW(launch_blocks_cbor_decode(st, cbuf.d_bytes, len, h.first_off, B, h.tau, t_max, cbuf.d_counts, cbuf.d_offs,
                                         cbuf.d_cand, cbuf.d_ends, dT, A.input_mv, A.mv, A.has_write, A.wsym,
                                         static_cast<BlocksCborVerdict*>(cbuf.d_verdict)));
  const BlocksCborVerdict v =
      *static_cast<const BlocksCborVerdict*>(cbor_verdict_home(sizeof(BlocksCborVerdict), info.ms_h2d, info.ms_decode));
  info.block_candidates = v.block_candidates;
  info.step_candidates = v.step_candidates;
  const CborDecision d = blocks_cbor_decide(v, h);
  if (d.reason) {
    info.reason = d.reason;
    info.index = d.index;
    return false;
  }
  // ---- the tables come home: one copy, then into the store's vectors
  std::vector<uint64_t> home((tab_bytes + 7) / 8);
  HIP_OR_THROW(hipMemcpyAsync(home.data(), cbuf.d_tables, tab_bytes, hipMemcpyDeviceToHost, st));
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
  steps.input_mv = A.input_mv;
  steps.mv = A.mv;
  steps.has_write = A.has_write;
  steps.wsym = A.wsym;
  return true;
}

void sezkp_ctx::decode_blocks_cbor(const uint8_t* data, size_t len, BlockStore& out, sezkp_block_view& steps) {
  bcbor.drop_pending();
  bcbor.info = sezkp_blocks_ingest_info{};
  bcbor.info.bytes = len;
  bcbor.have_info = true;
  device_else_host(
      bcbor.info, [&] { return decode_blocks_cbor_device(data, len, out, steps); },
      [&](std::string& e) { return sezkp::decode_blocks_cbor(data, len, out, e); });
  if (bcbor.info.path == SEZKP_INGEST_DEVICE) return;
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
    BlocksCborIngest& b;
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
