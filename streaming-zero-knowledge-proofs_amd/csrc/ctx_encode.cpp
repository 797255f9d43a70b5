// ctx_encode.cpp — a context's CBOR files written on the device
// (prover_ctx.h): the blocks file of the active trace image, the blocks file
// of any block view, a TraceFile. What the encoder reads is put into device
// memory where it is not there already (a view's block tables, host step
// arrays), cbor_encode.hip measures the file, the host sizes the file image
// by the length that comes home, the device writes it, and the bytes come
// home through the pinned staging block. The host encoders (codec.cpp) stay
// the yardstick; SEZKP_CBOR_ENCODE_HOST=1 runs them on arrays read back.
// Nothing here touches the trace image, the upload workspace, the ingest
// buffers' contents, the dictionary tables or a proof's state.
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <memory>
#include <string>
#include <vector>

#include "cbor_emit_plan.h"
#include "prover_ctx.h"

namespace sezkp::detail {
void EncodeBuffers::release() {
  for (void* p : {(void*)d_out, (void*)d_counts, (void*)d_offs, (void*)d_blen, (void*)d_pre, (void*)d_first,
                  (void*)d_tables, (void*)d_steps, (void*)d_words})
    if (p) (void)hipFree(p);
  if (h_words) (void)hipHostFree(h_words);
  for (auto& e : ev)
    if (e) (void)hipEventDestroy(e);
  *this = EncodeBuffers{};
}
}  // namespace sezkp::detail

namespace {
using clk = std::chrono::steady_clock;
double ms_since(clk::time_point t0) { return std::chrono::duration<double, std::milli>(clk::now() - t0).count(); }

// SEZKP_CBOR_ENCODE_HOST=1, read per call
bool forced_to_host() {
  const char* force = getenv("SEZKP_CBOR_ENCODE_HOST");
  return force && !strcmp(force, "1");
}

struct FreeBytes {
  void operator()(uint8_t* p) const { free(p); }
};

// The file of (sh, A, T), all in device memory, into malloc'd memory.
void encode_device(sezkp_ctx& c, const CborEmitShape& sh, const CborEmitSteps& A, const CborEmitTables& T,
                   sezkp_buf* out) {
  EncodeBuffers& e = c.enc;
  hipStream_t st = c.st;
  for (auto& v : e.ev)
    if (!v) HIP_OR_THROW(hipEventCreate(&v));
  if (!e.d_words) HIP_OR_THROW(hipMalloc(&e.d_words, 16));
  if (!e.h_words) HIP_OR_THROW(hipHostMalloc(&e.h_words, 16, hipHostMallocDefault));
  const uint64_t tiles = cbor_emit_tiles(sh.t, cbor_emit_tile_steps(sh.tau));
  if (tiles) {
    cbor_grow(e.d_counts, e.counts_cap, (size_t)tiles * 4);
    cbor_grow(e.d_offs, e.offs_cap, (size_t)tiles * 8);
  }
  cbor_grow(e.d_blen, e.blen_cap, (size_t)sh.B * 4);
  cbor_grow(e.d_pre, e.pre_cap, (size_t)sh.B * 8);
  cbor_grow(e.d_first, e.first_cap, (size_t)sh.B * 8);
  // ---- the lengths; the two totals come home
  HIP_OR_THROW(hipEventRecord(e.ev[0], st));
  HIP_OR_THROW(launch_cbor_emit_lengths(st, sh, A, T, e.d_counts, e.d_offs, e.d_blen, e.d_pre, e.d_words));
  HIP_OR_THROW(hipEventRecord(e.ev[1], st));
  HIP_OR_THROW(hipMemcpyAsync(e.h_words, e.d_words, 16, hipMemcpyDeviceToHost, st));
  HIP_OR_THROW(hipStreamSynchronize(st));
  const uint64_t steps_total = e.h_words[0], len = e.h_words[0] + e.h_words[1];
  if (steps_total > sh.t * cbor_step_max_len(sh.tau) || len > cbor_emit_len_bound(sh))
    throw Err{SEZKP_E_DEVICE, "encode: the device measured a file of " + std::to_string(len) +
                                  " bytes, more than its shape allows (" + std::to_string(cbor_emit_len_bound(sh)) + ")"};
  std::unique_ptr<uint8_t, FreeBytes> host(static_cast<uint8_t*>(malloc(len ? (size_t)len : 1)));
  if (!host) throw Err{SEZKP_E_NOMEM, "out of host memory"};
  cbor_grow(e.d_out, e.out_cap, (size_t)len);
  // ---- the file image
  HIP_OR_THROW(hipEventRecord(e.ev[2], st));
  HIP_OR_THROW(launch_cbor_emit(st, sh, A, T, e.d_offs, e.d_blen, e.d_pre, e.d_first, steps_total, e.d_out, len));
  HIP_OR_THROW(hipEventRecord(e.ev[3], st));
  // ---- home, through the two halves of the staging block: while one half is
  // copied out into the caller's memory the other is on the link
  c.cbor_stage_block();
  constexpr size_t H = CborBuffers::STAGE_HALF;
  CborBuffers& cb = c.cbuf;
  size_t prev_o = 0, prev_n = 0, k = 0;
  for (size_t o = 0; o < (size_t)len; k++) {
    const size_t n = std::min(H, (size_t)len - o), half = k & 1;
    HIP_OR_THROW(hipMemcpyAsync(cb.h_stage + half * H, e.d_out + o, n, hipMemcpyDeviceToHost, st));
    HIP_OR_THROW(hipEventRecord(cb.stage_ev[half], st));
    if (k) {
      HIP_OR_THROW(hipEventSynchronize(cb.stage_ev[1 - half]));
      memcpy(host.get() + prev_o, cb.h_stage + (1 - half) * H, prev_n);
    }
    prev_o = o;
    prev_n = n;
    o += n;
  }
  if (k) {
    const size_t half = (k - 1) & 1;
    HIP_OR_THROW(hipEventSynchronize(cb.stage_ev[half]));
    memcpy(host.get() + prev_o, cb.h_stage + half * H, prev_n);
  }
  HIP_OR_THROW(hipEventRecord(e.ev[4], st));
  HIP_OR_THROW(hipStreamSynchronize(st));
  float a = 0, b = 0, d = 0;
  HIP_OR_THROW(hipEventElapsedTime(&a, e.ev[0], e.ev[1]));
  HIP_OR_THROW(hipEventElapsedTime(&b, e.ev[2], e.ev[3]));
  HIP_OR_THROW(hipEventElapsedTime(&d, e.ev[3], e.ev[4]));
  e.info.path = SEZKP_INGEST_DEVICE;
  e.info.bytes = len;
  e.info.ms_kernels = (double)a + b;
  e.info.ms_d2h = d;
  out->data = host.release();
  out->len = (size_t)len;
}

// a step array where the device reads it: as given when it lies in device
// memory, else copied behind `*cursor` in enc.d_steps
template <class Tp>
const Tp* steps_on_device(sezkp_ctx& c, const Tp* src, size_t count, uint8_t*& cursor) {
  const size_t bytes = count * sizeof(Tp);
  if (!bytes) return reinterpret_cast<const Tp*>(cursor);
  if (on_device(src, c.device)) return src;
  Tp* dst = reinterpret_cast<Tp*>(cursor);
  copy_chunked(dst, src, bytes, COPY_CHUNK, hipMemcpyHostToDevice, c.st);
  cursor += (bytes + 15) & ~(size_t)15;
  return dst;
}
CborEmitSteps step_arrays_on_device(sezkp_ctx& c, const int8_t* input_mv, const int8_t* mv, const uint8_t* has_write,
                                    const uint16_t* wsym, uint64_t t, uint32_t tau) {
  const size_t cells = (size_t)t * tau;
  cbor_grow(c.enc.d_steps, c.enc.steps_cap, 4 * cells + (size_t)t + 64);
  uint8_t* cursor = c.enc.d_steps;
  CborEmitSteps A{};
  A.wsym = steps_on_device(c, wsym, cells, cursor);
  A.mv = steps_on_device(c, mv, cells, cursor);
  A.has_write = steps_on_device(c, has_write, cells, cursor);
  A.input_mv = steps_on_device(c, input_mv, (size_t)t, cursor);
  return A;
}
// ... and where the host reads it: as given, else read back into `keep`
template <class Tp>
const Tp* steps_on_host(sezkp_ctx& c, const Tp* src, size_t count, std::vector<Tp>& keep) {
  if (!count || !on_device(src, c.device)) return src;
  keep.resize(count);
  HIP_OR_THROW(hipMemcpyAsync(keep.data(), src, count * sizeof(Tp), hipMemcpyDeviceToHost, c.st));
  HIP_OR_THROW(hipStreamSynchronize(c.st));
  return keep.data();
}

void check_steps(const char* who, uint64_t t, uint32_t tau, const int8_t* input_mv, const int8_t* mv,
                 const uint8_t* has_write, const uint16_t* wsym) {
  if (tau > 255)  // TraceFile::tau is a u8; a block's window count has two bytes at the most
    throw Err{SEZKP_E_INVALID, std::string(who) + ": tau must be at most 255 (got " + std::to_string(tau) + ")"};
  if (t && (!input_mv || (tau && (!mv || !has_write || !wsym))))
    throw Err{SEZKP_E_INVALID, std::string(who) + ": null step array"};
}

void host_file(sezkp_ctx& c, const std::vector<uint8_t>& bytes, clk::time_point t0, sezkp_buf* out) {
  to_buf(bytes, out);
  c.enc.info.path = SEZKP_INGEST_HOST;
  c.enc.info.bytes = bytes.size();
  c.enc.info.ms_host = ms_since(t0);
}

void new_report(sezkp_ctx& c, uint64_t t, uint32_t tau, uint32_t n_blocks) {
  c.enc.info = sezkp_encode_info{};
  c.enc.info.t = t;
  c.enc.info.tau = tau;
  c.enc.info.n_blocks = n_blocks;
  c.enc.have_info = true;
}
}  // namespace

void sezkp_ctx::encode_trace_blocks_cbor(sezkp_buf* out) {
  if (sharded())
    throw Err{SEZKP_E_INVALID,
              "encode_trace_blocks_cbor: not on a sharded context (a rank holds only its own blocks' tables)"};
  TraceSlot& t = require_trace_image("encode_trace_blocks_cbor");
  const uint64_t n = sp.n;
  const uint32_t tau = sp.tau, nblk = sp.nblk;
  new_report(*this, n, tau, nblk);
  HIP_OR_THROW(hipSetDevice(device));
  if (forced_to_host()) {
    enc.info.reason = SEZKP_ENCODE_R_FORCED;
    const auto t0 = clk::now();
    BlockStore s;
    trace_blocks(nullptr, s);
    host_file(*this, sezkp::encode_blocks_cbor(s.view), t0, out);
    return;
  }
  // the image's own copy of the step arrays is the row-major one in `raw`
  // (wsym | mv | has_write); the block fields follow from (t, b) and the
  // device's metadata image
  const size_t cells = (size_t)tau * n;
  const CborEmitShape sh{0, tau, nblk, n, t.tm.b, nullptr};
  const CborEmitSteps A{t.imv, reinterpret_cast<const int8_t*>(t.raw + 2 * cells), t.raw + 3 * cells,
                        reinterpret_cast<const uint16_t*>(t.raw)};
  CborEmitTables T{};
  T.in_head_in = t.tm.in_head_in;
  T.in_head_out = t.tm.in_head_out;
  T.win_left = t.tm.win_left;
  T.win_right = t.tm.win_right;
  T.off_in = t.tm.off_in;
  T.off_out = t.tm.off_out;
  encode_device(*this, sh, A, T, out);
}

void sezkp_ctx::encode_blocks_cbor(const sezkp_block_view& v, sezkp_buf* out) {
  // ---- every check on the host, before any device call
  const uint32_t B = v.n_blocks, tau = v.tau;
  if (tau > 255)
    throw Err{SEZKP_E_INVALID, "block view: tau must be at most 255 (got " + std::to_string(tau) + ")"};
  if (B && (!v.version || !v.block_id || !v.step_lo || !v.step_hi || !v.ctrl_in || !v.ctrl_out || !v.in_head_in ||
            !v.in_head_out || !v.step_start || (tau && (!v.win_left || !v.win_right || !v.off_in || !v.off_out))))
    throw Err{SEZKP_E_INVALID, "block view: null block table"};
  if (B && v.step_start[0] != 0) throw Err{SEZKP_E_INVALID, "block view: step_start[0] must be 0"};
  for (uint32_t k = 0; k < B; k++)
    if (v.step_start[k + 1] < v.step_start[k])
      throw Err{SEZKP_E_INVALID, "block view: step_start decreases at block " + std::to_string(k)};
  const uint64_t t = B ? v.step_start[B] : 0;
  check_steps("block view", t, tau, v.input_mv, v.mv, v.has_write, v.wsym);
  new_report(*this, t, tau, B);
  const auto t0 = clk::now();
  if (B == 0) {
    enc.info.reason = SEZKP_ENCODE_R_EMPTY;
    host_file(*this, std::vector<uint8_t>{0x80}, t0, out);
    return;
  }
  HIP_OR_THROW(hipSetDevice(device));
  const size_t cells = (size_t)t * tau, nt = (size_t)B * tau;
  if (forced_to_host()) {
    enc.info.reason = SEZKP_ENCODE_R_FORCED;
    std::vector<int8_t> k_imv, k_mv;
    std::vector<uint8_t> k_hw;
    std::vector<uint16_t> k_ws;
    sezkp_block_view h = v;
    h.input_mv = steps_on_host(*this, v.input_mv, (size_t)t, k_imv);
    h.mv = steps_on_host(*this, v.mv, cells, k_mv);
    h.has_write = steps_on_host(*this, v.has_write, cells, k_hw);
    h.wsym = steps_on_host(*this, v.wsym, cells, k_ws);
    host_file(*this, sezkp::encode_blocks_cbor(h), t0, out);
    return;
  }
  // ---- the block tables in one block, the widest fields first, one copy:
  // step_lo | step_hi | in_head_in | in_head_out | step_start (B + 1) |
  // win_left | win_right | block_id | off_in | off_out | version | ctrl_in | ctrl_out
  const size_t words = 5 * (size_t)B + 1 + 2 * nt, bytes = words * 8 + ((size_t)B + 2 * nt) * 4 + 3 * (size_t)B * 2;
  std::vector<uint64_t> pack((bytes + 7) / 8);
  uint64_t* q = pack.data();
  uint32_t* d = reinterpret_cast<uint32_t*>(q + words);
  uint16_t* w = reinterpret_cast<uint16_t*>(d + B + 2 * nt);
  memcpy(q, v.step_lo, (size_t)B * 8);
  memcpy(q + B, v.step_hi, (size_t)B * 8);
  memcpy(q + 2 * (size_t)B, v.in_head_in, (size_t)B * 8);
  memcpy(q + 3 * (size_t)B, v.in_head_out, (size_t)B * 8);
  memcpy(q + 4 * (size_t)B, v.step_start, ((size_t)B + 1) * 8);
  if (nt) {
    memcpy(q + 5 * (size_t)B + 1, v.win_left, nt * 8);
    memcpy(q + 5 * (size_t)B + 1 + nt, v.win_right, nt * 8);
    memcpy(d + B, v.off_in, nt * 4);
    memcpy(d + B + nt, v.off_out, nt * 4);
  }
  memcpy(d, v.block_id, (size_t)B * 4);
  memcpy(w, v.version, (size_t)B * 2);
  memcpy(w + B, v.ctrl_in, (size_t)B * 2);
  memcpy(w + 2 * (size_t)B, v.ctrl_out, (size_t)B * 2);
  cbor_grow(enc.d_tables, enc.tables_cap, bytes);
  copy_chunked(enc.d_tables, pack.data(), bytes, COPY_CHUNK, hipMemcpyHostToDevice, st);
  const uint64_t* dq = reinterpret_cast<const uint64_t*>(enc.d_tables);
  const uint32_t* dd = reinterpret_cast<const uint32_t*>(dq + words);
  const uint16_t* dw = reinterpret_cast<const uint16_t*>(dd + B + 2 * nt);
  CborEmitTables T{};
  T.step_lo = dq;
  T.step_hi = dq + B;
  T.in_head_in = reinterpret_cast<const int64_t*>(dq + 2 * (size_t)B);
  T.in_head_out = reinterpret_cast<const int64_t*>(dq + 3 * (size_t)B);
  T.win_left = reinterpret_cast<const int64_t*>(dq + 5 * (size_t)B + 1);
  T.win_right = T.win_left + nt;
  T.block_id = dd;
  T.off_in = dd + B;
  T.off_out = dd + B + nt;
  T.version = dw;
  T.ctrl_in = dw + B;
  T.ctrl_out = dw + 2 * (size_t)B;
  const CborEmitShape sh{0, tau, B, t, 0, dq + 4 * (size_t)B};
  const CborEmitSteps A = step_arrays_on_device(*this, v.input_mv, v.mv, v.has_write, v.wsym, t, tau);
  encode_device(*this, sh, A, T, out);  // synchronises st: `pack` and the caller's arrays are read by then
}

void sezkp_ctx::encode_trace_cbor(const sezkp_trace_view* tv, sezkp_buf* out) {
  sezkp_trace_view v{};
  if (tv) {
    check_steps("trace view", tv->t, tv->tau, tv->input_mv, tv->mv, tv->has_write, tv->wsym);
    v = *tv;
  } else {
    if (sharded())
      throw Err{SEZKP_E_INVALID, "encode_trace_cbor: not on a sharded context (a rank holds only its own rows)"};
    TraceSlot& t = require_trace_image("encode_trace_cbor");
    const size_t cells = (size_t)sp.tau * sp.n;
    v.t = sp.n;
    v.tau = sp.tau;
    v.input_mv = t.imv;
    v.mv = reinterpret_cast<const int8_t*>(t.raw + 2 * cells);
    v.has_write = t.raw + 3 * cells;
    v.wsym = reinterpret_cast<const uint16_t*>(t.raw);
  }
  new_report(*this, v.t, v.tau, 0);
  HIP_OR_THROW(hipSetDevice(device));
  const size_t cells = (size_t)v.t * v.tau;
  if (forced_to_host()) {
    enc.info.reason = SEZKP_ENCODE_R_FORCED;
    const auto t0 = clk::now();
    std::vector<int8_t> k_imv, k_mv;
    std::vector<uint8_t> k_hw;
    std::vector<uint16_t> k_ws;
    sezkp_trace_view h = v;
    h.input_mv = steps_on_host(*this, v.input_mv, (size_t)v.t, k_imv);
    h.mv = steps_on_host(*this, v.mv, cells, k_mv);
    h.has_write = steps_on_host(*this, v.has_write, cells, k_hw);
    h.wsym = steps_on_host(*this, v.wsym, cells, k_ws);
    host_file(*this, sezkp::encode_trace_cbor(h), t0, out);
    return;
  }
  // one pseudo-block of all t steps
  const CborEmitShape sh{1, v.tau, 1, v.t, v.t ? v.t : 1, nullptr};
  const CborEmitSteps A = step_arrays_on_device(*this, v.input_mv, v.mv, v.has_write, v.wsym, v.t, v.tau);
  encode_device(*this, sh, A, CborEmitTables{}, out);
}
