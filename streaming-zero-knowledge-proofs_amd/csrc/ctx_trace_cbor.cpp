// ctx_trace_cbor.cpp — a context's TraceFile ingest (prover_ctx.h): the file's
// CBOR bytes go to the device, trace_cbor.hip decodes them into the four step
// arrays there, and the host decides on the verdict words that come home
// (trace_cbor_plan.h: head, candidate count, steps, chain, tail). A file the
// device path declines, for whatever reason, is decoded by the host pull
// parser (codec.cpp), which alone words the errors.
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <string>

#include "prover_ctx.h"

namespace sezkp::detail {
void TraceCborBuffers::release() {
  for (void* p : {(void*)d_bytes, (void*)d_counts, (void*)d_offs, (void*)d_cand, (void*)d_arrays, (void*)d_verdict})
    if (p) (void)hipFree(p);
  if (h_verdict) (void)hipHostFree(h_verdict);
  if (h_stage) (void)hipHostFree(h_stage);
  for (auto& e : stage_ev)
    if (e) (void)hipEventDestroy(e);
  for (auto& e : ev)
    if (e) (void)hipEventDestroy(e);
  *this = TraceCborBuffers{};
}
void cbor_grow(void** p, size_t& cap, size_t bytes) {
  if (*p && bytes <= cap) return;
  if (*p) (void)hipFree(*p);
  *p = nullptr;
  cap = 0;
  const size_t want = bytes + bytes / 4 + 64;
  HIP_OR_THROW(hipMalloc(p, want));
  cap = want;
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
}  // namespace

void sezkp_ctx::cbor_bytes_to_device(const uint8_t* data, size_t len) {
  for (auto& e : cbor.ev)
    if (!e) HIP_OR_THROW(hipEventCreate(&e));
  cbor_grow(cbor.d_bytes, cbor.bytes_cap, len);
  // ---- the bytes: straight from pinned memory, else through the staging block
  HIP_OR_THROW(hipEventRecord(cbor.ev[0], st));
  if (host_pinned(data)) {
    copy_chunked(cbor.d_bytes, data, len, COPY_CHUNK, hipMemcpyHostToDevice, st);
  } else {
    constexpr size_t H = TraceCborBuffers::STAGE_HALF;
    if (!cbor.h_stage) {
      void* q = nullptr;
      HIP_OR_THROW(hipHostMalloc(&q, 2 * H, hipHostMallocDefault));
      cbor.h_stage = static_cast<uint8_t*>(q);
      for (auto& e : cbor.stage_ev) HIP_OR_THROW(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    }
    size_t k = 0;
    for (size_t o = 0; o < len; k++) {
      const size_t n = std::min(H, len - o), half = k & 1;
      if (k >= 2) HIP_OR_THROW(hipEventSynchronize(cbor.stage_ev[half]));  // the half's previous copy
      memcpy(cbor.h_stage + half * H, data + o, n);
      HIP_OR_THROW(hipMemcpyAsync(cbor.d_bytes + o, cbor.h_stage + half * H, n, hipMemcpyHostToDevice, st));
      HIP_OR_THROW(hipEventRecord(cbor.stage_ev[half], st));
      o += n;
    }
  }
  HIP_OR_THROW(hipEventRecord(cbor.ev[1], st));
}

// true: the arrays are in cbor.d_arrays (st synchronised), tv points at them.
// false: declined, cbor.info.reason says why. Throws only for device errors.
bool sezkp_ctx::decode_trace_cbor_device(const uint8_t* data, size_t len, sezkp_trace_view& tv) {
  sezkp_trace_ingest_info& info = cbor.info;
  const char* force = getenv("SEZKP_TRACE_CBOR_HOST");  // read per call
  if (force && !strcmp(force, "1")) {
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
  const uint64_t t = h.t, cells = t * h.tau;  // t <= len / 18
  uint64_t tail_off = h.steps_off;
  HIP_OR_THROW(hipSetDevice(device));
  // buffers of an earlier call may still be read by the upload it fed; a
  // pending block-file ingest holds its steps in the same arrays
  HIP_OR_THROW(hipStreamSynchronize(st));
  bcbor.drop_pending();
  cbor_grow(cbor.d_arrays, cbor.arrays_cap, (size_t)(4 * cells + t));
  uint16_t* d_ws = reinterpret_cast<uint16_t*>(cbor.d_arrays);
  int8_t* d_mv = reinterpret_cast<int8_t*>(cbor.d_arrays + 2 * cells);
  uint8_t* d_hw = cbor.d_arrays + 3 * cells;
  int8_t* d_imv = reinterpret_cast<int8_t*>(cbor.d_arrays + 4 * cells);
  if (t) {
    const size_t ntiles = (size_t)trace_cbor_tiles(len);
    if (ntiles > cbor.tiles_cap || !cbor.d_counts) {
      size_t c0 = 0, c1 = 0;
      if (cbor.d_counts) (void)hipFree(cbor.d_counts);
      if (cbor.d_offs) (void)hipFree(cbor.d_offs);
      cbor.d_counts = nullptr;
      cbor.d_offs = nullptr;
      cbor.tiles_cap = 0;
      cbor_grow(cbor.d_counts, c0, ntiles * 4);
      cbor_grow(cbor.d_offs, c1, ntiles * 8);
      cbor.tiles_cap = ntiles;
    }
    cbor_grow(cbor.d_cand, cbor.cand_cap, (size_t)t * 8);
    if (!cbor.d_verdict) {
      void* q = nullptr;
      HIP_OR_THROW(hipMalloc(&q, sizeof(TraceCborVerdict)));
      cbor.d_verdict = static_cast<TraceCborVerdict*>(q);
      HIP_OR_THROW(hipHostMalloc(&q, sizeof(TraceCborVerdict), hipHostMallocDefault));
      cbor.h_verdict = static_cast<TraceCborVerdict*>(q);
    }
    cbor_bytes_to_device(data, len);
    HIP_OR_THROW(launch_trace_cbor_decode(st, cbor.d_bytes, len, h.steps_off, t, h.tau, cbor.d_counts, cbor.d_offs,
                                          cbor.d_cand, d_imv, d_mv, d_hw, d_ws, cbor.d_verdict));
    HIP_OR_THROW(hipEventRecord(cbor.ev[2], st));
    HIP_OR_THROW(hipMemcpyAsync(cbor.h_verdict, cbor.d_verdict, sizeof(TraceCborVerdict), hipMemcpyDeviceToHost, st));
    HIP_OR_THROW(hipStreamSynchronize(st));
    float ms = 0;
    HIP_OR_THROW(hipEventElapsedTime(&ms, cbor.ev[0], cbor.ev[1]));
    info.ms_h2d = ms;
    HIP_OR_THROW(hipEventElapsedTime(&ms, cbor.ev[1], cbor.ev[2]));
    info.ms_decode = ms;
    const TraceCborVerdict& v = *cbor.h_verdict;
    info.candidates = v.candidates;
    if (v.candidates < t) {
      info.reason = SEZKP_INGEST_R_CANDIDATES;
      return false;
    }
    if (v.bad_step != ~0ull && v.bad_step <= v.bad_link) {
      info.reason = SEZKP_INGEST_R_STEP;
      info.index = v.bad_step;
      return false;
    }
    if (v.bad_link != ~0ull) {
      info.reason = SEZKP_INGEST_R_CHAIN;
      info.index = v.bad_link;
      return false;
    }
    tail_off = v.tail_off;
  }
  if (tail_off > len || !trace_cbor_tail_ok(data, len, (size_t)tail_off)) {
    info.reason = SEZKP_INGEST_R_TAIL;
    return false;
  }
  tv = sezkp_trace_view{};
  tv.t = t;
  tv.tau = h.tau;
  tv.input_mv = d_imv;
  tv.mv = d_mv;
  tv.has_write = d_hw;
  tv.wsym = d_ws;
  return true;
}

void sezkp_ctx::decode_trace_cbor(const uint8_t* data, size_t len, BlockStore& host, sezkp_trace_view& tv) {
  cbor.info = sezkp_trace_ingest_info{};
  cbor.info.bytes = len;
  cbor.have_info = true;
  if (decode_trace_cbor_device(data, len, tv)) {
    cbor.info.path = SEZKP_INGEST_DEVICE;
    return;
  }
  cbor.info.path = SEZKP_INGEST_HOST;
  using clk = std::chrono::steady_clock;
  const auto t0 = clk::now();
  std::string e;
  const bool ok = sezkp::decode_trace_cbor(data, len, host, e);
  cbor.info.ms_host = std::chrono::duration<double, std::milli>(clk::now() - t0).count();
  if (!ok) throw Err{SEZKP_E_DECODE, e};
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
