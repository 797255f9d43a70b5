// abi_blocks.h — the block set behind the C ABI's sezkp_blocks handle: the
// decoders and the simulator fill it (abi_host.cpp), sezkp_ctx_trace_blocks
// fills it from a trace image on the device (abi_ctx.cpp). And the trace
// behind sezkp_trace: sezkp_trace_decode_cbor fills it (abi_host.cpp), and
// sezkp_ctx_decode_trace_cbor from the device's arrays (abi_ctx.cpp).
#pragma once
#include <stdint.h>

#include <vector>

#include "codec.h"

struct sezkp_blocks {
  sezkp::BlockStore s;
  std::vector<uint64_t> line_off;  // sezkp_blocks_decode_jsonl_meta: each line's byte offset
};

// TraceFile CBOR (sezkp-trace io.rs; format.rs:59-68)
struct sezkp_trace {
  sezkp::BlockStore s;  // the four step arrays and tau
  sezkp_trace_view view{};
  void bind() {  // (re)point view at the arrays; b = 0: the caller sets it on a copy
    view.t = s.input_mv.size();
    view.tau = s.tau;
    view.b = 0;
    view.input_mv = s.input_mv.data();
    view.mv = s.mv.data();
    view.has_write = s.has_write.data();
    view.wsym = s.wsym.data();
  }
};
