// abi_blocks.h — the block set behind the C ABI's sezkp_blocks handle: the
// decoders and the simulator fill it (abi_host.cpp), sezkp_ctx_trace_blocks
// fills it from a trace image on the device (abi_ctx.cpp).
#pragma once
#include <stdint.h>

#include <vector>

#include "codec.h"

struct sezkp_blocks {
  sezkp::BlockStore s;
  std::vector<uint64_t> line_off;  // sezkp_blocks_decode_jsonl_meta: each line's byte offset
};
