// blocks_cbor_check.cpp — the device decoder of block-file CBOR
// (blocks_cbor.hip) run serially on the host through the functions it shares
// with the host (blocks_cbor_plan.h, trace_cbor_plan.h), as a stand-alone
// program (no GPU, no ROCm headers, no Python), for
// tests/test_blocks_cbor_host.py: the same mark, compact, heads, steps and
// chain passes over the same accessor, so the sanitizers see every read a lane
// would make, and the same decision on the verdict words.
//
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -o blocks_cbor_check tools/blocks_cbor_check.cpp
//   ./blocks_cbor_check < blocks.cbor
//       the verdict and, when the file is taken, the tables and the arrays:
//         device blocks=B tau=TAU t=T block_candidates=C step_candidates=C
//         version COUNT CRC32     (one line per array: its length and the CRC-32 of its
//                                  bytes; step_start without its last entry, which is t)
//       or  decline REASON [INDEX]   (head, block_candidates, step_candidates,
//                                     block_head K, step I, chain I, block_tail K)
//   ./blocks_cbor_check batch < records
//       the same for every record `u64 little-endian length | bytes`, each
//       held in a heap block of exactly its length.
//   ./blocks_cbor_check tiling
//       JSON: the signature lengths and the block and step length bounds.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <memory>
#include <vector>

#include "../streaming-zero-knowledge-proofs_amd/csrc/blocks_cbor_plan.h"

using namespace sezkp;

// CRC-32 (the zlib polynomial) of an array's bytes: the test compares it
// with zlib.crc32 of the host decoder's array
static uint32_t crc32_of(const void* data, size_t n) {
  static uint32_t table[256];
  if (!table[1])
    for (uint32_t i = 0; i < 256; i++) {
      uint32_t c = i;
      for (int k = 0; k < 8; k++) c = c & 1u ? 0xEDB88320u ^ (c >> 1) : c >> 1;
      table[i] = c;
    }
  uint32_t c = 0xFFFFFFFFu;
  const uint8_t* p = static_cast<const uint8_t*>(data);
  for (size_t i = 0; i < n; i++) c = table[(c ^ p[i]) & 0xFFu] ^ (c >> 8);
  return c ^ 0xFFFFFFFFu;
}
template <class Tp>
static void line(const char* name, const Tp* p, uint64_t n) {
  printf("%s %llu %u\n", name, (unsigned long long)n, crc32_of(p, (size_t)n * sizeof(Tp)));
}

static void run(const uint8_t* data, uint64_t len) {
  const CborSpan s{data, len};
  BlocksCborHead h;
  if (!blocks_cbor_head(s, h)) {
    printf("decline head\n");
    return;
  }
  const uint64_t B = h.n_blocks, t_max = h.t_max;
  const uint32_t tau = h.tau;
  BlocksCborVerdict V;
  memset(&V, 0xFF, sizeof V);
  // mark + compact: the tiles in order, 16 positions per lane as k_blocks_marks
  std::vector<uint64_t> cand_b, cand_s;
  V.block_candidates = V.step_candidates = 0;
  for (uint64_t pos = 0; pos < len; pos += TRACE_CBOR_LANE_BYTES) {
    const Cbor16 a = cbor_load16(s, pos), b = cbor_load16(s, pos + 16);
    const uint32_t mb = cbor_block_sig_mask(a, b), ms = cbor_sig_mask(a, b);
    for (uint32_t bit = 0; bit < 16; bit++) {
      if (pos + bit < h.first_off) continue;
      if (mb >> bit & 1u) {
        if (V.block_candidates < B) cand_b.push_back(pos + bit);
        V.block_candidates++;
      }
      if (ms >> bit & 1u) {
        if (V.step_candidates < t_max) cand_s.push_back(pos + bit);
        V.step_candidates++;
      }
    }
  }
  std::vector<uint8_t> mem(blocks_cbor_tables_bytes(B, tau) + 8);
  const BlocksCborTables T = blocks_cbor_tables_at(mem.data() + (8 - reinterpret_cast<uintptr_t>(mem.data()) % 8) % 8, B, tau);
  std::vector<int8_t> imv, mv;
  std::vector<uint8_t> hw;
  std::vector<uint16_t> ws;
  if (V.block_candidates >= B) {
    // heads
    for (uint64_t k = 0; k < B; k++) {
      BlockCborHead bh{};
      uint64_t end = cbor_parse_block_head(s, cand_b[k], tau, false, bh, T.win_left + k * tau, T.win_right + k * tau,
                                           T.off_in + k * tau, T.off_out + k * tau);
      if (k == 0 && cand_b[0] != h.first_off) end = 0;
      blocks_cbor_store_head(T, k, bh, end);
      if (!end && V.bad_head == ~0ull) V.bad_head = k;
    }
    // scan
    uint64_t t = 0;
    for (uint64_t k = 0; k < B; k++) {
      T.step_start[k] = t;
      t += T.n_steps[k];
    }
    V.t = t;
    if (V.bad_head == ~0ull && t <= t_max && V.step_candidates >= t) {
      imv.resize(t);
      mv.resize(t * tau);
      hw.resize(t * tau);
      ws.resize(t * tau);
      std::vector<uint64_t> ends(t);
      // steps
      for (uint64_t i = 0; i < t; i++) {
        ends[i] = cbor_parse_step(s, cand_s[i], tau, &imv[i], mv.data() + i * tau, hw.data() + i * tau, ws.data() + i * tau);
        if (!ends[i]) {
          if (V.bad_step == ~0ull) V.bad_step = i;
          continue;
        }
        if (i + 1 < t && cand_s[i + 1] != ends[i]) {
          const uint64_t k = blocks_cbor_block_of(T.step_start, B, i + 1);
          if (T.step_start[k] != i + 1 && i + 1 < V.bad_link) V.bad_link = i + 1;
        }
      }
      // chain
      for (uint64_t k = 0; k < B; k++) {
        const uint64_t a = T.step_start[k], n = T.n_steps[k];
        if (cand_s[a] != T.steps_off[k] && a < V.bad_link) V.bad_link = a;
        const uint64_t e = ends[a + n - 1];
        if (!e) continue;
        const uint64_t tail_end = cbor_parse_block_tail(s, e, tau);
        const uint64_t want = k + 1 < B ? cand_b[k + 1] : len;
        if ((!tail_end || tail_end != want) && V.bad_tail == ~0ull) V.bad_tail = k;
      }
    }
  }
  const BlocksCborDecision d = blocks_cbor_decide(V, h);
  static const char* const why[] = {"", "head", "block_candidates", "step_candidates", "block_head", "step", "chain",
                                    "block_tail"};
  if (d.reason) {
    if (d.reason >= 4) printf("decline %s %llu\n", why[d.reason], (unsigned long long)d.index);
    else printf("decline %s\n", why[d.reason]);
    return;
  }
  const uint64_t t = V.t, nt = B * tau;
  printf("device blocks=%llu tau=%u t=%llu block_candidates=%llu step_candidates=%llu\n", (unsigned long long)B, tau,
         (unsigned long long)t, (unsigned long long)V.block_candidates, (unsigned long long)V.step_candidates);
  line("version", T.version, B);
  line("block_id", T.block_id, B);
  line("step_lo", T.step_lo, B);
  line("step_hi", T.step_hi, B);
  line("ctrl_in", T.ctrl_in, B);
  line("ctrl_out", T.ctrl_out, B);
  line("in_head_in", T.in_head_in, B);
  line("in_head_out", T.in_head_out, B);
  line("win_left", T.win_left, nt);
  line("win_right", T.win_right, nt);
  line("off_in", T.off_in, nt);
  line("off_out", T.off_out, nt);
  line("step_start", T.step_start, B);
  line("input_mv", imv.data(), t);
  line("mv", mv.data(), t * tau);
  line("has_write", hw.data(), t * tau);
  line("wsym", ws.data(), t * tau);
}

// exactly n bytes from stdin into a heap block of exactly n bytes
static std::unique_ptr<uint8_t[]> read_exact(uint64_t n) {
  std::unique_ptr<uint8_t[]> p(new uint8_t[n ? n : 1]);
  if (n && fread(p.get(), 1, n, stdin) != n) {
    fprintf(stderr, "short read\n");
    exit(2);
  }
  return p;
}

int main(int argc, char** argv) {
  if (argc > 1 && !strcmp(argv[1], "tiling")) {
    printf("{\"tile\": %u, \"block_sig_len\": %u, \"step_sig_len\": %u, \"block_min\": [%llu, %llu, %llu], "
           "\"step_min\": [%u, %u, %u]}\n",
           TRACE_CBOR_TILE, BLOCKS_CBOR_SIG_LEN, TRACE_CBOR_SIG_LEN, (unsigned long long)cbor_block_min_len(0),
           (unsigned long long)cbor_block_min_len(8), (unsigned long long)cbor_block_min_len(24), cbor_step_min_len(0),
           cbor_step_min_len(8), cbor_step_min_len(24));
    return 0;
  }
  if (argc > 1 && !strcmp(argv[1], "batch")) {
    for (;;) {
      uint8_t lb[8];
      const size_t got = fread(lb, 1, 8, stdin);
      if (got == 0) return 0;
      if (got != 8) return 2;
      uint64_t n = 0;
      for (int i = 0; i < 8; i++) n |= (uint64_t)lb[i] << (8 * i);
      if (n > (1ull << 32)) return 2;
      const std::unique_ptr<uint8_t[]> p = read_exact(n);
      run(p.get(), n);
    }
  }
  std::vector<uint8_t> all;
  uint8_t buf[1 << 16];
  size_t got;
  while ((got = fread(buf, 1, sizeof buf, stdin)) > 0) all.insert(all.end(), buf, buf + got);
  std::unique_ptr<uint8_t[]> p(new uint8_t[all.size() ? all.size() : 1]);
  if (!all.empty()) memcpy(p.get(), all.data(), all.size());
  run(p.get(), all.size());
  return 0;
}
