// cbor_check.cpp — the device decoders of TraceFile and block-file CBOR
// (cbor_decode.hip) run index by index on the host, as a stand-alone program
// (no GPU, no ROCm headers, no Python), for tests/test_trace_cbor_host.py and
// tests/test_blocks_cbor_host.py. Nothing of a pass is written here: each loop
// below calls, per index, the function that is the body of the kernel
// (trace_cbor_plan.h, blocks_cbor_plan.h), with a plain minimum where the
// device takes an atomic one, and the decision on the verdict words is the
// product's. Every buffer a lane indexes is a heap block of its own, of exactly
// the size the product gives it, and the file one of exactly its length, so
// the sanitizers see every read and write a lane would make. A TraceFile's
// tail is parsed by codec.cpp, as in the product.
//
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -o cbor_check tools/cbor_check.cpp
//       streaming-zero-knowledge-proofs_amd/csrc/codec.cpp streaming-zero-knowledge-proofs_amd/csrc/host_crypto.cpp
//       -pthread            (one command line)
//   ./cbor_check trace < trace.cbor
//       the verdict and, when the file is taken, the arrays:
//         device t=T tau=TAU candidates=C
//         input_mv v v ...        (one line per array, row-major)
//         mv ...
//         has_write ...
//         wsym ...
//       or  decline REASON [INDEX]   (head, candidates, step I, chain I, tail)
//   ./cbor_check blocks < blocks.cbor
//       the verdict and, when the file is taken, the tables and the arrays:
//         device blocks=B tau=TAU t=T block_candidates=C step_candidates=C
//         version COUNT CRC32     (one line per array: its length and the CRC-32 of its
//                                  bytes; step_start without its last entry, which is t)
//       or  decline REASON [INDEX]   (head, block_candidates, step_candidates,
//                                     block_head K, step I, chain I, block_tail K)
//   ./cbor_check trace|blocks batch < records
//       the same for every record `u64 little-endian length | bytes`.
//   ./cbor_check trace|blocks tiling
//       JSON: the tile, lane, scan-pass and signature sizes and the length bounds.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <memory>
#include <vector>

#include "../streaming-zero-knowledge-proofs_amd/csrc/blocks_cbor_plan.h"
#include "../streaming-zero-knowledge-proofs_amd/csrc/codec.h"

using namespace sezkp;

// n elements in a heap block of exactly that size
template <class Tp>
static std::unique_ptr<Tp[]> block_of(uint64_t n) {
  return std::unique_ptr<Tp[]>(new Tp[n]());
}
// the step arrays of `rows` steps, as CborBuffers::step_arrays sizes them
struct StepArrays {
  std::unique_ptr<int8_t[]> input_mv, mv;
  std::unique_ptr<uint8_t[]> has_write;
  std::unique_ptr<uint16_t[]> wsym;
  StepArrays(uint64_t rows, uint32_t tau)
      : input_mv(block_of<int8_t>(rows)), mv(block_of<int8_t>(rows * tau)), has_write(block_of<uint8_t>(rows * tau)),
        wsym(block_of<uint16_t>(rows * tau)) {}
};
// mark and compact, lane by lane in file order: the first cap[q] candidates
// of each kind into cand[q], the number of all of them into total[q]
template <int KINDS>
static void mark_and_compact(const CborSpan& s, uint64_t lo, uint64_t* const* cand, const uint64_t* cap, uint64_t* total) {
  for (int q = 0; q < KINDS; q++) total[q] = 0;
  for (uint64_t pos = 0; pos < trace_cbor_tiles(s.len) * TRACE_CBOR_TILE; pos += TRACE_CBOR_LANE_BYTES) {
    uint32_t m[KINDS];
    cbor_lane_marks<KINDS>(s, lo, pos, m);
    for (int q = 0; q < KINDS; q++) total[q] = cbor_store_marks(m[q], pos, total[q], cand[q], cap[q]);
  }
}

static void run_trace(const uint8_t* data, uint64_t len) {
  const CborSpan s{data, len};
  TraceCborHead h;
  if (!trace_cbor_head(s, h)) {
    printf("decline head\n");
    return;
  }
  const uint64_t t = h.t;
  const uint32_t tau = h.tau;
  const std::unique_ptr<uint64_t[]> cand = block_of<uint64_t>(t);
  const StepArrays A(t, tau);
  TraceCborVerdict V{0, ~0ull, ~0ull, h.steps_off};
  uint64_t* const cands = cand.get();
  mark_and_compact<1>(s, h.steps_off, &cands, &t, &V.candidates);
  for (uint64_t i = 0; i < t; i++)
    trace_cbor_step_pass(s, h.steps_off, cands, t, tau, A.input_mv.get(), A.mv.get(), A.has_write.get(), A.wsym.get(), &V,
                         i, CborSerialMin{});
  CborDecision d = trace_cbor_decide(V, h);
  if (!d.reason && (V.tail_off > len || !trace_cbor_tail_ok(data, len, V.tail_off))) d.reason = 5;
  static const char* const why[] = {"", "head", "candidates", "step", "chain", "tail"};
  if (d.reason) {
    if (d.reason == 3 || d.reason == 4) printf("decline %s %llu\n", why[d.reason], (unsigned long long)d.index);
    else printf("decline %s\n", why[d.reason]);
    return;
  }
  printf("device t=%llu tau=%u candidates=%llu\n", (unsigned long long)t, tau, (unsigned long long)V.candidates);
  printf("input_mv");
  for (uint64_t i = 0; i < t; i++) printf(" %d", A.input_mv[i]);
  printf("\nmv");
  for (uint64_t i = 0; i < t * tau; i++) printf(" %d", A.mv[i]);
  printf("\nhas_write");
  for (uint64_t i = 0; i < t * tau; i++) printf(" %u", A.has_write[i]);
  printf("\nwsym");
  for (uint64_t i = 0; i < t * tau; i++) printf(" %u", A.wsym[i]);
  printf("\n");
}

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

static void run_blocks(const uint8_t* data, uint64_t len) {
  const CborSpan s{data, len};
  BlocksCborHead h;
  if (!blocks_cbor_head(s, h)) {
    printf("decline head\n");
    return;
  }
  const uint64_t B = h.n_blocks, t_max = h.t_max;
  const uint32_t tau = h.tau;
  const std::unique_ptr<uint64_t[]> cand_s = block_of<uint64_t>(t_max), cand_b = block_of<uint64_t>(B),
                                    ends = block_of<uint64_t>(t_max);
  const std::unique_ptr<uint8_t[]> tables = block_of<uint8_t>(blocks_cbor_tables_bytes(B, tau));  // new[]: 16-byte aligned
  const StepArrays A(t_max, tau);
  const BlocksCborTables T = blocks_cbor_tables_at(tables.get(), B, tau);
  BlocksCborVerdict V;
  memset(&V, 0xFF, sizeof V);
  uint64_t* const cand[2] = {cand_s.get(), cand_b.get()};
  const uint64_t cap[2] = {t_max, B};
  uint64_t total[2];
  mark_and_compact<2>(s, h.first_off, cand, cap, total);
  V.step_candidates = total[0];
  V.block_candidates = total[1];
  for (uint64_t k = 0; k < B; k++) blocks_cbor_head_pass(s, h.first_off, cand[1], B, tau, T, &V, k, CborSerialMin{});
  V.t = 0;  // the scan
  for (uint64_t k = 0; k < B; k++) {
    T.step_start[k] = V.t;
    V.t += T.n_steps[k];
  }
  for (uint64_t i = 0; i < t_max; i++)
    blocks_cbor_step_pass(s, cand[0], t_max, B, T.step_start, tau, A.input_mv.get(), A.mv.get(), A.has_write.get(),
                          A.wsym.get(), ends.get(), &V, i, CborSerialMin{});
  for (uint64_t k = 0; k < B; k++)
    blocks_cbor_chain_pass(s, cand[1], cand[0], t_max, B, tau, T, ends.get(), &V, k, CborSerialMin{});
  const CborDecision d = blocks_cbor_decide(V, h);
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
  line("input_mv", A.input_mv.get(), t);
  line("mv", A.mv.get(), t * tau);
  line("has_write", A.has_write.get(), t * tau);
  line("wsym", A.wsym.get(), t * tau);
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
  const bool blocks = argc > 1 && !strcmp(argv[1], "blocks");
  if (!blocks && !(argc > 1 && !strcmp(argv[1], "trace"))) {
    fprintf(stderr, "usage: cbor_check trace|blocks [batch|tiling]\n");
    return 2;
  }
  void (*const run)(const uint8_t*, uint64_t) = blocks ? run_blocks : run_trace;
  if (argc > 2 && !strcmp(argv[2], "tiling")) {
    printf("{\"tile\": %u, \"lane_bytes\": %u, \"threads\": %u, \"scan_pass\": %u, \"sig_len\": %u, \"block_sig_len\": %u, "
           "\"step_sig_len\": %u, \"step_min\": [%u, %u, %u], \"step_max\": [%u, %u, %u], \"block_min\": [%llu, %llu, %llu]}\n",
           TRACE_CBOR_TILE, TRACE_CBOR_LANE_BYTES, TRACE_CBOR_THREADS, TRACE_CBOR_SCAN_PASS, TRACE_CBOR_SIG_LEN,
           BLOCKS_CBOR_SIG_LEN, TRACE_CBOR_SIG_LEN, cbor_step_min_len(0), cbor_step_min_len(8), cbor_step_min_len(24),
           cbor_step_max_len(0), cbor_step_max_len(8), cbor_step_max_len(24), (unsigned long long)cbor_block_min_len(0),
           (unsigned long long)cbor_block_min_len(8), (unsigned long long)cbor_block_min_len(24));
    return 0;
  }
  if (argc > 2 && !strcmp(argv[2], "batch")) {
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
