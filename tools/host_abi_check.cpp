// host_abi_check.cpp — the host-only part of the C ABI (csrc/abi_host.cpp:
// the block, trace and manifest codecs, the manifest commitment, the
// simulator) as a stand-alone host program (no GPU, no ROCm headers, no
// Python), for tests/test_host_abi_sanitized.py: the round trips and error
// paths that tests/test_host_abi.py asserts through ctypes, here under the
// address and undefined-behaviour sanitizers.
//
//   g++ -std=c++17 -g -O1 -Wall -Werror -fsanitize=address,undefined -fno-sanitize-recover=all
//       -o host_abi_check tools/host_abi_check.cpp csrc/abi_host.cpp csrc/codec.cpp csrc/host_crypto.cpp
//       csrc/tracegen.cpp -pthread                                   (one command line)
//   ./host_abi_check GOLDEN_DIR
//
// GOLDEN_DIR: tests/golden (ref_blocks.cbor, riscv_blocks.cbor, their
// *_manifest.cbor, riscv_trace.cbor). Prints one line per check; the first
// failed check ends the program with status 1.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../include/sezkp_stark.h"

typedef std::vector<uint8_t> Bytes;

#define CHECK(cond, ...)                      \
  do {                                        \
    if (!(cond)) {                            \
      fprintf(stderr, "FAILED %s:%d: %s: ", __FILE__, __LINE__, #cond); \
      fprintf(stderr, __VA_ARGS__);           \
      fprintf(stderr, "\n");                  \
      exit(1);                                \
    }                                         \
  } while (0)

static Bytes read_file(const std::string& path) {
  FILE* f = fopen(path.c_str(), "rb");
  CHECK(f != nullptr, "cannot read %s", path.c_str());
  Bytes out;
  uint8_t buf[4096];
  for (size_t got; (got = fread(buf, 1, sizeof buf, f)) > 0;) out.insert(out.end(), buf, buf + got);
  fclose(f);
  return out;
}

static Bytes take(sezkp_buf* b) {
  Bytes out(b->data, b->data + b->len);
  sezkp_buf_free(b);
  CHECK(b->data == nullptr && b->len == 0, "sezkp_buf_free leaves the buffer set");
  return out;
}

static Bytes blocks_cbor(const sezkp_block_view* v) {
  sezkp_buf b{};
  CHECK(sezkp_blocks_encode_cbor(v, &b) == SEZKP_OK, "encode_cbor");
  return take(&b);
}

static sezkp_blocks* decode_cbor(const Bytes& raw) {
  sezkp_blocks* h = nullptr;
  char err[256] = "";
  const int32_t rc = sezkp_blocks_decode_cbor(raw.data(), raw.size(), &h, err, sizeof err);
  CHECK(rc == SEZKP_OK && h, "decode_cbor: %d %s", rc, err);
  return h;
}

// the codecs and the commitment over one fixture pair
static void check_blocks(const std::string& dir, const char* blocks_file, const char* manifest_file) {
  const Bytes raw = read_file(dir + "/" + blocks_file);
  char err[256] = "";
  sezkp_blocks* h = decode_cbor(raw);
  const sezkp_block_view* v = sezkp_blocks_view(h);
  CHECK(v && v->n_blocks > 0, "no blocks in %s", blocks_file);
  CHECK(blocks_cbor(v) == raw, "%s: CBOR -> CBOR changes the bytes", blocks_file);

  // CBOR -> JSONL -> blocks -> CBOR
  sezkp_buf jb{};
  CHECK(sezkp_blocks_encode_jsonl(v, &jb) == SEZKP_OK, "encode_jsonl");
  const Bytes jl = take(&jb);
  sezkp_blocks* hj = nullptr;
  int32_t rc = sezkp_blocks_decode_jsonl(jl.data(), jl.size(), &hj, err, sizeof err);
  CHECK(rc == SEZKP_OK && hj, "decode_jsonl: %d %s", rc, err);
  CHECK(blocks_cbor(sezkp_blocks_view(hj)) == raw, "%s: CBOR -> JSONL -> CBOR changes the bytes", blocks_file);
  sezkp_blocks_free(hj);

  // the sliced decoder over the whole file, steps included, and its line offsets
  sezkp_blocks* hl = nullptr;
  rc = sezkp_blocks_decode_jsonl_lines(jl.data(), jl.size(), 0, jl.size(), 1, &hl, err, sizeof err);
  CHECK(rc == SEZKP_OK && hl, "decode_jsonl_lines: %d %s", rc, err);
  CHECK(blocks_cbor(sezkp_blocks_view(hl)) == raw, "%s: the lines of [0, len) are other blocks", blocks_file);
  const uint64_t* off = nullptr;
  size_t noff = 0;
  CHECK(sezkp_blocks_line_offsets(hl, &off, &noff) == SEZKP_OK, "line_offsets");
  size_t lines = 0;
  for (uint8_t c : jl) lines += c == '\n';
  CHECK(noff == lines && noff == v->n_blocks, "%zu offsets, %zu lines, %u blocks", noff, lines, v->n_blocks);
  for (size_t i = 0; i < noff; i++)
    CHECK(off[i] < jl.size() && (i == 0 ? off[i] == 0 : jl[(size_t)off[i] - 1] == '\n'), "offset %zu not at a line start", i);
  sezkp_blocks_free(hl);

  // the manifest: the committed root, and both roots again over the leaf hashes
  const Bytes mraw = read_file(dir + "/" + manifest_file);
  uint8_t want[32], root[32], froot[32], again[32];
  uint32_t n_leaves = 0;
  rc = sezkp_manifest_decode(mraw.data(), mraw.size(), 0, want, &n_leaves, err, sizeof err);
  CHECK(rc == SEZKP_OK, "manifest_decode: %d %s", rc, err);
  CHECK(n_leaves == v->n_blocks, "manifest of %u leaves, %u blocks", n_leaves, v->n_blocks);
  CHECK(sezkp_manifest_root(v, root) == SEZKP_OK && memcmp(root, want, 32) == 0, "%s: root differs from %s",
        blocks_file, manifest_file);
  CHECK(sezkp_manifest_frontier_root(v, froot) == SEZKP_OK, "frontier_root");
  Bytes leaves((size_t)v->n_blocks * 32);
  CHECK(sezkp_manifest_leaf_hashes(v, leaves.data()) == SEZKP_OK, "leaf_hashes");
  CHECK(sezkp_merkle_root_of_leaves(leaves.data(), v->n_blocks, 0, again) == SEZKP_OK && memcmp(again, root, 32) == 0,
        "%s: batch root over the leaves", blocks_file);
  CHECK(sezkp_merkle_root_of_leaves(leaves.data(), v->n_blocks, 1, again) == SEZKP_OK && memcmp(again, froot, 32) == 0,
        "%s: frontier root over the leaves", blocks_file);
  printf("%s: %u blocks, tau %u, %zu JSONL bytes: codecs and manifest ok\n", blocks_file, v->n_blocks, v->tau,
         jl.size());
  sezkp_blocks_free(h);
}

// every proper prefix must be refused with a message; returns how many decoded
template <class Decode>
static size_t check_prefixes(const Bytes& raw, const char* what, Decode&& decode) {
  size_t valid = 0;
  for (size_t len = 0; len < raw.size(); len++) {
    // a copy of exactly len bytes: a read past the prefix is a report, not a read of the rest
    const Bytes cut(raw.begin(), raw.begin() + (ptrdiff_t)len);
    char err[256] = "";
    const int32_t rc = decode(cut.data(), cut.size(), err, sizeof err);
    if (rc == SEZKP_OK) {
      valid++;
      continue;
    }
    CHECK(rc == SEZKP_E_DECODE, "%s cut to %zu bytes: code %d", what, len, rc);
    CHECK(err[0] != 0, "%s cut to %zu bytes: no message", what, len);
  }
  printf("%s: %zu prefixes refused, %zu decode\n", what, raw.size() - valid, valid);
  return valid;
}

int main(int argc, char** argv) {
  if (argc != 2) {
    fprintf(stderr, "usage: %s GOLDEN_DIR\n", argv[0]);
    return 1;
  }
  const std::string dir = argv[1];
  CHECK(sezkp_abi_version() == SEZKP_ABI_VERSION && sezkp_version()[0], "versions");
  check_blocks(dir, "ref_blocks.cbor", "ref_manifest.cbor");
  check_blocks(dir, "riscv_blocks.cbor", "riscv_manifest.cbor");

  // TraceFile CBOR and back
  const Bytes traw = read_file(dir + "/riscv_trace.cbor");
  {
    sezkp_trace* t = nullptr;
    char err[256] = "";
    const int32_t rc = sezkp_trace_decode_cbor(traw.data(), traw.size(), &t, err, sizeof err);
    CHECK(rc == SEZKP_OK && t, "trace_decode_cbor: %d %s", rc, err);
    const sezkp_trace_view* tv = sezkp_trace_view_of(t);
    CHECK(tv && tv->t > 0, "empty trace");
    sezkp_buf b{};
    CHECK(sezkp_trace_encode_cbor(tv, &b) == SEZKP_OK, "trace_encode_cbor");
    CHECK(take(&b) == traw, "riscv_trace.cbor: CBOR -> CBOR changes the bytes");
    printf("riscv_trace.cbor: %llu steps, tau %u: codec ok\n", (unsigned long long)tv->t, tv->tau);
    sezkp_trace_free(t);
  }

  // truncations: no prefix of either file is a file of its kind
  size_t valid = check_prefixes(read_file(dir + "/ref_blocks.cbor"), "ref_blocks.cbor",
                                [](const uint8_t* d, size_t n, char* err, size_t el) {
                                  sezkp_blocks* h = nullptr;
                                  const int32_t rc = sezkp_blocks_decode_cbor(d, n, &h, err, el);
                                  sezkp_blocks_free(h);
                                  return rc;
                                });
  valid += check_prefixes(traw, "riscv_trace.cbor", [](const uint8_t* d, size_t n, char* err, size_t el) {
    sezkp_trace* t = nullptr;
    const int32_t rc = sezkp_trace_decode_cbor(d, n, &t, err, el);
    sezkp_trace_free(t);
    return rc;
  });
  CHECK(valid == 0, "%zu truncated files decode", valid);

  // the simulator's blocks through the codec and the commitment
  {
    sezkp_blocks* h = nullptr;
    char err[256] = "";
    const int32_t rc = sezkp_simulate_blocks(64, 8, 2, 42, &h, err, sizeof err);
    CHECK(rc == SEZKP_OK && h, "simulate_blocks: %d %s", rc, err);
    const sezkp_block_view* v = sezkp_blocks_view(h);
    CHECK(v->n_blocks == 8 && v->tau == 2 && v->step_start[8] == 64, "simulate: %u blocks", v->n_blocks);
    const Bytes enc = blocks_cbor(v);
    sezkp_blocks* back = decode_cbor(enc);
    CHECK(blocks_cbor(sezkp_blocks_view(back)) == enc, "simulate: CBOR -> CBOR changes the bytes");
    uint8_t r0[32], r1[32];
    CHECK(sezkp_manifest_root(v, r0) == SEZKP_OK && sezkp_manifest_root(sezkp_blocks_view(back), r1) == SEZKP_OK &&
              memcmp(r0, r1, 32) == 0,
          "simulate: the decoded blocks commit to another root");
    sezkp_blocks_free(back);
    sezkp_blocks_free(h);
    printf("simulate t=64 b=8 tau=2: %zu CBOR bytes: codec and manifest ok\n", enc.size());
  }
  return 0;
}
