// cli.cpp — `sezkp-cli` drop-in for the STARK path on MI355X:
//   prove  --backend stark --blocks B --manifest M --out P [--stream] [--assume-committed] [--host-decode]
//          [--ingest-stats]
//          (a .cbor block file is decoded on the device, sezkp_ctx_ingest_blocks_cbor: the steps never visit the
//          host, the precheck runs on the block fields that come home; --host-decode: decoded on the host, as
//          before the device decoder; same messages, exit codes and output either way; --ingest-stats: one
//          line on stderr with what sezkp_ctx_blocks_ingest_stats reports of the device route)
//   prove  --backend stark --trace T.cbor --b STEPS_PER_BLOCK --out P [--out-blocks F] [--out-manifest F]
//          [--manifest M] [--stream] [--host-decode]
//          (from the movement log: decode, partition and manifest on the device; --manifest is compared with
//          its root; --host-decode: the trace file is decoded on the host first, as before the device decoder)
//   verify --backend stark --blocks B --manifest M --proof P [--assume-committed] [--gpu]
//          (--gpu: the Merkle paths are hashed on device 0, sezkp_stark_v1_verify_batch; same output)
//   commit --blocks B(.cbor|.json|.jsonl|.ndjson) --out M
//   verify-commit --blocks B --manifest M
//   export-jsonl --input B(.cbor|.json|.jsonl|.ndjson) --output B.jsonl
//   audit --blocks B(.cbor|.json|.jsonl|.ndjson) [--json] [--host-decode]
//          (full-trace AIR audit; exit 3 when a row violates; a .cbor file is decoded on the device as for prove)
// Semantics follow crates/sezkp-cli/src/main.rs:429-578 (manifest precheck,
// .json/.cbor block files only for prove/verify, write_proof_auto by extension)
// and crates/sezkp-merkle/src/lib.rs:259-337 (commit / precheck).
#include <stdio.h>
#include <string.h>

#include <sys/stat.h>

#include <algorithm>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "../../include/sezkp_stark.h"
#include "codec.h"
#include "host_crypto.h"

using namespace sezkp;

namespace {

std::string ext_lower(const std::string& p) {
  size_t d = p.find_last_of('.');
  size_t s = p.find_last_of('/');
  if (d == std::string::npos || (s != std::string::npos && d < s)) return "";
  std::string e = p.substr(d + 1);
  for (auto& c : e) c = (char)tolower((unsigned char)c);
  return e;
}
std::string hex(const uint8_t* p, size_t n) {
  static const char* H = "0123456789abcdef";
  std::string s;
  for (size_t i = 0; i < n; i++) { s += H[p[i] >> 4]; s += H[p[i] & 15]; }
  return s;
}
bool read_file(const std::string& path, std::vector<uint8_t>& out, std::string& err) {
  std::ifstream f(path, std::ios::binary);
  if (!f) { err = "open " + path; return false; }
  out.assign(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
  return true;
}
bool write_file(const std::string& path, const std::vector<uint8_t>& data, std::string& err) {
  std::ofstream f(path, std::ios::binary);
  if (!f) { err = "create " + path; return false; }
  f.write((const char*)data.data(), (std::streamsize)data.size());
  return (bool)f;
}

bool is_jsonl_like(const std::string& path) {  // sezkp-merkle lib.rs:410-412
  const std::string e = ext_lower(path);
  return e == "jsonl" || e == "ndjson";
}
bool load_blocks(const std::string& path, BlockStore& bs, std::string& err) {  // io.rs:78-88
  const std::string e = ext_lower(path);
  std::vector<uint8_t> raw;
  if (e != "json" && e != "cbor") {
    err = e.empty() ? "path has no extension (expected .json or .cbor)"
                    : "unsupported blocks extension: " + e + " (supported: .json, .cbor)";
    return false;
  }
  if (!read_file(path, raw, err)) return false;
  if (e == "cbor") return decode_blocks_cbor(raw.data(), raw.size(), bs, err);
  return decode_blocks_json((const char*)raw.data(), raw.size(), bs, err);
}
bool load_manifest(const std::string& path, uint8_t root[32], uint32_t* n_leaves, std::string& err) {
  const std::string e = ext_lower(path);
  std::vector<uint8_t> raw;
  if (e != "json" && e != "cbor") {
    err = e.empty() ? "path has no extension (expected .json or .cbor)" : "unsupported manifest extension: " + e;
    return false;
  }
  if (!read_file(path, raw, err)) return false;
  if (e == "cbor") return decode_manifest_cbor(raw.data(), raw.size(), root, n_leaves, err);
  return decode_manifest_json((const char*)raw.data(), raw.size(), root, n_leaves, err);
}

// serde_json::to_writer_pretty layout of a ProofArtifact
std::string pretty_artifact(const Artifact& a) {
  std::ostringstream o;
  auto arr = [&](const std::vector<uint8_t>& v) {
    if (v.empty()) { o << "[]"; return; }
    o << "[\n";
    for (size_t i = 0; i < v.size(); i++) o << "    " << (unsigned)v[i] << (i + 1 < v.size() ? ",\n" : "\n");
    o << "  ]";
  };
  o << "{\n  \"backend\": \"" << a.backend << "\",\n  \"manifest_root\": ";
  arr(a.manifest_root);
  o << ",\n  \"proof_bytes\": ";
  arr(a.proof_bytes);
  o << ",\n  \"meta\": " << a.meta_json << "\n}";
  return o.str();
}

struct Args {
  std::string cmd, backend = "stark", blocks, manifest, out, proof, input, trace, out_blocks, out_manifest;
  bool stream = false, assume = false, json = false, gpu = false, b_given = false, host_decode = false, ingest_stats = false;
  std::string t = "32", b = "4", tau = "2";  // simulate defaults (main.rs:87-100)
};

// The blocks file of `commit` and of the precheck: .jsonl/.ndjson through the
// line reader (io_jsonl.rs:43-84), .json/.cbor through read_block_summaries_auto
bool load_blocks_any(const std::string& path, BlockStore& bs, std::string& err) {
  if (!is_jsonl_like(path)) return load_blocks(path, bs, err);
  std::vector<uint8_t> raw;
  if (!read_file(path, raw, err)) return false;
  return decode_blocks_jsonl((const char*)raw.data(), raw.size(), bs, err);
}
// commit_block_file (lib.rs:259-295): the Frontier root for JSON Lines, the
// batch merkle_root otherwise
void file_root(const std::string& path, const BlockStore& bs, uint8_t root[32]) {
  if (is_jsonl_like(path)) manifest_frontier_root(bs.view, root);
  else manifest_root(bs.view, root);
}

// verify_block_file_against_manifest (lib.rs:302-337), run on the blocks path
// before anything else reads it (main.rs:454-457). `bs` keeps the decoded
// blocks so a .json/.cbor file is read once.
int precheck(const Args& a, BlockStore& bs) {
  uint8_t mroot[32], got[32];
  uint32_t nl = 0;
  std::string err;
  if (!load_manifest(a.manifest, mroot, &nl, err)) {
    fprintf(stderr, "Error: blocks/manifest mismatch: %s\n", err.c_str());
    return 1;
  }
  if (!load_blocks_any(a.blocks, bs, err)) {
    fprintf(stderr, "Error: blocks/manifest mismatch: read blocks %s: %s\n", a.blocks.c_str(), err.c_str());
    return 1;
  }
  file_root(a.blocks, bs, got);
  if (memcmp(got, mroot, 32) != 0) {
    fprintf(stderr, "Error: blocks/manifest mismatch: root mismatch: manifest=%s, recomputed=%s\n",
            hex(mroot, 32).c_str(), hex(got, 32).c_str());
    return 1;
  }
  if (nl != bs.view.n_blocks) {
    fprintf(stderr, "Error: blocks/manifest mismatch: leaf count mismatch: manifest=%u, recomputed=%u\n", nl,
            bs.view.n_blocks);
    return 1;
  }
  return 0;
}

// precheck unless --assume-committed, then the manifest, then the blocks
// through read_block_summaries_auto (.json/.cbor only: a .jsonl file that
// passed the precheck is refused here, as main.rs:503-513 does)
int load_inputs(const Args& a, BlockStore& bs, uint8_t mroot[32]) {
  std::string err;
  bool have = false;
  if (!a.assume) {
    if (precheck(a, bs)) return 1;
    have = !is_jsonl_like(a.blocks);
  }
  if (!load_manifest(a.manifest, mroot, nullptr, err)) { fprintf(stderr, "Error: reading manifest: %s\n", err.c_str()); return 1; }
  if (!have && !load_blocks(a.blocks, bs, err)) { fprintf(stderr, "Error: reading blocks: %s\n", err.c_str()); return 1; }
  return 0;
}

// A .cbor block file is decoded on the device (at the headline
// shape the copy and the kernels take 12 ms against the host decoder's 323 ms)
bool blocks_on_device(const Args& a) { return ext_lower(a.blocks) == "cbor" && !a.host_decode; }

void usage();
int write_artifact(const Args& a, const std::vector<uint8_t>& cbor, uint32_t tau);
std::vector<uint8_t> manifest_json(const uint8_t root[32], uint32_t n_leaves);

// `prove --trace`: the movement log (TraceFile CBOR) instead of blocks and a
// manifest. The device partitions it into blocks of --b steps and commits the
// manifest (sezkp_ctx_upload_trace); --manifest, when given, must carry that
// root; --out-blocks / --out-manifest write what `simulate` and `commit` would
// have written for the same trace.
int cmd_prove_trace(const Args& a) {
  if (!a.blocks.empty()) { fprintf(stderr, "Error: --blocks and --trace are mutually exclusive\n"); usage(); return 2; }
  if (ext_lower(a.trace) != "cbor") { fprintf(stderr, "Error: --trace reads a .cbor trace file\n"); usage(); return 2; }
  if (!a.b_given || a.out.empty()) { fprintf(stderr, "Error: prove --trace needs --b and --out\n"); usage(); return 2; }
  const unsigned long long b = strtoull(a.b.c_str(), nullptr, 10);
  if (b == 0 || b > 0xFFFFFFFFull) { fprintf(stderr, "Error: --b must be in 1..=2^32-1\n"); return 2; }
  if (!a.out_blocks.empty()) {
    const std::string e = ext_lower(a.out_blocks);
    if (e != "cbor" && e != "jsonl" && e != "ndjson") {
      fprintf(stderr, "Error: --out-blocks must end in .cbor, .jsonl or .ndjson\n");
      return 2;
    }
  }
  std::string err;
  std::vector<uint8_t> raw;
  if (!read_file(a.trace, raw, err)) { fprintf(stderr, "Error: reading trace: %s\n", err.c_str()); return 1; }
  char msg[512] = {0};
  // A file with the canonical head goes to the device as bytes and is decoded
  // there (sezkp_ctx_upload_trace_cbor); any other, and every file with
  // --host-decode, is decoded here first, as it always was.
  uint64_t head_t = 0, head_off = 0;
  uint32_t head_tau = 0;
  const bool by_bytes = !a.host_decode && sezkp_trace_cbor_head(raw.data(), raw.size(), &head_t, &head_tau, &head_off) == 1;
  sezkp_trace* th = nullptr;
  sezkp_trace_view tv{};
  if (!by_bytes) {
    if (sezkp_trace_decode_cbor(raw.data(), raw.size(), &th, msg, sizeof msg)) {
      fprintf(stderr, "Error: reading trace: %s\n", msg);
      return 1;
    }
    tv = *sezkp_trace_view_of(th);
  } else {
    tv.t = head_t;
    tv.tau = head_tau;
  }
  tv.b = (uint32_t)b;
  uint8_t want[32], root[32];
  const bool have_manifest = !a.manifest.empty();
  int rc = 1;
  sezkp_ctx* ctx = nullptr;
  sezkp_buf pb{};
  do {
    if (have_manifest && !load_manifest(a.manifest, want, nullptr, err)) {
      fprintf(stderr, "Error: reading manifest: %s\n", err.c_str());
      break;
    }
    ctx = sezkp_ctx_create(0, msg, sizeof msg);
    if (!ctx) { fprintf(stderr, "Error: stark-v1 proof failed: %s\n", msg); break; }
    if (by_bytes) {
      // from the pageable bytes as they were read: the context stages them
      // through its own page-locked block (11.6 ms at the headline shape,
      // against 8.6 ms from bytes that are page-locked already; locking 239 MB
      // for one copy was not shown to cost less than the 3 ms it could save)
      const int32_t urc = sezkp_ctx_upload_trace_cbor(ctx, raw.data(), raw.size(), tv.b, msg, sizeof msg);
      if (urc == SEZKP_E_DECODE) { fprintf(stderr, "Error: reading trace: %s\n", msg); break; }
      if (urc) { fprintf(stderr, "Error: stark-v1 proof failed: %s\n", msg); break; }
      // the shape of what was decoded, on whichever path
      sezkp_trace_ingest_info ii{};
      if (sezkp_ctx_trace_ingest_stats(ctx, &ii)) { fprintf(stderr, "Error: stark-v1 proof failed: no ingest report\n"); break; }
      tv.t = ii.t;
      tv.tau = ii.tau;
    } else if (sezkp_ctx_upload_trace(ctx, &tv, msg, sizeof msg)) {
      fprintf(stderr, "Error: stark-v1 proof failed: %s\n", msg);
      break;
    }
    if (sezkp_ctx_manifest_root(ctx, 0, root, msg, sizeof msg)) {
      fprintf(stderr, "Error: stark-v1 proof failed: %s\n", msg);
      break;
    }
    if (have_manifest && memcmp(want, root, 32) != 0) {
      fprintf(stderr, "Error: stark-v1 proof failed: manifest root mismatch: manifest=%s, trace=%s\n",
              hex(want, 32).c_str(), hex(root, 32).c_str());
      break;
    }
    const uint32_t flags = SEZKP_FLAG_ROOT_FROM_TRACE | (a.stream ? SEZKP_FLAG_STREAMING : 0);
    if (sezkp_ctx_prove(ctx, nullptr, flags, &pb, msg, sizeof msg)) {
      fprintf(stderr, "Error: stark-v1 proof failed: %s\n", msg);
      break;
    }
    const uint32_t nblk = (uint32_t)((tv.t + b - 1) / b);
    if (!a.out_blocks.empty() && ext_lower(a.out_blocks) == "cbor" && !a.host_decode) {
      // written on the device from the resident image: only the file's bytes
      // come home (sezkp_ctx_encode_trace_blocks_cbor; adopted by DESIGN §14's
      // measurement). --host-decode keeps the former order throughout.
      sezkp_buf buf{};
      if (sezkp_ctx_encode_trace_blocks_cbor(ctx, &buf, msg, sizeof msg)) {
        fprintf(stderr, "Error: %s\n", msg);
        break;
      }
      std::vector<uint8_t> out(buf.data, buf.data + buf.len);
      sezkp_buf_free(&buf);
      if (!write_file(a.out_blocks, out, err)) { fprintf(stderr, "Error: %s\n", err.c_str()); break; }
    } else if (!a.out_blocks.empty()) {
      sezkp_blocks* bh = nullptr;
      // decoded on the device: the steps come back from there (NULL steps)
      if (sezkp_ctx_trace_blocks(ctx, by_bytes ? nullptr : &tv, &bh, msg, sizeof msg)) {
        fprintf(stderr, "Error: %s\n", msg);
        break;
      }
      sezkp_buf buf{};
      const int32_t erc = ext_lower(a.out_blocks) == "cbor" ? sezkp_blocks_encode_cbor(sezkp_blocks_view(bh), &buf)
                                                            : sezkp_blocks_encode_jsonl(sezkp_blocks_view(bh), &buf);
      sezkp_blocks_free(bh);
      if (erc != SEZKP_OK) { fprintf(stderr, "Error: encoding blocks failed (%d)\n", erc); break; }
      std::vector<uint8_t> out(buf.data, buf.data + buf.len);
      sezkp_buf_free(&buf);
      if (!write_file(a.out_blocks, out, err)) { fprintf(stderr, "Error: %s\n", err.c_str()); break; }
    }
    if (!a.out_manifest.empty()) {
      // the root `commit` gives for the blocks file: the Frontier for JSON Lines
      uint8_t mroot[32];
      memcpy(mroot, root, 32);
      if (is_jsonl_like(a.out_blocks) && sezkp_ctx_manifest_root(ctx, 1, mroot, msg, sizeof msg)) {
        fprintf(stderr, "Error: %s\n", msg);
        break;
      }
      const std::vector<uint8_t> out =
          ext_lower(a.out_manifest) == "cbor" ? encode_manifest_cbor(mroot, nblk) : manifest_json(mroot, nblk);
      if (!write_file(a.out_manifest, out, err)) { fprintf(stderr, "Error: %s\n", err.c_str()); break; }
    }
    std::vector<uint8_t> proof(pb.data, pb.data + pb.len);
    uint64_t domain_n = 0;
    for (int i = 7; i >= 0; i--) domain_n = (domain_n << 8) | proof[i];
    std::vector<MetaEntry> meta = {{"proto", true, "stark-v1", 0}, {"domain_n", false, "", domain_n},
                                   {"tau", false, "", tv.tau}};
    if (a.stream) meta.push_back({"mode", true, "streaming", 0});
    rc = write_artifact(a, encode_artifact_cbor("stark", root, proof, meta), tv.tau);
  } while (false);
  sezkp_buf_free(&pb);
  if (ctx) sezkp_ctx_destroy(ctx);
  sezkp_trace_free(th);
  return rc;
}

// `prove --blocks X.cbor` with the file decoded on the device: ingest, then
// the precheck (verify_block_file_against_manifest, lib.rs:302-337) on the
// block fields that came home (the manifest root reads no step), then the
// upload of the ingest, then the proof. Messages and exit codes are those of
// precheck / load_inputs / cmd_prove below. -1: no device could be opened.
int cmd_prove_blocks_device(const Args& a) {
  // without a device the host's order below answers, with the lines it always had
  char msg[512] = {0};
  sezkp_ctx* ctx = sezkp_ctx_create(0, msg, sizeof msg);
  if (!ctx) return -1;
  struct Close {
    sezkp_ctx* c;
    ~Close() { sezkp_ctx_destroy(c); }
  } close{ctx};
  uint8_t mroot[32], got[32];
  uint32_t nl = 0;
  std::string err;
  if (!a.assume && !load_manifest(a.manifest, mroot, &nl, err)) {
    fprintf(stderr, "Error: blocks/manifest mismatch: %s\n", err.c_str());
    return 1;
  }
  auto blocks_error = [&](const char* what) {
    if (a.assume) fprintf(stderr, "Error: reading blocks: %s\n", what);
    else fprintf(stderr, "Error: blocks/manifest mismatch: read blocks %s: %s\n", a.blocks.c_str(), what);
  };
  std::vector<uint8_t> raw;
  if (!read_file(a.blocks, raw, err)) { blocks_error(err.c_str()); return 1; }
  int rc = 1;
  sezkp_blocks* meta = nullptr;
  sezkp_buf pb{};
  do {
    static const uint8_t none = 0;  // an empty file is still a file: the decoder answers
    const int32_t irc = sezkp_ctx_ingest_blocks_cbor(ctx, raw.empty() ? &none : raw.data(), raw.size(), &meta, msg, sizeof msg);
    if (irc == SEZKP_E_DECODE) { blocks_error(msg); break; }
    if (irc) { fprintf(stderr, "Error: stark-v1 proof failed: %s\n", msg); break; }
    sezkp_blocks_ingest_info ii{};
    if (a.ingest_stats && sezkp_ctx_blocks_ingest_stats(ctx, &ii) == SEZKP_OK)
      fprintf(stderr, "blocks ingest: path=%s reason=%u index=%llu bytes=%llu blocks=%u t=%llu tau=%u h2d_ms=%.3f "
              "decode_ms=%.3f host_ms=%.3f\n", ii.path == SEZKP_INGEST_DEVICE ? "device" : "host", ii.reason,
              (unsigned long long)ii.index, (unsigned long long)ii.bytes, ii.n_blocks, (unsigned long long)ii.t, ii.tau,
              ii.ms_h2d, ii.ms_decode, ii.ms_host);
    const sezkp_block_view* v = sezkp_blocks_view(meta);
    if (!a.assume) {
      manifest_root(*v, got);
      if (memcmp(got, mroot, 32) != 0) {
        fprintf(stderr, "Error: blocks/manifest mismatch: root mismatch: manifest=%s, recomputed=%s\n",
                hex(mroot, 32).c_str(), hex(got, 32).c_str());
        break;
      }
      if (nl != v->n_blocks) {
        fprintf(stderr, "Error: blocks/manifest mismatch: leaf count mismatch: manifest=%u, recomputed=%u\n", nl,
                v->n_blocks);
        break;
      }
    }
    if (!load_manifest(a.manifest, mroot, nullptr, err)) { fprintf(stderr, "Error: reading manifest: %s\n", err.c_str()); break; }
    const uint32_t flags = a.stream ? SEZKP_FLAG_STREAMING : 0;
    if (sezkp_ctx_upload_ingested(ctx, msg, sizeof msg) || sezkp_ctx_prove(ctx, mroot, flags, &pb, msg, sizeof msg)) {
      fprintf(stderr, "Error: stark-v1 proof failed: %s\n", msg);
      break;
    }
    std::vector<uint8_t> proof(pb.data, pb.data + pb.len);
    uint64_t domain_n = 0;
    for (int i = 7; i >= 0; i--) domain_n = (domain_n << 8) | proof[i];
    std::vector<MetaEntry> m = {{"proto", true, "stark-v1", 0}, {"domain_n", false, "", domain_n},
                                {"tau", false, "", v->tau}};
    if (a.stream) m.push_back({"mode", true, "streaming", 0});
    rc = write_artifact(a, encode_artifact_cbor("stark", mroot, proof, m), v->tau);
  } while (false);
  sezkp_buf_free(&pb);
  sezkp_blocks_free(meta);
  return rc;
}

int cmd_prove(const Args& a) {
  if (!a.trace.empty()) return cmd_prove_trace(a);
  if (blocks_on_device(a)) {
    const int rc = cmd_prove_blocks_device(a);
    if (rc >= 0) return rc;
  }
  std::string err;
  BlockStore bs;
  uint8_t mroot[32];
  if (load_inputs(a, bs, mroot)) return 1;
  sezkp_buf art{};
  char msg[512] = {0};
  const int32_t rc = sezkp_stark_v1_prove_artifact_cbor(&bs.view, mroot, a.stream ? SEZKP_FLAG_STREAMING : 0, &art,
                                                        msg, sizeof msg);
  if (rc) { fprintf(stderr, "Error: stark-v1 proof failed: %s\n", msg); return 1; }
  std::vector<uint8_t> cbor(art.data, art.data + art.len);
  sezkp_buf_free(&art);
  return write_artifact(a, cbor, bs.view.tau);
}

// write_proof_auto (io.rs:199-205): the artifact as CBOR, or as JSON unless the path ends in .cbor
int write_artifact(const Args& a, const std::vector<uint8_t>& cbor, uint32_t tau) {
  std::string err;
  Artifact dec;
  decode_artifact_cbor(cbor.data(), cbor.size(), dec, err);
  std::vector<uint8_t> outb = cbor;
  if (ext_lower(a.out) != "cbor") {  // write_proof_auto: JSON unless .cbor (io.rs:199-205)
    const bool streaming = a.stream;
    uint64_t domain_n = 0;
    for (int i = 7; i >= 0; i--) domain_n = (domain_n << 8) | dec.proof_bytes[i];
    std::vector<MetaEntry> meta = {{"proto", true, "stark-v1", 0}, {"domain_n", false, "", domain_n},
                                   {"tau", false, "", tau}};
    if (streaming) meta.push_back({"mode", true, "streaming", 0});
    // serde_json pretty nests the meta object one level deeper
    std::string mj = meta_to_json(meta);
    std::string nested = "{\n";
    {
      std::vector<MetaEntry> m = meta;
      std::sort(m.begin(), m.end(), [](const MetaEntry& x, const MetaEntry& y) { return x.key < y.key; });
      for (size_t i = 0; i < m.size(); i++)
        nested += "    \"" + m[i].key + "\": " + (m[i].is_str ? "\"" + m[i].s + "\"" : std::to_string(m[i].u)) +
                  (i + 1 < m.size() ? ",\n" : "\n");
      nested += "  }";
    }
    (void)mj;
    dec.meta_json = nested;
    std::string js = pretty_artifact(dec);
    outb.assign(js.begin(), js.end());
  }
  if (!write_file(a.out, outb, err)) { fprintf(stderr, "Error: writing proof to %s: %s\n", a.out.c_str(), err.c_str()); return 1; }
  printf("Proved with Stark, wrote %s (%zu bytes)\n", a.out.c_str(), dec.proof_bytes.size());
  return 0;
}

int cmd_verify(const Args& a) {
  std::string err;
  BlockStore bs;
  uint8_t mroot[32];
  if (load_inputs(a, bs, mroot)) return 1;
  std::vector<uint8_t> raw;
  if (!read_file(a.proof, raw, err)) { fprintf(stderr, "Error: reading proof artifact: %s\n", err.c_str()); return 1; }
  if (ext_lower(a.proof) != "cbor") { fprintf(stderr, "Error: only .cbor proof artifacts are supported for verify\n"); return 1; }
  Artifact art;
  if (!decode_artifact_cbor(raw.data(), raw.size(), art, err)) { fprintf(stderr, "Error: %s\n", err.c_str()); return 1; }
  if (art.backend != "stark") { fprintf(stderr, "Error: stark-v1 verification failed: backend kind mismatch: expected STARK\n"); return 1; }
  if (art.manifest_root.size() != 32 || memcmp(art.manifest_root.data(), mroot, 32)) {
    fprintf(stderr, "Error: stark-v1 verification failed: manifest root mismatch\n");
    return 1;
  }
  char msg[512] = {0};
  if (a.gpu && !(bs.view.n_blocks && bs.view.tau == 0)) {  // a tau of 0 to check: only the host call can say it
    sezkp_proof_ref ref{art.proof_bytes.data(), art.proof_bytes.size(), mroot, bs.view.n_blocks ? bs.view.tau : 0, 0};
    sezkp_verify_result res{};
    if (sezkp_stark_v1_verify_batch(&ref, 1, &res, msg, sizeof msg)) {
      fprintf(stderr, "Error: stark-v1 verification on the GPU could not run: %s\n", msg);
      return 1;
    }
    if (res.code) {
      fprintf(stderr, "Error: stark-v1 verification failed: %s\n", res.msg);
      return 1;
    }
  } else if (sezkp_stark_v1_verify(art.proof_bytes.data(), art.proof_bytes.size(), &bs.view, mroot, msg, sizeof msg)) {
    fprintf(stderr, "Error: stark-v1 verification failed: %s\n", msg);
    return 1;
  }
  printf("OK: proof verified\n");
  return 0;
}

int cmd_commit(const Args& a) {
  std::string err;
  BlockStore bs;
  if (!load_blocks_any(a.blocks, bs, err)) { fprintf(stderr, "Error: read blocks %s: %s\n", a.blocks.c_str(), err.c_str()); return 1; }
  uint8_t root[32];
  file_root(a.blocks, bs, root);
  std::vector<uint8_t> out;
  if (ext_lower(a.out) == "cbor") out = encode_manifest_cbor(root, bs.view.n_blocks);
  else out = manifest_json(root, bs.view.n_blocks);
  if (!write_file(a.out, out, err)) { fprintf(stderr, "Error: %s\n", err.c_str()); return 1; }
  printf("Committed %u leaves, root=%s, wrote manifest %s\n", bs.view.n_blocks, hex(root, 32).c_str(), a.out.c_str());
  return 0;
}

std::vector<uint8_t> manifest_json(const uint8_t root[32], uint32_t n_leaves) {
  std::string s = "{\n  \"version\": 1,\n  \"root\": [\n";
  for (int i = 0; i < 32; i++) s += "    " + std::to_string(root[i]) + (i < 31 ? ",\n" : "\n");
  s += "  ],\n  \"n_leaves\": " + std::to_string(n_leaves) + "\n}";
  return std::vector<uint8_t>(s.begin(), s.end());
}

// `verify-commit` (main.rs:377-398): the precheck of prove/verify on its own
int cmd_verify_commit(const Args& a) {
  BlockStore bs;
  if (precheck(a, bs)) return 1;
  printf("OK: %s matches manifest %s\n", a.blocks.c_str(), a.manifest.c_str());
  return 0;
}

// mkdir -p of the output's parent directory (main.rs:299-307)
bool ensure_parent_dir(const std::string& path, std::string& err) {
  const size_t s = path.find_last_of('/');
  if (s == std::string::npos || s == 0) return true;
  const std::string dir = path.substr(0, s);
  for (size_t i = 1; i <= dir.size(); i++) {
    if (i < dir.size() && dir[i] != '/') continue;
    const std::string part = dir.substr(0, i);
    struct stat st;
    if (stat(part.c_str(), &st) == 0) {
      if (!S_ISDIR(st.st_mode)) { err = "creating parent directory " + dir + ": not a directory"; return false; }
    } else if (mkdir(part.c_str(), 0777) != 0) {
      err = "creating parent directory " + dir;
      return false;
    }
  }
  return true;
}

// `export-jsonl` (main.rs:400-424): any blocks file (stream_block_summaries_auto,
// io.rs:111-139: .jsonl/.ndjson, .json, .cbor) -> one serde_json object per line
// (the layout of write_block_summaries_jsonl, io_jsonl.rs:93-106)
int cmd_export_jsonl(const Args& a) {
  if (a.input.empty() || a.out.empty()) { fprintf(stderr, "Error: export-jsonl needs --input and --output\n"); return 2; }
  const std::string e = ext_lower(a.input);
  if (e != "jsonl" && e != "ndjson" && e != "json" && e != "cbor") {
    fprintf(stderr, "Error: open input stream: %s\n",
            e.empty() ? "path has no extension (expected .json, .cbor, .jsonl, or .ndjson)"
                      : ("unsupported blocks extension: " + e + " (supported: .json, .cbor, .jsonl, .ndjson)").c_str());
    return 1;
  }
  std::string err;
  BlockStore bs;
  if (!load_blocks_any(a.input, bs, err)) { fprintf(stderr, "Error: open input stream: %s\n", err.c_str()); return 1; }
  sezkp_buf buf{};
  const int32_t rc = sezkp_blocks_encode_jsonl(&bs.view, &buf);
  if (rc != SEZKP_OK) { fprintf(stderr, "Error: serialize block as JSON line (%d)\n", rc); return 1; }
  std::vector<uint8_t> out(buf.data, buf.data + buf.len);
  sezkp_buf_free(&buf);
  if (!ensure_parent_dir(a.out, err) || !write_file(a.out, out, err)) {
    fprintf(stderr, "Error: %s\n", err.c_str());
    return 1;
  }
  printf("Exported %u blocks \xe2\x86\x92 %s\n", bs.view.n_blocks, a.out.c_str());
  return 0;
}

// `simulate` (main.rs:317-350): generate_trace + partition_trace, written as
// CBOR (.cbor) or NDJSON (.jsonl/.ndjson) by extension
int cmd_simulate(const Args& a) {
  char* end = nullptr;
  const unsigned long long t = strtoull(a.t.c_str(), &end, 10);
  const unsigned long long b = strtoull(a.b.c_str(), nullptr, 10);
  const unsigned long long tau = strtoull(a.tau.c_str(), nullptr, 10);
  if (t == 0 || t > 0xFFFFFFFFull || b == 0 || tau == 0 || tau > 255) {
    fprintf(stderr, "Error: need --t in 1..=2^32-1, --b >= 1, --tau in 1..=255\n");
    return 2;
  }
  if (b > t) {
    fprintf(stderr, "Error: number of blocks b (%llu) cannot exceed trace length T (%llu)\n", b, t);
    return 1;
  }
  const std::string e = ext_lower(a.out);
  if (e != "cbor" && e != "jsonl" && e != "ndjson") {
    fprintf(stderr, "Error: --out-blocks must end in .cbor, .jsonl or .ndjson\n");
    return 2;
  }
  sezkp_blocks* h = nullptr;
  char err[512] = {0};
  if (sezkp_simulate_blocks(t, (uint32_t)b, (uint32_t)tau, 42, &h, err, sizeof err) != SEZKP_OK) {
    fprintf(stderr, "Error: %s\n", err);
    return 1;
  }
  const sezkp_block_view* v = sezkp_blocks_view(h);
  const uint32_t nb = v->n_blocks;
  sezkp_buf buf{};
  const int32_t rc = e == "cbor" ? sezkp_blocks_encode_cbor(v, &buf) : sezkp_blocks_encode_jsonl(v, &buf);
  sezkp_blocks_free(h);
  if (rc != SEZKP_OK) { fprintf(stderr, "Error: encoding blocks failed (%d)\n", rc); return 1; }
  std::vector<uint8_t> out(buf.data, buf.data + buf.len);
  sezkp_buf_free(&buf);
  std::string werr;
  if (!write_file(a.out, out, werr)) { fprintf(stderr, "Error: %s\n", werr.c_str()); return 1; }
  printf("Simulated trace: T=%llu, b=%llu, \xcf\x84=%llu \xe2\x86\x92 %u blocks \xe2\x86\x92 %s\n", t, b, tau, nb,
         a.out.c_str());
  return 0;
}

// `audit`: the full-trace AIR audit (sezkp_stark_v1_air_audit; no counterpart
// in the reference CLI). Exit 0 when the AIR holds on every row, 3 when a row
// violates it.
int cmd_audit(const Args& a) {
  if (a.blocks.empty()) { fprintf(stderr, "Error: audit needs --blocks\n"); return 2; }
  std::string err;
  BlockStore bs;
  sezkp_air_audit au;
  char msg[512] = {0};
  sezkp_ctx* ctx = blocks_on_device(a) ? sezkp_ctx_create(0, msg, sizeof msg) : nullptr;
  if (ctx) {
    // the file's bytes to the device, decoded and audited there (without a
    // device the host's order below answers, as it always did)
    std::vector<uint8_t> raw;
    int32_t rc = SEZKP_OK;
    if (!read_file(a.blocks, raw, err)) {
      fprintf(stderr, "Error: read blocks %s: %s\n", a.blocks.c_str(), err.c_str());
      rc = 1;
    } else {
      static const uint8_t none = 0;
      rc = sezkp_ctx_upload_blocks_cbor(ctx, raw.empty() ? &none : raw.data(), raw.size(), msg, sizeof msg);
      if (rc == SEZKP_E_DECODE) fprintf(stderr, "Error: read blocks %s: %s\n", a.blocks.c_str(), msg);
      else if (rc || (rc = sezkp_ctx_air_audit(ctx, &au, nullptr, nullptr, msg, sizeof msg)))
        fprintf(stderr, "Error: AIR audit failed: %s\n", msg);
    }
    sezkp_ctx_destroy(ctx);
    if (rc) return 1;
  } else {
    if (!load_blocks_any(a.blocks, bs, err)) { fprintf(stderr, "Error: read blocks %s: %s\n", a.blocks.c_str(), err.c_str()); return 1; }
    if (sezkp_stark_v1_air_audit(&bs.view, &au, nullptr, nullptr, msg, sizeof msg)) {
      fprintf(stderr, "Error: AIR audit failed: %s\n", msg);
      return 1;
    }
  }
  static const char* NAME[SEZKP_AIR_FAMILIES] = {"mv_domain", "head_range", "slack_range", "sym_range", "boundary"};
  // NUM_QUERIES = 30 independent draws mod n (params.rs:31,95-105)
  double miss = 1.0;
  for (int q = 0; q < 30; q++) miss *= 1.0 - (double)au.rows_rejectable / (double)au.n_rows;
  const double p_reject = 1.0 - miss;
  auto row = [](uint64_t r) { return r == UINT64_MAX ? std::string("null") : std::to_string(r); };
  if (a.json) {
    printf("{\"n_rows\": %llu, \"tau\": %u, \"ok\": %s, \"families\": {", (unsigned long long)au.n_rows, au.tau,
           au.rows_violating ? "false" : "true");
    for (int f = 0; f < SEZKP_AIR_FAMILIES; f++) {
      const sezkp_air_family& m = au.fam[f];
      printf("%s\"%s\": {\"cells\": %llu, \"rows\": %llu, \"first_row\": %s, \"first_tape\": %u, \"first_value\": %llu}",
             f ? ", " : "", NAME[f], (unsigned long long)m.cells, (unsigned long long)m.rows, row(m.first_row).c_str(),
             m.first_tape, (unsigned long long)m.first_value);
    }
    printf("}, \"rows_violating\": %llu, \"first_violating\": %s, \"rows_rejectable\": %llu, \"first_rejectable\": %s, "
           "\"verify_reject_probability\": %.17g}\n",
           (unsigned long long)au.rows_violating, row(au.first_violating).c_str(),
           (unsigned long long)au.rows_rejectable, row(au.first_rejectable).c_str(), p_reject);
  } else {
    printf("AIR audit: %llu rows, tau=%u\n", (unsigned long long)au.n_rows, au.tau);
    for (int f = 0; f < SEZKP_AIR_FAMILIES; f++) {
      const sezkp_air_family& m = au.fam[f];
      if (m.cells)
        printf("%-12s cells=%llu rows=%llu first: row %llu tape %u value %llu\n", NAME[f], (unsigned long long)m.cells,
               (unsigned long long)m.rows, (unsigned long long)m.first_row, m.first_tape,
               (unsigned long long)m.first_value);
      else
        printf("%-12s cells=0 rows=0\n", NAME[f]);
    }
    printf("violating rows:  %llu (first %s)\n", (unsigned long long)au.rows_violating, row(au.first_violating).c_str());
    printf("rejectable rows: %llu (first %s)\n", (unsigned long long)au.rows_rejectable,
           row(au.first_rejectable).c_str());
    printf("verifier rejects with probability %.6g (30 queries)\n", p_reject);
  }
  return au.rows_violating ? 3 : 0;
}

void usage() {
  fprintf(stderr,
          "usage: sezkp-cli prove  --backend stark --blocks B --manifest M --out P [--stream] [--assume-committed]\n"
          "                        [--host-decode] [--ingest-stats]\n"
          "       sezkp-cli prove  --backend stark --trace T.cbor --b STEPS_PER_BLOCK --out P [--out-blocks F]\n"
          "                        [--out-manifest F] [--manifest M] [--stream] [--host-decode]\n"
          "       sezkp-cli verify --backend stark --blocks B --manifest M --proof P [--assume-committed] [--gpu]\n"
          "       sezkp-cli commit --blocks B --out M\n"
          "       sezkp-cli verify-commit --blocks B --manifest M\n"
          "       sezkp-cli export-jsonl --input B --output B.jsonl\n"
          "       sezkp-cli simulate --t T --b STEPS_PER_BLOCK --tau TAU --out-blocks B(.cbor|.jsonl)\n"
          "       sezkp-cli audit --blocks B [--json] [--host-decode]\n");
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 2) { usage(); return 2; }
  Args a;
  a.cmd = argv[1];
  for (int i = 2; i < argc; i++) {
    std::string s = argv[i];
    auto val = [&](std::string& dst) {
      if (i + 1 >= argc) { usage(); exit(2); }
      dst = argv[++i];
    };
    if (s == "--backend" || s == "-b") val(a.backend);
    else if (s == "--blocks") val(a.blocks);
    else if (s == "--manifest") val(a.manifest);
    else if (s == "--out" || s == "-o") val(a.out);
    else if (s == "--proof") val(a.proof);
    else if (s == "--out-blocks") {  // simulate's output; with prove --trace the partition beside the proof
      val(a.out_blocks);
      if (a.cmd != "prove") a.out = a.out_blocks;
    } else if (s == "--output") val(a.out);
    else if (s == "--trace") val(a.trace);
    else if (s == "--host-decode") a.host_decode = true;
    else if (s == "--ingest-stats") a.ingest_stats = true;
    else if (s == "--out-manifest") val(a.out_manifest);
    else if (s == "--input") val(a.input);
    else if (s == "--t") val(a.t);
    else if (s == "--b") { val(a.b); a.b_given = true; }
    else if (s == "--tau") val(a.tau);
    else if (s == "--stream") a.stream = true;
    else if (s == "--assume-committed") a.assume = true;
    else if (s == "--json") a.json = true;
    else if (s == "--gpu") a.gpu = true;
    else { fprintf(stderr, "unknown argument %s\n", s.c_str()); usage(); return 2; }
  }
  for (auto& c : a.backend) c = (char)tolower((unsigned char)c);
  if (a.cmd == "commit") return cmd_commit(a);
  if (a.cmd == "simulate") return cmd_simulate(a);
  if (a.cmd == "verify-commit") return cmd_verify_commit(a);
  if (a.cmd == "export-jsonl") return cmd_export_jsonl(a);
  if (a.cmd == "audit") return cmd_audit(a);
  if (a.backend != "stark") {
    fprintf(stderr, "Error: only --backend stark is implemented by the MI355X build\n");
    return 2;
  }
  if (a.cmd == "prove") return cmd_prove(a);
  if (a.cmd == "verify") return cmd_verify(a);
  usage();
  return 2;
}
