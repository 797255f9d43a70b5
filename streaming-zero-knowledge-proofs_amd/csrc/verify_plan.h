// verify_plan.h — the two phases of verify_v1 (verify.cpp) as the host and the
// GPU back ends share them. verify_parse walks the proof bytes once, keeps
// offsets only and lists every Merkle chain the verifier can ask about as a
// VerifyJob; verify_decide walks the reference's sequence of checks and asks
// for a job's outcome wherever it hashed a path before. outcome == nullptr
// hashes the chain on the spot (sezkp_stark_v1_verify); otherwise outcome[j]
// is the word k_verify_chains (verify_gpu.hip) wrote for job j.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <memory>
#include <string>
#include <vector>

#include "../../include/sezkp_stark.h"

namespace sezkp {

// tag = label id (low 56 bits) | leaf kind | flags
constexpr uint64_t VJ_LEAF_U64 = 0ull << 56;      // leaf = BLAKE3(8 value bytes)
constexpr uint64_t VJ_LEAF_LABELED = 1ull << 56;  // leaf = BLAKE3("col_leaf" || len || label || 8 value bytes)
constexpr uint64_t VJ_DIGEST = 2ull << 56;        // the chain starts from 32 given bytes (path_to_chunk)
constexpr uint64_t VJ_KIND_MASK = 3ull << 56;
constexpr uint64_t VJ_ROOT_TABLE = 4ull << 56;    // root = column index (the header's roots are not aligned)
constexpr uint64_t VJ_HOST = 8ull << 56;          // not for the kernel: the host back end answers it
constexpr uint64_t VJ_LABEL_MASK = (1ull << 56) - 1;

// Offsets are bytes from the proof's first byte; every range a job names was
// shown to lie inside the proof before the job was created.
struct VerifyJob {
  uint64_t leaf;   // the 8 value bytes, or the 32-byte digest
  uint64_t sibs;   // nsib x 32 bytes
  uint64_t root;   // the expected 32 bytes (VJ_ROOT_TABLE: the column index)
  uint64_t index;  // leaf index; bit 0 picks the side, then it shifts down (to 0 past 64 siblings)
  uint64_t nsib;
  uint64_t tag;
};
// The job as the kernel reads it: offsets into the slice's bytes (the root's
// into the root table with VJ_ROOT_TABLE), and the result word it writes
// (the job's number among all of the slice's jobs: VJ_HOST jobs are not sent).
struct VerifyJobDev {
  uint64_t leaf, sibs, root, index;
  uint32_t nsib;  // <= VERIFY_MAX_DEV_SIBS
  uint32_t out;
  uint64_t tag;
};
static_assert(sizeof(VerifyJobDev) == 48, "device layout");

// Message template of a labelled leaf (one 64-byte block: the labels the
// verifier constructs are at most 28 bytes): the value goes at byte `off`.
struct VerifyLabel {
  uint32_t words[16];
  uint32_t off;
  uint32_t pad;
};
// Label ids: 0 input_mv, 1 is_first, 2 is_last, 3 + 7 t + u for tape t and
// u = mv, wflag, wsym, head, winlen, in_off, out_off.
std::string verify_label_name(uint64_t id);
void verify_label_template(uint64_t id, VerifyLabel& out);

// what the kernel is given: longer chains and larger label ids go to the host
constexpr uint64_t VERIFY_MAX_DEV_SIBS = 1024;
constexpr uint64_t VERIFY_MAX_DEV_LABELS = 1u << 16;

struct ParsedProof;
struct VerifyItem {
  sezkp_proof_ref ref{};          // ref.tau is not read: check_tau / tau_want are
  bool check_tau = false;         // "tau mismatch vs. block windows" against tau_want
  uint64_t tau_want = 0;
  bool decided = false;  // the verdict is final (code, msg)
  int32_t code = SEZKP_OK;
  std::string msg;
  size_t hdr_len = 0;               // bytes before the body (from there on every field is 8-byte aligned)
  std::vector<uint64_t> col_roots;  // offset of each column root
  std::vector<VerifyJob> jobs;
  uint64_t n_dev_labels = 0;        // 1 + the largest label id of a job without VJ_HOST
  std::shared_ptr<ParsedProof> parsed;
};
// Neither throws. parse: the checks sezkp_stark_v1_verify makes before the
// body and the bincode walk; a failure there is the verdict (decided).
void verify_parse(VerifyItem& it);
void verify_decide(VerifyItem& it, const uint32_t* outcome);
// the chain of one job on the host (what outcome[j] == 1 stands for)
bool verify_job_on_host(const VerifyItem& it, const VerifyJob& job);

}  // namespace sezkp
