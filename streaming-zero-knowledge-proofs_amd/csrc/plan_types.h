// plan_types.h — the shapes and constants the upload's planning arithmetic
// (prove_plan.h) shares with the kernels (sezkp_internal.h includes this):
// plain structs and integer helpers, no HIP, so a host-only program can plan.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#ifdef __HIPCC__
#define SEZKP_HD __host__ __device__
#else
#define SEZKP_HD
#endif

namespace sezkp {

// A binary Merkle tree over 2^logLen leaves whose levels >= lstore are kept
// in HBM: level l (lstore <= l <= logLen) starts at node
// off(l) = 2^(logLen-lstore+1) - 2^(logLen-l+1); 8 u32 words per node.
// Lower levels are recomputed from the leaf values when a path is opened.
struct TreeDev {
  uint32_t* nodes;
  uint32_t* root;   // 8 words
  int logLen;
  int lstore;
};
SEZKP_HD inline uint64_t tree_level_off(int logLen, int lstore, int l) {
  return (1ULL << (logLen - lstore + 1)) - (1ULL << (logLen - l + 1));
}
SEZKP_HD inline uint64_t tree_stored_nodes(int logLen, int lstore) {
  return logLen >= lstore ? (1ULL << (logLen - lstore + 1)) - 1 : 0;
}

// Per-column BLAKE3 message template for labelled leaves
// BLAKE3("col_leaf" || u32 len || label || v LE)  (merkle.rs:132-147).
struct ColTemplate {
  uint32_t words[16];
  uint32_t block_len;  // 20 + len(label)
  uint32_t kind;       // 0 input_mv,1 is_first,2 is_last,3+k: per-tape kind k
  uint32_t tape;
  uint32_t off;        // byte offset of the value = 12 + len(label)
  uint64_t tab;        // node offset of this column's leaf/uniform table, or NO_TAB
  uint32_t tab_log;    // leaf table: log2(entries) (8 or 16); 0 otherwise
  uint32_t pad;
};
constexpr uint64_t NO_TAB = ~0ULL;
constexpr int U_LEVELS = 11;  // uniform-subtree hashes U_0..U_10 (chunk = 2^10 rows)

// Column kinds whose leaf depends on a small raw domain (i8 / u8 / u16):
// leaves come from a per-column table of all possible labelled leaves.
SEZKP_HD inline bool kind_has_leaf_table(uint32_t kind) { return kind == 0 || kind == 3 || kind == 4 || kind == 5; }
// Columns that are piecewise constant along the trace (per-block constants and
// the block-boundary flags): committed from uniform-subtree hashes.
SEZKP_HD inline bool kind_piecewise(uint32_t kind) { return kind == 1 || kind == 2 || kind >= 7; }

// Dictionary (memoized subtree) commitment of dense small-range columns.
constexpr int DICT_LEVELS = 5;          // tables T_0..T_4
constexpr uint32_t DICT_CAP = 65536;    // entries per table level
struct DictCol {
  uint32_t col;
  uint32_t mv;   // head columns: dictionary index of the same tape's mv column (delta plan), else NO_DICT
  uint64_t tab;  // node offset of this column's DICT_LEVELS x DICT_CAP tables
};
SEZKP_HD inline bool kind_dict(uint32_t kind) { return kind == 0 || (kind >= 3 && kind <= 6); }
// Chunk levels 6..9 of every dictionary column (16 + 8 + 4 + 2 nodes per
// 1024-row chunk), written by the commitment, read by the openings.
constexpr int DICT_LANE_LOG = 6;  // rows per lane of the dictionary commitment (level-6 nodes)
constexpr int DLEV_NODES = 30;
constexpr uint32_t NO_DICT = 0xFFFFFFFFu;
// Status words per dictionary column for the wide head ladder, behind the
// piecewise form words (written by k_dict_plan and k_col_commit_dict, home
// with the column roots): [0,1] lo, [2,3] hi (i64), [4] mlo, [5] mhi (i32),
// [6] delta plan, then the 8-row groups taken [7] from L3, [8] through the
// 4-row nodes for a block start, [9] the same for a head or move outside
constexpr int HW_STAT_WORDS = 10;
constexpr int OPEN_REQ_WORDS = 5;  // column, row lo, row hi, ordinal, dictionary index

constexpr int LSTORE_FRI = 6;
constexpr int COL_CHUNK_LOG2 = 10;
// Device image of the bincode ProofV1 body (proof.rs:80-98) after the
// column-root header: every record there is 8-byte aligned and fixed-size,
// so the opening and path kernels write proof bytes in place.
//   0                 u64 #queries
//   8 + q*q_bytes     u64 row, u64 tau, then open_per_q openings of open_bytes
//   fr_off            u64 k+1, (k+1) x 32 B FRI roots            (host)
//   fq_off            u64 #queries
//   fq_off+8+q*fq_bytes  u64 k+1, k+1 positions, u64 k, 2k path records
//   tail_off          final value (8 B), manifest root (32 B)     (root: host)
struct ProofLayout {
  uint32_t* base;          // device pointer, 8-byte aligned
  uint64_t open_bytes;     // 80 + 32*log2(n)
  uint64_t q_bytes;        // 16 + open_per_q * open_bytes
  uint64_t fr_off, fq_off, fq_bytes, tail_off, total;
  uint32_t open_per_q;     // 9*tau + 3
  uint32_t nq;             // queries (params.rs:31)
  int k;                   // log2(N)
  uint32_t tau;
};

constexpr int FS_MAX_BETAS = 64;  // challenge record: betas of one proof (DevChal)

// Upper-level reduction job: one WG reduces <= 1024 stored nodes of `tree`
// from level `from` (WG index wg within that level).
struct UpperJob {
  TreeDev tree;
  int from;
  uint32_t wg;
  int to;  // last level to build (0: up to the root)
  uint32_t pad;
  // sharded cap of a run layer: level `from` (12) comes from the allgathered
  // run roots (rank-major: rank d's nrun roots at [d nrun, (d + 1) nrun)),
  // cap node g = root g >> logP of rank g & (P - 1); the job stores it too
  const uint32_t* gath = nullptr;
  uint64_t nrun = 0;
  int logP = 0;
  int pad2 = 0;
};
// the passes (one launch each) that build levels from + 1 .. `to` of T
inline void plan_upper_jobs(const TreeDev& T, int from, std::vector<std::vector<UpperJob>>& passes, int to = 0,
                            const uint32_t* gath = nullptr, uint64_t nrun = 0, int logP = 0) {
  const int top = (to > 0 && to < T.logLen) ? to : T.logLen;
  if (gath && from == top) {  // a one-node cap (P = 1): the job copies the gathered root into it
    if (passes.empty()) passes.resize(1);
    UpperJob J{T, from, 0u, to, 0};
    J.gath = gath;
    J.nrun = nrun;
    J.logP = logP;
    passes[0].push_back(J);
    return;
  }
  int p = 0;
  while (from < top) {
    const int c = top - from;
    const int step = c < 10 ? c : 10;
    if ((int)passes.size() <= p) passes.resize(p + 1);
    for (uint64_t w = 0; w < (1ULL << (T.logLen - from - step)); w++) {
      UpperJob J{T, from, (uint32_t)w, to, 0};
      if (p == 0 && gath) {  // the first pass reads the gathered run roots (and stores them)
        J.gath = gath;
        J.nrun = nrun;
        J.logP = logP;
      }
      passes[p].push_back(J);
    }
    from += step;
    p++;
  }
}

constexpr int L16_LOG = 12;  // leaves per WG of the 16-leaves-per-lane layer kernel
constexpr int L16S_LOG = 10; // leaves per WG of its 4-leaves-per-lane form (small trees)
constexpr int L16M_LOG = 11; // leaves per WG of its 8-leaves-per-lane form
constexpr int TAIL_MAX = 12;  // small FRI layers of one tail launch (TailArgs)

}  // namespace sezkp
