// prove_plan.h — the arithmetic of sezkp_ctx::upload as pure functions: from
// the trace's shape (tau, block boundaries, rank, P) to sizes and ELEMENT
// OFFSETS, no device pointer and no HIP call. upload (ctx_upload.cpp) runs the
// planners, allocates from their totals and binds pointers as base + offset;
// tools/prove_plan_check.cpp prints the same plans on a machine without a GPU.
// A shape the prover does not take throws PlanError (SEZKP_E_INVALID).
#pragma once
#include <string.h>

#include <algorithm>
#include <string>
#include <utility>
#include <vector>

#include "plan_types.h"

namespace sezkp {

constexpr int NUM_QUERIES = 30;  // params.rs:31
constexpr int BLOWUP_LOG2 = 3;   // params.rs:28

struct PlanError {
  std::string msg;
};

inline int ilog2(uint64_t x) {
  int l = 0;
  while (l < 63 && (1ULL << l) < x) l++;
  return l;
}

// ------------------------------------------------------------------ shape
// The column chunks [ch_lo, ch_hi) rank g of 2^logP commits (all of them on
// one device) and the blocks holding their rows [ch_lo * 1024, ch_hi * 1024]
// (the extra row: compose and the next_* openings read row i + 1; the last
// row's wrap to row 0 is never read: row n - 1 is a block's last row, where
// the head-update term vanishes, and its next_* openings belong to rank 0).
inline void shard_range(const uint64_t* step_start, uint32_t nblk, int logn, int rank, int logP, uint64_t& ch_lo,
                        uint64_t& ch_hi, uint32_t& blk_lo, uint32_t& blk_cnt) {
  const uint64_t n = 1ULL << logn;
  const int logChunks = logn > COL_CHUNK_LOG2 ? logn - COL_CHUNK_LOG2 : 0;
  const uint64_t nchunks = 1ULL << logChunks, chunk_rows = n < 1024 ? n : 1024;
  ch_lo = (nchunks >> logP) * (uint64_t)rank;
  ch_hi = ch_lo + (nchunks >> logP);
  const uint64_t r0 = ch_lo * chunk_rows, r1 = std::min<uint64_t>(ch_hi * chunk_rows, n - 1);
  auto block_of = [&](uint64_t row) {
    return (uint32_t)(std::upper_bound(step_start, step_start + nblk + 1, row) - step_start - 1);
  };
  blk_lo = block_of(r0);
  blk_cnt = block_of(r1) - blk_lo + 1;
}

struct ShapePlan {
  uint32_t tau = 0, nblk = 0;
  uint64_t n = 0, N = 0;
  int logn = 0, logN = 0, ncols = 0, logChunks = 0;
  bool sharded = false;  // the sharded algorithm (also at P = 1 when forced)
  int rank = 0, logP = 0;
  uint64_t ch_lo = 0, ch_hi = 0;     // this rank's column chunks
  uint32_t blk_lo = 0, blk_cnt = 0;  // blocks overlapping this rank's rows (+ the next row)
  uint64_t M = 0;                    // local LDE length N / P
  int logM = 0;
  int rR = -1;  // run layers 0..rR (len >= 4096 P), the rest replicated
  // leaves per WG of the layer-0 tree and the forest: 2048 (L16M_LOG), or 1024
  // (L16S_LOG) when the local LDE has at most 2^21 points. The 2^21 threshold
  // was measured in round 4 (tools/r4i.sh), when the larger size was still
  // 4096 leaves: with 1024-leaf WGs config 3 (N = 2^21, 512 WGs of 4096) in
  // flight went 0.499 -> 0.479 ms per proof and a P = 8 rank's trees were even;
  // at 2^22 points (a P = 4 rank) the larger WGs were faster (layer-0 tree
  // 0.186 against 0.208 ms). Round 5 halved the larger size to 2048
  // (shape_of_logn below).
  int tree_wg_log = L16_LOG;
  bool full_lde = false;  // P = 2: every rank computes the whole N-point LDE
  // level the run-layer WGs reduce to: the run root (12) when run roots are
  // allgathered, else 6 so the upper jobs build levels 7.. with every lane busy
  int tree_stop() const { return sharded ? L16_LOG : LSTORE_FRI; }
  int wg_stop() const { return std::min(tree_stop(), tree_wg_log); }
};

// the kernels index the step arrays through step_start: it must start at 0
inline void plan_require_start0(const uint64_t* step_start, uint32_t nblk) {
  if (nblk && step_start[0] != 0) throw PlanError{"step_start[0] must be 0"};
}

// everything of the shape that follows from log2(n) alone (not the rank's
// chunks and blocks, which need the block boundaries: plan_shape)
inline ShapePlan shape_of_logn(uint32_t tau, uint32_t nblk, int logn, int rank, int logP, bool sharded) {
  if (logn + BLOWUP_LOG2 > FS_MAX_BETAS) throw PlanError{"LDE domain too large for the challenge record"};
  ShapePlan s;
  s.tau = tau;
  s.nblk = nblk;
  s.logn = logn;
  s.n = 1ULL << logn;
  s.logN = s.logn + BLOWUP_LOG2;
  s.N = 1ULL << s.logN;
  s.ncols = 3 + 7 * (int)tau;
  s.logChunks = s.logn > COL_CHUNK_LOG2 ? s.logn - COL_CHUNK_LOG2 : 0;
  s.sharded = sharded;
  s.rank = rank;
  s.logP = logP;
  if (sharded && (s.logn < 12 + logP || logP > 3))
    throw PlanError{"sharded proving needs n >= 4096 * P rows and P <= 8 (n = " + std::to_string(s.n) +
                    ", P = " + std::to_string(1 << logP) + ")"};
  s.full_lde = sharded && logP == 1;
  s.M = s.N >> logP;
  s.logM = s.logN - logP;
  // tree workgroups of 2048 leaves (1024 on small per-device LDEs): alone a
  // 4096-leaf workgroup is as fast, but with proofs in flight the half-size
  // ones let the concurrent proofs' kernels interleave (+5% in flight, round 5,
  // profiles/r05/ab/tree_wg2048_headline_ab.txt)
  s.tree_wg_log = s.M <= (1ULL << 21) ? L16S_LOG : L16M_LOG;
  const int k = s.logN;
  s.rR = sharded ? k - L16_LOG - logP : (k >= L16_LOG ? k - L16_LOG : -1);
  return s;
}

// rows = step_start[nblk]: upload has checked every block's step range
// against its step_start difference before it plans
inline ShapePlan plan_shape(uint32_t tau, const uint64_t* step_start, uint32_t nblk, int rank, int logP,
                            bool sharded) {
  plan_require_start0(step_start, nblk);
  const uint64_t rows = nblk ? step_start[nblk] : 0;
  if (rows == 0 || (rows & (rows - 1)) != 0)
    throw PlanError{"n_base must be a power of two (got " + std::to_string(rows) + ")"};  // lde.rs:51
  if (rows > (1ULL << 28)) throw PlanError{"trace too long for one device (n > 2^28)"};
  ShapePlan s = shape_of_logn(tau, nblk, ilog2(rows), rank, logP, sharded);
  // sharded: this rank commits chunks [ch_lo, ch_hi) of every column
  shard_range(step_start, nblk, s.logn, sharded ? rank : 0, sharded ? logP : 0, s.ch_lo, s.ch_hi, s.blk_lo,
              s.blk_cnt);
  return s;
}

// ---------------------------------------------------------------- columns
static const char* const KIND_NAME[7] = {"mv", "wflag", "wsym", "head", "winlen", "in_off", "out_off"};

inline std::string label_of(int c, uint32_t tau) {  // all_labels (openings.rs:89-116)
  if (c == 0) return "input_mv";
  if (c == 1) return "is_first";
  if (c == 2) return "is_last";
  return std::string(KIND_NAME[(c - 3) / tau]) + "_" + std::to_string((c - 3) % tau);
}

inline ColTemplate make_template(int c, uint32_t tau, const std::string& label) {
  ColTemplate t{};
  uint8_t b[64] = {0};
  memcpy(b, "col_leaf", 8);
  const uint32_t L = (uint32_t)label.size();
  for (int i = 0; i < 4; i++) b[8 + i] = (uint8_t)(L >> (8 * i));
  memcpy(b + 12, label.data(), L);
  for (int i = 0; i < 16; i++)
    t.words[i] = (uint32_t)b[4 * i] | (uint32_t)b[4 * i + 1] << 8 | (uint32_t)b[4 * i + 2] << 16 |
                 (uint32_t)b[4 * i + 3] << 24;
  t.off = 12 + L;
  t.block_len = 20 + L;
  if (c < 3) { t.kind = c; t.tape = 0; }
  else { t.kind = 3 + (c - 3) / tau; t.tape = (c - 3) % tau; }
  return t;
}

struct ColumnPlan {
  std::vector<std::string> labels;
  std::vector<ColTemplate> tmpl;    // tab / tab_log set: node offsets into the table buffer
  uint64_t tab_nodes = 0;           // leaf tables + uniform-subtree tables
  uint64_t tab_units = 0;           // most entries of one table
  std::vector<uint32_t> tab_cols;   // columns with a table
  std::vector<uint32_t> pw_cols;    // piecewise-constant columns
  std::vector<uint32_t> pw_chunks;  // this rank's chunks committed by the piecewise kernel
  std::vector<uint8_t> dense_chunk; // per chunk: this rank commits it densely for every column
  std::vector<uint32_t> work;       // dense (column, chunk) pairs
  std::vector<DictCol> dcols;       // dense small-range columns (dictionary commitment)
  std::vector<uint32_t> dict_of;    // column -> dictionary index or NO_DICT
};

// use_dict: the caller's SEZKP_NO_DICT switch; the dictionary also needs whole chunks
inline ColumnPlan plan_columns(const ShapePlan& s, const uint64_t* step_start, bool use_dict_wanted) {
  ColumnPlan p;
  const uint32_t tau = s.tau, nblk = s.nblk;
  const uint64_t n = s.n;
  const int ncols = s.ncols;
  // ---- column templates + outer trees (all levels kept)
  for (int c = 0; c < ncols; c++) {
    p.labels.push_back(label_of(c, tau));
    if (p.labels.back().size() > 44) throw PlanError{"column label too long"};
    p.tmpl.push_back(make_template(c, tau, p.labels.back()));
  }
  // per-column tables: leaf tables for small raw domains (i8/u8: 256, u16:
  // 65536 entries) and uniform-subtree tables U_0..U_10 for piecewise columns
  const bool use_dict = n >= (1ULL << COL_CHUNK_LOG2) && use_dict_wanted;
  for (int c = 0; c < ncols; c++) {
    ColTemplate& t = p.tmpl[c];
    t.tab = NO_TAB;
    t.tab_log = 0;
    if (use_dict && kind_dict(t.kind)) {
      p.dcols.push_back(DictCol{(uint32_t)c, NO_DICT, (uint64_t)p.dcols.size() * DICT_LEVELS * DICT_CAP});
    } else if (kind_has_leaf_table(t.kind)) {
      t.tab_log = t.kind == 5 ? 16 : 8;
      t.tab = p.tab_nodes;
      p.tab_nodes += 1ULL << t.tab_log;
      p.tab_units = std::max<uint64_t>(p.tab_units, 1ULL << t.tab_log);
      p.tab_cols.push_back(c);
    } else if (kind_piecewise(t.kind)) {
      const uint64_t units = (t.kind == 1 || t.kind == 2) ? 2 : nblk;
      t.tab = p.tab_nodes;
      p.tab_nodes += units * U_LEVELS;
      p.tab_units = std::max<uint64_t>(p.tab_units, units);
      p.tab_cols.push_back(c);
      p.pw_cols.push_back(c);
    }
  }
  // chunks whose rows cross few block boundaries go to the piecewise kernel;
  // the rest (many short blocks) are committed densely for every column
  const uint64_t nchunks = 1ULL << s.logChunks, chunk_rows = n < 1024 ? n : 1024;
  p.dense_chunk.assign(nchunks, 0);
  {
    uint32_t k = 0;
    for (uint64_t ch = 0; ch < nchunks; ch++) {
      const uint64_t c0 = ch * chunk_rows, c1 = c0 + chunk_rows;
      while (k < nblk && step_start[k] <= c0) k++;
      int inside = 0;
      for (uint32_t j = k; j < nblk && step_start[j] < c1; j++)
        if (j == 0 || step_start[j] != step_start[j - 1]) inside++;
      if (ch < s.ch_lo || ch >= s.ch_hi) continue;
      if (inside <= 16) p.pw_chunks.push_back((uint32_t)ch);
      else p.dense_chunk[ch] = 1;
    }
  }
  for (int c = 0; c < ncols; c++) {
    if (use_dict && kind_dict(p.tmpl[c].kind)) continue;
    const bool pw = kind_piecewise(p.tmpl[c].kind);
    for (uint64_t ch = s.ch_lo; ch < s.ch_hi; ch++)
      if (!pw || p.dense_chunk[ch]) { p.work.push_back((uint32_t)c); p.work.push_back((uint32_t)ch); }
  }
  for (DictCol& h : p.dcols)  // head columns: the same tape's mv column (delta plan)
    if (p.tmpl[h.col].kind == 6)
      for (size_t i = 0; i < p.dcols.size(); i++)
        if (p.tmpl[p.dcols[i].col].kind == 3 && p.tmpl[p.dcols[i].col].tape == p.tmpl[h.col].tape) h.mv = (uint32_t)i;
  p.dict_of.assign(ncols, NO_DICT);
  for (size_t i = 0; i < p.dcols.size(); i++) p.dict_of[p.dcols[i].col] = (uint32_t)i;
  return p;
}

// ---------------------------------------------------------- FRI workspace
// Layer r has 2^(k-r) leaves. Run layers (r <= rR, >= 4096 P leaves) are held
// as this rank's runs of 4096 (all of it when P = 1); the remaining small
// layers are replicated on every rank. Values live in one of three buffers
// (layer 0 is the local LDE), every tree node in one node buffer, every root
// in a table of k + 2 slots (slot k + 1: the dummy that a sharded run tree's
// local root goes to).
enum FriBuf { FRI_BUF_LDE = 0, FRI_BUF_FRI = 1, FRI_BUF_REP = 2 };
struct FriLayerPlan {
  bool run = false;
  int buf = FRI_BUF_LDE;       // where the layer's values live
  uint64_t val_off = 0;        // values into that buffer
  uint64_t val_len = 0;        // values this rank holds
  uint64_t node_off = 0;       // local tree: first node in the node buffer
  int logLen = 0, lstore = LSTORE_FRI;
  int root_slot = 0;
  // sharded run layers: the cap (levels >= 12, global indices) and the
  // allgathered run roots behind it; otherwise the cap is the local tree
  bool has_cap = false;
  uint64_t cap_off = 0;
  int cap_logLen = 0, cap_lstore = LSTORE_FRI, cap_root_slot = 0;
  uint64_t gather_off = 0, gather_nodes = 0;
};
struct ForestEntryPlan {
  int layer;
  uint32_t wg_start;  // first WG of this layer in the forest launch
  uint32_t stop;      // level the WG reduces to (launch_layer16)
};
// a pass of upper jobs: jobs [first, first + count) of FriPlan::jobs, one launch
typedef std::pair<size_t, int> JobRange;
struct FriPlan {
  int k = 0;
  std::vector<FriLayerPlan> layers;  // k + 1
  uint64_t lde_vals = 0, run_vals = 0, rep_vals = 0, total_nodes = 0;
  int root_slots = 0;                // k + 2
  std::vector<int> rep16;            // replicated layers with >= 4096 leaves (P > 1)
  int tail_first = 1;                // first layer of the small-layer tail kernel
  std::vector<ForestEntryPlan> forest;
  uint32_t forest_wgs = 0;
  bool tailbuf = false;              // single device: fold-replay scratch of the small-layer workgroups
  // upper-level passes. A job's tree carries logLen / lstore only: its
  // pointers are bound from job_layer / job_cap (the layer's cap or local
  // tree), and a non-null gath stands for that layer's gathered run roots
  std::vector<UpperJob> jobs;
  std::vector<int> job_layer;
  std::vector<uint8_t> job_cap;
  std::vector<JobRange> jobs0, jobsF;    // layer 0, then all fold layers
  std::vector<JobRange> jobsL0, jobsLR;  // sharded, 1024-leaf WGs: run trees' levels 11..12
};

inline FriPlan plan_fri(const ShapePlan& s) {
  FriPlan f;
  const int k = s.logN, rR = s.rR, logP = s.logP;
  const uint64_t N = s.N, S = 1ULL << L16_LOG;
  const bool sharded = s.sharded;
  f.k = k;
  f.lde_vals = s.M;
  f.root_slots = k + 2;
  f.rep_vals = sharded ? (S << logP) : 0;  // sharded: first the whole layer rR
  for (int r = 1; r <= k; r++) {
    if (r <= rR) f.run_vals += (N >> r) >> logP;
    else f.rep_vals += N >> r;
  }
  for (int r = 0; r <= k; r++) {
    const int ll = r <= rR ? k - r - logP : k - r;
    f.total_nodes += tree_stored_nodes(ll, LSTORE_FRI);
    if (sharded && r <= rR) f.total_nodes += tree_stored_nodes(k - r, L16_LOG) + ((N >> r) >> L16_LOG);
  }
  uint64_t off = 0, voff = 0, roff = sharded ? (S << logP) : 0;
  f.layers.assign(k + 1, FriLayerPlan{});
  for (int r = 0; r <= k; r++) {
    FriLayerPlan& L = f.layers[r];
    L.run = r <= rR;
    L.val_len = L.run ? (N >> r) >> logP : N >> r;
    if (r == 0) { L.buf = FRI_BUF_LDE; L.val_off = 0; }
    else if (L.run) { L.buf = FRI_BUF_FRI; L.val_off = voff; voff += L.val_len; }
    else { L.buf = FRI_BUF_REP; L.val_off = roff; roff += L.val_len; }
    L.node_off = off;
    L.logLen = L.run ? k - r - logP : k - r;
    L.lstore = LSTORE_FRI;
    L.root_slot = (L.run && sharded) ? k + 1 : r;
    off += tree_stored_nodes(L.logLen, LSTORE_FRI);
    if (L.run && sharded) {
      L.has_cap = true;
      L.cap_off = off;
      L.cap_logLen = k - r;
      L.cap_lstore = L16_LOG;
      L.cap_root_slot = r;
      off += tree_stored_nodes(k - r, L16_LOG);
      L.gather_off = off;
      L.gather_nodes = (N >> r) >> L16_LOG;
      off += L.gather_nodes;
    } else {
      L.cap_off = L.node_off;
      L.cap_logLen = L.logLen;
      L.cap_lstore = L.lstore;
      L.cap_root_slot = L.root_slot;
    }
  }
  // replicated layers of >= 4096 leaves (P > 1), then the small-layer tail
  f.tail_first = rR + 1 > 1 ? rR + 1 : 1;
  while (f.tail_first <= k && k - f.tail_first >= L16_LOG) f.rep16.push_back(f.tail_first++);
  // forest of the run layers 1..rR (local runs of 4096 leaves per WG) and,
  // sharded, of the replicated layers of >= 4096 leaves (whole subtrees of
  // 4096, level 12 and up from the upper jobs): their WGs run beside the run
  // layers' instead of as three serial few-WG launches after them, and come
  // first in the grid (each is one WG's 4096-leaf chain: started last, they
  // would set the launch's end)
  {
    uint32_t wgs = 0;
    for (int r : f.rep16) {
      f.forest.push_back(ForestEntryPlan{r, wgs, (uint32_t)std::min(L16_LOG, s.tree_wg_log)});
      wgs += (uint32_t)(1ULL << (f.layers[r].logLen - s.tree_wg_log));
    }
    for (int r = 1; r <= rR; r++) {
      f.forest.push_back(ForestEntryPlan{r, wgs, (uint32_t)s.wg_stop()});
      wgs += (uint32_t)(1ULL << (f.layers[r].logLen - s.tree_wg_log));
    }
    f.forest_wgs = wgs;
    f.tailbuf = !sharded;
  }
  // upper levels (> 12): layer 0's cap, then every other cap / replicated tree
  {
    static const uint32_t gath_mark = 0;  // stands for "this layer's gathered run roots"
    std::vector<std::vector<UpperJob>> p0, pF, pL0, pLR;
    auto tree_of = [&](int r, bool cap) {
      const FriLayerPlan& L = f.layers[r];
      return TreeDev{nullptr, nullptr, cap ? L.cap_logLen : L.logLen, cap ? L.cap_lstore : L.lstore};
    };
    // plan_upper_jobs appends to the passes: note which tree the new jobs reduce
    std::vector<std::vector<std::pair<int, uint8_t>>> t0, tF, tL0, tLR;
    auto plan = [&](std::vector<std::vector<UpperJob>>& ps, std::vector<std::vector<std::pair<int, uint8_t>>>& ts,
                    int r, bool cap, int from, int to, const uint32_t* gath, uint64_t nrun) {
      plan_upper_jobs(tree_of(r, cap), from, ps, to, gath, nrun, logP);
      ts.resize(ps.size());
      for (size_t i = 0; i < ps.size(); i++) ts[i].resize(ps[i].size(), {r, (uint8_t)cap});
    };
    // run layers start from the level their layer16 WGs stopped at
    const int from = s.tree_stop();
    // sharded: a run layer's cap starts from its allgathered run roots (the
    // first pass permutes them into cap order itself: no scatter launch)
    auto gath_of = [&](int r) -> const uint32_t* { return sharded && r <= rR ? &gath_mark : nullptr; };
    auto nrun_of = [&](int r) -> uint64_t { return sharded ? (N >> r) >> (L16_LOG + logP) : 0; };
    if (rR >= 0 && (f.layers[0].cap_logLen > from || gath_of(0))) plan(p0, t0, 0, true, from, 0, gath_of(0), nrun_of(0));
    const int rep_from = std::min(L16_LOG, s.tree_wg_log);
    for (int r = 1; r <= k; r++) {
      const bool runl = r <= rR;
      if ((runl || std::find(f.rep16.begin(), f.rep16.end(), r) != f.rep16.end()) &&
          (f.layers[r].cap_logLen > (runl ? from : rep_from) || (runl && gath_of(r))))
        plan(pF, tF, r, true, runl ? from : rep_from, 0, runl ? gath_of(r) : nullptr, nrun_of(r));
    }
    // sharded with 1024-leaf WGs: the run trees' levels 11..12 (the run roots
    // the caps are gathered from) by upper jobs before each allgather
    if (sharded && s.wg_stop() < L16_LOG && rR >= 0) {
      plan(pL0, tL0, 0, false, s.wg_stop(), L16_LOG, nullptr, 0);
      for (int r = 1; r <= rR; r++) plan(pLR, tLR, r, false, s.wg_stop(), L16_LOG, nullptr, 0);
    }
    auto add = [&](std::vector<std::vector<UpperJob>>& ps, std::vector<std::vector<std::pair<int, uint8_t>>>& ts,
                   std::vector<JobRange>& out) {
      for (size_t i = 0; i < ps.size(); i++) {
        out.push_back({f.jobs.size(), (int)ps[i].size()});
        f.jobs.insert(f.jobs.end(), ps[i].begin(), ps[i].end());
        for (auto& t : ts[i]) { f.job_layer.push_back(t.first); f.job_cap.push_back(t.second); }
      }
    };
    add(p0, t0, f.jobs0);
    add(pF, tF, f.jobsF);
    add(pL0, tL0, f.jobsL0);
    add(pLR, tLR, f.jobsLR);
  }
  return f;
}

// ------------------------------------------------------------ proof layout
// (proof.rs:80-98, bincode fixint LE): the header bytes (domain_n, tau, the
// labelled column roots, zero until the proof fills them) and the body's
// layout (ProofLayout::base is the caller's to bind)
struct ProofPlan {
  std::vector<uint8_t> header;
  std::vector<size_t> root_pos;  // byte offset of each column root in the header
  size_t hdr_bytes = 0;
  ProofLayout PL{};
  size_t max_fri_req = 0, max_open_req = 0;
};

inline ProofPlan plan_proof(const ShapePlan& s, const std::vector<std::string>& labels) {
  ProofPlan p;
  const int k = s.logN;
  const uint32_t tau = s.tau;
  auto u64 = [&](uint64_t x) {
    for (int i = 0; i < 8; i++) p.header.push_back((uint8_t)(x >> (8 * i)));
  };
  u64(s.N);
  u64(tau);
  u64((uint64_t)s.ncols);
  p.root_pos.assign(s.ncols, 0);
  for (int c = 0; c < s.ncols; c++) {
    u64(labels[c].size());
    p.header.insert(p.header.end(), labels[c].begin(), labels[c].end());
    p.root_pos[c] = p.header.size();
    p.header.insert(p.header.end(), 32, 0);
  }
  p.hdr_bytes = p.header.size();
  ProofLayout& PL = p.PL;
  PL.open_per_q = 9 * tau + 3;
  PL.nq = NUM_QUERIES;
  PL.k = k;
  PL.tau = tau;
  PL.open_bytes = 80 + 32 * (uint64_t)s.logn;  // path_in_chunk + path_to_chunk = log2(n) levels
  PL.q_bytes = 16 + PL.open_per_q * PL.open_bytes;
  PL.fr_off = 8 + NUM_QUERIES * PL.q_bytes;
  PL.fq_off = PL.fr_off + 8 + 32 * (uint64_t)(k + 1);
  PL.fq_bytes = 8 + 8 * (uint64_t)(k + 1) + 8;
  for (int r = 0; r < k; r++) PL.fq_bytes += 2 * (16 + 32 * (uint64_t)(k - r));
  PL.tail_off = PL.fq_off + 8 + NUM_QUERIES * PL.fq_bytes;
  PL.total = PL.tail_off + 8 + 32;
  p.max_fri_req = (size_t)NUM_QUERIES * 2 * k;
  p.max_open_req = (size_t)NUM_QUERIES * (3 + 9 * tau);
  return p;
}

// ------------------------------------------------------------ status words
// The one small D2H copy of a proof's first phase, in u32 WORD offsets from
// the column roots: the roots, the 16 guard words ([0] this rank's guard,
// [8 + r] rank r's when sharded; on a single device the eight words at +8
// hold a trace image's manifest root), then the dictionary cache's status
// words (k_dict_plan), one word per column for the piecewise tables' form
// (k_col_tables), the wide head ladder's status words and, for a sharded
// trace image, its manifest root. The allocation, the
// device pointers, the host buffer, the copy and its parse all read this.
constexpr int GUARD_WORDS = 16;
struct StatusLayout {
  size_t roots = 0;       // 8 words per column
  size_t guard = 0;       // GUARD_WORDS
  size_t trace_root = 0;  // guard + 8
  size_t dict = 0;        // 2 words per dictionary column: rebuilt, entries
  size_t pw = 0;          // 1 word per column
  size_t hw = 0;          // HW_STAT_WORDS per dictionary column
  // a sharded trace image only: the manifest root, eight words appended (the
  // eight at trace_root are the ranks' guard words there); else = total
  size_t shard_root = 0;
  size_t total = 0;
};
inline StatusLayout plan_status(int ncols, int n_dict, bool shard_root = false) {
  StatusLayout s;
  s.roots = 0;
  s.guard = s.roots + 8 * (size_t)ncols;
  s.trace_root = s.guard + 8;
  s.dict = s.guard + GUARD_WORDS;
  s.pw = s.dict + 2 * (size_t)n_dict;
  s.hw = s.pw + (size_t)ncols;
  s.shard_root = s.hw + (size_t)HW_STAT_WORDS * (size_t)n_dict;
  s.total = s.shard_root + (shard_root ? 8 : 0);
  return s;
}

// ------------------------------------------------------ wide head ladder
// The host side of the persistent 8-row head tables (HeadWideDev,
// sezkp_internal.h): per head column, when the ladder is built, kept,
// re-spanned and dropped. The entry of (first head, 7 moves) depends on the
// column's label and on those values only, so the ladder is keyed by value
// over a span [olo, olo + span) of heads and a range [dmin, dmin + dR) of
// moves, and lives as long as the dictionary epoch does.
//  - The first proof of an epoch builds nothing: a one-shot proof would hash
//    span dR^7 entries to save fewer compressions.
//  - From the second proof on the span is the last completed proof's head
//    range widened by HEAD_WIDE_MARGIN values on each side (head ranges of
//    one machine shape move by a few values from trace to trace; a walk of
//    512 steps moves its extremes by less than 8 in most redraws, and a group
//    outside the span only takes the 4-row path), while span dR^7 <= cap.
//  - A proof whose groups left the span in more than 1 / HEAD_WIDE_RESPAN of
//    all groups re-spans the ladder at the next proof: to the union of the
//    old span and the new range when that fits the cap (so two alternating
//    traces settle after one rebuild), else to the new range alone.
constexpr uint32_t HEAD_WIDE_CAP_DEFAULT = 1u << 19;  // L3 entries per column (SEZKP_HEAD_WIDE_CAP)
constexpr uint32_t HEAD_WIDE_CAP_MAX = 1u << 24;      // the commit indexes L3 in 32 bits
constexpr int64_t HEAD_WIDE_MARGIN = 8;
constexpr uint64_t HEAD_WIDE_RESPAN = 64;

// what a completed proof reports of one head column (the status words)
struct HeadWideObs {
  int64_t lo = 0, hi = -1;    // head range on this device's rows
  int64_t mlo = 0, mhi = -1;  // its tape's move range
  uint32_t delta = 0;         // the column's plan is a delta plan
  uint32_t wide = 0, fb_start = 0, fb_span = 0;  // 8-row groups: from L3, fallen back at a block start, outside the span
};
struct HeadWideCol {
  uint64_t epoch = 0;  // epoch of the ladder in place (0: none)
  int64_t olo = 0, dmin = 0;
  uint32_t span = 0, dR = 0;
  uint64_t seen_epoch = 0;  // epoch of `seen`
  HeadWideObs seen;
  bool respan = false;
};
struct HeadWideDecision {
  bool use = false;    // the commit reads the ladder
  bool build = false;  // ... after this proof has built it
  uint64_t l3_entries = 0, low_entries = 0;  // of the ladder in place or to build
};
// entries of L3 and of the lower levels L0 | L1 | L2 over the widened value range
inline bool head_wide_sizes(uint64_t span, uint64_t dR, int64_t dmin, uint64_t cap, uint64_t& l3, uint64_t& low) {
  if (span == 0 || dR == 0 || dR > 256) return false;
  uint64_t p7 = 1;
  for (int i = 0; i < 7; i++) p7 *= dR;  // <= 2^56
  if (cap > HEAD_WIDE_CAP_MAX) cap = HEAD_WIDE_CAP_MAX;
  if (p7 > cap || span > cap / p7) return false;
  const int64_t dmax = dmin + (int64_t)dR - 1;
  const int64_t neg = dmin < 0 ? dmin : 0, pos = dmax > 0 ? dmax : 0;
  const uint64_t sw = span + 7 * (uint64_t)(pos - neg);
  l3 = span * p7;
  low = sw * (1 + dR + dR * dR * dR);
  return true;
}
inline HeadWideDecision head_wide_decide(HeadWideCol& c, uint64_t epoch, uint64_t cap) {
  HeadWideDecision d;
  if (c.epoch == epoch && !c.respan) {  // in place
    d.use = head_wide_sizes(c.span, c.dR, c.dmin, cap, d.l3_entries, d.low_entries);
    if (!d.use) c.epoch = 0;  // the cap was lowered: the ladder is dropped
    return d;
  }
  const HeadWideObs& s = c.seen;
  if (c.seen_epoch != epoch || !s.delta || s.lo > s.hi || s.mlo > s.mhi) {
    if (c.epoch != epoch) c.epoch = 0;
    return d;
  }
  int64_t lo = s.lo - HEAD_WIDE_MARGIN, hi = s.hi + HEAD_WIDE_MARGIN, mlo = s.mlo, mhi = s.mhi;
  if (c.epoch == epoch) {  // a re-span: the union with the old span, if that qualifies
    const int64_t ulo = std::min(lo, c.olo), uhi = std::max(hi, c.olo + (int64_t)c.span - 1);
    const int64_t umlo = std::min(mlo, c.dmin), umhi = std::max(mhi, c.dmin + (int64_t)c.dR - 1);
    uint64_t a, b;
    if (head_wide_sizes((uint64_t)(uhi - ulo) + 1, (uint64_t)(umhi - umlo) + 1, umlo, cap, a, b)) {
      lo = ulo; hi = uhi; mlo = umlo; mhi = umhi;
    }
  }
  c.respan = false;
  c.epoch = 0;
  if (!head_wide_sizes((uint64_t)(hi - lo) + 1, (uint64_t)(mhi - mlo) + 1, mlo, cap, d.l3_entries, d.low_entries))
    return d;
  c.epoch = epoch;
  c.olo = lo;
  c.span = (uint32_t)(hi - lo + 1);
  c.dmin = mlo;
  c.dR = (uint32_t)(mhi - mlo + 1);
  d.use = d.build = true;
  return d;
}
// after a proof of `epoch` has completed
inline void head_wide_observe(HeadWideCol& c, uint64_t epoch, const HeadWideObs& o) {
  c.seen_epoch = epoch;
  c.seen = o;
  const uint64_t groups = (uint64_t)o.wide + o.fb_start + o.fb_span;
  if (c.epoch == epoch && o.delta && (uint64_t)o.fb_span * HEAD_WIDE_RESPAN > groups) c.respan = true;
}

}  // namespace sezkp
