// dict_commit.hip — the dictionary commitment of the dense columns for CDNA4
// (gfx950): per-column ranges and plans, the table levels T_0..T_K, the
// gathered chunk commitment and the wide head ladder. The scheme is described
// in dict_nodes.h, which also holds the node providers that the openings
// (col_open.hip) share with k_col_commit_dict.
#include "dev_common.h"
#include "col_dev.h"
#include "dict_nodes.h"
#include "sezkp_internal.h"

namespace sezkp {

constexpr int DICT_WG_ROWS = 64 << DICT_LANE_LOG;  // 4096: row0 / nrows alignment of a sliced commit
constexpr int DICT_RANGE_STEP = TR_THREADS * 16;                     // rows per WG sweep

// CNT keys of 1 or 2 bytes (a multiple of 16 bytes, 16-byte aligned) as
// 16-byte loads: k_dict_range's sweep
template <typename Key, int CNT>
__device__ __forceinline__ void load_keys(const Key* __restrict__ p, int64_t (&k)[CNT]) {
  constexpr int BYTES = CNT * (int)sizeof(Key);
  static_assert(BYTES % 16 == 0 && sizeof(Key) <= 2, "whole 16-byte words of narrow keys");
  constexpr int PER = 16 / (int)sizeof(Key);
#pragma unroll
  for (int q = 0; q < BYTES / 16; q++) {
    const uint4 w = reinterpret_cast<const uint4*>(p)[q];
    const uint32_t ww[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
    for (int i = 0; i < PER; i++) {
      const int bit = i * 8 * (int)sizeof(Key);
      const uint32_t raw = (ww[bit / 32] >> (bit % 32)) & ((1u << (8 * sizeof(Key))) - 1u);
      k[q * PER + i] = (int64_t)(Key)raw;
    }
  }
}

// WG-wide min / max of one column's partial ranges (result valid on tid 0)
__device__ __forceinline__ void reduce_parts(const int64_t* pp, uint32_t nparts, int64_t& lo, int64_t& hi,
                                             int64_t* slo, int64_t* shi) {
  const int tid = threadIdx.x;
  lo = INT64_MAX;
  hi = INT64_MIN;
  for (uint32_t i = tid; i < nparts; i += TR_THREADS) {
    lo = pp[2 * i] < lo ? pp[2 * i] : lo;
    hi = pp[2 * i + 1] > hi ? pp[2 * i + 1] : hi;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const int64_t a = __shfl_xor(lo, o, 64), b = __shfl_xor(hi, o, 64);
    lo = a < lo ? a : lo;
    hi = b > hi ? b : hi;
  }
  if ((tid & 63) == 0) { slo[tid >> 6] = lo; shi[tid >> 6] = hi; }
  __syncthreads();
  for (int w = 0; w < TR_THREADS / 64; w++) {
    lo = slo[w] < lo ? slo[w] : lo;
    hi = shi[w] > hi ? shi[w] : hi;
  }
  __syncthreads();
}

// Table level K by cost: table entries + n / 2^K gathered nodes (one hash
// each). Pricing gathers from tables of > 1 MB higher (they miss the reading
// XCD's L2) was measured slower in round 3: the extra compressions of the
// lower levels cost more than the misses save. (lo, hi): the column's range;
// (mlo, mhi): its tape's move range (head columns, has_mv), for the delta plan.
__device__ __forceinline__ DictPlan make_plan(int64_t lo, int64_t hi, bool has_mv, int64_t mlo, int64_t mhi,
                                              uint64_t n, uint64_t nrows, uint32_t tab_cap) {
  DictPlan P{};
  P.min = lo;
  P.K = -1;
  const uint64_t R = hi >= lo ? (uint64_t)hi - (uint64_t)lo + 1 : 1;
  if (R <= DICT_CAP) {
    P.R = (uint32_t)R;
    // cost of level K: the tables' entries + the nodes this device gathers
    // (nrows, not n: a sharded rank builds the same tables for 1/P of the rows)
    uint64_t best = 2 * nrows, tabcost = 0, sz = R;  // K = -1: nrows leaves + parents
    bool open = true;
    // unrolled: constant pw[] indices keep P in registers (a runtime index put
    // it in scratch memory, and the kernel took ~23 us for 33 tiny workgroups)
#pragma unroll
    for (int k = 0; k < DICT_LEVELS; k++) {
      open = open && (1ULL << k) <= n && sz <= (k ? tab_cap : DICT_CAP);
      if (open) {
        P.pw[k] = (uint32_t)sz;
        tabcost += sz;
        const uint64_t cost = tabcost + (nrows >> k);
        if (cost < best) { best = cost; P.K = k; }
        sz = sz * sz;
      }
    }
#pragma unroll
    for (int k = 0; k < DICT_LEVELS; k++)
      if (k > P.K) P.pw[k] = 0;
    // head delta plan (see DictPlan): 4-row groups from (head, 3 moves)
    const uint64_t dR = mhi >= mlo ? (uint64_t)mhi - (uint64_t)mlo + 1 : 0;
    if (has_mv && P.K <= 1 && n >= 4 && dR && R * R <= tab_cap && dR <= 256 && R * dR * dR * dR <= tab_cap) {
      P.K = 2;
      P.delta = 1;
      P.dmin = mlo;
      P.dR = (uint32_t)dR;
      P.pw[0] = (uint32_t)R;
      P.pw[1] = (uint32_t)(R * R);
      P.pw[2] = (uint32_t)(R * dR * dR * dR);
      for (int k = 3; k < DICT_LEVELS; k++) P.pw[k] = 0;
    }
  }
  // a lane's rows: 2^(6 + a), a = dict_extra(K) lowered one step per halving
  // of the device's rows below 2^22, so the commit has waves enough to fill
  // the chip (one wave per 64-lane WG, 4 per SIMD) on every shape: at 2^21
  // rows the K >= 3 columns take 128 rows per lane, the K = 2 ones 64
  // (round 5: k_col_commit_dict 314 -> 291 us per launch; a second step
  // 306 us, profiles/r05/ab/dict_rows_per_lane_ab{1,2}.txt)
  int a = dict_extra(P.K);
  for (uint64_t r = nrows; r < (1ULL << 22) && a > 0; r <<= 1) a--;
  P.a = (uint32_t)a;
  return P;
}

// per-(column, part) min / max of the raw integers: `sweeps` (1..8) sweeps of
// 16 rows per lane (one 16-byte-or-less load each); parts of 32768 rows keep
// the grid at ~2K workgroups for 2^21 rows, and a device with fewer rows (a
// sharded rank) takes smaller parts, so every column still has ~64 of them
__global__ void __launch_bounds__(TR_THREADS) k_dict_range(TraceDev T, const ColTemplate* __restrict__ tmpl,
                                                           const DictCol* __restrict__ dcols,
                                                           int64_t* __restrict__ part, uint32_t nparts,
                                                           uint64_t row0, uint64_t row_end, int sweeps) {
  __shared__ int64_t slo[TR_THREADS / 64], shi[TR_THREADS / 64];
  const ColTemplate ct = tmpl[dcols[blockIdx.y].col];
  const int tid = threadIdx.x;
  int64_t lo = INT64_MAX, hi = INT64_MIN;
  if (ct.kind == 6) {  // head: the per-block ranges of k_expand over the blocks meeting this part
    const uint64_t prow = (uint64_t)sweeps * DICT_RANGE_STEP;
    const uint64_t p0 = row0 + (uint64_t)blockIdx.x * prow;
    const uint64_t p1 = p0 + prow < row_end ? p0 + prow : row_end;
    const int64_t* hr = T.head_rng + 2 * ((uint64_t)ct.tape * T.nblk);
    for (uint32_t b = T.row_blk[p0] + tid; b <= T.row_blk[p1 - 1]; b += TR_THREADS) {
      lo = hr[2 * b] < lo ? hr[2 * b] : lo;
      hi = hr[2 * b + 1] > hi ? hr[2 * b + 1] : hi;
    }
  } else {  // narrow keys: 32-bit min / max
    int32_t l32 = INT32_MAX, h32 = INT32_MIN;
    for (int sw = 0; sw < sweeps; sw++) {
      const uint64_t r0 = row0 + (uint64_t)blockIdx.x * ((uint64_t)sweeps * DICT_RANGE_STEP) + (uint64_t)sw * DICT_RANGE_STEP +
                          (uint64_t)tid * 16;
      if (r0 >= row_end) break;
      int64_t k[16];
      switch (ct.kind) {
        case 0: case 3: load_keys<int8_t, 16>(dict_keys<int8_t>(T, ct) + r0, k); break;
        case 4: load_keys<uint8_t, 16>(dict_keys<uint8_t>(T, ct) + r0, k); break;
        default: load_keys<uint16_t, 16>(dict_keys<uint16_t>(T, ct) + r0, k); break;
      }
#pragma unroll
      for (int i = 0; i < 16; i++) {
        l32 = min(l32, (int32_t)k[i]);
        h32 = max(h32, (int32_t)k[i]);
      }
    }
    if (l32 <= h32) {
      lo = l32;
      hi = h32;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const int64_t a = __shfl_xor(lo, o, 64), b = __shfl_xor(hi, o, 64);
    lo = a < lo ? a : lo;
    hi = b > hi ? b : hi;
  }
  if ((tid & 63) == 0) { slo[tid >> 6] = lo; shi[tid >> 6] = hi; }
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < TR_THREADS / 64; w++) {
      lo = slo[w] < lo ? slo[w] : lo;
      hi = shi[w] > hi ? shi[w] : hi;
    }
    int64_t* o = part + 2 * ((uint64_t)blockIdx.y * nparts + blockIdx.x);
    o[0] = lo;
    o[1] = hi;
  }
}

// one WG per dictionary column: reduce the partial ranges (and, for a head
// column, its tape's move ranges) and choose the plan. (Folding this into
// k_dict_range's last workgroup through agent-scope completion counters was
// measured 100 us slower per proof in round 5: the release / acquire cache
// maintenance of ~2000 workgroups disturbs the L2s the commit then gathers from.)
// Then the reuse decision (DictCache): the column's tables T_0..T_K are a
// function of (lo, hi, mlo, mhi) and of the host-side inputs that `epoch`
// stands for, so a column whose stored key equals the new one keeps the tables
// the context already holds; any other column stores the new key and is
// rebuilt. A level some column rebuilds gets this proof's `seq` in its word.
__global__ void __launch_bounds__(TR_THREADS) k_dict_plan(const int64_t* __restrict__ part, uint32_t nparts,
                                                          uint64_t n, uint64_t nrows, const DictCol* __restrict__ dcols,
                                                          DictPlan* __restrict__ plans, uint32_t tab_cap, DictCache dc) {
  __shared__ int64_t slo[TR_THREADS / 64], shi[TR_THREADS / 64];
  int64_t lo, hi, mlo = 0, mhi = -1;
  reduce_parts(part + 2 * (uint64_t)blockIdx.x * nparts, nparts, lo, hi, slo, shi);
  const uint32_t mvc = dcols[blockIdx.x].mv;
  if (mvc != NO_DICT) reduce_parts(part + 2 * (uint64_t)mvc * nparts, nparts, mlo, mhi, slo, shi);
  if (threadIdx.x == 0) {
    const DictPlan P = make_plan(lo, hi, mvc != NO_DICT, mlo, mhi, n, nrows, tab_cap);
    plans[blockIdx.x] = P;
    DictKey* key = dc.keys + blockIdx.x;
    const DictKey old = *key;
    const bool same = old.lo == lo && old.hi == hi && old.mlo == mlo && old.mhi == mhi && old.epoch == dc.epoch;
    uint32_t entries = 0;
    if (!same) {
      *key = DictKey{lo, hi, mlo, mhi, dc.epoch};
#pragma unroll
      for (int k = 0; k < DICT_LEVELS; k++) {  // static indices only (pw is 0 above K)
        entries += P.pw[k];
        if (P.pw[k]) dc.lvl_seq[k] = dc.seq;  // every writer of one proof stores the same value
      }
    }
    dc.reuse[blockIdx.x] = same ? 1u : 0u;
    dc.status[2 * blockIdx.x] = same ? 0u : 1u;
    dc.status[2 * blockIdx.x + 1] = entries;
    // the host's inputs for the wide head ladder, and the commit's group counters zeroed
    uint32_t* hs = dc.hwstat + HW_STAT_WORDS * blockIdx.x;
    hs[0] = (uint32_t)(uint64_t)lo; hs[1] = (uint32_t)((uint64_t)lo >> 32);
    hs[2] = (uint32_t)(uint64_t)hi; hs[3] = (uint32_t)((uint64_t)hi >> 32);
    hs[4] = (uint32_t)(int32_t)mlo; hs[5] = (uint32_t)(int32_t)mhi;
    hs[6] = P.delta;
    hs[7] = hs[8] = hs[9] = 0;
  }
}

// entry e of table level `lvl` of one dictionary column
__device__ __forceinline__ void dict_entry(const ColTemplate& ct, const DictCol& dc, const DictPlan& P, uint32_t S,
                                           uint32_t* __restrict__ tabs, int lvl, uint32_t e) {
  uint32_t* tl = tabs + 8 * (dc.tab + (uint64_t)lvl * DICT_CAP);
  uint32_t h[8];
  if (lvl == 2 && P.delta) {  // TD: (head code, 3 move codes) -> H(T_1, T_1)
    const uint32_t* t1 = tl - 8 * (uint64_t)DICT_CAP;
    const int64_t R = P.R, dR = P.dR;
    int64_t c[4];
    c[0] = e % R;
    int64_t rest = e / R;
    bool ok = true;
#pragma unroll
    for (int j = 1; j < 4; j++) {
      c[j] = c[j - 1] + P.dmin + rest % dR;
      rest /= dR;
      ok = ok && c[j] >= 0 && c[j] < R;
    }
    if (!ok) return;  // not a reachable group: never read
    uint32_t a[8], b[8];
    node_load(t1 + 8 * (uint64_t)(c[0] + R * c[1]), a);
    node_load(t1 + 8 * (uint64_t)(c[2] + R * c[3]), b);
    b3_parent(a, b, h);
  } else if (lvl == 0) {
    leaf_labeled_rt(ct, gl_from_i64(P.min + (int64_t)e), h);
  } else {
    const uint32_t* tp = tl - 8 * (uint64_t)DICT_CAP;
    uint32_t a[8], b[8];
    node_load(tp + 8 * (uint64_t)(e % S), a);
    node_load(tp + 8 * (uint64_t)(e / S), b);
    b3_parent(a, b, h);
  }
  node_store(tl + 8 * (uint64_t)e, h);
}

// Table level `lvl` of every dictionary column in one flat index space: each
// WG sizes the level per column from the plans (prefix sums in LDS) and
// grid-strides over all (column, entry) pairs, so a few hundred WGs share the
// big levels evenly and the empty ones cost one plan scan. A reused column
// (k_dict_plan) counts 0 entries: its tables of the same key are in place. A
// rebuilt column rebuilds every level 0..K it reads, and the levels above a
// new, lower K (left from an earlier key) are never read. A level that no
// column rebuilds in this proof costs a workgroup one load.
constexpr int DICT_FLAT_MAX = 1024;  // columns one WG can index
constexpr int DICT_FLAT_WGS = 2048;  // 8 waves per SIMD for the big levels
__global__ void __launch_bounds__(TR_THREADS) k_dict_level(const ColTemplate* __restrict__ tmpl,
                                                           const DictCol* __restrict__ dcols,
                                                           const DictPlan* __restrict__ plans,
                                                           const uint32_t* __restrict__ reuse,
                                                           const uint64_t* __restrict__ lvl_seq, uint64_t seq,
                                                           uint32_t* __restrict__ tabs, int ndict, int lvl) {
  if (lvl_seq[lvl] != seq) return;  // nothing to build at this level (uniform per grid)
  // columns [0, ndict) of the arrays passed (the host offsets them per chunk)
  __shared__ uint32_t off[DICT_FLAT_MAX + 1];
  const int tid = threadIdx.x;
  for (int c = tid; c < ndict; c += TR_THREADS) {
    const DictPlan& P = plans[c];
    uint32_t size = 0;
#pragma unroll
    for (int k = 0; k < DICT_LEVELS; k++)  // static indices only (no scratch copy of P)
      if (k == lvl && lvl <= P.K) size = P.pw[k];
    off[c + 1] = reuse[c] ? 0 : size;
  }
  __syncthreads();
  if (tid == 0) {
    off[0] = 0;
    for (int c = 0; c < ndict; c++) off[c + 1] += off[c];
  }
  __syncthreads();
  const uint32_t total = off[ndict];
  for (uint32_t g = blockIdx.x * TR_THREADS + tid; g < total; g += gridDim.x * TR_THREADS) {
    int lo = 0, hi = ndict;  // column c with off[c] <= g < off[c + 1]
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if (off[mid] <= g) lo = mid;
      else hi = mid;
    }
    const DictPlan P = plans[lo];
    uint32_t S = 0;
#pragma unroll
    for (int k = 0; k + 1 < DICT_LEVELS; k++)
      if (k + 1 == lvl) S = P.pw[k];
    const DictCol dc = dcols[lo];
    dict_entry(tmpl[dc.col], dc, P, S, tabs, lvl, g - off[lo]);
  }
}

template <typename Key>
__device__ __forceinline__ void dict_lane(const Key* p, const DictPlan& P, const uint32_t* tab,
                                          const ColTemplate* ct, uint32_t (&h)[8]) {
  // a lane covers 2^(6 + a) rows: 2^(6+a-K) table nodes
  const uint32_t* tk = tab + 8 * (uint64_t)DICT_CAP * (P.K > 0 ? P.K : 0);
  switch (P.K * 4 + (int)P.a) {
    case 0 * 4 + 0: lane_tree_pf<6>(DictNodes<Key, 0>{p, tk, P.min, P.R}, h); break;
    case 1 * 4 + 0: lane_tree_pf<5>(DictNodes<Key, 1>{p, tk, P.min, P.R}, h); break;
    case 2 * 4 + 0: lane_tree_pf<4>(DictNodes<Key, 2>{p, tk, P.min, P.R}, h); break;
    case 2 * 4 + 1: lane_tree_pf<5>(DictNodes<Key, 2>{p, tk, P.min, P.R}, h); break;
    case 3 * 4 + 0: lane_tree_pf<3>(DictNodes<Key, 3>{p, tk, P.min, P.R}, h); break;
    case 3 * 4 + 1: lane_tree_pf<4>(DictNodes<Key, 3>{p, tk, P.min, P.R}, h); break;
    case 3 * 4 + 2: lane_tree_pf<5>(DictNodes<Key, 3>{p, tk, P.min, P.R}, h); break;
    case 4 * 4 + 0: lane_tree_pf<2>(DictNodes<Key, 4>{p, tk, P.min, P.R}, h); break;
    case 4 * 4 + 1: lane_tree_pf<3>(DictNodes<Key, 4>{p, tk, P.min, P.R}, h); break;
    case 4 * 4 + 2: lane_tree_pf<4>(DictNodes<Key, 4>{p, tk, P.min, P.R}, h); break;
    default: lane_tree<6>(RawLeaves<Key>{p, ct}, h); break;
  }
}

// 256-lane WG (4 waves) = 2^(llog + 8) rows of one dictionary column: each
// lane folds its 2^llog rows (llog = 6 + a) to one node in registers, and the
// levels llog+1..10 of the WG's chunks are computed from an LDS image by the
// first lanes of the WORKGROUP, so a level of 2^j parents keeps 2^j lanes of
// whole waves busy (128 parents: waves 0-1, the others wait at the barrier
// and leave their SIMD to other workgroups) instead of 32, 16, 8 of one
// wave's 64 lanes (round 5's one-wave workgroups: a third of a wave's issue
// slots at the upper levels went to idle lanes). Levels ping-pong between two
// LDS images: one barrier per level. The chunk roots are written as leaves of
// the column's outer tree. Requires n >= 1024; rows [row0, row_end) may end
// inside a workgroup (small sharded slices): lanes and parents past row_end
// are skipped (their LDS slots hold garbage that feeds only skipped parents).
// (__launch_bounds__(256, 5) for 5 waves per SIMD: 96 VGPRs with 97 spilled to
// scratch, 291-293 vs 280-284 us per launch, round 6: not kept)
constexpr int DICT_WG_LANES = 256;
__global__ void __launch_bounds__(DICT_WG_LANES) k_col_commit_dict(TraceDev T, const ColTemplate* __restrict__ tmpl,
                                                                   const DictCol* __restrict__ dcols,
                                                                   const DictPlan* __restrict__ plans,
                                                                   const uint32_t* __restrict__ tabs,
                                                                   uint32_t* __restrict__ outer, uint64_t outer_stride,
                                                                   uint64_t row0, uint64_t row_end,
                                                                   uint32_t* __restrict__ dlev,
                                                                   const HeadWideDev* __restrict__ hw,
                                                                   const uint32_t* __restrict__ hwtabs,
                                                                   uint64_t epoch, uint32_t* __restrict__ hwstat) {
  __shared__ uint32_t lds[2][8][DICT_WG_LANES];
  // (XCD-interleaved column orders, so that one XCD's workgroups gather
  // from one column's tables at a time, measured slower in rounds 1 and 3)
  const uint32_t by = blockIdx.y, bx = blockIdx.x;
  const DictCol dc = dcols[by];
  const ColTemplate* ctp = tmpl + dc.col;
  const ColTemplate ct = *ctp;
  const DictPlan P = plans[by];
  const uint32_t* tab = tabs + 8 * dc.tab;
  const int lane = threadIdx.x;
  // high-K columns give each lane more rows (fewer LDS levels per row)
  const int a = (int)P.a;
  const int llog = DICT_LANE_LOG + a;  // rows per lane (log2)
  const uint64_t wg_row = row0 + ((uint64_t)bx << (llog + 8));
  if (wg_row >= row_end) return;  // grid is sized for a = 0 (uniform per WG: no barrier is skipped by half a WG)
  const uint64_t lrow = wg_row + ((uint64_t)lane << llog);
  const uint64_t nch_all = T.n >> COL_CHUNK_LOG2;
  uint32_t* dl = dlev + 8 * (uint64_t)by * nch_all * DLEV_NODES;
  // the wide head ladder of this column, if it is this epoch's (uniform per workgroup)
  bool wide = false;
  uint32_t wcnt = 0;
  HeadWideDev W{};
  if (hw && ct.kind == 6 && P.delta) {
    W = hw[by];
    wide = W.epoch == epoch && W.span != 0;
  }
  if (lrow < row_end) {
    uint32_t h[8];
    switch (ct.kind) {
      case 0: case 3: dict_lane<int8_t>(dict_keys<int8_t>(T, ct) + lrow, P, tab, ctp, h); break;
      case 4: dict_lane<uint8_t>(dict_keys<uint8_t>(T, ct) + lrow, P, tab, ctp, h); break;
      case 5: dict_lane<uint16_t>(dict_keys<uint16_t>(T, ct) + lrow, P, tab, ctp, h); break;
      default:
        if (P.delta) {
          const uint64_t o = (uint64_t)ct.tape * T.n + lrow;
          const DeltaNodes dn{T.head + o, T.mv + o, T.row_flags + lrow, tab + 8 * (uint64_t)DICT_CAP,
                              tab + 16 * (uint64_t)DICT_CAP, P.min, P.dmin, P.R, P.dR};
          if (wide) {  // 8-row groups: 2^(3 + a) per lane
            const bool moves_in = P.dmin >= W.dmin && P.dmin + (int64_t)P.dR <= W.dmin + (int64_t)W.dR;
            const WideNodes wn{dn, hwtabs + 8 * W.l3, W.olo, (int32_t)W.dmin, moves_in ? W.span : 0u, W.dR, 0u};
            if (a == 1) lane_tree_pf<4>(wn, h);
            else lane_tree_pf<3>(wn, h);
            wcnt = wn.cnt;
          } else if (a == 1) lane_tree_pf<5>(dn, h);  // 4-row groups: 2^(4 + a) per lane
          else lane_tree_pf<4>(dn, h);
        } else {
          dict_lane<int32_t>(dict_keys<int32_t>(T, ct) + lrow, P, tab, ctp, h);
        }
        break;
    }
#pragma unroll
    for (int w = 0; w < 8; w++) lds[0][w][lane] = h[w];
    // chunk levels llog..9 are kept for the openings (DLEV_NODES per chunk)
    node_store(dl + 8 * ((lrow >> COL_CHUNK_LOG2) * DLEV_NODES + dlev_base(llog) +
                         ((lrow >> llog) & ((1u << (COL_CHUNK_LOG2 - llog)) - 1))),
               h);
  }
  if (wide) {  // the wave's group counts: one atomic per non-zero counter
    uint32_t p = (wcnt & 0x3ffu) | (((wcnt >> 10) & 0x3ffu) << 16), q = wcnt >> 20;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      p += __shfl_xor(p, o, 64);
      q += __shfl_xor(q, o, 64);
    }
    if ((lane & 63) == 0) {
      uint32_t* hs = hwstat + HW_STAT_WORDS * by;
      if (p & 0xffffu) atomicAdd(hs + 7, p & 0xffffu);
      if (p >> 16) atomicAdd(hs + 8, p >> 16);
      if (q) atomicAdd(hs + 9, q);
    }
  }
  __syncthreads();
  int cnt = DICT_WG_LANES, cur = 0;
  for (int lv = llog + 1; lv <= COL_CHUNK_LOG2; lv++) {
    const int half = cnt >> 1;
    // parent `lane` of this level covers rows from prow: skip it past row_end
    const uint64_t prow = wg_row + ((uint64_t)lane << lv);
    if (lane < half && prow < row_end) {
      uint32_t l[8], r[8], h[8];
#pragma unroll
      for (int w = 0; w < 8; w++) {
        const uint2 pr = *reinterpret_cast<const uint2*>(&lds[cur][w][2 * lane]);
        l[w] = pr.x;
        r[w] = pr.y;
      }
      b3_parent(l, r, h);
#pragma unroll
      for (int w = 0; w < 8; w++) lds[cur ^ 1][w][lane] = h[w];
      if (lv < COL_CHUNK_LOG2)
        node_store(dl + 8 * ((prow >> COL_CHUNK_LOG2) * DLEV_NODES + dlev_base(lv) +
                             ((prow >> lv) & ((1u << (COL_CHUNK_LOG2 - lv)) - 1))),
                   h);
    }
    __syncthreads();
    cur ^= 1;
    cnt = half;
  }
  // cnt chunk roots of this WG -> leaves of the column's outer tree
  for (int i = lane; i < cnt * 8; i += DICT_WG_LANES) {
    const uint64_t ch = (wg_row >> COL_CHUNK_LOG2) + (i >> 3);
    if (ch < nch_all && (ch << COL_CHUNK_LOG2) < row_end)
      outer[(uint64_t)dc.col * outer_stride * 8 + ch * 8 + (i & 7)] = lds[cur][i & 7][i >> 3];
  }
}

// Level LVL of the wide head ladders (HeadWideDev) that proof `seq` builds:
// grid (entries, dictionary columns), grid-stride over the level's entries.
// An entry of L1 / L2 whose heads leave the widened range [wlo, wlo + sw) is
// never read (no group that starts in the span reaches it) and is skipped.
template <int LVL>
__global__ void __launch_bounds__(TR_THREADS) k_head_ladder(const ColTemplate* __restrict__ tmpl,
                                                            const DictCol* __restrict__ dcols,
                                                            const HeadWideDev* __restrict__ hw, uint64_t seq,
                                                            uint32_t* __restrict__ tabs) {
  const HeadWideDev W = hw[blockIdx.y];
  if (W.build_seq != seq) return;
  constexpr int NM = (1 << LVL) - 1;             // moves of an entry
  constexpr int HALF = LVL > 0 ? 1 << (LVL - 1) : 0;  // rows of a child
  const uint32_t dR = W.dR;
  const int64_t dmax = W.dmin + (int64_t)dR - 1;
  const int64_t neg = W.dmin < 0 ? W.dmin : 0, pos = dmax > 0 ? dmax : 0;
  const int64_t wlo = W.olo + 7 * neg;
  const uint32_t sw = W.span + 7u * (uint32_t)(pos - neg);
  const uint32_t d3 = dR * dR * dR;
  uint32_t* l0 = tabs + 8 * W.low;
  uint32_t* l1 = l0 + 8 * (uint64_t)sw;
  uint32_t* l2 = l1 + 8 * (uint64_t)sw * dR;
  uint32_t* l3 = tabs + 8 * W.l3;
  const uint32_t s = LVL == 3 ? W.span : sw;  // first heads of the level
  const uint32_t cnt = LVL == 0 ? sw : LVL == 1 ? sw * dR : LVL == 2 ? sw * d3 : W.span * d3 * d3 * dR;
  const uint32_t base = LVL == 3 ? (uint32_t)(W.olo - wlo) : 0u;  // code (head - wlo) of the first one
  const ColTemplate ct = tmpl[dcols[blockIdx.y].col];
  for (uint32_t e = blockIdx.x * TR_THREADS + threadIdx.x; e < cnt; e += gridDim.x * TR_THREADS) {
    uint32_t h[8];
    if constexpr (LVL == 0) {
      leaf_labeled_rt(ct, gl_from_i64(wlo + (int64_t)e), h);
      node_store(l0 + 8 * (uint64_t)e, h);
    } else {
      const uint32_t c = base + e % s;
      uint32_t rest = e / s;
      int64_t run = c, cr = 0;
      uint32_t li = 0, ri = 0, lm = 1, rm = 1;
      bool ok = true;
#pragma unroll
      for (int i = 1; i <= NM; i++) {
        const uint32_t d = rest % dR;
        rest /= dR;
        run += W.dmin + (int64_t)d;
        ok = ok && run >= 0 && run < (int64_t)sw;
        if (i < HALF) { li += d * lm; lm *= dR; }
        else if (i == HALF) cr = run;
        else { ri += d * rm; rm *= dR; }
      }
      if (!ok) continue;
      const uint32_t* ch = LVL == 1 ? l0 : LVL == 2 ? l1 : l2;
      uint32_t* dst = LVL == 1 ? l1 : LVL == 2 ? l2 : l3;
      uint32_t a[8], b[8];
      node_load(ch + 8 * (uint64_t)(c + sw * li), a);
      node_load(ch + 8 * (uint64_t)((uint32_t)cr + sw * ri), b);
      b3_parent(a, b, h);
      node_store(dst + 8 * (uint64_t)e, h);
    }
  }
}

// ------------------------------------------------------------------ host
hipError_t launch_head_ladder(hipStream_t st, const ColTemplate* d_tmpl, const DictCol* d_dcols, int ndict,
                              const HeadWideDev* d_hw, uint64_t seq, uint32_t* d_hwtabs, uint64_t max_entries) {
  if (ndict == 0 || max_entries == 0) return hipSuccess;
  if (max_entries > (1ull << 24)) return hipErrorInvalidValue;
  // the lower levels are small: the grid of L3 would only read the record
  const unsigned g3 = (unsigned)std::min<uint64_t>((max_entries + TR_THREADS - 1) / TR_THREADS, 2048);
  const unsigned glow = std::min(g3, 64u);
  hipLaunchKernelGGL(k_head_ladder<0>, dim3(glow, ndict), dim3(TR_THREADS), 0, st, d_tmpl, d_dcols, d_hw, seq, d_hwtabs);
  hipLaunchKernelGGL(k_head_ladder<1>, dim3(glow, ndict), dim3(TR_THREADS), 0, st, d_tmpl, d_dcols, d_hw, seq, d_hwtabs);
  hipLaunchKernelGGL(k_head_ladder<2>, dim3(glow, ndict), dim3(TR_THREADS), 0, st, d_tmpl, d_dcols, d_hw, seq, d_hwtabs);
  hipLaunchKernelGGL(k_head_ladder<3>, dim3(g3, ndict), dim3(TR_THREADS), 0, st, d_tmpl, d_dcols, d_hw, seq, d_hwtabs);
  return hipGetLastError();
}
static hipError_t dict_shape_ok(const TraceDev& T, uint64_t row0, uint64_t nrows) {
  if (T.n < (1ULL << COL_CHUNK_LOG2)) return hipErrorInvalidValue;
  if (row0 + nrows > T.n || (nrows != T.n && (row0 % DICT_WG_ROWS || nrows % DICT_WG_ROWS))) return hipErrorInvalidValue;
  return hipSuccess;
}
// The dictionary commitment, in this order on one stream: ranges + plans +
// reuse flags, the table levels of the columns marked for rebuild (every
// level 0..K of a column before its commit), and the commit of every column.
hipError_t launch_dict_commit(hipStream_t st, const TraceDev& T, const ColTemplate* d_tmpl, const DictCol* d_dcols,
                              int ndict, int64_t* d_part, DictPlan* d_plans, uint32_t* d_dtabs, uint32_t* outer_nodes,
                              uint64_t outer_stride_nodes, uint64_t row0, uint64_t nrows, uint32_t* d_dlev,
                              const DictCache& dc, uint32_t tab_cap, uint64_t plan_rows) {
  if (ndict == 0) return hipSuccess;
  hipError_t e = dict_shape_ok(T, row0, nrows);
  if (e != hipSuccess) return e;
  if (tab_cap == 0 || tab_cap > DICT_CAP) return hipErrorInvalidValue;
  if (!dc.hwstat || (dc.hw && !dc.hwtabs)) return hipErrorInvalidValue;
  // parts of 1..8 sweeps: ~64 per column (the partial buffer holds n / 4096)
  const int sweeps = (int)std::max<uint64_t>(1, std::min<uint64_t>(8, nrows / (64ull * DICT_RANGE_STEP)));
  const uint64_t prow = (uint64_t)sweeps * DICT_RANGE_STEP;
  const uint32_t nparts = (uint32_t)((nrows + prow - 1) / prow);
  hipLaunchKernelGGL(k_dict_range, dim3(nparts, ndict), dim3(TR_THREADS), 0, st, T, d_tmpl, d_dcols, d_part, nparts,
                     row0, row0 + nrows, sweeps);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  hipLaunchKernelGGL(k_dict_plan, dim3(ndict), dim3(TR_THREADS), 0, st, d_part, nparts, T.n,
                     plan_rows ? plan_rows : nrows, d_dcols, d_plans, tab_cap, dc);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  for (int l = 0; l < DICT_LEVELS; l++) {
    // one flat launch per level (and per DICT_FLAT_MAX columns): all WGs
    // share every column's entries
    for (int c0 = 0; c0 < ndict; c0 += DICT_FLAT_MAX) {
      const int nc = ndict - c0 < DICT_FLAT_MAX ? ndict - c0 : DICT_FLAT_MAX;
      hipLaunchKernelGGL(k_dict_level, dim3(DICT_FLAT_WGS), dim3(TR_THREADS), 0, st, d_tmpl, d_dcols + c0,
                         d_plans + c0, dc.reuse + c0, dc.lvl_seq, dc.seq, d_dtabs, nc, l);
      if ((e = hipGetLastError()) != hipSuccess) return e;
    }
  }
  const uint64_t wg_rows = (uint64_t)DICT_WG_LANES << DICT_LANE_LOG;  // rows of a WG at a = 0
  const unsigned gx = (unsigned)((nrows + wg_rows - 1) / wg_rows);
  hipLaunchKernelGGL(k_col_commit_dict, dim3(gx, ndict), dim3(DICT_WG_LANES), 0, st, T, d_tmpl, d_dcols, d_plans, d_dtabs,
                     outer_nodes, outer_stride_nodes, row0, row0 + nrows, d_dlev, dc.hw, dc.hwtabs, dc.epoch, dc.hwstat);
  return hipGetLastError();
}

}  // namespace sezkp
