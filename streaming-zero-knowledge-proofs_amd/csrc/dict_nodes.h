// dict_nodes.h — device code shared by the dictionary commitment
// (dict_commit.hip) and the column openings (col_open.hip): the dense columns'
// keys, the table-node providers and the per-lane Merkle reductions over them.
// An opening recomputes the nodes the commitment gathered, so both sides take
// them from here.
#pragma once
#include "dev_common.h"
#include "col_leaf.h"
#include "sezkp_internal.h"

namespace sezkp {

// ------------------------------------------------ dictionary commitments
// Exact memoization for the dense columns (input_mv, mv, write_flag,
// write_sym, head). Their raw integers lie in a small range [min, min+R) on
// real traces (the AIR constrains mv/input_mv to {-1,0,1} and write_flag to
// {0,1}; symbols come from a small alphabet; heads are block-relative walks).
// The hash of an aligned 2^k-row subtree is a function of its k-tuple of
// codes (raw - min), so tables T_k[e], e = sum_i code_i * R^i (row i of the
// subtree), built level by level (T_0 = labelled leaves, T_{k+1} = H(T_k||T_k)),
// replace the bottom K levels of every chunk tree. K is chosen per column on
// the device from the measured range (cost = table entries + n / 2^K);
// R^(2^K) <= DICT_CAP. Columns whose range is too wide use K = -1 (leaves
// computed per row). The commitment is bit-identical either way.

template <typename Key>
__device__ __forceinline__ const Key* dict_keys(const TraceDev& T, const ColTemplate& ct) {
  const uint64_t o = (uint64_t)ct.tape * T.n;
  if constexpr (sizeof(Key) == 4) return reinterpret_cast<const Key*>(T.head + o);
  else if constexpr (sizeof(Key) == 2) return reinterpret_cast<const Key*>(T.wsym + o);
  else {
    if (ct.kind == 0) return reinterpret_cast<const Key*>(T.input_mv);
    if (ct.kind == 3) return reinterpret_cast<const Key*>(T.mv + o);
    return reinterpret_cast<const Key*>(T.wflag + o);
  }
}
// raw integer of a dense column at `row` (signed for i8 / i64 kinds)
__device__ __forceinline__ int64_t dict_key_at(const TraceDev& T, const ColTemplate& ct, uint64_t row) {
  const uint64_t o = (uint64_t)ct.tape * T.n + row;
  switch (ct.kind) {
    case 0: return T.input_mv[row];
    case 3: return T.mv[o];
    case 4: return T.wflag[o];
    case 5: return T.wsym[o];
    default: return T.head[o];
  }
}

// Node providers for lane_tree: node j of the lane's 2^D nodes. The gathered
// providers derive a node in two steps, raw(j) (the node's key bytes, one
// load) and node(raw) (table index, node load), which lane_tree_pf pipelines;
// get(j) is the two in a row, so the commitment and the openings index the
// tables by the same code.
template <typename Key, int K>
struct DictNodes {
  const Key* p;           // first row of the lane
  const uint32_t* tab;    // T_K
  int64_t mn;
  uint32_t R;
  static constexpr int CNT = 1 << K;
  static constexpr int BYTES = CNT * (int)sizeof(Key);
  static constexpr int NW = BYTES >= 4 ? BYTES / 4 : 1;
  struct Raw {
    uint32_t w[NW];
  };
  __device__ __forceinline__ void get(int j, uint32_t (&h)[8]) const { node(raw(j), j, h); }
  // the node's 2^K keys in one load of up to 16 bytes instead of 2^K narrow
  // ones: the lanes of a wave sit 2^(6+a) rows apart, so every load
  // instruction touches 64 cache lines and the commit was bound by load issue
  // (mv: 8 byte loads per node, wsym: 4 short loads). p + (j << K) must be
  // aligned to min(16, 2^K sizeof(Key)) bytes.
  __device__ __forceinline__ Raw raw(int j) const {
    Raw r;
    const Key* q = p + ((uint64_t)j << K);
    if constexpr (BYTES >= 16) {
#pragma unroll
      for (int i = 0; i < BYTES / 16; i++) {
        const uint4 v = reinterpret_cast<const uint4*>(q)[i];
        r.w[4 * i] = v.x; r.w[4 * i + 1] = v.y; r.w[4 * i + 2] = v.z; r.w[4 * i + 3] = v.w;
      }
    } else if constexpr (BYTES == 8) {
      const uint2 v = *reinterpret_cast<const uint2*>(q);
      r.w[0] = v.x; r.w[1] = v.y;
    } else if constexpr (BYTES == 4) {
      r.w[0] = *reinterpret_cast<const uint32_t*>(q);
    } else if constexpr (BYTES == 2) {
      r.w[0] = *reinterpret_cast<const uint16_t*>(q);
    } else {
      r.w[0] = *reinterpret_cast<const uint8_t*>(q);
    }
    return r;
  }
  __device__ __forceinline__ void node(const Raw& r, int, uint32_t (&h)[8]) const {
    uint32_t idx = 0;
#pragma unroll
    for (int i = CNT - 1; i >= 0; i--) {
      int64_t k;
      if constexpr (sizeof(Key) == 8) {
        k = (int64_t)((uint64_t)r.w[2 * i] | ((uint64_t)r.w[2 * i + 1] << 32));
      } else if constexpr (sizeof(Key) == 4) {
        k = (int64_t)(int32_t)r.w[i];
      } else {
        const int bit = i * 8 * (int)sizeof(Key);
        k = (int64_t)(Key)((r.w[bit / 32] >> (bit % 32)) & ((1u << (8 * sizeof(Key))) - 1u));
      }
      idx = idx * R + (uint32_t)(k - mn);
    }
    node_load(tab + 8 * (uint64_t)idx, h);
  }
};
// head delta plan: node j = the 4-row group at row 4j of the lane
struct DeltaNodes {
  const int32_t* hp;      // head, first row of the lane
  const int8_t* mp;       // mv of the same tape
  const uint8_t* fp;      // row_flags (bit 0 = block start)
  const uint32_t* t1;     // T_1
  const uint32_t* td;     // TD
  int64_t mn, dmin;
  uint32_t R, dR;
  __device__ __forceinline__ void get(int j, uint32_t (&h)[8]) const { node(raw(j), j, h); }
  // lane_tree_pf split: flags, moves and the first head of the group (the
  // other three heads are read only in the rare block-start case)
  struct Raw {
    uint32_t f, m;
    int64_t h0;
  };
  __device__ __forceinline__ Raw raw(int j) const {
    const uint64_t g = (uint64_t)j << 2;
    return Raw{*reinterpret_cast<const uint32_t*>(fp + g), *reinterpret_cast<const uint32_t*>(mp + g), hp[g]};
  }
  __device__ __forceinline__ void node(const Raw& r, int j, uint32_t (&h)[8]) const {
    const int64_t c0 = r.h0 - mn;
    if (!(r.f & 0x01010100u)) {
      const int64_t d1 = (int64_t)(int8_t)(r.m >> 8) - dmin, d2 = (int64_t)(int8_t)(r.m >> 16) - dmin,
                    d3 = (int64_t)(int8_t)(r.m >> 24) - dmin;
      node_load(td + 8 * (uint64_t)(c0 + (int64_t)R * (d1 + (int64_t)dR * (d2 + (int64_t)dR * d3))), h);
    } else {  // a block starts inside the group: two T_1 nodes
      const uint64_t g = (uint64_t)j << 2;
      uint32_t a[8], b[8];
      node_load(t1 + 8 * (uint64_t)(c0 + (int64_t)R * (hp[g + 1] - mn)), a);
      node_load(t1 + 8 * (uint64_t)((hp[g + 2] - mn) + (int64_t)R * (hp[g + 3] - mn)), b);
      b3_parent(a, b, h);
    }
  }
};
// head delta plan with the wide ladder (HeadWideDev): node j = the 8-row
// group at row 8j of the lane, one L3 node; a group the ladder does not cover
// is the parent of its two DeltaNodes nodes, so the lane's root never depends
// on the ladder's coverage. cnt: this lane's groups, 10 bits each: from L3,
// fallen back for a block start in rows 1..7, fallen back for a first head
// outside the span (span = 0: the proof's moves are not all the ladder's)
struct WideNodes {
  DeltaNodes dn;
  const uint32_t* l3;
  int64_t olo;
  int32_t wdmin;
  uint32_t span, wdR;
  mutable uint32_t cnt;
  struct Raw {
    uint64_t f, m;
    int64_t h0;
  };
  __device__ __forceinline__ Raw raw(int j) const {
    const uint64_t g = (uint64_t)j << 3;
    return Raw{*reinterpret_cast<const uint64_t*>(dn.fp + g), *reinterpret_cast<const uint64_t*>(dn.mp + g),
               dn.hp[g]};
  }
  __device__ __forceinline__ void node(const Raw& r, int j, uint32_t (&h)[8]) const {
    const uint64_t c0 = (uint64_t)(r.h0 - olo);
    const bool starts = (r.f & 0x0101010101010100ull) != 0;
    if (!starts && c0 < span) {
      uint32_t idx = 0;
#pragma unroll
      for (int i = 7; i >= 1; i--) idx = idx * wdR + (uint32_t)((int32_t)(int8_t)(r.m >> (8 * i)) - wdmin);
      node_load(l3 + 8 * (uint64_t)((uint32_t)c0 + span * idx), h);  // < span dR^7 <= 2^24
      cnt += 1u;
    } else {
      uint32_t a[8], b[8];
      dn.get(2 * j, a);
      dn.get(2 * j + 1, b);
      b3_parent(a, b, h);
      cnt += starts ? 1u << 10 : 1u << 20;
    }
  }
};
template <typename Key>
struct RawLeaves {
  const Key* p;
  const ColTemplate* ct;
  __device__ __forceinline__ void get(int j, uint32_t (&h)[8]) const {
    leaf_labeled_rt(*ct, gl_from_i64((int64_t)p[j]), h);
  }
};

// Binary-counter Merkle step: node x (index j of the lane's run) merges with
// the pending left siblings s[L], s[L+1], ... while bit L of j is set, then
// waits at its level (or is the root). Template recursion keeps every stack
// index static: the stack stays in registers.
template <int L, int D>
__device__ __forceinline__ void counter_push(uint32_t (&s)[D > 0 ? D : 1][8], uint32_t (&x)[8], int j,
                                             uint32_t (&h)[8]) {
  if constexpr (L == D) {
#pragma unroll
    for (int w = 0; w < 8; w++) h[w] = x[w];
  } else {
    if ((j >> L) & 1) {
      b3_parent(s[L], x, x);
      counter_push<L + 1, D>(s, x, j, h);
    } else {
#pragma unroll
      for (int w = 0; w < 8; w++) s[L][w] = x[w];
    }
  }
}

// Binary-counter Merkle reduction of 2^D consecutive nodes in a rolled loop:
// the stack is indexed statically (merges unrolled per level, branch on the
// uniform loop counter), so code size is D+1 compressions, not 2^(D+1).
template <int D, class Prov>
__device__ __forceinline__ void lane_tree(const Prov& P, uint32_t (&h)[8]) {
  uint32_t s[D > 0 ? D : 1][8];
  for (int j = 0; j < (1 << D); j++) {
    uint32_t x[8];
    P.get(j, x);
    counter_push<0, D>(s, x, j, h);
  }
}
// lane_tree with the gathers software-pipelined: while node j is merged, the
// table node of j + 1 and the key bytes of j + 2 are in flight, so a lane's
// dependent key -> index -> node chain is paid once per lane, not per node
// (the rolled loop of lane_tree issues each node's loads only after the
// previous node's compressions)
template <int D, class Prov>
__device__ __forceinline__ void lane_tree_pf(const Prov& P, uint32_t (&h)[8]) {
  constexpr int N = 1 << D;
  uint32_t s[D > 0 ? D : 1][8];
  uint32_t nx[8];
  typename Prov::Raw k1 = P.raw(0);
  P.node(k1, 0, nx);
  if (N > 1) k1 = P.raw(1);
  for (int j = 0; j < N; j++) {
    uint32_t x[8];
#pragma unroll
    for (int w = 0; w < 8; w++) x[w] = nx[w];
    if (j + 1 < N) P.node(k1, j + 1, nx);
    if (j + 2 < N) k1 = P.raw(j + 2);
    counter_push<0, D>(s, x, j, h);
  }
}

// level-K node of a dictionary column covering rows [row, row + 2^K) (the
// commitment's DictNodes / DeltaNodes for one node). row is a multiple of 2^K
// (4 for the delta plan) and a column starts at a multiple of n >= 1024 keys,
// so the provider's single 2^K sizeof(Key)-byte key load is aligned.
__device__ __forceinline__ void dict_node_at(const TraceDev& T, const ColTemplate& ct, const DictPlan& P,
                                             const uint32_t* __restrict__ tab, uint64_t row, uint32_t (&h)[8]) {
  if (P.delta) {
    const uint64_t o = (uint64_t)ct.tape * T.n + row;
    DeltaNodes{T.head + o, T.mv + o, T.row_flags + row, tab + 8 * (uint64_t)DICT_CAP, tab + 16 * (uint64_t)DICT_CAP,
               P.min, P.dmin, P.R, P.dR}
        .get(0, h);
    return;
  }
#define SEZKP_DN(KEY)                                                                                           \
  {                                                                                                             \
    const KEY* p = dict_keys<KEY>(T, ct) + row;                                                                 \
    switch (P.K) {                                                                                              \
      case 0: DictNodes<KEY, 0>{p, tab, P.min, P.R}.get(0, h); break;                                           \
      case 1: DictNodes<KEY, 1>{p, tab + 8 * (uint64_t)DICT_CAP, P.min, P.R}.get(0, h); break;                  \
      case 2: DictNodes<KEY, 2>{p, tab + 16 * (uint64_t)DICT_CAP, P.min, P.R}.get(0, h); break;                 \
      case 3: DictNodes<KEY, 3>{p, tab + 24 * (uint64_t)DICT_CAP, P.min, P.R}.get(0, h); break;                 \
      default: DictNodes<KEY, 4>{p, tab + 32 * (uint64_t)DICT_CAP, P.min, P.R}.get(0, h); break;                \
    }                                                                                                           \
  }
  switch (ct.kind) {
    case 0: case 3: SEZKP_DN(int8_t) break;
    case 4: SEZKP_DN(uint8_t) break;
    case 5: SEZKP_DN(uint16_t) break;
    default: SEZKP_DN(int32_t) break;
  }
#undef SEZKP_DN
}

// path_in_chunk siblings at levels glog..9 of a dictionary column, stored by
// the commitment: thread (level, word), one round of loads
__device__ __forceinline__ void copy_dlev_siblings(const uint32_t* __restrict__ lev, uint64_t in, int glog,
                                                   uint32_t* __restrict__ o) {
  const int lvl = glog + (threadIdx.x >> 3), w = threadIdx.x & 7;
  if (lvl < COL_CHUNK_LOG2) o[18 + 8 * lvl + w] = lev[8 * (dlev_base(lvl) + ((in >> lvl) ^ 1)) + w];
}

}  // namespace sezkp
